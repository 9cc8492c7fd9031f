"""The host twin of the reads split (kslam_tail_split_reads, include/kslam_readsplit.h) against the plain-Python restatement
(tests/readsplit_ref.py): terminators, the end-of-stream rules, headers, line lengths at every width the device copy
distinguishes, max_pairs, single-end; and the partition property.  No GPU."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import readsplit_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()


@pytest.fixture(scope="module")
def RS(kslam):
    return importlib.import_module("kslam_amd.readsplit")


def test_the_restatement_itself():
    assert R.lines(b"a\nb\r\nc\rd") == [b"a", b"b", b"c", b"d", b""]
    assert R.lines(b"a\n") == [b"a", b""] and R.lines(b"") == [b""] and R.lines(b"a\n", at_eof=False) == [b"a"]
    assert R.lines(b"a\r", at_eof=False) == [] and R.lines(b"a\r\n\r", at_eof=False) == [b"a"]
    assert R.records(b"@h\nAC\n+\nII") == [b"@h\nAC\n+\nII\n"] and R.records(b"@h\n\n+\n") == [b"@h\n\n+\n\n"]
    assert R.records(b"@h\nAC\n+\nII", at_eof=False) == []


def test_library_exports_every_readsplit_symbol(kslam, RS):
    h = open(os.path.join(ROOT, "include", "kslam_readsplit.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 11 and declared == sorted(RS.EXPORTS) and all(hasattr(L, n) for n in declared)
    assert ctypes.sizeof(RS.ReadsOut) == 88
    assert ctypes.sizeof(kslam.BatchResult) == 232   # kslam_batch_result keeps its size: callers allocate it


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_twin_matches_the_restatement(RS, case):
    name, r1, r2, max_pairs, at_eof = case
    n = len(R.records(r1, max_pairs, at_eof))
    if r2 is not None:
        assert len(R.records(r2, max_pairs, at_eof)) == n
    for pname, sel in R.patterns(n).items():
        for which in (1, 2, 3):
            exp, n_exp = R.split(r1, r2, sel, which, max_pairs, at_eof)
            got = RS.tail_split_reads(r1, r2, R.read_pairs(sel, n, paired=r2 is not None), which, max_pairs, at_eof)
            assert got["blocks"] == exp, (name, pname, which)
            assert got["n_records"] == n_exp and got["flags"] == RS.FLAG_HOST_MEMORY
        # the partition: disjoint, and merged back by record number exactly the records taken
        both = RS.tail_split_reads(r1, r2, R.read_pairs(sel, n, paired=r2 is not None), 3, max_pairs, at_eof)["blocks"]
        for k, text in enumerate([r1] + ([r2] if r2 is not None else [])):
            assert R.merge(both[k], both[2 + k], sel, n) == b"".join(R.records(text, max_pairs, at_eof))


def test_lf_text_comes_out_verbatim(RS):
    r1, r2 = R.text_of(9), R.text_of(9, mate=2)
    got = RS.tail_split_reads(r1, r2, R.read_pairs(list(range(9)), 9), 3)["blocks"]
    assert got[0] == r1 and got[1] == r2 and got[2] == b"" and got[3] == b""
    crlf = RS.tail_split_reads(R.text_of(9, b"\r\n"), R.text_of(9, b"\r", mate=2), R.read_pairs([], 9), 2)["blocks"]
    assert crlf == [None, None, r1, r2]


def test_refusals(kslam, RS):
    r1, r2 = R.text_of(4), R.text_of(4, mate=2)
    for which in (0, 4, 7):
        with pytest.raises(Exception, match="mask"):
            RS.tail_split_reads(r1, r2, R.read_pairs([0], 4), which)
    with pytest.raises(Exception, match="outside the batch"):
        RS.tail_split_reads(r1, r2, R.read_pairs([4], 4), 3)
    bad = R.read_pairs([1], 4)
    bad["r2_read"] = 6
    with pytest.raises(Exception, match="outside the batch"):
        RS.tail_split_reads(r1, r2, bad, 3)
    with pytest.raises(Exception, match="mismatch in R1 and R2 size"):
        RS.tail_split_reads(r1, R.text_of(3, mate=2), R.read_pairs([0], 4), 3)
