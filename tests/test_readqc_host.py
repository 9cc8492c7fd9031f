"""The host side of the read QC report (host/readqc.cpp, include/kslam_readqc.h): kslam_tail_read_qc equals the plain-Python
restatement (tests/readqc_ref.py) field for field on the case set the device is held to, kslam_read_qc_write equals the
restatement's bytes and json.loads takes them, the argument errors are returned, the library exports what the header declares.
No GPU."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

import readqc_ref as R
from test_readqc_ref import HEADER_EXAMPLE

ERR_ARG = 1   # include/kslam.h: kslam_status
CASES = R.cases()


@pytest.fixture(scope="module")
def RQ(kslam):
    return importlib.import_module("kslam_amd.readqc")


@pytest.fixture(scope="module")
def expected():
    """the restatement's tables per case, computed once"""
    return {c["name"]: R.tables(c["bases"], c["quality"], c["paired"], c["cycles"]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_equals_restatement(RQ, expected, case):
    exp = expected[case["name"]]
    got = RQ.tail_read_qc(case["bases"], case["quality"], case["paired"], case["cycles"])
    assert got["max_cycles"] == exp["max_cycles"] and got["paired"] == exp["paired"]
    for z in range(2):
        for key, want in exp["streams"][z].items():
            assert got["streams"][z][key] == want, (case["name"], z, key)
    text = RQ.report_bytes(got)
    assert text == R.text(exp)
    doc = json.loads(text)
    assert doc["summary"]["total_reads"] == len(case["bases"]) and doc["summary"]["total_bases"] == sum(len(b) for b in case["bases"])
    parsed = RQ.parse(text)
    assert parsed["max_cycles"] == exp["max_cycles"] and isinstance(parsed["summary"]["q30_rate"], float)


def test_the_headers_example_and_the_parser(RQ):
    t = RQ.tail_read_qc([b"ACGTN", b"GGC"], [b"IIII#", b"5?~"], True, 4)
    assert RQ.report_bytes(t) == HEADER_EXAMPLE
    doc = RQ.parse(HEADER_EXAMPLE)
    assert doc["read1"]["length_counts"] == {">4": 1} and doc["read2"]["length_counts"] == {3: 1}
    assert doc["read1"]["quality_counts"] == {2: [0, 0, 0, 0, 1], 40: [1, 1, 1, 1]} and doc["read1"]["quality_mean"] == [40.0] * 4
    assert doc["summary"]["gc_content"] == pytest.approx(5 / 7, abs=1e-6)
    with pytest.raises(ValueError):
        RQ.parse(b'{"kslam_read_qc": 2}')
    assert RQ.unpack(*RQ.pack(t)) == t


def test_argument_errors(kslam, RQ):
    L = RQ.lib()
    T = importlib.import_module("kslam_amd.tail")
    bases, quality = np.frombuffer(b"ACGTAC", dtype=np.uint8), np.frombuffer(b"IIIIII", dtype=np.uint8)
    good = np.array([0, 3, 6], dtype=np.uint64)

    def call(boff, qoff, n, paired, cycles=0, t=None):
        t = t if t is not None else RQ.Tables()
        rc = L.kslam_tail_read_qc(bases.ctypes.data, boff.ctypes.data, quality.ctypes.data, qoff.ctypes.data, n, paired, cycles, C.byref(t))
        if rc == 0:
            L.kslam_tail_read_qc_free(C.byref(t))
        else:
            assert not t.block
        return rc

    assert call(good, good, 2, 1) == 0
    assert call(good, np.array([0, 2, 6], dtype=np.uint64), 2, 0) == ERR_ARG          # 3 bases, 2 quality bytes
    assert b"read 0 has 3 bases and 2 quality bytes" in T.lib().kslam_tail_last_error()
    assert call(np.array([0, 4, 3], dtype=np.uint64), np.array([0, 4, 3], dtype=np.uint64), 2, 0) == ERR_ARG   # offsets that do not ascend
    assert call(np.array([0, 2, 4, 6], dtype=np.uint64), np.array([0, 2, 4, 6], dtype=np.uint64), 3, 1) == ERR_ARG   # paired, odd
    assert call(good, good, 2, 0, cycles=65537) == ERR_ARG
    assert call(good, good, 2, 0, cycles=65536) == 0
    assert L.kslam_tail_read_qc(None, None, None, None, 1, 0, 0, C.byref(RQ.Tables())) == ERR_ARG
    assert L.kslam_tail_read_qc(None, None, None, None, 0, 0, 0, None) == ERR_ARG
    # the writer: tables nobody laid out
    t = RQ.Tables()
    assert L.kslam_read_qc_write(C.byref(t), -1) == ERR_ARG and L.kslam_read_qc_write(None, -1) == ERR_ARG
    block = np.zeros(2 * RQ.words(4), dtype=np.uint64)
    t.max_cycles, t.words_per_stream, t.block = 4, RQ.words(4) + 1, block.ctypes.data
    assert L.kslam_read_qc_write(C.byref(t), -1) == ERR_ARG
    t.words_per_stream = RQ.words(4)
    assert L.kslam_read_qc_write(C.byref(t), -1) == ERR_ARG and b"writing the read QC report failed" in T.lib().kslam_tail_last_error()   # a bad descriptor
    with pytest.raises(ValueError):
        RQ.add(None, [b"AC"], [b"I"])


def test_library_exports_every_declared_symbol(kslam, RQ):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "kslam_readqc.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = C.CDLL(kslam.LIB_PATH)
    assert len(declared) == 12 and sorted(RQ.EXPORTS) == declared
    for name in declared:
        assert hasattr(L, name), "missing export " + name
    assert C.sizeof(RQ.StreamView) == 72 and C.sizeof(RQ.Tables) == 24 + 2 * 72
    assert RQ.words(512) == 4 + 514 + 513 * 101 + 195
