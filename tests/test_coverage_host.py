"""The host twin of the coverage table (kslam_tail_coverage) and the report writer (kslam_coverage_write,
include/kslam_coverage.h) against the plain-Python restatement (tests/coverage_ref.py): the case list the device is held to and
200 seeded random cases; the report byte for byte against the restatement's formatter.  No GPU."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()


@pytest.fixture(scope="module")
def CV(kslam):
    return importlib.import_module("kslam_amd.coverage")


@pytest.fixture(scope="module")
def T(kslam):
    return importlib.import_module("kslam_amd.tail")


def test_the_restatement_itself():
    c = R.build("x", [70, 10], [([(0, (0, 3, 5), (0, 5, 66))], [(1, (1, 0, 9), None)]), ([(1, (1, 9, 9), None), (0, (0, 0, 0), None)], [])])
    rows, skipped, cov = R.table(c["lengths"], c["ov"], c["rp"], c["pr"])
    assert rows.tolist() == [(2, 1, 3 + 62 + 1, 65), (1, 0, 1, 1)] and skipped == 0
    assert R.words(cov[0]).tolist() == [0xFFFFFFFFFFFFFFF9, 0x7] and R.words(cov[1]).tolist() == [1 << 9]
    assert R.words(np.zeros(0, dtype=bool)).tolist() == []
    assert R.report(rows, [70, 10], [b"a", b"b"], [7, 9]) == R.HEADER + b"0\ta\t7\t70\t2\t1\t66\t65\t0.928571\t0.9429\n1\tb\t9\t10\t1\t0\t1\t1\t0.100000\t0.1000\n"


def test_library_exports_every_coverage_symbol(kslam, CV):
    h = open(os.path.join(ROOT, "include", "kslam_coverage.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 11 and declared == sorted(CV.EXPORTS) and all(hasattr(L, n) for n in declared)
    assert CV.ROW_DT.itemsize == 32 and CV.HEADER == R.HEADER
    assert ctypes.sizeof(kslam.BatchResult) == 232   # kslam_batch_result keeps its size: callers allocate it


def _check(CV, c):
    rows, skipped, _ = R.table(c["lengths"], c["ov"], c["rp"], c["pr"])
    got, got_skipped = CV.tail_coverage(c["lengths"], c["ov"], c["rp"], c["pr"])
    assert got.tolist() == rows.tolist(), c["name"]
    assert got_skipped == skipped, c["name"]
    return rows, skipped


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_twin_matches_the_restatement(CV, case):
    _check(CV, case)


def test_what_the_cases_are_there_for(CV):
    by = {c["name"]: c for c in CASES}
    rows, skipped = _check(CV, by["contention"])
    assert rows[0].tolist() == (20000, 20000, 20000 * 150 + sum(33 + k % 31 - k % 32 for k in range(20000)), 150) and skipped == 0
    rows, _ = _check(CV, by["dead"])
    assert rows["alignments"].tolist() == [1, 2, 1, 0] and rows[3].tolist() == (0, 0, 0, 0)
    rows, _ = _check(CV, by["mates"])
    assert rows[1].tolist() == (1, 1, 91 + 91, 141)
    rows, _ = _check(CV, by["unique"])
    assert rows["unique_read_pairs"].tolist() == [1, 1, 1] and rows["alignments"].tolist() == [4, 9999, 3]
    rows, skipped = _check(CV, by["skipped"])
    assert skipped == 4 and rows.tolist() == [(2, 2, 111, 100), (3, 3, 6 + 1 + 10, 17)]
    rows, _ = _check(CV, by["entries-odd"])
    assert rows["covered_bases"].tolist() == [0, 63, 0, 65, 0, 129]


def test_200_random_cases(CV):
    for seed in range(200):
        _check(CV, R.random_case("random-%d" % seed, seed, 1 + 3 * seed, 1 + seed % 9, 1 + (37 * seed) % 400))


def test_the_report_byte_for_byte(CV, T):
    rng = np.random.default_rng(11)
    for c in [c for c in CASES if c["name"] in ("unique", "skipped", "dead", "entries-odd", "grid-70001", "grid-0")]:
        n = len(c["lengths"])
        loci = [b"LOCUS_%d.%d" % (e, e % 3) for e in range(n)]
        tax = rng.integers(1, 1 << 31, n)
        index = T.IndexArrays(np.zeros(int(c["lengths"].sum()), dtype=np.uint8), np.concatenate([[0], np.cumsum(c["lengths"])]), loci, tax)
        rows, _ = CV.tail_coverage(c["lengths"], c["ov"], c["rp"], c["pr"])
        text = CV.report_bytes(index, rows)
        assert text == R.report(rows, c["lengths"], loci, tax), c["name"]
        parsed = CV.parse_report(text)
        assert [r["entry"] for r in parsed] == [e for e in range(n) if rows[e]["alignments"]]
        if c["name"] == "dead":
            assert [r["entry"] for r in parsed] == [0, 1, 2]   # the entry only dead records point at has no line
        assert all(r["covered_bases"] == int(rows[r["entry"]]["covered_bases"]) and r["locus"] == loci[r["entry"]].decode() for r in parsed)
    with pytest.raises(ValueError):
        CV.parse_report(b"entry\tlocus\n")
    with pytest.raises(Exception, match="not of this index"):
        CV.report_bytes(index, rows[:-1] if len(rows) else np.zeros(1, dtype=CV.ROW_DT))


def test_refusals(CV):
    c = R.build("x", [100], [([(0, (0, 0, 9), (0, 5, 20))], []), ([(0, (0, 1, 2), None)], [])])
    bad = c["pr"].copy()
    bad["r2"][0] = len(c["ov"])
    with pytest.raises(Exception, match="refers to overlap record"):
        CV.tail_coverage(c["lengths"], c["ov"], c["rp"], bad)
    rp = c["rp"].copy()
    rp["count"][1] = 2
    with pytest.raises(Exception, match="outside the pairs array"):
        CV.tail_coverage(c["lengths"], c["ov"], rp, c["pr"])
    rp = c["rp"].copy()
    rp["first"][1] = 0
    with pytest.raises(Exception, match="ascend"):
        CV.tail_coverage(c["lengths"], c["ov"], rp, c["pr"])
