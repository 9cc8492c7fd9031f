"""The three literal kernels at every seam: k_sw_striped and k_sw_long (k-slam_amd/csrc/sw.hip) and the one-lane banded_sw
(k-slam_amd/csrc/cigar.hip: k_banded_lds<0>, and k_banded_lds_wide with the reference's int32 rows).

Each case is a batch of tests/sw_literal_cases.py (tests/test_sw_literal_cases.py makes sure, on the CPU, that the families
reach what they are built for).  For every case:
  1. every row field and every CIGAR word equals oracle.align_to_database (the striped emulation, which the CPU tests hold
     to the real ssw.c): integers, compared exactly;
  2. a second align_batch on the same context is byte-identical;
  3. the lines KSLAM_DEBUG=1 prints say which path ran: every candidate through the literal kernels, no tier planning,
     k_sw_striped for a scoring outside the envelope and for any chunk in which match x longest read passes 32 767,
     k_sw_long otherwise, int32 CIGAR rows exactly where that product passes 32 767, one chunk per class run.
S9 (saturation inside the envelope) additionally runs the same reads with match lowered until nothing can saturate: the
k_sw_long route, so that the routing cannot hide a regression of that kernel.
"""
import re
import time

import numpy as np
import pytest

import sw_literal_cases as C
from align_compare import compare_alignments

pytestmark = pytest.mark.gpu

_expected = {}


def expected(oracle, name, sc):
    key = (name, sc)
    if key not in _expected:
        B = C.build(name)
        p = oracle.Params.default(match=sc[0], mismatch=sc[1], gap_open=sc[2], gap_extend=sc[3])
        _expected[key] = oracle.align_to_database(B.reads, B.entries, p)[:2]
    return _expected[key]


def class_runs(B, sc, exp):
    """(first read, longest read) of every run of reads of one class that has a candidate: the chunks of the batch"""
    import sw_plan_ref as R
    cap = R.short_cap(sc) if C.in_envelope(sc) else 0
    has = np.zeros(len(B.reads) + 1, dtype=bool)
    has[exp["read"]] = True
    runs, start = [], 0
    for i in range(1, len(B.reads) + 1):
        if i == len(B.reads) or (len(B.reads[i]) > cap) != (len(B.reads[start]) > cap):
            if has[start:i].any():
                runs.append((len(B.reads[start]) > cap, int(np.bincount(exp["read"], minlength=i)[start:i].sum()),
                             max(len(r) for r in B.reads[start:i])))
            start = i
    return runs


def run_case(kslam, oracle, monkeypatch, capfd, name, sc):
    B = C.build(name)
    exp, ecig = expected(oracle, name, sc)
    monkeypatch.setenv("KSLAM_DEBUG", "1")
    c = kslam.Context(match=sc[0], mismatch=sc[1], gap_open=sc[2], gap_extend=sc[3])
    try:
        c.reload_tuning()
        c.set_index(B.entries)
        capfd.readouterr()
        t0 = time.perf_counter()
        got, gcig = c.align_batch(B.reads)
        seconds = time.perf_counter() - t0
        err = capfd.readouterr().err
        again, acig = c.align_batch(B.reads)
        capfd.readouterr()
    finally:
        c.close()
    compare_alignments(got, gcig, exp, ecig)
    assert got.tobytes() == again.tobytes() and gcig.tobytes() == acig.tobytes()
    # ---- which path ran
    runs = class_runs(B, sc, exp)
    chunks = [(int(a), int(b)) for a, b in re.findall(r"\[kslam\] SW: (\d+) candidates, (\d+) needed", err)]
    longs = [(int(n), k, int(L)) for n, k, L in
             re.findall(r"\[kslam\] SW long chunk: (\d+) candidates through (k_sw_\w+) \(longest read (\d+)\)", err)]
    planned = re.findall(r"\[kslam\] SW planned", err)
    wide = [int(L) for L in re.findall(r"\[kslam\] cigar: int32 rows \(match \d+ x longest read (\d+)\)", err)]
    assert [n for _, n, _ in runs] == [n for n, _ in chunks], ("one chunk per class run", runs, chunks)
    want_long = [(n, "k_sw_striped" if not C.in_envelope(sc) or C.saturates(sc, L) else "k_sw_long", L)
                 for is_long, n, L in runs if is_long]
    assert longs == want_long, (longs, want_long)
    assert len(planned) == sum(not is_long for is_long, _, _ in runs)
    for (is_long, n, _), (m, full) in zip(runs, chunks):
        if is_long:
            assert full == m == n                      # every candidate through the literal kernels
    assert wide == [L for is_long, _, L in runs if is_long and C.saturates(sc, L)], wide
    return got, seconds


@pytest.mark.parametrize("name", list(C.CASES))
def test_literal_kernels_equal_the_oracle(kslam, oracle, monkeypatch, capfd, name):
    sc, group = C.CASES[name][1], C.CASES[name][2]
    got, seconds = run_case(kslam, oracle, monkeypatch, capfd, name, sc)
    B = C.build(name)
    longest = max(len(r) for r in B.reads)
    if group in ("S6", "S9") and name not in C.BELOW_SATURATION:
        assert int(got["score"].max()) == C.SAT
    if group == "S9":
        low = C.lowered(sc, B)
        assert C.in_envelope(low) and not C.saturates(low, longest)
        _, low_seconds = run_case(kslam, oracle, monkeypatch, capfd, name, low)
        print("%s with match lowered to %d (k_sw_long): first align_batch %.2f s" % (name, low[0], low_seconds))
    print("%s under %s: %d rows, first align_batch %.2f s" % (name, sc, len(got), seconds))
