"""The device tail front (csrc/pairs.hip) alone, at every hand-over inside it: the cases of tests/tail_seams.py -- a read pair of
exactly 256 / 257 rows, a group of exactly 96 / 97 alignment pairs, an entry of exactly 4000 / 4001 spans, stretches of 63 / 64 /
65 reads without rows, the insert-size statistics on 1 .. 200 values and at a ladder step of 1000 / 1001, chains decided at
sorted index 63 / 64 / 65 -- against the host tail on the same input, byte for byte.  tests/test_tail_seams.py proves on the
CPU that every case has the count it claims and that the host tail equals the oracle's restatement there."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_seams as S  # noqa: E402
from test_gpu_tail import _compacted  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = S.all_cases()


def _name(case):
    return case["name"]


@pytest.fixture(scope="module")
def T(kslam):
    return importlib.import_module("kslam_amd.tail")


@pytest.fixture(scope="module")
def ctx(kslam):
    c = kslam.Context()
    yield c
    c.close()


def _host(T, case, stages):
    reads = T.Reads([b"A" * S.READ_LEN] * case["n_reads"])
    P = T.TailParams.default(paired=case["paired"], report_cigar=False, threads=4, score_threshold=case["score_threshold"],
                             score_fraction=case["score_fraction"], pseudo_assembly=bool(stages & 4), stages=stages)
    return T.tail_pairs(P, reads, case["ov"])


def _device(c, case, stages):
    got = c.pair_screen_overlaps(case["ov"], case["read_lens"], paired=case["paired"], score_threshold=case["score_threshold"],
                                 score_fraction=case["score_fraction"], stages=stages)
    rp, pr = c.take_pairs()
    return got, rp, pr


def check_case(T, c, case):
    name, stages = case["name"], case["stages"]
    done = (stages & (3 if case["paired"] else 2)) | (4 if stages & 4 and case["on_device"] else 0)
    rp, pr, st = _host(T, case, stages if case["on_device"] else stages & 3)
    got, grp, gpr = _device(c, case, stages)
    assert got["stages_done"] == done, name
    if stages & 4:
        grp, gpr = _compacted(grp, gpr)
    assert grp.tobytes() == rp.tobytes(), name
    assert gpr.tobytes() == pr.tobytes(), name
    assert got["n_overlaps_screened"] == st.n_overlaps_screened and got["n_paired_initial"] == st.n_paired_initial, name
    assert got["n_read_pairs"] == len(rp) and got["n_pairs"] == len(pr), name
    if case["paired"] and stages & 1:
        assert got["max_insert_size"] == st.max_insert_size and got["n_insert_sizes"] == st.n_insert_sizes, name
        if "max_insert_size" in case["claim"]:
            assert got["max_insert_size"] == case["claim"]["max_insert_size"], name
    return grp, gpr


@pytest.mark.parametrize("case", CASES["A"], ids=_name)
def test_first_row_table_at_stretches_of_63_64_65_reads_without_rows(kslam, T, ctx, case):
    """k_row_starts / k_fill_gaps: stretches before the first row, inside mate 1, across the mate boundary and after the last
    row; stretches beyond k_fill_gaps' block of 256 threads and more of them than its 64 blocks; one mate without rows; no rows"""
    check_case(T, ctx, case)


@pytest.mark.parametrize("case", CASES["B"], ids=_name)
def test_pairing_hands_over_to_the_wavefront_at_257_rows(kslam, T, ctx, case):
    """k_pair up to 256 rows a read pair, k_pair_big from 257: 1, 64, 65, 128, 129, 257 entries a pair, entries of one mate
    only, thresholds that remove some rows or all, big pairs at the edges of the batch and of a 256-thread block, batches of 1 /
    255 / 256 / 257 read pairs, a block without insert sizes, 2049 big pairs for the 2048 blocks of the grid"""
    check_case(T, ctx, case)


@pytest.mark.parametrize("case", CASES["C"], ids=_name)
def test_insert_size_statistics_on_few_values_and_at_the_ladder_step(kslam, T, ctx, case):
    """1 .. 200 insert sizes, a percentile step of exactly 1000 / 1001, negative values, quartiles of -3 / -2, squares that wrap
    int32, records at the limit and one above: the limit equals the host tail's and the plain restatement's"""
    check_case(T, ctx, case)


def test_insert_size_sums_beyond_2p53_fall_back_to_the_sequential_sum(kslam, T, ctx):
    """4.4 M kept values whose squares add up past 2^53, handed to phase B as a device array (no 8 M rows needed): the limit
    equals tail_seams.insert_limit_ref's, which test_tail_seams.py holds to the host tail on every small case"""
    import torch
    v = S.stats_beyond_2p53()
    want = S.insert_limit_ref(v)
    case = CASES["A"][-1]                 # two reads, one alignment pair
    c = kslam.Context()
    try:
        c.load_reads([b"A" * S.READ_LEN] * case["n_reads"])
        d_ov = torch.from_numpy(case["ov"].view(np.uint8).copy()).cuda()
        d_cig = torch.zeros(4, dtype=torch.int32, device="cuda")
        c.adopt_results_device(d_ov.data_ptr(), len(case["ov"]), d_cig.data_ptr(), 0)
        _, n_own = c.pair_phase_a(True, 0)
        assert n_own == 1
        d_v = torch.from_numpy(v).cuda()
        torch.cuda.synchronize()
        st, _, n_pairs = c.pair_phase_b(d_v.data_ptr(), len(v), 0.95, 1)
        assert st["max_insert_size"] == want and st["n_insert_sizes"] == len(v) and n_pairs == 1
    finally:
        c.close()


@pytest.mark.parametrize("case", CASES["D"], ids=_name)
def test_screens_hand_over_to_the_wavefront_at_97_alignment_pairs(kslam, T, ctx, case):
    """k_screen up to 96 alignment pairs a group, k_screen_big from 97: none / half / all beyond the insert-size limit (the group
    doubles inside its region), the score bar at equality, fraction 1, all scores equal, 4100 pairs in a group, a big pair that
    the threshold empties, each stage alone, read pairs without records first / last / between"""
    check_case(T, ctx, case)


@pytest.mark.parametrize("case", CASES["E"], ids=_name)
def test_pseudo_assembly_at_4000_spans_the_cap_and_the_64_span_step(kslam, T, ctx, monkeypatch, case):
    """entries of 4000 (LDS) and 4001 (global memory) spans in one batch; KSLAM_PSEUDO_CAP = c: c spans stay on the device, c + 1
    return the stage to the host with nothing changed; the chain rule at reach - 20 / reach - 19 with the deciding span at sorted
    index 63 / 64 / 65 and the reach set several 64-span steps earlier; degenerate spans; equal starts; 1, 2, 3 bucket-sort passes"""
    if case["pseudo_cap"] is None:
        check_case(T, ctx, case)
        return
    monkeypatch.setenv("KSLAM_PSEUDO_CAP", str(case["pseudo_cap"]))
    c = kslam.Context()
    try:
        grp, gpr = check_case(T, c, case)
        got3, rp3, pr3 = _device(c, case, case["stages"] & 3)
        same = grp.tobytes() == rp3.tobytes() and gpr.tobytes() == pr3.tobytes()
        assert same == (not case["on_device"]), case["name"]      # handed back: "returns false, having changed nothing"
    finally:
        c.close()
