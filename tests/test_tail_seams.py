"""The cases of tests/tail_seams.py on the CPU: at exactly these inputs the host tail (k-slam_amd/host/tail.cpp, the reference of
tests/test_gpu_tail_seams.py) equals the oracle's serial restatement byte for byte, every case sits on the seam it claims -- the
claimed count is recomputed from the input and from the host tail's output and must be equal, not beyond --, the plain
restatement of the insert-size statistics equals the host tail's, and the thresholds the cases are built around are the
ones csrc/pairs.hip has."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_seams as S  # noqa: E402

CASES = S.all_cases()


@pytest.fixture(scope="module")
def T(kslam):
    return importlib.import_module("kslam_amd.tail")


def host_tail(T, case, stages=None, pseudo=None):
    """the host tail on a case -> (read_pairs, pairs, stats); stages: the case's own unless given (0 = pairing only)"""
    stages = case["stages"] if stages is None else stages
    pseudo = bool(stages & 4) if pseudo is None else pseudo
    reads = T.Reads([b"A" * S.READ_LEN] * case["n_reads"])
    P = T.TailParams.default(paired=case["paired"], report_cigar=False, threads=4, score_threshold=case["score_threshold"],
                             score_fraction=case["score_fraction"], pseudo_assembly=pseudo, stages=stages if stages else T.STAGE_PAIRING_ONLY)
    return T.tail_pairs(P, reads, case["ov"]) + (P, reads)


def _chains(start, stop):
    """chains of one entry's spans (no equal starts among them: the order is the sort's whatever its tie rule) -> their number,
    and for every span that starts within one base of the chain rule's edge (start == reach - 20: joins, reach - 19: starts a
    chain): (its sorted index, whether it joins, the sorted index of the span whose stop is that reach)"""
    order = np.argsort(start, kind="stable")
    n, reach, setter, probes = 0, -1000000, -1, []
    for pos, i in enumerate(order):
        if start[i] in (reach - S.CHAIN_SLACK, reach - S.CHAIN_SLACK + 1):
            probes.append((pos, int(start[i] == reach - S.CHAIN_SLACK), setter))
        if start[i] > reach - S.CHAIN_SLACK:
            n, reach, setter = n + 1, stop[i], pos
        elif stop[i] > reach:
            reach, setter = stop[i], pos
    return n, probes


def measure(T, case, names):
    """the claimed counts, recomputed from the case's input and the host tail's output"""
    ov, n_reads, paired = case["ov"], case["n_reads"], case["paired"]
    mid = n_reads // 2
    units = mid if paired else n_reads
    unit = ov["read"].astype(np.int64) % mid if paired else ov["read"].astype(np.int64)
    per_unit = np.bincount(unit, minlength=units)
    big = int(per_unit.argmax()) if len(ov) else 0
    m = {"n_rows": len(ov), "n_units": units, "gap_cap": n_reads // 64 + 2}
    m["rows_largest_pair"] = m["rows_largest_read"] = int(per_unit.max()) if len(ov) else 0
    m["rows_smallest_pair"] = int(per_unit.min())
    m["n_big_pairs"] = int((per_unit > S.PAIR_BIG).sum()) if paired else 0
    m["rows_mate1"], m["rows_mate2"] = int((ov["read"] < mid).sum()), int((ov["read"] >= mid).sum())
    m["rows_mate1_largest"], m["rows_mate2_largest"] = int((ov["read"] == big).sum()), int((ov["read"] == big + mid).sum())
    m["heads_largest_pair"] = len(np.unique(ov["entry"][unit == big]))
    edges = np.concatenate([[-1], ov["read"].astype(np.int64), [n_reads]])     # k_row_starts: prev and cur of every i in 0 .. n
    m["longest_empty_stretch"] = int(np.diff(edges).max() - 1)
    m["long_stretches"] = int((np.diff(edges) > S.GAP).sum())
    rp0, pr0, st0 = host_tail(T, case, 0)[:3]                                   # after pairing
    m["kept_rows"] = int(st0.n_overlaps_screened)
    m["pairs_largest_group"] = int(rp0["count"].max()) if len(rp0) else 0
    m["n_inserts"] = int((pr0["insert_size"] != 0).sum())
    g0 = rp0[int(rp0["count"].argmax())] if len(rp0) else None
    mine0 = pr0[int(g0["first"]):int(g0["first"] + g0["count"])] if g0 is not None else pr0[:0]
    m["distinct_scores_largest_group"] = len(np.unique(mine0["combined_score"]))
    grp_of = np.repeat(rp0["r1_read"], rp0["count"].astype(np.int64)) if len(rp0) else np.zeros(0, np.uint32)
    m["inserts_in_units_0_255"] = int(((pr0["insert_size"] != 0) & (grp_of < 256)).sum())
    ins = pr0["insert_size"][pr0["insert_size"] != 0].view(np.int32)
    m["inserts_above_46340"] = int((ins > 46340).sum())
    if paired:
        st1 = host_tail(T, case, 1)[2]
        limit = int(st1.max_insert_size)
        assert st1.n_insert_sizes == len(ins) and S.insert_limit_ref(ins) == limit, case["name"]
        m["max_insert_size"] = limit
        m["cut_largest_group"] = int((mine0["insert_size"] <= limit).sum())
        m["records_at_limit"] = int((pr0["insert_size"] == limit).sum())
        m["records_at_limit_plus_1"] = int((pr0["insert_size"] == limit + 1).sum())
        if len(ins):
            sz = np.sort(ins)
            m["lower_quartile"], m["upper_quartile"] = int(sz[int(len(sz) * 0.25)]), int(sz[int(len(sz) * 0.75)])
            if len(sz) == 100:
                step = np.nonzero(np.diff(sz))[0]
                m["ladder_position"] = int(step[0]) if len(step) else -1
                m["ladder_step"] = int(sz[-1] - sz[0])
    rp3, pr3, _ = host_tail(T, case, case["stages"] & 3, False)[:3]             # after the screens, before pseudo-assembly
    if len(pr3):
        per_entry = np.sort(np.bincount(pr3["entry"]))[::-1]
        m["spans_largest_entry"], m["spans_second_entry"] = int(per_entry[0]), int(per_entry[1]) if len(per_entry) > 1 else 0
        m["largest_entry"] = int(pr3["entry"].max())
        m["distinct_starts_entry6"] = len(np.unique(pr3["ref_start"][pr3["entry"] == 6]))
        if "chains_largest_entry" in names:
            e = pr3["entry"] == np.bincount(pr3["entry"]).argmax()
            m["chains_largest_entry"], probes = _chains(pr3["ref_start"][e], pr3["ref_end"][e])
            assert len(probes) == 1, case["name"]                 # one deciding span
            m["probe_index"], m["probe_joins"], m["reach_setter_index"] = probes[0]
            m["steps_between_setter_and_probe"] = probes[0][0] // 64 - probes[0][2] // 64
            s = np.sort(pr3["ref_start"][e])
            assert len(np.unique(s)) == len(s)
    m["pairs_before_second_screen"] = len(pr3)
    rp, pr, st = host_tail(T, case, case["stages"] if case["on_device"] else case["stages"] & 3)[:3]
    m["n_groups_out"], m["pairs_out"] = len(rp), len(pr)
    if len(rp):
        m["first_group_out"], m["last_group_out"] = int(rp["r1_read"][0]), int(rp["r1_read"][-1])
        m["top_score_out"] = int(pr["combined_score"].max())
        m["zero_scores_out"] = int((pr["combined_score"] == 0).sum())
        where = np.nonzero(rp["r1_read"] == big)[0]
        m["pairs_out_largest_group"] = int(rp["count"][where[0]]) if len(where) else 0
    return m


def check_case(kslam, oracle, T, case):
    assert case["ov"].dtype == kslam.OVERLAP_DT
    ov = case["ov"]
    assert (np.lexsort((ov["rel"], ov["entry"], ov["read"])) == np.arange(len(ov))).all()      # as alignToDatabase leaves them
    rp, pr, st, P, reads = host_tail(T, case)
    orp, opr = oracle.tail_pairs(P, reads.view, ov)
    assert rp.tobytes() == orp.tobytes() and pr.tobytes() == opr.tobytes(), case["name"]
    m = measure(T, case, case["claim"])
    got = {k: m.get(k) for k in case["claim"]}
    assert got == case["claim"], case["name"]
    if "long_stretches" in case["claim"]:
        assert m["long_stretches"] < m["gap_cap"]


@pytest.mark.parametrize("letter", sorted(CASES))
def test_every_case_sits_on_its_seam_and_host_tail_equals_the_restatement(kslam, oracle, T, letter):
    names = [c["name"] for c in CASES[letter]]
    assert len(set(names)) == len(names)
    for case in CASES[letter]:
        check_case(kslam, oracle, T, case)


def test_pseudo_cap_cases_leave_the_host_the_same_records_either_way(kslam, T):
    """the hand-back case is compared with the stages = 3 result on the device: here, that the pseudo-assembly would have
    changed something (else "changed nothing" could not be told from "did it")"""
    for case in CASES["E"]:
        if case["pseudo_cap"] is None:
            continue
        _, pr7, _ = host_tail(T, case, 7)[:3]
        _, pr3, _ = host_tail(T, case, case["stages"] & 3)[:3]
        assert pr7.tobytes() != pr3.tobytes(), case["name"]


def test_insert_limit_restatement_on_the_large_array_is_finite_and_past_2p53():
    v = S.stats_beyond_2p53().astype(np.int64)
    assert (v * v < 2 ** 31).all() and int((v * v).sum()) > 2 ** 53 and len(v) < 5_000_000
    r = S.insert_limit_ref(v)
    assert 46001 < r < 50000


def test_thresholds_are_the_ones_in_the_device_source():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "k-slam_amd", "csrc", "pairs.hip")) as fh:
        src = fh.read()

    def const(name):
        m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*([^;]+);" % name, src)
        assert m, name
        text = m.group(1).strip()
        sh = re.fullmatch(r"1u?\s*<<\s*(\d+)", text)
        return 1 << int(sh.group(1)) if sh else int(text.rstrip("u"))

    assert const("PAIR_BIG") == S.PAIR_BIG and const("SCREEN_BIG") == S.SCREEN_BIG
    assert const("PSEUDO_CAP") == S.PSEUDO_CAP and const("PSEUDO_CAP_GLOBAL") == S.PSEUDO_CAP_GLOBAL
    assert re.findall(r"cur - prev > (\d+)", src) == [str(S.GAP)]
    assert re.findall(r"\.start > before - (\d+)", src) == [str(S.CHAIN_SLACK)]
    assert re.findall(r"v\[i \+ 1\] - v\[i\] > (\d+)", src) == [str(S.LADDER_STEP)]
    assert "gap_cap = (uint32_t)(n_reads / 64 + 2)" in src
