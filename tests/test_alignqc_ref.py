"""The plain-Python restatement of the alignment QC report (tests/alignqc_ref.py; include/kslam_alignqc.h): on the header's worked
example it gives the header's numbers and the header's JSON text -- both typed in here by hand from the header, not produced by
any code --, every case of the case builder holds the seam it is named for, and the tables' invariants hold on every case.  No
library, no GPU."""
import json

import numpy as np
import pytest

import alignqc_ref as R

CASES = R.cases()
BY_NAME = {c["name"]: c for c in CASES}

HEADER_EXAMPLE = b"""{
  "kslam_align_qc": 1,
  "paired": false,
  "max_cycles": 4,
  "summary": {
    "records": 2,
    "reverse": 1,
    "skipped": 0,
    "without_quality": 0,
    "m_columns": 9,
    "compared": 9,
    "mismatches": 4,
    "error_rate": "0.444444",
    "ins_events": 1,
    "ins_bases": 1,
    "del_events": 1,
    "del_bases": 1,
    "unaligned_bases": 0,
    "mean_identity": "0.454545",
    "read_pairs": 1,
    "pairs_both": 1,
    "pairs_r1_only": 0,
    "pairs_r2_only": 0,
    "insert_size_mean": "9.000000",
    "insert_size_median": "9"
  },
  "read1": {
    "records": 2,
    "reverse": 1,
    "skipped": 0,
    "without_quality": 0,
    "m_columns": 9,
    "compared": 9,
    "mismatches": 4,
    "error_rate": "0.444444",
    "ins_events": 1,
    "ins_bases": 1,
    "del_events": 1,
    "del_bases": 1,
    "unaligned_bases": 0,
    "mean_identity": "0.454545",
    "mismatch_rate_by_cycle": ["0.500000", "0.500000", "0.000000", "1.000000"],
    "mismatch_rate_tail": "0.500000",
    "compared_by_cycle": [2, 2, 2, 1],
    "mismatches_by_cycle": [1, 1, 0, 1],
    "inserted_bases_by_cycle": [0, 0, 0, 1],
    "deletions_by_cycle": [0, 1],
    "tail": [2, 1, 0, 0],
    "substitutions": {"A>C": 1, "A>G": 0, "A>T": 1, "C>A": 0, "C>G": 0, "C>T": 0, "G>A": 0, "G>C": 0, "G>T": 0, "T>A": 0, "T>C": 1, "T>G": 1, "matches": 5},
    "by_quality": {"2": [1, 0, "0.000000"], "20": [4, 3, "1.249387"], "40": [4, 1, "6.020600"]},
    "insertion_lengths": {"1": 1},
    "deletion_lengths": {"1": 1},
    "edit_distance_counts": {"2": 1, "4": 1},
    "identity_counts": {"20": 1, "66": 1}
  },
  "insert_size_counts": {"9": 1}
}
"""


def _s(case, C=512, z=0):
    return R.tables(case if isinstance(case, dict) else BY_NAME[case], C)["streams"][z]


def _row(s, C, c):
    return s["cycle"][4 * c:4 * c + 4]


def test_the_headers_example():
    t = R.tables(R.header_example(), 4)
    s, other = t["streams"]
    # the header's numbers, by hand
    assert [s[n] for n in R.SCALARS] == [2, 1, 0, 0, 9, 9, 4, 1, 1, 1, 1, 0]
    assert s["cycle"] == [2, 1, 0, 0, 2, 1, 0, 1, 2, 0, 0, 0, 1, 1, 1, 0, 2, 1, 0, 0]
    subst = {"AA": 1, "CC": 1, "GG": 2, "TT": 1, "AC": 1, "AT": 1, "TC": 1, "TG": 1}
    assert s["subst"] == [subst.get(r + q, 0) for r in "ACGT" for q in "ACGT"]
    assert {i: v for i, v in enumerate(s["nm"]) if v} == {2: 1, 4: 1} and {i: v for i, v in enumerate(s["identity"]) if v} == {20: 1, 66: 1}
    assert s["ins_len"][0] == 1 and s["del_len"][0] == 1 and sum(s["ins_len"]) == 1 and sum(s["del_len"]) == 1
    cq = np.array(s["cq_compared"]).reshape(5, 95)
    assert cq[:, 40].tolist() == [1, 1, 1, 0, 1] and cq[:, 20].tolist() == [1, 1, 1, 1, 0] and cq[:, 2].tolist() == [0, 0, 0, 0, 1] and cq.sum() == 9
    cm = np.array(s["cq_mismatch"]).reshape(5, 95)
    assert cm[:, 40].tolist() == [0, 0, 0, 0, 1] and cm[:, 20].tolist() == [1, 1, 0, 1, 0] and cm.sum() == 4
    assert [t[n] for n in R.PAIR_SCALARS] == [1, 1, 0, 0, 9] and t["insert"][9] == 1 and sum(t["insert"]) == 1
    assert not any(other[n] for n in R.SCALARS) and not t["paired"]
    # ... and the header's text
    assert R.text(t) == HEADER_EXAMPLE
    assert json.loads(HEADER_EXAMPLE)["read1"]["by_quality"]["20"] == [4, 3, "1.249387"]


def test_the_header_holds_the_example():
    """the text above IS the header's: every line of it stands in include/kslam_alignqc.h behind the comment's ' *   '"""
    import os
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kslam_alignqc.h")).read()
    for line in HEADER_EXAMPLE.decode().splitlines():
        assert " *   " + line + "\n" in h, line


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129])
def test_m_run_cases_hold_their_seam(n):
    s = _s("m-%d" % n)
    want = len({0, n - 1} | {x for x in (63, 64, 65, 127, 128) if x < n})
    assert s["n_records"] == 2 and s["n_reverse"] == 1 and s["m_columns"] == s["compared"] == 2 * n and s["mismatches"] == 2 * want
    assert _row(s, 512, 0)[:2] == [2, 2] and _row(s, 512, n - 1)[:2] == [2, 2] and _row(s, 512, n) == [0, 0, 0, 0]   # both strands meet both ends


def test_long_read_feeds_the_pooled_row():
    small, large = _s("long-300", 4), _s("long-300", 512)
    assert small["m_columns"] == large["m_columns"] == 2 * 297 and small["ins_bases"] == 6 and small["del_bases"] == 8
    assert _row(small, 4, 4)[0] == small["compared"] - sum(_row(small, 4, c)[0] for c in range(4)) > 580     # row C takes nearly all
    assert _row(large, 512, 512) == [0, 0, 0, 0] and _row(large, 512, 299)[0] == 2 and _row(large, 512, 300)[0] == 0
    assert sum(1 for v in large["cq_compared"] if v) > 280       # the quality bytes differ by cycle: a cell per cycle, three tiles of rows
    assert _row(large, 512, 130)[2] == 1 and _row(large, 512, 169)[2] == 1   # the insertion at query 130..132: cycle 130 forward, 299 - 130 reverse


def test_both_strands_of_one_read_text():
    s = _s("both-strands")
    assert s["n_records"] == 2 and s["n_reverse"] == 1 and s["mismatches"] == 4
    # forward: entry 22, 50 -> cycles 2, 30; reverse: entry 112, 170 -> query 2, 60 -> cycles 67, 9
    assert [c for c in range(70) if _row(s, 512, c)[1]] == [2, 9, 30, 67]
    cm = np.array(s["cq_mismatch"]).reshape(513, 95)
    assert [int(np.nonzero(cm[c])[0][0]) for c in (2, 9, 30, 67)] == [40 + c - 33 for c in (2, 9, 30, 67)]   # the quality byte of the cycle
    assert R.tables(BY_NAME["both-strands"], 512)["insert"][160] == 1


@pytest.mark.parametrize("name,col,fwd,rev", [("i-first", 2, (0, 1), (99, 98)), ("i-last", 2, (98, 99), (1, 0)), ("i-at-64", 2, (64, 65), (35, 34)),
                                              ("i-over-64", 2, (63, 64), (36, 35)), ("d-first", 3, (0,), (99,)), ("d-last", 3, (99,), (0,)),
                                              ("d-at-64", 3, (64,), (35,)), ("d-at-63", 3, (63,), (36,))])
def test_indel_cases_hold_their_cycles(name, col, fwd, rev):
    s = _s(name)
    got = {c: _row(s, 512, c)[col] for c in range(100) if _row(s, 512, c)[col]}
    want = {}
    for c in fwd + rev:
        want[c] = want.get(c, 0) + 1
    assert got == want and s["n_skipped"] == 0
    if col == 3:
        assert s["del_events"] == 2 and s["del_bases"] in (2, 4) and s["ins_events"] == 0
    else:
        assert s["ins_events"] == 2 and s["ins_bases"] == 4 and s["unaligned_bases"] == 0


@pytest.mark.parametrize("n", [1, 64, 65, 66])
def test_indel_length_bins(n):
    s = _s("indel-len-%d" % n)
    want = [0] * 65
    want[min(n, 65) - 1] = 1
    assert s["ins_len"] == want and s["del_len"] == want and s["ins_bases"] == n and s["del_bases"] == n
    assert {i for i, v in enumerate(s["nm"]) if v} == {min(n, 64)}


def test_nm_and_identity_edges():
    s = _s("nm-identity")
    assert {i: v for i, v in enumerate(s["nm"]) if v} == {0: 1, 30: 1, 63: 1, 64: 3}      # 64, 65 and 3 + 97 pool in the last entry
    ident = {i: v for i, v in enumerate(s["identity"]) if v}
    assert ident[100] == 1 and ident[0] == 2 and ident[37] == 1 and ident[36] == 1 and ident[35] == 1


@pytest.mark.parametrize("strand", ["fwd", "rev"])
def test_alphabet_is_counted_in_m_columns_alone(strand):
    s = _s("alphabet-" + strand)
    # entry N a N g under query C C N g, and query n a over upper case: six columns are not compared; one true mismatch
    assert s["m_columns"] == 60 and s["compared"] == 54 and s["mismatches"] == 1 and sum(s["subst"]) == 54


def test_quality_byte_edges():
    s = _s("quality-bytes")
    cq, cm = np.array(s["cq_compared"]).reshape(513, 95).sum(axis=0), np.array(s["cq_mismatch"]).reshape(513, 95).sum(axis=0)
    assert cq[0] == 4 and cq[93] == 4 and cq[94] == 16 and cq.sum() == 24      # 33 and 126 are the edges of the valid columns
    assert cm.sum() == 12 and cm[94] == 8


def test_a_batch_without_quality():
    case = BY_NAME["without-quality"]
    t = R.tables(case, 512)
    for z in range(2):
        s = t["streams"][z]
        assert s["n_records"] == 3 and s["n_without_quality"] == 1 and s["compared"] == 150 and sum(s["cq_compared"]) == 100
    assert t["paired"] and t["pairs_both"] == 3 and t["insert"][130] == 3 and t["streams"][1]["n_reverse"] == 3


@pytest.mark.parametrize("why", ["no-cigar", "entry-outside", "negative-begin", "m-past-entry", "m-past-read", "i-past-read", "d-past-entry"])
def test_each_skip_reason(why):
    s = _s("skip-" + why)
    assert s["n_records"] == 2 and s["n_skipped"] == 1 and s["m_columns"] == 40 and sum(s["nm"]) == 1


@pytest.mark.parametrize("strand", ["fwd", "rev"])
def test_one_byte_past_the_end_is_skipped(strand):
    case = BY_NAME["past-the-end-" + strand]
    b = case["batches"][0]
    s = _s(case)
    assert s["n_records"] == 5 and s["n_skipped"] == 3 and s["m_columns"] == 80 and s["mismatches"] == 0
    last = b["ov"][-1]
    assert int(last["read"]) == len(b["roff"]) - 2 and int(last["entry"]) == len(b["goff"]) - 2      # the last read, the last entry
    assert int(b["roff"][-1]) == len(b["rbases"]) and int(b["goff"][-1]) == len(b["gbases"])           # ... and nothing behind them


def test_contributing_set_and_pairs():
    t = R.tables(BY_NAME["contributing"], 512)
    a, b = t["streams"]
    assert a["n_records"] == 1 and b["n_records"] == 2 and b["mismatches"] == 3 and a["mismatches"] == 1       # `dead` is named by dead pairs alone
    assert [t[n] for n in R.PAIR_SCALARS] == [3, 1, 2, 1, 45] and sum(t["insert"]) == 1      # the group with count == 0 is no read pair
    t = R.tables(BY_NAME["insert-sizes"], 512)
    assert {i: v for i, v in enumerate(t["insert"]) if v} == {0: 1, 300: 2, 1000: 1, 1001: 3}
    assert t["pairs_both"] == 7 and t["pairs_r1_only"] == 1 and t["pairs_r2_only"] == 2 and t["insert_sum"] == 3603 + 2 ** 32 - 1
    assert b'"insert_size_median": "1000"' in R.text(t) and b'">1000": 3' in R.text(t)


def test_single_end_no_reads_and_the_empty_read():
    t = R.tables(BY_NAME["single-end"], 512)
    assert not t["paired"] and t["streams"][0]["n_records"] == 3 and not any(t["streams"][1][n] for n in R.SCALARS) and b'"read2"' not in R.text(t)
    t = R.tables(BY_NAME["no-reads"], 4)
    assert t == R.empty(4, True) and b'"read2"' in R.text(t) and b'"insert_size_median": "0"' in R.text(t)
    s = _s("empty-read")
    assert s["del_events"] == 1 and s["del_bases"] == 2 and sum(s["cycle"]) == 0 and s["nm"][2] == 1 and s["identity"][0] == 1


def test_the_random_case_fills_the_grid():
    t = R.tables(BY_NAME["random-20000"], 512)
    a, b = t["streams"]
    assert a["n_records"] > 5000 and b["n_records"] > 5000 and a["n_records"] + b["n_records"] > 19000     # more than one workgroup, both streams
    assert a["n_skipped"] + b["n_skipped"] and a["ins_events"] and a["del_events"] and a["n_reverse"] and t["insert"][1001] and t["pairs_r1_only"] and t["pairs_r2_only"]


@pytest.mark.parametrize("C", R.CYCLES)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_invariants(case, C):
    t = R.tables(case, C)
    all_quality = all(b["rqual"] is not None for b in case["batches"])
    for s in t["streams"]:
        cyc = np.array(s["cycle"]).reshape(C + 1, 4)
        assert sum(s["subst"]) == s["compared"] == cyc[:, 0].sum() and cyc[:, 1].sum() == s["mismatches"]
        assert s["compared"] <= s["m_columns"] and s["mismatches"] == s["compared"] - sum(s["subst"][5 * k] for k in range(4))
        if all_quality:
            assert sum(s["cq_compared"]) == s["compared"] and sum(s["cq_mismatch"]) == s["mismatches"]
        assert sum(s["nm"]) == s["n_records"] - s["n_skipped"] and sum(s["identity"]) <= sum(s["nm"])
        assert sum(s["ins_len"]) == s["ins_events"] and sum(s["del_len"]) == s["del_events"] and cyc[:, 2].sum() == s["ins_bases"]
        assert cyc[:, 3].sum() <= s["del_events"] and s["n_reverse"] <= s["n_records"]
    assert sum(t["insert"]) == t["pairs_both"]
    json.loads(R.text(t))
