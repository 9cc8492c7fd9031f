"""The consensus caller's plain-Python restatement (tests/consensus_ref.py) against hand-written expectations on tiny entries, and
the host twin (kslam_tail_consensus, include/kslam_consensus.h) against the restatement on the case list the device is held to,
under every parameter set, and on seeded random cases.  No GPU."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consensus_ref as R  # noqa: E402

CASES = R.cases()


@pytest.fixture(scope="module")
def CN(kslam):
    return importlib.import_module("kslam_amd.consensus")


def twin(CN, c, params=R.DEFAULTS):
    return CN.tail_consensus(c["gbases"], c["goff"], c["ov"], c["pool"], c["rbases"], c["roff"], c["rp"], c["pr"], *params)


def check(CN, c, params=R.DEFAULTS):
    rows, seqs, stats = R.consensus(c, *params)
    got, seq, got_stats = twin(CN, c, params)
    assert got_stats == stats, (c["name"], params)
    assert R.fields(got) == R.fields(rows), (c["name"], params)
    assert R.split(got, seq) == seqs and len(seq) == sum(len(s) for s in seqs), (c["name"], params)
    return rows, seqs, stats


def test_the_restatement_by_hand():
    #                 0123456789
    b = R.CB("x", [b"ACGTACGTAC", b"GGNgG", b"TTTT"])
    for _ in range(3):      # G -> C at 2; position 5 deleted; TT inserted behind 6
        b.single(b.rec(b.read(b"ACCTAGTTTA"), 0, 0, b.cigar([(5, "M"), (1, "D"), (1, "M"), (2, "I"), (2, "M")])))
    b.single(b.rec(b.read(R.reverse_complement(b"CGTACGT")), 0, 1, b.cigar([(7, "M")]), 1))      # one plain read on the other strand
    b.single(b.rec(b.read(b"GGAAN"), 1, 0, b.cigar([(5, "M")])))                                 # N and g filled in with A; N over G: no vote
    b.single(b.rec(b.read(b"CC"), 2, 0, b.cigar([(2, "I")])))                                    # unanchored, and nothing else: not touched
    rows, seqs, stats = R.consensus(b.done())
    #   0 A, 1 C, 2 C (3 of 4), 3 T, 4 A, 5 deleted (3 of 4), 6 G + TT (3 of 4), 7 T, 8 A, 9 uncovered
    assert seqs == [b"ACCTAGTTTAN", b"GGAAN"]
    assert R.fields(rows) == [(0, 0, 11, 10, 9, 1, 1, 1, 2, 0), (1, 11, 5, 5, 5, 2, 0, 0, 0, 1)]
    assert stats == {"n_records": 6, "n_skipped": 0, "n_intervals": 11, "n_del_intervals": 3, "n_events": 6, "n_insertions": 3, "n_ins_unanchored": 1,
                     "n_ins_unrepresentable": 0, "n_entries_touched": 2, "n_entries_reported": 2}
    # a stricter call: 3 of 4 does not pass 750; REF fill; the second entry falls below min_covered
    rows, seqs, stats = R.consensus(b.done(), 1, 750, R.FILL_REF, 6)
    assert seqs == [b"ACNTANGTAC"] and R.fields(rows) == [(0, 0, 10, 10, 9, 0, 0, 0, 0, 2)]
    # depth 4 is needed: only 1 .. 7 have it (position 5 by one M column and three deletions)
    rows, seqs, stats = R.consensus(b.done(), 4, 500, R.FILL_N, 1)
    assert seqs == [b"NCCTAGTTTNN"] and R.fields(rows)[0][4:] == (7, 1, 1, 1, 2, 0) and stats["n_entries_reported"] == 1
    text = R.fasta_bytes(rows, seqs, [b"one", b"two", b"three"])
    assert text == b">one kslam_consensus entry_length=10 covered=7 substitutions=1 deletions=1 insertions=1 ambiguous=0\nNCCTAGTTTNN\n"


def test_two_pairs_at_one_anchor_by_hand():
    b = R.CB("x", [b"ACGTACGTAC"])
    for _ in range(2):
        b.single(b.gapped(0, 0, [(4, "M"), (2, "I"), (2, "I"), (4, "M")], 0, ins=[b"GA", b"CT"]))
    rows, seqs, stats = R.consensus(b.done())
    assert seqs == [b"ACGT" + b"CT" + b"ACGT" + b"NN"] and stats["n_insertions"] == 4 and R.fields(rows)[0][7:9] == (1, 2)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_twin_matches_the_restatement(CN, case):
    for params in R.PARAMS:
        check(CN, case, params)


def test_what_the_cases_are_there_for(CN):
    by = {c["name"]: c for c in CASES}
    for n, stored in ((1, 3), (32, 3), (33, 0)):
        for s in ("fwd", "rev"):
            rows, seqs, stats = check(CN, by["walk-ins-%d-%s" % (n, s)])
            assert stats["n_insertions"] == stored and stats["n_ins_unrepresentable"] == 3 - stored
            assert R.fields(rows)[0][7:9] == ((1, n) if stored else (0, 0)) and len(seqs[0]) == 300 + (n if stored else 0)
    for tag in ("N", "lower"):
        _, seqs, stats = check(CN, by["walk-ins-" + tag])
        assert stats["n_ins_unrepresentable"] == 4 and stats["n_insertions"] == 1 and len(seqs[0]) == 300   # 1 of 5 does not pass
    assert check(CN, by["walk-ins-first"])[2]["n_ins_unanchored"] == 4
    rows, seqs, _ = check(CN, by["walk-ins-after-del"])
    assert R.fields(rows)[0][6:9] == (2, 1, 3) and len(seqs[0]) == 301
    rows, seqs, stats = check(CN, by["walk-two-ins"])
    assert stats["n_insertions"] == 18 and R.fields(rows)[0][7:9] == (3, 6) and b"CT" + by["walk-two-ins"]["gbases"][130:134].tobytes() in seqs[0]
    rows, seqs, _ = check(CN, by["walk-del-to-end"])
    assert R.fields(rows)[0][6] == 5 and len(seqs[0]) == 295
    _, _, stats = check(CN, by["walk-zero-ops"])
    assert stats["n_intervals"] == 9 and stats["n_del_intervals"] == 0 and stats["n_insertions"] == 3 and stats["n_events"] == 6
    rows, seqs, _ = check(CN, by["alphabet"])
    assert seqs[0][10:16] == b"CNANNT" and seqs[0][30:32] == b"NN"
    rows, seqs, stats = check(CN, by["entries"])
    assert [r[0] for r in R.fields(rows)] == [1, 2, 4, 5, 7] and stats["n_entries_touched"] == 5
    assert seqs[1].endswith(b"GC") and len(seqs[1]) == 52 and len(seqs[2]) == 40 and len(seqs[4]) == 33 and seqs[4][31:] == b"NN"   # a tie of bases and deletion
    assert [r[0] for r in R.fields(check(CN, by["entries"], (2, 500, R.FILL_N, 1))[0])] == [1, 2, 4, 7]   # entry 5: touched, not reported
    c = by["call"]
    ref = c["gbases"].tobytes()
    at500 = check(CN, c)[1][0]
    at750 = check(CN, c, (1, 750, R.FILL_N, 1))[1][0]
    assert at500[60] == ord("N") and at500[70] != ref[70] and at500[70] != ord("N") and at750[70] == ord("N") and at750[80] == at500[80] != ref[80]
    assert len(at500) == 300 - 5 + 2 and at500[150:160] == ref[153:163]
    rows = check(CN, c)[0]
    assert R.fields(rows)[0][6:9] == (5, 1, 2)     # 150 .. 152 and 208 .. 209 deleted; AG behind 209; nothing behind 229
    rows, seqs, stats = check(CN, by["call-5000"])
    assert stats["n_insertions"] == 2600 and R.fields(rows)[0][5:9] == (1, 0, 1, 4)
    assert check(CN, by["grid-skip-in-wave"])[2]["n_skipped"] == 1
    assert check(CN, by["random-0"])[2] == dict.fromkeys(R.STAT_NAMES, 0)
    fill_n, fill_ref = check(CN, by["call"])[1][0], check(CN, by["call"], (1, 500, R.FILL_REF, 1))[1][0]
    assert fill_n[:50] == b"N" * 50 and fill_ref[:50] == ref[:50]
    assert len(check(CN, by["entries"], (1, 500, R.FILL_N, 21))[0]) == 1 and len(check(CN, by["entries"], (1, 500, R.FILL_N, 20))[0]) == 3   # covered: 1, 10, 20, 30, 20


def test_40_random_cases(CN):
    for seed in range(40):
        c = R.random_case("random-%d" % seed, 1000 + seed, 1 + 5 * seed, 1 + seed % 9, 1 + (37 * seed) % 300)
        check(CN, c, R.PARAMS[seed % len(R.PARAMS)])


def test_the_planted_differences_on_the_checker_s_alignments(oracle):
    """The choice of tests/test_gpu_consensus.py's planted case, checked without a GPU: the checker's aligner places the 3-base
    deletion and the 2-base insertion where they were planted (the bases around them leave no other placement), and the restatement
    over its alignments, every one a read pair of its own, gives the mutated copy back over the span with full coverage."""
    entry, copy, n_subs, reads = R.planted()
    rng = np.random.default_rng(98)
    ents = [entry, R.random_bases(rng, 3000), R.random_bases(rng, 3000)]
    al, cig, _ = oracle.align_to_database(list(reads), ents)
    ov = np.zeros(len(al), dtype=R.OVERLAP_DT)
    for f in R.OVERLAP_DT.names:
        if f in al.dtype.names:
            ov[f] = al[f]
    goff = np.concatenate([[0], np.cumsum([len(e) for e in ents])]).astype(np.uint64)
    roff = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    case = R.arrays("planted", b"".join(ents), goff, b"".join(reads), roff, cig, ov, [(int(a["read"]), 0, i, 1) for i, a in enumerate(al)],
                    [(int(a["entry"]), i, R.NO_OVERLAP) for i, a in enumerate(al)])
    rows, seqs, stats = R.consensus(case, 3, 500, R.FILL_N, 1)
    assert stats["n_skipped"] == 0 and stats["n_del_intervals"] > 20 and stats["n_insertions"] > 20 and [r["entry"] for r in rows] == [0]
    assert (rows[0]["deleted"], rows[0]["insertions"], rows[0]["inserted_bases"], rows[0]["substitutions"], rows[0]["ambiguous"]) == (3, 1, 2, n_subs, 0)
    assert len(seqs[0]) == len(copy) and seqs[0][200:-200] == copy[200:-200]
