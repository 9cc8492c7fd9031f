"""The plain-Python restatement of the indel table (tests/indels_ref.py) held to properties that share no code with it: a row's
allele gives the haplotype its raw events gave, no row can be shifted one step further, every placement of one haplotype change
-- from forward and from reverse-complemented records -- meets in one key, and the writer's bytes for a hand-written table.
No GPU, no library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import indels_ref as R  # noqa: E402

CASES = [c for c in R.cases() if c["name"] != "limits"]   # (the 70 000-base entry adds nothing here)


def _haplotype(ref, kind, p, n, s):
    """the raw event applied where the read put it"""
    return ref[:p] + ref[p + n:] if kind == R.DEL else ref[:p] + s + ref[p:]


def _can_step(ref, anchor, kind, n, s):
    """one more step to the left, tested on the haplotypes and the alphabet alone"""
    p = anchor + 1
    if p < 2 or ref[p - 1:p] not in (b"A", b"C", b"G", b"T"):
        return False
    if kind == R.DEL:
        return _haplotype(ref, kind, p - 1, n, s) == _haplotype(ref, kind, p, n, s)
    return _haplotype(ref, kind, p - 1, n, s[-1:] + s[:-1]) == _haplotype(ref, kind, p, n, s)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_rows_keep_the_haplotype_and_are_leftmost(case):
    rows, stats = R.table(case)
    assert stats["n_sites"] == len(rows) and (stats["n_deletions"] + stats["n_insertions"] > 0 or case["name"] == "x")
    keys = {r[:5] for r in rows}
    assert len(keys) == len(rows) and rows == sorted(rows)
    seen = 0
    for o in case["ov"]:
        got = R.raw_events(case, o)
        if got is None:
            continue
        e = int(o["entry"])
        ref = R.entry_bytes(case, e)
        for kind, p, n, s in got[1]:
            anchor, kind2, n2, s2 = R.normalised(ref, kind, p, n, s)
            assert (kind2, n2, len(s2)) == (kind, n, len(s)) and 0 <= anchor < p
            assert R.apply_allele(ref, anchor, kind, n, s2) == _haplotype(ref, kind, p, n, s)      # (a)
            assert not _can_step(ref, anchor, kind, n, s2)                                         # (b)
            seen += 1
    assert seen > 0
    for e, pos, kind, n, s, fwd, rev, dp in rows:
        assert fwd + rev >= 1 and (kind == R.DEL) == (s == b"") and all(b in R.ACGT for b in s)


def test_every_placement_of_one_change_gives_one_key():
    """(c) random small entries of ACGT alone, a random indel, every position p >= 1 at which an indel of that length gives the same
    haplotype: one key.  Then the same through records of both strands."""
    rng = np.random.default_rng(2027)
    checked = 0
    for trial in range(300):
        ref = bytes(rng.choice(np.frombuffer(b"AC" if trial % 2 else b"ACGT", dtype=np.uint8), int(rng.integers(8, 30))).tobytes())
        n = int(rng.integers(1, 5))
        kind = int(rng.integers(0, 2))
        p = int(rng.integers(1, len(ref) - n))
        s = bytes(rng.choice(np.frombuffer(b"AC", dtype=np.uint8), n).tobytes()) if kind == R.INS else b""
        hap = _haplotype(ref, kind, p, n, s)
        same = []
        for q in range(1, len(ref) - n if kind == R.DEL else len(ref) + 1):
            t = hap[q:q + n] if kind == R.INS else b""
            if _haplotype(ref, kind, q, n, t) == hap:
                same.append((q, t))
        assert (p, s) in same
        keys = {R.normalised(ref, kind, q, n, t) for q, t in same}
        assert len(keys) == 1, (ref, kind, p, n, s, same)
        if len(same) < 2:
            continue
        checked += 1
        b = R.Builder("x", [ref])
        for k, (q, t) in enumerate(same):
            if q < len(ref):
                R.al(b, 0, 0, R.split_at(len(ref), q, "D" if kind == R.DEL else "I", n), rc=k & 1, fill=t or b"A")
        rows, stats = R.table(b.done())
        assert len(rows) == 1 and rows[0][:5] == (0,) + next(iter(keys))
        assert rows[0][5] + rows[0][6] == len(b.ov) and (len(b.ov) < 2 or (rows[0][5] > 0 and rows[0][6] > 0))
    assert checked > 100


def test_named_cases_give_what_they_are_there_for():
    by = {c["name"]: c for c in R.cases() if c["name"] != "limits"}
    a = len(R.LEFT) - 1
    rows, stats = R.table(by["homopolymer"])
    assert [r[:5] for r in rows] == [(0, a, R.DEL, 1, b""), (0, a, R.INS, 1, b"A")] and rows[0][5] + rows[0][6] == 8 and rows[1][5] + rows[1][6] == 9
    rows, _ = R.table(by["tandem-2"])
    assert [r[:5] for r in rows] == [(0, a, R.DEL, 2, b""), (0, a, R.INS, 2, b"CA")] and rows[0][5] + rows[0][6] == 11
    rows, _ = R.table(by["tandem-3"])
    assert [r[:5] for r in rows] == [(0, a, R.DEL, 3, b""), (0, a, R.DEL, 6, b""), (0, a, R.INS, 3, b"CAG"), (0, a, R.INS, 6, b"CAGCAG")]
    rows, _ = R.table(by["entry-start"])           # p == 1 is not stepped from: the entry's first base is the anchor
    assert [r[:5] for r in rows] == [(0, 0, R.DEL, 1, b""), (0, 0, R.INS, 1, b"A")]
    rows, _ = R.table(by["entry-start-tandem"])    # every phase ends at p == 1: the inserted bases are rotated to that phase
    assert [r[:5] for r in rows] == [(0, 0, R.DEL, 2, b""), (0, 0, R.INS, 2, b"AC")]
    rows, _ = R.table(by["after-same-base"])       # the entry before ends in the same base: not stepped into
    assert [r[:5] for r in rows] == [(1, 0, R.DEL, 1, b""), (1, 0, R.INS, 1, b"A")]
    rows, stats = R.table(by["depth"])
    assert [r[:5] for r in rows[:6]] == [(0, 49, R.DEL, 2, b""), (0, 49, R.INS, 1, b"A"), (0, 49, R.INS, 2, b"AT"), (0, 49, R.INS, 2, b"TA"),
                                         (0, 49, R.INS, 3, b"ATA"), (0, 100, R.DEL, 1, b"")]
    assert rows[2][5:] == (1, 2, rows[0][7]) and rows[5][5:] == (3, 0, 2)      # AO 3 over DP 2: the two plain reads over position 100
    rows, stats = R.table(by["long-shift"])
    far = [r for r in rows if r[1] == a]
    assert [r[:5] for r in far] == [(0, a, R.DEL, 1, b""), (0, a, R.INS, 1, b"A")] and [r[5:7] for r in far] == [(1, 0), (0, 1)]
    rows, stats = R.table(by["alphabet"])
    assert stats["n_unrepresentable"] == 4 and (0, len(R.LEFT) + 4, R.DEL, 1, b"") in [r[:5] for r in rows]
    rows, stats = R.table(by["strands"])
    assert [(r[2], r[5], r[6]) for r in rows] == [(R.DEL, 2, 3), (R.INS, 2, 3)]
    rows, stats = R.table(by["skipped"])
    assert stats["n_skipped"] == 8 and stats["n_records"] == 10 and len(rows) == 2


def test_limits():
    c = [c for c in R.cases() if c["name"] == "limits"][0]
    rows, stats = R.table(c)
    assert stats["n_long_del"] == 1 and stats["n_unrepresentable"] == 2 and stats["n_unanchored"] == 3
    assert sorted({r[3] for r in rows if r[2] == R.INS}) == [1, 2, 32] and max(r[3] for r in rows if r[2] == R.DEL) == 65536
    same_anchor = [r[:5] for r in rows if r[0] == 0 and r[1] == 54]
    assert same_anchor == [(0, 54, R.DEL, 3, b""), (0, 54, R.INS, 2, b"GT")]


def test_writer_bytes_for_a_hand_written_table():
    entries = [b"GATTTACA", b"CCNaG"]
    rows = [(0, 1, R.DEL, 3, b"", 2, 1, 4), (0, 1, R.INS, 2, b"GC", 0, 5, 2), (1, 2, R.DEL, 1, b"", 1, 0, 0)]
    text = R.vcf_bytes(rows, entries, [b"one", b"two"], b"v9")
    assert text == (b"##fileformat=VCFv4.2\n##source=v9\n##contig=<ID=one,length=8>\n##contig=<ID=two,length=5>\n" + b"".join(R.INFO_LINES) + R.COLUMNS +
                    b"one\t2\t.\tATTT\tA\t.\t.\tDP=4;AO=3;SAF=2;SAR=1;AF=0.750000;TYPE=del;LEN=3\n"
                    b"one\t2\t.\tA\tAGC\t.\t.\tDP=2;AO=5;SAF=0;SAR=5;AF=2.500000;TYPE=ins;LEN=2\n"
                    b"two\t3\t.\tNa\tN\t.\t.\tDP=0;AO=1;SAF=1;SAR=0;AF=0.000000;TYPE=del;LEN=1\n")
