"""The restatement of the CIGAR stage's driver (tests/cigar_plan_ref.py) against the oracle, and the preconditions of the
family batches (tests/cigar_seams.py): the seams tests/test_gpu_cigar_seams.py is built for are really reached.  CPU only.
"""
import json
import os

import numpy as np
import pytest

import cigar_plan_ref as P
import cigar_seams as S


@pytest.mark.parametrize("name", list(S.CASES))
def test_restatement_agrees_with_the_oracle(oracle, name):
    """Per row: the CIGAR the restatement's banded_sw call leaves equals the oracle's own (so do the op counts), bw0 is
    what the oracle's spans imply, an inline row carries exactly <n>M, and every row the oracle aligned is taken."""
    c = S.case(name, oracle)
    assert len(c.cand) == len(c.rows) and len(c.rows) >= 1
    got_reads = set(int(r) for r in c.rows["read"])
    assert got_reads == set(range(len(c.reads))), ("reads without a candidate",
                                                   [c.fam[r] for r in set(range(len(c.reads))) - got_reads][:8])
    for k, x in enumerate(c.cand):
        row = c.rows[k]
        ecig = c.cig[int(row["cigar_off"]):int(row["cigar_off"]) + int(row["cigar_len"])]
        assert x.want == (int(row["cigar_len"]) > 0), (k, c.fam[x.read])
        if not x.want:
            continue
        assert x.status == 0, ("trace back error", k, c.fam[x.read])
        mine = x.cigar[::-1] if x.rc else x.cigar            # SmithWaterman.h:212-216
        assert x.ops == len(ecig) and np.array_equal(mine, ecig), (k, c.fam[x.read], x.ops, len(ecig))
        rl = int(row["ref_end"]) - int(row["ref_begin"]) + 1
        ql = int(row["query_end"]) - int(row["query_begin"]) + 1
        assert (x.ref_len, x.read_len) == (rl, ql)
        if x.inline:
            assert len(ecig) == 1 and int(ecig[0]) == ql << 4 and rl == ql, (k, c.fam[x.read])
        else:
            assert x.bw0 == abs(rl - ql) + 1 and x.band >= x.bw0
            # M and I consume the read span (the window span may lose a deletion next to row 0: the walk ends at i == 0)
            read_used = sum(int(o) >> 4 for o in ecig if (int(o) & 15) in (0, 1))
            assert read_used == ql, (k, c.fam[x.read])


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorded():
    """the counts one run on an MI355X printed, per case and tuning (parse_debug's shape)"""
    z = json.load(open(os.path.join(GOLD, "cigar_seams_counts.json")))
    for v in z.values():
        v["classes"] = {int(k): n for k, n in v["classes"].items()}
        v["big"] = [tuple(b) for b in v["big"]]
    return z


def _fam(c, x):
    return c.fam[x.read]


def _all(oracle):
    return [S.case(n, oracle) for n in S.CASES]


def _banded(c):
    return [x for x in c.cand if x.want and not x.inline]


def test_bw0_edges_each_sign_each_strand(oracle):
    """Every bin edge h and h + 1 is asked for as the initial band by at least 4 candidates of each sign (I: the read span
    is the longer one, D: the window span) on each strand.  bw0 = 1 has no sign (refLen == readLen and not inline: an
    insertion and a deletion of one size); it is asked for by at least 4 candidates per strand."""
    n = {}
    for c in _all(oracle):
        for x in _banded(c):
            sign = "I" if x.read_len > x.ref_len else "D" if x.ref_len > x.read_len else "="
            n[(x.bw0, sign, x.rc)] = n.get((x.bw0, sign, x.rc), 0) + 1
    missing = []
    for h in S.EDGES:
        for bw0 in (h, h + 1):
            for rc in (False, True):
                for sign in ("=",) if bw0 == 1 else ("I", "D"):
                    if n.get((bw0, sign, rc), 0) < 4:
                        missing.append((bw0, sign, rc, n.get((bw0, sign, rc), 0)))
    assert not missing, missing
    for bw0 in (256, 257):                                   # class 8 asked for directly
        assert sum(v for (b, s, r), v in n.items() if b == bw0) >= 2, bw0


def test_doubling_reaches_every_bin_and_class(oracle):
    """Every bin 1..6 and class 6, 7 and 8 receives at least 4 candidates by doubling; the doubled widths that are not
    powers of two occur; at least 10 chains have three or more attempts."""
    arrivals, classes, seen, long_chains = [0] * 7, {}, set(), 0
    for c in _all(oracle):
        for x in _banded(c):
            ws = P.widths(x)
            long_chains += len(ws) >= 3
            for w in ws[1:]:
                seen.add(w)
                if w < 64:
                    arrivals[P.cig_bin(w)] += 1
                else:
                    classes[P.band_class(w)] = classes.get(P.band_class(w), 0) + 1
    assert all(arrivals[b] >= 4 for b in range(1, 7)), arrivals
    assert all(classes.get(k, 0) >= 4 for k in (6, 7, 8)), classes
    assert {6, 12, 24, 48, 96, 10, 20, 40, 80} <= seen, sorted(seen)
    assert long_chains >= 10, long_chains


def test_hand_over_rule_at_equality(oracle):
    """refLen - (2 bw + 1) in {-1, 0, 1, 2} occurs at least 4 times each for an attempt on a systolic kernel (default
    tuning) and for an attempt on a register kernel (KSLAM_CIGAR_SYS=0: bands up to 15, family R's 32-base windows), at
    least 10 handed-over members have a row where the sentinel write lands on a live cell, and both kinds of kernel
    hand candidates over."""
    slack = {"sys": {}, "reg": {}}
    handed = {"sys": 0, "reg": 0}
    sentinel = 0
    for c in _all(oracle):
        if c.long_chunk:
            continue
        for tn, key in (("default", "sys"), ("registers", "reg")):
            p = S.plan_of(c, tn)
            for x in _banded(c):
                for a in p.attempts[x.row]:
                    on_sys = a.impl.startswith("k_cigar_systolic")
                    on_reg = a.impl.startswith("k_banded_lds<") and not a.impl.endswith("<0>")
                    if a.cls is None and (on_sys if key == "sys" else on_reg):
                        slack[key][a.slack] = slack[key].get(a.slack, 0) + 1
                        handed[key] += a.handed
                        assert a.handed == (a.slack <= 0), (c.name, p.describe(x))
                        sentinel += bool(a.handed and P.sentinel_rows(x, a.bw))
    for key in ("sys", "reg"):
        assert all(slack[key].get(d, 0) >= 4 for d in (-1, 0, 1, 2)), (key, [(d, slack[key].get(d, 0)) for d in (-1, 0, 1, 2)])
        assert handed[key] >= 10, (key, handed)
    assert sentinel >= 10, sentinel


def _first_gap(x):
    """(row, column) of the first cell behind the first indel of a CIGAR in un-flipped alignment order"""
    i = j = 0
    for o in x.cigar:
        n, op = int(o) >> 4, int(o) & 15
        if op != 0:
            return i, j
        i += n
        j += n
    return None


def test_word_seams_every_residue(oracle):
    """Family W, per band: the aligned read span's length, the row of the indel and the systolic turn of that cell
    ((i + j - k0 - (q & 1)) >> 1, k0 = -1 for an odd band) take all six residues of the six-cells-per-word packing."""
    res = {}
    for c in _all(oracle):
        for x in _banded(c):
            f = _fam(c, x)
            if not f.startswith("W "):
                continue
            bw = int(f.split("band=")[1].split()[0])
            if x.band != bw:
                continue
            i, j = _first_gap(x)
            k0 = -1 if bw & 1 else 0
            q = (j - i + bw) & 1
            r = res.setdefault(bw, (set(), set(), set()))
            r[0].add(x.read_len % 6)
            r[1].add(i % 6)
            r[2].add(((i + j - k0 - q) >> 1) % 6)
    for bw in (1, 2, 4, 7, 15):
        assert bw in res and all(len(s) == 6 for s in res[bw]), (bw, res.get(bw))


def test_staging_every_residue(oracle):
    """Family S: the first byte of both staged spans takes all sixteen residues mod 16 on both strands, and shift + len
    lands on a multiple of 16 and one either side."""
    c = S.case("L150_staging", oracle)
    for rc in (False, True):
        xs = [x for x in _banded(c) if x.rc == rc]
        assert {x.shift_q for x in xs} == set(range(16)), rc
        assert {x.shift_r for x in xs} == set(range(16)), rc
        assert {(x.shift_q + x.read_len) % 16 for x in xs} >= {15, 0, 1}, rc
        assert {(x.shift_r + x.ref_len) % 16 for x in xs} >= {15, 0, 1}, rc
    assert {len(r) for r in c.reads} == {150, 151}


def test_cap_overflow_both_endings(oracle):
    """Op counts 23, 24, 25 and 26 -- both sides of the 24-op temp slot -- occur with both endings of the traceback (on a
    match; on an indel, `1M <n>I ...`), and so do 21, 27 and 29 ending on a match; tracebacks of a systolic launch
    overflow too.  (A local alignment starts and ends on a match, so an even count needs an insertion that touches a
    deletion: family C's blocks of four mismatches under (10, 8, 6, 3).)"""
    seen = {}
    sys_ovf = 0
    for c in _all(oracle):
        p = S.plan_of(c, "default")
        for x in _banded(c):
            seen[(x.ops, x.ends_on_indel)] = seen.get((x.ops, x.ends_on_indel), 0) + 1
            if P.overflows(x) and p.attempts[x.row][-1].impl.startswith("k_cigar_systolic"):
                sys_ovf += 1
    for ops in (21, 23, 24, 25, 26, 27, 29):
        assert seen.get((ops, False), 0) >= 2, (ops, "ends on a match", seen.get((ops, False)))
    for ops in (23, 24, 25, 26):
        assert seen.get((ops, True), 0) >= 2, (ops, "ends on an indel", seen.get((ops, True)))
    assert sys_ovf >= 4, sys_ovf


def test_inline_rule_at_its_edge(oracle):
    """sw_epilogue's `dsum == score` with equal spans: at equality with mismatches inside the span (inline <n>M although
    the read is not perfect) and one point below (a gap pair beats the diagonal by one) at least 10 times each."""
    eq = below = 0
    for c in _all(oracle):
        for x in c.cand:
            if x.want and x.dsum is not None:
                eq += x.inline and x.dsum < c.sc[0] * x.read_len
                below += x.dsum == x.score - 1
    assert eq >= 10 and below >= 10, (eq, below)


def test_list_seams(oracle):
    """Family N: the band-2 list holds exactly the member count; one case has a single gapped candidate."""
    for n in (63, 64, 65, 127, 128, 129):
        p = S.plan_of(S.case("list%d" % n, oracle), "default")
        assert p.bins0 == [0, n, 0, 0, 0, 0, 0, 0], (n, p.bins0)
    p = S.plan_of(S.case("one_gapped", oracle), "default")
    assert sum(p.bins0) == 1


def test_long_chunk_runs_only_the_lds_kernel(oracle):
    c = S.case("long512", oracle)
    assert c.long_chunk
    for tn in P.TUNINGS:
        p = S.plan_of(c, tn)
        assert p.handed == 0 and len(p.attempts) >= 40
        assert all(a.impl == "k_banded_lds<0>" and not a.handed for at in p.attempts.values() for a in at)


def test_perturbed_restatements_differ_on_named_members(oracle):
    """The restatement has teeth: a hand-over rule of `<` in place of `<=` changes the handed-over count through family H's
    slack-0 members alone, and a temp slot of 23 ops changes the big rerun through family C's 24-op members, with both
    endings of the traceback."""
    c = S.case("sc10", oracle)
    a, b = S.plan_of(c, "default"), S.plan_of(c, "default", hand_le=False)
    assert a.handed != b.handed
    diff = [x for x in _banded(c) if [t.handed for t in a.attempts[x.row]] != [t.handed for t in b.attempts[x.row]]]
    assert diff and all(any(t.slack == 0 for t in a.attempts[x.row]) for x in diff)
    assert any(" d=0 " in _fam(c, x) and _fam(c, x).startswith("H ") for x in diff), [_fam(c, x) for x in diff][:5]
    got = dict(bins=[a.bins0], handed=a.handed, classes=a.classes, arrivals=a.arrivals, big=[a.big] if a.big else [])
    assert P.explain(a, got, True) == []
    told = P.explain(b, got, True)
    assert len(told) == 1 and told[0].startswith("handed over") and "refLen - (2 bw + 1) = -1)" in told[0], told
    c = S.case("sc10_even", oracle)
    a, b = S.plan_of(c, "default"), S.plan_of(c, "default", cap=23)
    assert a.big != b.big
    diff = [x for x in _banded(c) if (x.row in a.big_rows) != (x.row in b.big_rows)]
    assert diff and all(x.ops == 24 and _fam(c, x).startswith("C block") for x in diff)
    assert {x.ends_on_indel for x in diff} == {False, True}


@pytest.mark.parametrize("name", list(S.CASES))
def test_restatement_equals_the_recorded_counts(oracle, name):
    """The counts the library printed for this case on an MI355X (tests/golden/cigar_seams_counts.json, recorded with
    the families as they are here) are the restatement's under all four tunings -- on a machine without a GPU this
    keeps the families and the restatement from drifting -- and the two perturbed restatements are told apart from
    them by the count they touch, with the members behind it."""
    rec = _recorded()
    c = S.case(name, oracle)
    room0 = c.env.get("KSLAM_SWEEP_ROOM") == "0"
    for tn in P.TUNINGS:
        got = rec["%s/%s" % (name, tn)]
        assert P.explain(S.plan_of(c, tn), got, room0) == [], (name, tn)
        lt = S.plan_of(c, tn, hand_le=False)
        if lt.handed != S.plan_of(c, tn).handed:
            told = P.explain(lt, got, room0)
            assert len(told) == 1 and told[0].startswith("handed over") and "refLen - (2 bw + 1) = -1)" in told[0], told
        short = S.plan_of(c, tn, cap=23)
        if short.big != S.plan_of(c, tn).big:
            told = P.explain(short, got, room0)
            assert len(told) == 1 and told[0].startswith("big rerun") and "ops 24" in told[0], told


def test_the_perturbations_are_seen_somewhere(oracle):
    n_lt = n_cap = 0
    for name in S.CASES:
        c = S.case(name, oracle)
        for tn in P.TUNINGS:
            n_lt += S.plan_of(c, tn, hand_le=False).handed != S.plan_of(c, tn).handed
            n_cap += S.plan_of(c, tn, cap=23).big != S.plan_of(c, tn).big
    assert n_lt >= 6 and n_cap >= 4, (n_lt, n_cap)
