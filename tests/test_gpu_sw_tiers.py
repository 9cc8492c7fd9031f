"""Smith-Waterman tier routing (k-slam_amd/csrc/sw.hip) candidate by candidate, at every tier's edge.

Each batch comes from closed-form families that sweep a parameter across the band edges of every tier (h = ND / 2):
  A  indels of h - 1, h and h + 1 bases, the shorter side's length crossing the tie match m = gO + (delta - 1) gE;
  B  tandem repeats of period h - 1, h, h + 1 between unique flanks (a copy-number change of one unit);
  C  near-perfect reads whose planner sum sits exactly at, and one point below, the score that certifies each tier;
  D  reads hanging off an entry's start or end, and entries shorter than a read;
  G  a deletion of 1-2 bases with mismatches and Ns that put the gapped band score at zero slack or one diagonal
     short of each tier (the tier a gapped candidate starts in is the only one whose certificate can fail).
For every batch:
  1. parity: rows and CIGARs equal the oracle and the same context under KSLAM_SW_FULL=1;
  2. exact routing: the counts KSLAM_DEBUG=1 prints on a fresh context's first chunk (planned, round 0 per tier,
     full matrix) equal the restatement tests/sw_plan_ref.py, and the two runs after it (the sized sweep from the
     context's history) keep the planned / full-matrix counts and every row;
and across the file, preconditions on the restatement make sure the families reach every edge they are built for.
"""
import re

import numpy as np
import pytest

import sw_plan_ref as R
from align_compare import compare_alignments

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _rc(s):
    return s[::-1].translate(COMP)


def _hs(L, sc, tiers=None):
    t = tiers or R.tier_set(min(L, 511), sc) or R.tier_set(min(L, 511), R.DEFAULT)   # (the widths of the class)
    return sorted({nd // 2 for nd in t.nd})


class Builder:
    """Reads and one database; every read gets fresh random sequence of its own (no cross hits)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.reads, self.entries = [], [b""]
        self.fam = []

    def bases(self, n):
        return ACGT[self.rng.integers(0, 4, n)].tobytes()

    def piece(self, n):
        """n fresh bases appended to the shared entry (entry 0), separated by junk"""
        s = self.bases(n)
        self.entries[0] += self.bases(64) + s
        return s

    def add(self, read, fam, rc=None):
        if rc is None:
            rc = self.rng.random() < 0.5
        self.reads.append(_rc(read) if rc else read)
        self.fam.append(fam)

    def sub(self, s, rate):
        a = bytearray(s)
        for i in np.nonzero(self.rng.random(len(a)) < rate)[0]:
            a[i] = ACGT[(list(ACGT).index(a[i]) + int(self.rng.integers(1, 4))) % 4]
        return bytes(a)


def fam_indels(B, L, sc, hs):
    """A: an insertion or deletion of delta in {h - 1, h, h + 1} with the shorter side m around the tie
    m match = gO + (delta - 1) gE; and one with >= 47 bases on both sides (both seeds are candidates)."""
    ma, gO, gE = sc[0], sc[2], sc[3]
    for h in hs:
        for delta in (h - 1, h, h + 1):
            if delta < 1:
                continue
            cost = gO + (delta - 1) * gE
            t = cost // ma
            ms = sorted({m for m in (t - 1, t, t + 1, (cost + ma - 1) // ma + 1) if 1 <= m <= L - delta - 47})
            ms.append((L - delta) // 2) if (L - delta) // 2 >= 47 else None
            for m in ms:
                for kind in ("del", "ins"):
                    for short_first in (True, False):
                        g = B.piece(L + delta + 2)
                        if kind == "del":
                            if short_first:
                                r = g[:m] + g[m + delta:L + delta]
                            else:
                                r = g[:L - m] + g[L - m + delta:L + delta]
                        else:
                            ins = B.bases(delta)
                            if short_first:
                                r = g[:m] + ins + g[m:L - delta]
                            else:
                                r = g[:L - m - delta] + ins + g[L - m - delta:L - delta]
                        B.add(r, "A")


def fam_repeats(B, L, sc, hs):
    """B: a tandem repeat of period P in {h - 1, h, h + 1} between unique flanks of >= 47 bases; the read holds one
    unit more or less than the entry, lightly mutated."""
    for h in hs:
        for P in (h - 1, h, h + 1):
            if P < 1 or L - 94 < P:
                continue
            for dn in (-1, 1):
                for _ in range(1):
                    unit = B.bases(P)
                    nr = max(1, (L - 94) // P)
                    a = int(B.rng.integers(47, L - nr * P - 47 + 1))
                    b = L - nr * P - a
                    fa, fb = B.bases(a + 20), B.bases(b + 20)
                    ng = nr - dn if nr - dn >= 0 else nr + 1
                    g = fa + unit * ng + fb
                    B.entries[0] += B.bases(64) + g
                    r = fa[20:] + unit * nr + fb[:b]
                    B.add(B.sub(r, 0.01), "B")


def fam_mismatch_ladder(B, L, sc, tiers):
    """C: reads equal to their window but for k mismatches and n Ns, (k, n) chosen so that the planner's best
    ma (L - k - n) - mx k certifies each tier with zero slack, or misses it by one point of amin."""
    ma, mx = sc[0], sc[1]
    targets = {}
    for nd in tiers.nd:
        h = nd // 2
        for want in (L - h + 1, L - h):                    # W - amin == dhi (zero slack), == dhi + 1
            targets[want] = nd
    found = {}
    for k in range(0, L // 6):
        for n in range(0, L // 6):
            best = ma * (L - k - n) - mx * k
            if best <= 0:
                continue
            a = int(R.certificate_amin(best, L, L, sc))
            if a in targets and len(found.setdefault(a, [])) < 3:
                found[a].append((k, n))
    for a, kns in found.items():
        for k, n in kns:
            for rc in (False, True):
                g = B.piece(L)
                r = bytearray(g)
                pos = np.linspace(9, L - 10, k + n + 2)[1:-1].astype(int) if k + n else []
                order = B.rng.permutation(len(pos))
                for x, p in enumerate(np.asarray(pos)[order]):
                    if x < k:
                        r[p] = ACGT[(list(ACGT).index(r[p]) + 1) % 4]
                    else:
                        r[p] = ord("N")
                B.add(bytes(r), "C", rc)


def fam_gapped_ladder(B, L, sc, tiers):
    """C': a deletion of 1 or 2 bases in the middle (>= 47 bases either side: two candidates, each seed diagonal
    certifies nothing) with k mismatches and n Ns chosen so that the gapped band score puts amin at L - h + 1 or
    L - h: certified with zero slack, or failed by exactly one diagonal, in whichever tier it runs."""
    ma, mx, gO, gE = sc
    targets = set()
    for nd in tiers.nd:
        targets |= {L - nd // 2 + 1, L - nd // 2}
    for delta in (1, 2):
        found = {}
        for k in range(0, L // 8):
            for n in range(0, L // 8):
                best = ma * (L - delta - k - n) - mx * k - gO - (delta - 1) * gE
                if best <= 0:
                    continue
                a = int(R.certificate_amin(best, L, L, sc))
                if a in targets and len(found.setdefault(a, [])) < 4:
                    found[a].append((k, n))
        for a, kns in found.items():
            for k, n in kns + kns:
                g = B.piece(L + delta)
                cut = L // 2 + int(B.rng.integers(-10, 11))
                r = bytearray(g[:cut] + g[cut + delta:])
                pos = [p for p in np.linspace(9, L - 10, k + n + 4)[1:-1].astype(int) if abs(p - cut) > 4][:k + n]
                for x, p in enumerate(B.rng.permutation(pos)):
                    r[p] = ACGT[(list(ACGT).index(r[p]) + 1) % 4] if x < k else ord("N")
                B.add(bytes(r), "G")


def fam_geometry(B, L, sc, hs):
    """D: reads hanging off an entry's start (rel from -1 to -(L - 47)) or end (W from L - 1 down to 47), at steps
    landing on h and h +- 1 for each tier; entries shorter than a read."""
    offs = {1, 2, L - 47}
    for h in hs:
        offs |= {h - 1, h, h + 1, 2 * h - 1, 2 * h, 2 * h + 1}
    offs = sorted(o for o in offs if 1 <= o <= L - 47)
    for o in offs:
        for rc in (False, True):
            e = B.bases(L + 200)
            B.entries.append(e)
            B.add(B.sub(B.bases(o) + e[:L - o], 0.01), "D", rc)            # off the start
            e = B.bases(L + 200)
            B.entries.append(e)
            B.add(B.sub(e[-(L - o):] + B.bases(o), 0.01), "D", rc)         # off the end: W = L - o
    for n in (47, 60, L // 2, L - 1):
        e = B.bases(n)
        B.entries.append(e)
        pre = int(B.rng.integers(0, L - n + 1))
        B.add(B.bases(pre) + e + B.bases(L - n - pre), "D")


def build_case(seed, L, sc, fams, tiers=None, extra_short=0):
    B = Builder(seed)
    tiers = tiers or R.tier_set(min(L, 511), sc) or R.tier_set(min(L, 511), R.DEFAULT)
    hs = _hs(L, sc, tiers)
    if "A" in fams:
        fam_indels(B, L, sc, hs)
    if "B" in fams:
        fam_repeats(B, L, sc, hs)
    if "C" in fams:
        fam_mismatch_ladder(B, L, sc, tiers)
    if "D" in fams:
        fam_geometry(B, L, sc, hs)
    if "G" in fams:
        fam_gapped_ladder(B, L, sc, tiers)
    for _ in range(extra_short):                          # 150-base reads mixed into a longer chunk
        g = B.piece(150)
        B.add(B.sub(g, 0.02), "E")
    B.entries[0] += B.bases(64)
    return B


# name -> (seed, read length, scoring, families, environment)
CASES = {
    "A150": (1, 150, (2, 3, 5, 2), "AG", {}),
    "A250": (2, 250, (2, 3, 5, 2), "AG", {}),
    "B150": (3, 150, (2, 3, 5, 2), "B", {}),
    "B250": (4, 250, (2, 3, 5, 2), "B", {}),
    "C150": (5, 150, (2, 3, 5, 2), "C", {}),
    "C250": (6, 250, (2, 3, 5, 2), "C", {}),
    "D150": (7, 150, (2, 3, 5, 2), "D", {}),
    "D250": (8, 250, (2, 3, 5, 2), "D", {}),
    "seam160": (9, 160, (2, 3, 5, 2), "ACD", {}),
    "seam161": (10, 161, (2, 3, 5, 2), "ACD", {}),
    "seam256": (11, 256, (2, 3, 5, 2), "AC", {}),
    "seam257": (12, 257, (2, 3, 5, 2), "AC", {}),
    "seam511": (13, 511, (2, 3, 5, 2), "AC", {}),
    "mix150in511": (14, 511, (2, 3, 5, 2), "C", {"extra_short": 60}),
    "sc10_8_6_3_L511": (15, 511, (10, 8, 6, 3), "AC", {}),
    "sc11_8_6_3_L481": (16, 481, (11, 8, 6, 3), "AC", {}),
    "sc11_8_6_3_L482": (17, 482, (11, 8, 6, 3), "C", {}),
    "sc1_3_5_2": (18, 150, (1, 3, 5, 2), "ABCD", {}),
    "sc1_4_6_1": (19, 250, (1, 4, 6, 1), "ABCD", {}),
    "sc3_2_4_1": (20, 150, (3, 2, 4, 1), "ABCD", {}),
    "sc2_6_5_2": (21, 250, (2, 6, 5, 2), "ABCD", {}),
    "sc5_4_6_3": (22, 150, (5, 4, 6, 3), "ABCD", {}),
    "sc10_8_6_3": (23, 250, (10, 8, 6, 3), "ABCD", {}),
    "no48": (24, 150, (2, 3, 5, 2), "ABCDG", {"KSLAM_SW_NO48": "1"}),
    "no96": (25, 250, (2, 3, 5, 2), "ABCD", {"KSLAM_SW_NO96": "1"}),
    "unknown16": (26, 150, (2, 3, 5, 2), "ABDG", {"KSLAM_SW_UNKNOWN_ND": "16"}),
    "unknown32": (27, 150, (2, 3, 5, 2), "ABDG", {"KSLAM_SW_UNKNOWN_ND": "32"}),
    "unknown64": (28, 250, (2, 3, 5, 2), "ABDG", {"KSLAM_SW_UNKNOWN_ND": "64"}),
    "unknown96": (29, 250, (2, 3, 5, 2), "ABDG", {"KSLAM_SW_UNKNOWN_ND": "96"}),
    "unknown128": (30, 250, (2, 3, 5, 2), "ABDG", {"KSLAM_SW_UNKNOWN_ND": "128"}),
}


def tiers_of(env, max_short, sc):
    if max_short == 0:
        return None
    return R.tier_set(max_short, sc, no48="KSLAM_SW_NO48" in env, no96="KSLAM_SW_NO96" in env,
                      unknown_nd=int(env.get("KSLAM_SW_UNKNOWN_ND", "0")))


_cache = {}


def case(name, oracle):
    """(builder, scoring, env, candidates from the oracle's join, tiers or None, the restatement's route)"""
    if name not in _cache:
        seed, L, sc, fams, env = CASES[name]
        env = dict(env)
        extra = int(env.pop("extra_short", 0))
        B = build_case(seed, L, sc, fams, extra_short=extra,
                       tiers=tiers_of(env, min(L, R.short_cap(sc)), sc) if L <= R.short_cap(sc) else None)
        recs = np.concatenate([oracle.extract_kmers(B.reads, False, 1), oracle.extract_kmers(B.entries, True, 16)])
        cand, _ = oracle.find_overlaps(oracle.sort_kmers(recs), [len(r) for r in B.reads])
        cap = R.short_cap(sc)
        lens = np.array([len(r) for r in B.reads])
        assert (lens <= cap).all() or (lens > cap).all(), "one class of reads per batch: one chunk"
        max_short = int(lens[lens <= cap].max()) if (lens <= cap).any() else 0
        tiers = tiers_of(env, max_short, sc)
        _cache[name] = (B, sc, env, cand, tiers, R.route(cand, B.reads, B.entries, sc, tiers))
    return _cache[name]


def _parse(err):
    planned = [list(map(int, m.split(" / "))) for m in re.findall(r"\[kslam\] SW planned: ([\d / ]+)\n", err)]
    rounds = [(int(a), int(b), int(c), d) for a, b, c, d in
              re.findall(r"\[kslam\] SW round (\d+) tier (\d+) \((\d+) diagonals\): \d+ candidates(.*)\n", err)]
    r0 = {}
    for m in re.finditer(r"\[kslam\] SW round 0 tier (\d+) \((\d+) diagonals\): (\d+) candidates(.*)\n", err):
        r0[int(m.group(1))] = (int(m.group(2)), int(m.group(3)), m.group(4))
    full = [int(x) for x in re.findall(r"\[kslam\] SW full matrix: (\d+) candidates\n", err)]
    chunks = [(int(a), int(b)) for a, b in re.findall(r"\[kslam\] SW: (\d+) candidates, (\d+) needed", err)]
    later = [r for r in rounds if r[0] > 0]
    return planned, r0, full, chunks, later


@pytest.mark.parametrize("name", list(CASES))
def test_sw_tiers_route_and_parity(kslam, oracle, monkeypatch, capfd, name):
    B, sc, env, cand, tiers, rt = case(name, oracle)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("KSLAM_DEBUG", "1")
    c = kslam.Context(match=sc[0], mismatch=sc[1], gap_open=sc[2], gap_extend=sc[3])
    try:
        c.reload_tuning()
        c.set_index(B.entries)
        c.load_reads(B.reads)
        got_t, _ = c.find_overlaps()
        for f in ("read", "entry", "rel", "revcomp"):
            assert (got_t[f] == cand[f]).all(), f
        capfd.readouterr()
        got, gcig = c.align_batch(B.reads)
        err = capfd.readouterr().err
        planned, r0, full, chunks, later = _parse(err)
        n = len(cand)
        assert chunks == [(n, rt.n_full)], ("chunks", chunks, n, rt.n_full)
        if tiers is None:
            assert planned == [] and r0 == {} and full == [] and rt.n_full == n
        else:
            assert planned == [rt.planned_counts], ("planned", planned, rt.planned_counts)
            want = {k: (nd, rt.round0[k]) for k, nd in enumerate(tiers.nd) if rt.round0[k]}
            assert {k: v[:2] for k, v in r0.items()} == want, ("round 0", r0, want)
            assert later == [], later
            assert full == [rt.n_full], ("full matrix", full, rt.n_full)
        for _ in range(2):                                   # the sized sweep from the context's history
            again, acig = c.align_batch(B.reads)
            err = capfd.readouterr().err
            planned2, _, full2, chunks2, _ = _parse(err)
            assert chunks2 == [(n, rt.n_full)]
            if tiers is not None:
                assert planned2 == [rt.planned_counts] and full2 == [rt.n_full]
                assert "planned, sized for" in err
            compare_alignments(again, acig, got, gcig)
        monkeypatch.setenv("KSLAM_SW_FULL", "1")
        c.reload_tuning()
        fgot, fcig = c.align_batch(B.reads)
    finally:
        c.close()
    compare_alignments(got, gcig, fgot, fcig)
    p = oracle.Params.default(match=sc[0], mismatch=sc[1], gap_open=sc[2], gap_extend=sc[3])
    exp, ecig, _ = oracle.align_to_database(B.reads, B.entries, p)
    compare_alignments(got, gcig, exp, ecig)


def test_sw_tier_families_reach_every_edge(oracle):
    """Preconditions on the restatement, per band width over the whole file: candidates planned into it, failing its
    certificate, certified with zero slack, failing by exactly one diagonal, and whose band score needs its edge lanes;
    across the file: candidates that skip a tier, that end in the full matrix, and whose optimum sits on two
    diagonals."""
    per = {}
    skip = full = 0
    two_diag = 0
    for name in CASES:
        B, sc, env, cand, tiers, rt = case(name, oracle)
        full += rt.n_full
        if tiers is None:
            continue
        b = rt.batch
        for k, nd in enumerate(tiers.nd):
            s = per.setdefault(nd, dict(planned=0, failed=0, zero_slack=0, by_one=0, edge=0))
            s["planned"] += int((rt.planned == k).sum())
            idx = np.nonzero(rt.ran[:, k] >= 0)[0]
            if not len(idx):
                continue
            sc_k = rt.ran[idx, k]
            sb = b.sub(idx)
            dlo = sb.d0 - nd // 2
            dhi = dlo + nd - 1
            amin = R.certificate_amin(sc_k, sb.L, sb.W, sc)
            ok = rt.end[idx] == k
            s["failed"] += int((~ok).sum())
            fin = (amin >= 0) & (amin != R.INT32_MAX)
            s["zero_slack"] += int((ok & fin & ((amin - sb.L == dlo) | (sb.W - amin == dhi))).sum())
            over = np.maximum(dlo - (amin - sb.L), (sb.W - amin) - dhi)
            s["by_one"] += int((~ok & fin & (over == 1)).sum())
            lo = R.banded_dp(sb, dlo + 1, nd - 1, sc)
            hi = R.banded_dp(sb, dlo, nd - 1, sc)
            s["edge"] += int(((lo < sc_k) | (hi < sc_k)).sum())
        # skipping: sent on past at least one tier it never ran in
        ranmask = rt.ran >= 0
        for c in np.nonzero(ranmask.any(1))[0]:
            ks = np.nonzero(ranmask[c])[0]
            skip += int(len(ks) > 1 and (np.diff(ks) > 1).any())
        if name in ("B150", "A150", "sc1_3_5_2", "sc3_2_4_1"):
            fam = np.array(B.fam)[cand["read"]]
            sel = np.nonzero((fam == "A") | (fam == "B"))[0]
            _, nd_opt = R.optimum_diagonals(b.sub(sel), sc)
            two_diag += int((nd_opt >= 2).sum())
    for nd, s in sorted(per.items()):
        assert s["planned"] >= 20 and s["failed"] >= 20 and s["zero_slack"] >= 10 and s["by_one"] >= 10 \
            and s["edge"] >= 10, (nd, s)
    assert skip >= 10 and full >= 10 and two_diag >= 20, (skip, full, two_diag)
