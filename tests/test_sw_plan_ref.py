"""CPU checks of tests/sw_plan_ref.py, the numpy restatement of the Smith-Waterman tier routing (sw.hip), and of
the mathematics of its band certificate: the closed form against an explicit search, soundness against the plain DP,
the DP against the oracle, and hand-built planner cases with known diagonal sums."""
import numpy as np
import pytest

import oracle as O
import sw_plan_ref as R

SCORINGS = [(2, 3, 5, 2), (1, 3, 5, 2), (1, 4, 6, 1), (3, 2, 4, 1), (2, 6, 5, 2), (5, 4, 6, 3), (10, 8, 6, 3)]
LENGTHS = list(range(1, 65)) + [150, 160, 161, 250, 256, 257, 400, 481, 511]


@pytest.mark.parametrize("sc", SCORINGS, ids=lambda s: "%d_%d_%d_%d" % s)
def test_closed_form_certificate_equals_the_search(sc):
    """certificate_amin's "g = 0, 1 or the largest feasible g" equals the minimum of A(g) over every feasible g, for
    every L and W of LENGTHS and every score 1 .. min(L, W) match; the SmallDiv form equals the exact one everywhere."""
    ma, gE = sc[0], sc[3]
    branches = set()
    lens = np.array(LENGTHS, dtype=np.int64)
    for Lm in LENGTHS:
        score = np.arange(1, Lm * ma + 1, dtype=np.int64)
        want = R.amin_by_search(score, Lm, sc)
        # every (L, W) of the grid whose shorter side is Lm
        pairs = [(Lm, w) for w in lens[lens >= Lm]] + [(l, Lm) for l in lens[lens > Lm]]
        L = np.array([p[0] for p in pairs])[:, None]
        W = np.array([p[1] for p in pairs])[:, None]
        exact = R.certificate_amin(score[None, :], L, W, sc)
        fast = R.certificate_amin_fast(score[None, :], L, W, sc)
        bad = np.argwhere(exact != want[None, :])
        assert not len(bad), ("closed form", sc, Lm, pairs[bad[0][0]], int(score[bad[0][1]]),
                              int(exact[tuple(bad[0])]), int(want[bad[0][1]]))
        bad = np.argwhere(fast != exact)
        assert not len(bad), ("fast form", sc, pairs[bad[0][0]], int(score[bad[0][1]]), int(fast[tuple(bad[0])]),
                              int(exact[tuple(bad[0])]))
        branches.add(gE < ma)
    assert branches == {gE < ma}
    if sc == (10, 8, 6, 3):   # scores >= 4096 take the real division
        assert 511 * ma >= 4096


def _ssw(read, win, sc):
    res, _ = O.ssw_align(read.astype(np.int8), win.astype(np.int8), O.build_matrix(sc[0], sc[1]), sc[2], sc[3])
    return res


def _small_pairs(rng):
    """Pairs (read, window) with L, W <= 64: random, tandem repeats of period 1..12, N runs, W < L, read hanging off
    the window's start (an optimum on a negative diagonal)."""
    pairs = []
    for _ in range(60):
        L = int(rng.integers(8, 65))
        W = int(rng.integers(8, 65))
        a = rng.integers(0, 4, W)
        r = a[:L].copy() if L <= W else np.concatenate([a, rng.integers(0, 4, L - W)])
        r[rng.random(len(r)) < 0.1] = rng.integers(0, 4)
        if rng.random() < 0.3:
            r = rng.integers(0, 4, L)
        pairs.append((r, a))
    for per in range(1, 13):
        for _ in range(4):
            unit = rng.integers(0, 4, per)
            flank = rng.integers(0, 4, int(rng.integers(4, 16)))
            W = int(rng.integers(24, 65))
            a = np.concatenate([flank, np.resize(unit, W)])[:W]
            L = int(rng.integers(16, 65))
            shift = int(rng.integers(0, 2 * per + 1))
            r = np.concatenate([flank, np.resize(unit, L + shift)[shift:]])[:L].copy()
            r[rng.random(L) < 0.05] = rng.integers(0, 4)
            pairs.append((r, a))
    for _ in range(30):
        W = int(rng.integers(16, 65))
        a = rng.integers(0, 4, W)
        r = a[:int(rng.integers(8, W + 1))].copy()
        s = int(rng.integers(0, len(r)))
        r[s:s + int(rng.integers(1, 8))] = 4                       # an N run in the read
        if rng.random() < 0.5:
            a = a.copy()
            s = int(rng.integers(0, W))
            a[s:s + int(rng.integers(1, 8))] = 4                   # ... and one in the window
        pairs.append((r, a))
    for _ in range(30):                                            # W < L: the window cut by the entry's end
        L = int(rng.integers(20, 65))
        a = rng.integers(0, 4, L)
        W = int(rng.integers(6, L))
        r = a.copy()
        r[rng.random(L) < 0.05] = rng.integers(0, 4)
        pairs.append((r, a[:W].copy()))
    for _ in range(30):                                            # rel < 0: the read starts before the window
        L = int(rng.integers(20, 65))
        off = int(rng.integers(1, L - 4))
        a = rng.integers(0, 4, L)
        r = np.concatenate([rng.integers(0, 4, off), a[:L - off]])
        r[rng.random(L) < 0.05] = rng.integers(0, 4)
        pairs.append((r, a, -off))
    for _ in range(30):                                            # a gap: both sides kept, indel of 1..16
        L = int(rng.integers(30, 65))
        delta = int(rng.integers(1, 17))
        cut = int(rng.integers(4, L - 4))
        a = rng.integers(0, 4, L + delta)
        if rng.random() < 0.5:
            r = np.concatenate([a[:cut], a[cut + delta:]])[:L]     # deletion from the read
            a = a[:L]
        else:
            r = np.concatenate([a[:cut], rng.integers(0, 4, delta), a[cut:]])[:L]   # insertion
            a = a[:L]
        pairs.append((r, a))
    return pairs


@pytest.mark.parametrize("sc", [SCORINGS[0], SCORINGS[3], SCORINGS[4], SCORINGS[6]], ids=lambda s: "%d_%d_%d_%d" % s)
def test_certified_band_holds_every_optimum(sc):
    """Wherever band_certifies(band score) holds, the banded DP has the full DP's optimum, the same set of cells
    holding it (the reference's end rule chooses among them) and the reference's chosen alignment starts in the band."""
    rng = np.random.default_rng(1000 + sum(sc))
    pairs = _small_pairs(rng)
    b = R.Batch.of_pairs(pairs)
    opt, Hf = R.full_dp(b, sc, keep=True)
    amin = R.certificate_amin(opt, b.L, b.W, sc)
    rows, dl, nds = [], [], []
    for c in range(b.n):
        if opt[c] <= 0:
            continue
        L, W = int(b.L[c]), int(b.W[c])
        for nd in (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 48):
            for dlo in range(-L - 1, W + 1):
                if R.band_holds(amin[c], L, W, dlo, nd):   # necessary: band score <= optimum
                    rows.append(c)
                    dl.append(dlo)
                    nds.append(nd)
    rows, dl, nds = np.array(rows), np.array(dl), np.array(nds)
    bb = b.sub(rows)
    score, Hb = R.banded_dp(bb, dl, nds, sc, keep=True)
    cert = R.band_certifies(score, bb.L, bb.W, dl, nds, sc)
    assert cert.sum() > 2000
    zero_slack = 0
    ends = {}
    for x in np.nonzero(cert)[0]:
        c = int(rows[x])
        assert score[x] == opt[c], ("band score", c, int(dl[x]), int(nds[x]), int(score[x]), int(opt[c]))
        L, W = int(b.L[c]), int(b.W[c])
        full_cells = {(int(i), int(j)) for i, j in np.argwhere(Hf[c, :L, :L + W - 1] == opt[c])
                      for j in [j - (L - 1) + i]}
        band_cells = {(int(i), int(t) + int(dl[x]) + int(i)) for i, t in np.argwhere(Hb[x, :L, :nds[x]] == opt[c])}
        assert band_cells == full_cells, ("optimal cells", c, int(dl[x]), int(nds[x]))
        if c not in ends:
            ends[c] = _ssw(pairs[c][0], pairs[c][1], sc)
        r = ends[c]
        assert r.score1 == opt[c]
        assert dl[x] <= r.ref_begin1 - r.read_begin1 <= dl[x] + nds[x] - 1, ("start outside the band", c)
        a = int(R.certificate_amin(score[x], L, W, sc))
        zero_slack += a != R.INT32_MAX and (a - L == dl[x] or W - a == dl[x] + nds[x] - 1)
    assert zero_slack > 100


@pytest.mark.parametrize("sc", SCORINGS, ids=lambda s: "%d_%d_%d_%d" % s)
def test_restated_dp_equals_the_oracle(sc):
    """A band covering every diagonal gives ssw_align's score and ends on the same (column, row) pair (highest score,
    then smallest end column, then smallest end row)."""
    rng = np.random.default_rng(7 + sc[0] * 10 + sc[3])
    pairs = _small_pairs(rng)[::3]
    for L in (150, 257):
        a = rng.integers(0, 4, L + 20)
        r = np.concatenate([a[:60], a[66:L + 6]])
        r[rng.random(L) < 0.04] = 4
        pairs.append((r, a[:L]))
    b = R.Batch.of_pairs(pairs)
    opt, H = R.full_dp(b, sc, keep=True)
    for c, p in enumerate(pairs):
        res = _ssw(p[0], p[1], sc)
        assert res.score1 == opt[c], (c, res.score1, opt[c])
        if opt[c] == 0:
            continue
        L = int(b.L[c])
        cells = [(int(i) + int(t) - (L - 1), int(i)) for i, t in np.argwhere(H[c] == opt[c])]
        assert min(cells) == (res.ref_end1, res.read_end1), (c, min(cells), res.ref_end1, res.read_end1)


def _entry_batch(reads, entry, rels, rcs):
    cand = np.zeros(len(reads), dtype=[("read", "<u4"), ("entry", "<u4"), ("rel", "<i4"), ("revcomp", "u1")])
    cand["read"] = np.arange(len(reads))
    cand["rel"] = rels
    cand["revcomp"] = rcs
    return R.Batch(cand, reads, [entry]), cand


def _bases(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()


def _rc(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def test_planner_hand_built_cases():
    """The planner's sums and shortcuts on reads with known diagonal sums."""
    rng = np.random.default_rng(5)
    sc = R.DEFAULT
    entry = _bases(rng, 2000)
    L = 150
    reads, rels, rcs, want = [], [], [], []

    def add(read, rel, rc, **w):
        reads.append(read)
        rels.append(rel)
        rcs.append(rc)
        want.append(w)

    for rc in (0, 1):
        seg = entry[300:300 + L]
        base = _rc(seg) if rc else seg
        add(base, 300, rc, full=L, full_x=0, best=2 * L, perfect=True, shortcut=True)
        n = bytearray(base)
        n[70] = ord("N")
        add(bytes(n), 300, rc, full=L - 1, full_x=0, best=2 * (L - 1), perfect=False, shortcut=False)
        for x, short in ((0, True), (1, True), (L - 2, True), (L - 1, True), (75, True)):
            m = bytearray(base)
            m[x] = b"ACGT"[(b"ACGT".index(bytes([m[x]])) + 1) % 4]
            add(bytes(m), 300, rc, full=L - 1, full_x=1, best=2 * (L - 1) - 3, perfect=False, one=True,
                shortcut=short, xrow=x)
    # a window cut to W < L by the entry's end
    add(entry[-100:] + _bases(rng, 50), len(entry) - 100, 0, full=100, best=200,
        perfect=False, shortcut=False)
    # rel < 0: the read hangs off the entry's start by 30 bases, seed diagonal -30
    add(_bases(rng, 30) + entry[:120], -30, 0, full=120, best=240, perfect=False,
        shortcut=False)
    # a tandem repeat of period 1 next to the seed: the other two counted diagonals match as well
    add(b"A" * L, 0, 0, perfect=False)
    b, cand = _entry_batch(reads, entry, rels, rcs)
    tiers = R.tier_set(L, sc)
    p = R.plan(b, sc, tiers)
    for c, w in enumerate(want):
        for k, v in w.items():
            assert p[k][c] == v, (c, k, p[k][c], v)
    # W < L and rel < 0 windows
    assert b.W[-3] == 100 and b.W[-2] == 150 and b.d0[-2] == -30
    # a shortcut is in no tier; the perfect read certifies the narrowest tier through its shortcut anyway
    assert (p["tier"][p["shortcut"]] == R.SHORTCUT).all()
    assert (p["tier"][~p["shortcut"]] < len(tiers.nd)).all()
    # the two extra diagonals of the one-mismatch form: d0 - 2, d0 - 1, or d0 + 1, d0 + 2 when flipped
    assert (p["far_m"][:14] < L // 2).all()


def test_one_mismatch_shortcut_needs_a_strict_winner():
    """A mismatch in the middle of an even read under scoring (1, 1, 5, 2): the two halves tie with each other, S1 is
    taken from the whole read only when it is strictly the largest of the three runs."""
    rng = np.random.default_rng(9)
    for L, x, sc, short in ((10, 5, (2, 30, 40, 2), False), (11, 5, (2, 30, 40, 2), False),
                            (40, 20, (2, 3, 5, 2), True), (9, 4, (1, 8, 9, 1), False)):
        seg = _bases(rng, L)
        m = bytearray(seg)
        m[x] = b"ACGT"[(b"ACGT".index(bytes([m[x]])) + 2) % 4]
        b, _ = _entry_batch([bytes(m)], seg, [0], [0])
        p = R.plan(b, sc, R.tier_set(L, sc))
        assert p["one"][0]
        assert p["shortcut"][0] == short, (L, x, sc)


def test_tier_sets():
    """lm, the tier list, the switches, T.unknown and the band_ok gate."""
    sc = R.DEFAULT
    assert R.tier_set(160, sc).nd == (16, 32, 48, 64, 96) and R.tier_set(160, sc).unknown == 2
    assert R.tier_set(161, sc).nd == (16, 32, 48, 64, 96, 128) and R.tier_set(161, sc).unknown == 3
    assert R.tier_set(511, sc).lm == 2 and R.tier_set(256, sc).lm == 1 and R.tier_set(257, sc).lm == 2
    assert R.tier_set(150, sc, no48=True).nd == (16, 32, 64, 96) and R.tier_set(150, sc, no48=True).unknown == 1
    assert R.tier_set(250, sc, no96=True).nd == (16, 32, 48, 64, 128)
    assert [R.tier_set(250, sc, unknown_nd=u).unknown for u in (16, 32, 64, 96, 128)] == [0, 1, 3, 4, 5]
    assert R.tier_set(150, sc, unknown_nd=128).unknown == 4
    assert R.tier_set(511, (10, 8, 6, 3)) is not None            # 16 x 511 = 8176 <= 8187
    assert R.short_cap((11, 8, 6, 3)) == 481 and R.tier_set(481, (11, 8, 6, 3)) is not None
    assert R.tier_set(100, (24, 8, 12, 4)) is None                # match + 2 gE = 32 > 31


def test_route_sends_failures_on():
    """route() on a deletion of 20 bases: planned by the seed's sums, sent on by a certificate that needs more than the
    gap, certified in a wider tier; no band score exceeds the certified one."""
    rng = np.random.default_rng(11)
    sc = R.DEFAULT
    entry = _bases(rng, 600)
    reads = [entry[100:170] + entry[190:270], entry[100:250]]
    cand = np.zeros(2, dtype=[("read", "<u4"), ("entry", "<u4"), ("rel", "<i4"), ("revcomp", "u1")])
    cand["read"] = [0, 1]
    cand["rel"] = [100, 100]
    tiers = R.tier_set(150, sc)
    r = R.route(cand, reads, [entry], sc, tiers)
    assert r.planned[1] == R.SHORTCUT and r.end[1] == R.SHORTCUT
    ran = r.ran[0]
    assert r.end[0] not in (R.SHORTCUT, R.NT_FULL)
    k = int(r.end[0])
    assert tiers.nd[k] // 2 >= 20
    assert ran[k] == 2 * (70 + 60) - 5 - 19 * 2     # the window ends 20 bases into the read's second part
    assert r.planned[0] <= k and (ran[:k][ran[:k] >= 0] <= ran[k]).all()
    assert r.round0[k] == 1 and sum(r.round0) == int((ran >= 0).sum())
