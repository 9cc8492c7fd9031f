"""A plain numpy restatement of the Smith-Waterman tier routing of k-slam_amd/csrc/sw.hip.

sw_scores sends every candidate through k_sw_plan, which counts three diagonals next to the seed, short-cuts the
perfect and one-mismatch candidates and plans the narrowest band tier its lower bound certifies; k_sw_band then sweeps
[dlo, dlo + ND - 1] and keeps its score only when band_certifies holds, and sends the others on to the tier
certificate_amin / band_holds name, or to the full-matrix kernel.  This module states each step from scratch, on int64,
vectorised over candidates, so that a test can name the exact tier counts the library prints under KSLAM_DEBUG=1 and
check the certificate's mathematics against explicit searches.

Test infrastructure only (CPU, numpy); the oracle supplies the base coding.
"""
import numpy as np

import oracle as O

INT32_MAX = 2 ** 31 - 1
NEG = -(1 << 40)          # "no value" of the DP (far below any score)
NT_FULL = 7               # sw.hip: counts[NT_FULL] is the full-matrix list
SHORTCUT = 255            # sw.hip k_sw_plan: tier byte of a perfect / one-mismatch candidate
DEFAULT = (2, 3, 5, 2)    # (match, mismatch, gap_open, gap_extend), reference src/main.cpp:44-55


# ---- coding and windows (sw.hip stage_candidate_wide, :208-222; common.h ssw_code / ssw_code_complemented) ------------
_UPPER_ACGT = np.zeros(256, dtype=bool)
_UPPER_ACGT[list(b"ACGT")] = True


def codes(seq):
    """SSW codes of an ASCII sequence (A 0, C 1, G 2, T 3, U 0, else 4), as int64."""
    return O.translate(bytes(seq)).astype(np.int64)


def window(read_len, entry, rel, revcomp):
    """entry.substr(max(rel, 0), L) in SSW codes, reverse-complemented when revcomp (SmithWaterman.h:204-207):
    only upper-case A/C/G/T are complemented, every other byte keeps its code."""
    s0 = max(int(rel), 0)
    W = max(0, min(int(read_len), len(entry) - s0))
    seg = bytes(entry[s0:s0 + W])
    c = codes(seg)
    if revcomp:
        up = _UPPER_ACGT[np.frombuffer(seg, dtype=np.uint8)] if W else np.zeros(0, bool)
        c = np.where(up, 3 - c, c)[::-1].copy()
    return c


def score_of(q, w, sc):
    """The 5x5 matrix: +match / -mismatch, code 4 on either side scores 0 (ssw_cpp.cpp:25-49)."""
    match, mismatch = sc[0], sc[1]
    return np.where((q > 3) | (w > 3), 0, np.where(q == w, match, -mismatch))


class Batch:
    """Reads and windows of a list of candidates, padded with code 4 into rectangular int64 arrays.

    Q[c, i]: read base i (4 beyond L); Wp[c, P + j]: window base j (4 outside 0..W-1)."""

    def __init__(self, cand, reads, entries):
        self.n = n = len(cand)
        self.rel = np.asarray(cand["rel"], dtype=np.int64)
        self.rc = np.asarray(cand["revcomp"], dtype=np.int64) != 0
        self.L = np.array([len(reads[int(r)]) for r in cand["read"]], dtype=np.int64)
        wins = [window(self.L[c], entries[int(cand["entry"][c])], self.rel[c], self.rc[c]) for c in range(n)]
        self.W = np.array([len(w) for w in wins], dtype=np.int64)
        self.Lmax = int(self.L.max()) if n else 1
        self.Wmax = int(self.W.max()) if n else 1
        self.P = P = self.Lmax + 4
        self.Q = np.full((n, self.Lmax), 4, dtype=np.int64)
        self.Wp = np.full((n, self.Wmax + 2 * P), 4, dtype=np.int64)
        rq = {}
        for c in range(n):
            r = int(cand["read"][c])
            if r not in rq:
                rq[r] = codes(reads[r])
            self.Q[c, :self.L[c]] = rq[r]
            self.Wp[c, P:P + self.W[c]] = wins[c]
        self.d0 = np.where(self.rel < 0, self.rel, 0)      # seed diagonal: read base i on window base i + d0

    @classmethod
    def of_pairs(cls, pairs):
        """A batch of explicit (read codes, window codes, rel) triples (rel < 0 sets the seed diagonal)."""
        b = cls.__new__(cls)
        b.n = n = len(pairs)
        b.L = np.array([len(p[0]) for p in pairs], dtype=np.int64)
        b.W = np.array([len(p[1]) for p in pairs], dtype=np.int64)
        b.rel = np.array([p[2] if len(p) > 2 else 0 for p in pairs], dtype=np.int64)
        b.rc = np.array([bool(p[3]) if len(p) > 3 else False for p in pairs])
        b.Lmax, b.Wmax = max(1, int(b.L.max())), max(1, int(b.W.max()))
        b.P = P = b.Lmax + 4
        b.Q = np.full((n, b.Lmax), 4, dtype=np.int64)
        b.Wp = np.full((n, b.Wmax + 2 * P), 4, dtype=np.int64)
        for c, p in enumerate(pairs):
            b.Q[c, :b.L[c]] = p[0]
            b.Wp[c, P:P + b.W[c]] = p[1]
        b.d0 = np.where(b.rel < 0, b.rel, 0)
        return b

    def sub(self, idx):
        b = Batch.__new__(Batch)
        for k in ("rel", "rc", "L", "W", "Q", "Wp", "d0"):
            setattr(b, k, getattr(self, k)[idx])
        b.n = len(b.L)
        b.Lmax, b.Wmax, b.P = self.Lmax, self.Wmax, self.P
        return b

    def diagonal(self, d):
        """(matches, mismatches) of every candidate on its diagonal d[c] (j = i + d), cells inside the matrix only."""
        i = np.arange(self.Lmax)[None, :]
        w = np.take_along_axis(self.Wp, i + np.asarray(d)[:, None] + self.P, axis=1)
        q = self.Q
        real = (q < 4) & (w < 4)
        return (real & (q == w)).sum(1), (real & (q != w)).sum(1)


# ---- the certificate (sw.hip :300-365) ------------------------------------------------------------------------------
def certificate_amin(score, L, W, sc):
    """sw.hip certificate_amin (:325-339): the smallest A(g) = m0(g) - g over the feasible g; INT32_MAX when nothing
    needs bounding, -1 when the score certifies nothing."""
    ma, gO, gE = sc[0], sc[2], sc[3]
    score, L, W = np.broadcast_arrays(*(np.asarray(x, dtype=np.int64) for x in (score, L, W)))
    Lm = np.minimum(L, W)
    m00 = (score + ma - 1) // ma
    room = Lm * ma - score - gO
    g = np.minimum(room // gE + 1, 2047) if gE < ma else np.ones_like(room)
    m0 = (score + gO + (g - 1) * gE + ma - 1) // ma
    amin = np.where(room >= 0, np.minimum(m00, m0 - g), m00)
    return np.where(score <= 0, -1, np.where(m00 > Lm, INT32_MAX, amin))


def small_div(a, b):
    """sw.hip SmallDiv (:300-307): (a * (2^20 / b + 1)) >> 20 below 4096 (b < 256), the real division at and above."""
    a = np.asarray(a, dtype=np.int64)
    m = (1 << 20) // b + 1
    fast = (a >= 0) & (a < 4096) & (b < 256)
    return np.where(fast, ((a & 0xFFFFFFFF) * m) >> 20, np.floor_divide(a, b))


def certificate_amin_fast(score, L, W, sc):
    """sw.hip certificate_amin_fast (:309-324): certificate_amin with the two SmallDiv dividers."""
    ma, gO, gE = sc[0], sc[2], sc[3]
    score, L, W = np.broadcast_arrays(*(np.asarray(x, dtype=np.int64) for x in (score, L, W)))
    Lm = np.minimum(L, W)
    m00 = small_div(score + ma - 1, ma)
    room = Lm * ma - score - gO
    g = np.minimum(small_div(np.maximum(room, 0), gE) + 1, 2047) if gE < ma else np.ones_like(room)
    m0 = small_div(score + gO + (g - 1) * gE + ma - 1, ma)
    amin = np.where(room >= 0, np.minimum(m00, m0 - g), m00)
    return np.where(score <= 0, -1, np.where(m00 > Lm, INT32_MAX, amin))


def band_holds(amin, L, W, dlo, nd):
    """sw.hip band_holds (:340-344)."""
    amin, L, W, dlo, nd = np.broadcast_arrays(*(np.asarray(x, dtype=np.int64) for x in (amin, L, W, dlo, nd)))
    inside = (amin - L >= dlo) & (W - amin <= dlo + nd - 1)
    return np.where(amin < 0, False, np.where(amin == INT32_MAX, True, inside))


def band_certifies(score, L, W, dlo, nd, sc):
    """sw.hip band_certifies (:346-365): every alignment scoring >= score lies in [dlo, dlo + nd - 1]."""
    return (np.asarray(score) > 0) & band_holds(certificate_amin(score, L, W, sc), L, W, dlo, nd)


def amin_by_search(score, Lm, sc):
    """min over every g >= 0 with cost(g) <= Lm match - score of A(g) = ceil((score + cost(g)) / match) - g,
    cost(0) = 0, cost(g) = gO + (g - 1) gE: the certificate's definition, searched explicitly (vectorised over score)."""
    ma, gO, gE = sc[0], sc[2], sc[3]
    score = np.asarray(score, dtype=np.int64)
    best = -(-score // ma)
    g = 1
    while True:
        cost = gO + (g - 1) * gE
        ok = cost <= Lm * ma - score
        if not ok.any():
            break
        best = np.where(ok, np.minimum(best, -(-(score + cost) // ma) - g), best)
        g += 1
    return best


# ---- the tier set (sw.hip sw_scores, :1383-1418) ----------------------------------------------------------------------
def short_cap(sc):
    """api_align.hip: reads longer than this go to the plain long-read kernel (every candidate on the full matrix)."""
    return min(511, 8187 // max(1, sc[0] + 2 * sc[3]))


class Tiers:
    def __init__(self, nd, unknown, lm):
        self.nd, self.unknown, self.lm = tuple(nd), unknown, lm

    def __repr__(self):
        return "Tiers(nd=%s, unknown=%d, lm=%d)" % (self.nd, self.unknown, self.lm)


def tier_set(max_read_len, sc, no48=False, no96=False, unknown_nd=0):
    """The tiers a chunk whose longest (short) read has max_read_len bases runs through, or None when the band kernels
    cannot take the scoring (band_ok false: every candidate on the full matrix)."""
    if max_read_len > 511:
        raise ValueError("a chunk of short reads holds at most 511 bases")
    ma, gE = sc[0], sc[3]
    if not ((ma + 2 * gE) * max_read_len <= 8187 and ma + 2 * gE <= 31):
        return None
    lm = 0 if max_read_len <= 160 else (1 if max_read_len <= 256 else 2)
    base = (16, 32, 48, 64, 96) if lm == 0 else (16, 32, 48, 64, 96, 128)
    nd = [d for d in base if not ((d == 48 and no48) or (d == 96 and no96))]
    unk = unknown_nd if unknown_nd else (48 if lm == 0 else 64)
    unknown = 1
    for k, d in enumerate(nd):
        if d <= unk:
            unknown = k
    return Tiers(nd, unknown, lm)


# ---- the planner (sw.hip k_sw_plan, :539-658) -------------------------------------------------------------------------
def plan(b, sc, tiers):
    """Per candidate: the planner's sums and its decision.  Returns a dict of int64 / bool arrays:
    best, full, full_x, near_m, far_m (n, 2), perfect, one, shortcut, amin (the fast certificate of best) and tier
    (index into tiers.nd, or SHORTCUT)."""
    ma, mx, gO = sc[0], sc[1], sc[2]
    d0, rc, L, W, rel = b.d0, b.rc, b.L, b.W, b.rel
    dfirst = d0 - np.where(rc, 2, 0)                    # :545, the lowest of the three diagonals
    nm, nx = zip(*[b.diagonal(dfirst + k) for k in range(3)])
    nm, nx = np.stack(nm, 1), np.stack(nx, 1)
    best = np.maximum(0, (nm * ma - nx * mx).max(1))    # :564-570 (best starts at 0)
    seed = np.where(rc, 2, 0)                           # :571
    ar = np.arange(b.n)
    full, full_x = nm[ar, seed], nx[ar, seed]
    other = np.ones((b.n, 3), bool)
    other[ar, seed] = False
    near_m = np.where(other, nm, 0).max(1)
    perfect = (rel >= 0) & (W == L) & (L > 0) & (full == L)                      # :583
    one = ~perfect & (rel >= 0) & (W == L) & (L > 4) & (full == L - 1) & (full_x == 1)   # :602
    dsec = np.where(rc, 1, -2)                          # :606, the two diagonals not counted above
    far_m = np.stack([b.diagonal(d0 + dsec + k)[0] for k in range(2)], 1)
    # the row of the seed diagonal's one mismatch (:620-626)
    i = np.arange(b.Lmax)[None, :]
    w0 = np.take_along_axis(b.Wp, i + d0[:, None] + b.P, axis=1)
    mm = (b.Q < 4) & (w0 < 4) & (b.Q != w0)
    xrow = np.where(mm.any(1), b.Lmax - 1 - np.argmax(mm[:, ::-1], 1), -1)
    whole, left, right = ma * (L - 1) - mx, ma * xrow, ma * (L - 1 - xrow)
    S1 = np.where((whole > left) & (whole > right), whole,
                  np.where((left > whole) & (left > right), left,
                           np.where((right > whole) & (right > left), right, -1)))
    others = np.maximum(np.maximum(ma * (L - 3), ma * (L - 1) - gO), ma * np.maximum(near_m, far_m.max(1)))
    one_short = one & (xrow >= 0) & (xrow < L) & (S1 > 0) & (others < S1)
    shortcut = perfect | one_short
    amin = certificate_amin_fast(best, L, W, sc)
    tier = np.full(b.n, SHORTCUT, dtype=np.int64)
    if tiers is not None:
        choice = np.full(b.n, tiers.unknown, dtype=np.int64)
        for k in reversed(range(len(tiers.nd))):          # the narrowest that holds wins (:654-656)
            nd = tiers.nd[k]
            choice = np.where(band_holds(amin, L, W, d0 - nd // 2, nd), k, choice)
        tier = np.where(shortcut, SHORTCUT, choice)
    return dict(best=best, full=full, full_x=full_x, near_m=near_m, far_m=far_m, perfect=perfect, one=one,
                xrow=xrow, shortcut=shortcut, amin=amin, tier=tier, nm=nm, nx=nx)


# ---- banded local affine-gap DP ---------------------------------------------------------------------------------------
def banded_dp(b, dlo, nd, sc, keep=False, per_diagonal=False):
    """Local affine-gap Smith-Waterman restricted to the cells (i, j) with j - i in [dlo, dlo + nd - 1], 0 <= i < L,
    0 <= j < W; paths do not leave the band (k_sw_band: no E into the lowest diagonal, no F into the highest).
    dlo and nd are per candidate; returns the best score per candidate, and with keep=True also H[c, i, t] on band
    diagonal dlo + t (0 outside the matrix / the band), with per_diagonal=True the best H of each band diagonal.  Row by row as tests/golden/make_sw_tie_cases.py::sw, the E
    recurrence as one running maximum (gE < gO: an H made of E never opens a better E)."""
    ma, mx, gO, gE = sc
    dlo = np.broadcast_to(np.asarray(dlo, dtype=np.int64), (b.n,))
    nd = np.broadcast_to(np.asarray(nd, dtype=np.int64), (b.n,))
    NDm = int(nd.max()) if b.n else 1
    t = np.arange(NDm)[None, :]
    tt = t * gE
    Hp = np.zeros((b.n, NDm + 1), dtype=np.int64)       # row i - 1, one spare column on the right (outside the band)
    Fp = np.full((b.n, NDm + 1), NEG, dtype=np.int64)
    best = np.zeros(b.n, dtype=np.int64)
    Hk = np.zeros((b.n, b.Lmax, NDm), dtype=np.int64) if keep else None
    Dm = np.zeros((b.n, NDm), dtype=np.int64)
    inband = t < nd[:, None]
    for i in range(b.Lmax):
        j = i + dlo[:, None] + t
        valid = inband & (j >= 0) & (j < b.W[:, None]) & (i < b.L[:, None])
        w = np.take_along_axis(b.Wp, np.clip(j + b.P, 0, b.Wp.shape[1] - 1), axis=1)
        s = score_of(b.Q[:, i][:, None], w, sc)
        F = np.maximum(Fp[:, 1:] - gE, Hp[:, 1:] - gO)   # from (i - 1, j): band diagonal t + 1
        H0 = np.maximum(0, np.maximum(Hp[:, :-1] + s, F))
        H0 = np.where(valid, H0, 0)
        acc = np.maximum.accumulate(H0 - gO + tt, axis=1)   # E[t] = max_{t' < t} H0[t'] - gO - (t - 1 - t') gE
        E = np.full_like(H0, NEG)
        E[:, 1:] = acc[:, :-1] - tt[:, :-1]
        H = np.where(valid, np.maximum(H0, E), 0)
        Hp = np.concatenate([H, np.zeros((b.n, 1), np.int64)], 1)
        Fp = np.concatenate([np.where(valid, F, NEG), np.full((b.n, 1), NEG, np.int64)], 1)
        best = np.maximum(best, H.max(1))
        if keep:
            Hk[:, i] = H
        if per_diagonal:
            Dm = np.maximum(Dm, H)
    if per_diagonal:
        return best, Dm
    return (best, Hk) if keep else best


def full_dp(b, sc, keep=False, per_diagonal=False):
    """banded_dp over every diagonal of each candidate: the plain Smith-Waterman score."""
    return banded_dp(b, -(b.L - 1), b.L + b.W - 1, sc, keep, per_diagonal)


def optimum_diagonals(b, sc):
    """Per candidate: the optimum and the number of distinct diagonals holding a cell of that score."""
    best, D = full_dp(b, sc, per_diagonal=True)
    return best, ((D == best[:, None]) & (best[:, None] > 0)).sum(1)


# ---- the route (sw.hip sw_scores + k_sw_band's fail path, :989-1015) --------------------------------------------------
class Route:
    """Where every candidate of one chunk went.

    planned[c]: tier index or SHORTCUT; ran[c, k]: band score of tier k (-1: not run there); end[c]: the tier whose
    certificate held, NT_FULL for the full matrix, SHORTCUT for the shortcuts; planned_counts (6 values, as printed),
    round0[k] (every candidate tier k ran on a context's first chunk), n_full."""

    def __init__(self, planned, ran, end, tiers, plan_info, batch):
        self.planned, self.ran, self.end, self.tiers, self.plan, self.batch = planned, ran, end, tiers, plan_info, batch
        nt = len(tiers.nd) if tiers is not None else 0
        self.planned_counts = [int((planned == k).sum()) for k in range(6)]
        self.round0 = [int((ran[:, k] >= 0).sum()) for k in range(nt)]
        self.n_full = int((end == NT_FULL).sum())


def route(cand, reads, entries, sc, tiers, batch=None):
    """The whole routing of one chunk's candidates (cand: read, entry, rel, revcomp) under scoring sc through tiers
    (tier_set(...), or None: every candidate on the full matrix)."""
    b = batch if batch is not None else Batch(cand, reads, entries)
    n = b.n
    nt = len(tiers.nd) if tiers is not None else 0
    ran = np.full((n, max(nt, 1)), -1, dtype=np.int64)
    if tiers is None:
        return Route(np.full(n, SHORTCUT, np.int64), ran[:, :0], np.full(n, NT_FULL, np.int64), None, None, b)
    p = plan(b, sc, tiers)
    at = p["tier"].copy()                   # the list each candidate is in now
    end = np.where(p["shortcut"], SHORTCUT, -1).astype(np.int64)
    for k in range(nt):
        idx = np.nonzero(at == k)[0]
        if not len(idx):
            continue
        s = b.sub(idx)
        nd = tiers.nd[k]
        dlo = s.d0 - nd // 2
        score = banded_dp(s, dlo, nd, sc)
        ran[idx, k] = score
        ok = band_certifies(score, s.L, s.W, dlo, nd, sc)
        end[idx[ok]] = k
        amin = certificate_amin(score, s.L, s.W, sc)
        dest = np.full(len(idx), NT_FULL, dtype=np.int64)
        for k2 in reversed(range(k + 1, nt)):
            nd2 = tiers.nd[k2]
            hold = (score <= 0) | band_holds(amin, s.L, s.W, s.d0 - nd2 // 2, nd2)
            dest = np.where(hold, k2, dest)
        at[idx] = np.where(ok, -1, dest)
        full = idx[~ok & (dest == NT_FULL)]
        end[full] = NT_FULL
    return Route(p["tier"], ran[:, :nt], end, tiers, p, b)
