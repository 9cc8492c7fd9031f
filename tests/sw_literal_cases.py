"""Closed-form read families for the three literal kernels: k_sw_striped and k_sw_long (k-slam_amd/csrc/sw.hip) and the
one-lane banded_sw, k_banded_lds<0> / k_banded_lds_wide (k-slam_amd/csrc/cigar.hip).  Shared by
tests/test_sw_literal_cases.py (CPU: the preconditions, the real ssw.c, the stored vectors) and
tests/test_gpu_sw_literal_seams.py (GPU: rows and CIGARs against the oracle, and which path ran).

Every read gets fresh random sequence in the database, so a read has one candidate per diagonal it was planted on and no
cross hits.  The index samples an entry's 32-mers at offsets that are multiples of 16: a read carries a seed when 32 of its
bases equal the entry at such an offset (Builder.place puts a chosen base of a piece on one; 47 equal bases hold a seed
wherever they lie).

  S1  segment seams: read lengths around the multiples of 8 and 16 (segLen and the padding cells change there)
  S2  the byte / word hand-over `best + bias >= 255` (src/ssw.c:318): best scores 255 - bias - 2 .. 255 - bias + 2
  S3  Lazy-F across SSE lanes: one gap of 1, segLen - 1, segLen, segLen + 1, 2 segLen bases starting at k segLen - 1, k segLen,
      k segLen + 1, in the read and in the window, for the byte layout (16 lanes) and the word layout (8 lanes)
  S4  ends and `terminate`: starts at read 0 / window 0, reads hanging off an entry, entries shorter than the read, the empty
      read and a 31-base one, tandem repeats of period 7 / 8 (the best score at two end columns or rows)
  S5  Ns (score 0) in the first and last cell of a segment and in runs of segLen, in the read and in the window
  S6  word saturation outside the envelope (match 127 and 100)
  S7  reads around the 64 KiB LDS opt-in of k_sw_striped
  S8  k_sw_long: the lcap rounding, its own 64 KiB opt-in, 9000 bases, class runs of length one, ties and hang-offs at 600 bases
  S9  saturation INSIDE the envelope: match x length around 32767
  S10 the literal banded_sw on long chunks: every bin of initial bands, doubling, a span its band covers, a long CIGAR
"""
import zlib

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
DEFAULT = (2, 3, 5, 2)
# one scoring per way of leaving the envelope (api_core.hip scoring_in_envelope)
OUTSIDE = ((2, 9, 5, 2),            # mismatch > gO + gE
           (2, 8, 2, 3),            # gE >= gO
           (1, 1, 1, 1),            # gE = gO
           (2, 3, 5, 0),            # gE = 0
           (40, 3, 5, 2),           # match > 31
           (2, 40, 30, 20),         # mismatch > 32
           (127, 127, 255, 255))    # the type limits
S1_LENGTHS = (32, 33, 47, 48, 49, 63, 64, 65, 119, 120, 121, 127, 128, 129)
SAT = 32767                         # where adds_epi16 saturates (src/ssw.c word pass)


def revcomp(s):
    return s[::-1].translate(COMP)


def in_envelope(sc):
    m, x, go, ge = sc
    return 1 <= m <= 31 and x <= 32 and 1 <= ge < go and x <= go + ge


def gap_cost(sc, n):
    """what a gap of n bases costs: where gE > gO, opening again (H - gO) beats extending (E - gE) at every base"""
    return sc[2] + (n - 1) * min(sc[2], sc[3])


def sw_long_lds(lcap):
    """sw.hip sw_scores: the dynamic LDS of k_sw_long for a chunk whose longest read rounds up to lcap"""
    return 4 * (lcap + 2) * 4 + 2 * (lcap + 16)


def sw_striped_lds(lcap):
    """sw.hip sw_scores: the dynamic LDS of k_sw_striped"""
    return 4 * (lcap + 16) * 2 + 2 * (lcap + 16)


def lcap_of(L):
    return (L + 15) & ~15


def longest_below_opt_in(lds_of):
    """the longest read whose chunk still asks for at most 64 KiB"""
    L = 16
    while lds_of(lcap_of(L + 1)) <= 64 * 1024:
        L += 1
    return L


def saturates(sc, L):
    """sw.hip sw_scores: a chunk whose longest read has L bases goes through k_sw_striped whatever its scoring"""
    return sc[0] * L > SAT


class Builder:
    """Reads and one database; entry 0 is shared, every piece of it separated from the next by junk."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.reads, self.entries, self.fam = [], [b""], []

    def bases(self, n):
        return ACGT[self.rng.integers(0, 4, n)].tobytes()

    def other(self, s):
        """bases that differ from s position by position"""
        a = np.frombuffer(bytes(s), dtype=np.uint8)
        idx = np.searchsorted(ACGT, a)
        return ACGT[(idx + self.rng.integers(1, 4, len(a))) % 4].tobytes()

    def place(self, g, seed_at=0):
        """g appended to the shared entry after junk, g[seed_at] on an offset the index samples"""
        e = self.entries[0] + self.bases(64)
        e += self.bases((-(len(e) + seed_at)) % 16)
        self.entries[0] = e + g
        return g

    def piece(self, n, seed_at=0):
        return self.place(self.bases(n), seed_at)

    def own(self, g):
        """g as an entry of its own (its offset 0 is sampled)"""
        self.entries.append(g)
        return g

    def subs(self, s, k, keep=(0, 0)):
        """k substitutions at distinct random positions outside [keep[0], keep[1])"""
        a = bytearray(s)
        free = [p for p in range(len(a)) if not keep[0] <= p < keep[1]]
        for p in (self.rng.choice(free, size=min(k, len(free)), replace=False) if free and k else ()):
            a[p] = self.other(bytes(a[p:p + 1]))[0]
        return bytes(a)

    def add(self, read, fam, rc=False):
        self.reads.append(revcomp(read) if rc else read)
        self.fam.append(fam)

    def close(self):
        self.entries[0] += self.bases(64)
        return self


# ---- S1 ------------------------------------------------------------------------------------------------------------------
def fam_seams(B, sc):
    for L in S1_LENGTHS:
        for rc in (False, True):
            for rep in range(2):
                at = int(B.rng.integers(0, L - 32 + 1))
                g = B.piece(L, at)
                r = B.subs(g, (L - 32) // 25 + rep, (at, at + 32))
                if rep and L >= 63:
                    p = at + 40 if at + 40 < L else at - 5
                    r = r[:p] + b"N" + r[p + 1:]
                B.add(r, "S1", rc)


# ---- S2 ------------------------------------------------------------------------------------------------------------------
def handover_targets(sc):
    """best scores around the byte pass's overflow test that a seeded candidate can have at all: a candidate holds 32 matches
    (its seed), and every score is a multiple of the common divisor of match, mismatch and the two gap costs (gap_cost)"""
    g = int(np.gcd.reduce([v for v in (sc[0], sc[1], sc[2], min(sc[2], sc[3])) if v]))
    edge = 255 - sc[1]
    return [t for t in range(edge - 2, edge + 3) if t % g == 0 and t >= 32 * sc[0]]


def fam_handover(B, sc):
    """Reads equal to their window but for k mismatches, n Ns and at most one insertion of `gap` bases, chosen so that
    match (L - gap - k - n) - mismatch k - cost(gap) is the target, every flank long enough to be worth crossing for."""
    ma, mx = sc[0], sc[1]
    for t in handover_targets(sc):
        found = []
        for gap in (0, 1, 2, 3):
            for k in range(0, 5):
                for n in range(0, 3):
                    cost = mx * k + (gap_cost(sc, gap) if gap else 0)
                    if (t + cost) % ma:
                        continue
                    a = (t + cost) // ma
                    L = a + gap + k + n
                    parts = k + n + (1 if gap else 0) + 1
                    flank = (a - 40) // parts
                    if not 80 <= L <= 300 or flank * ma <= max(mx, gap_cost(sc, gap) if gap else 0) + ma:
                        continue
                    found.append((L, k, n, gap))
        found.sort(key=lambda f: (f[3] > 0, f[1] + f[2], f[0]))
        for x, (L, k, n, gap) in enumerate(found[:4]):
            for rc in (False, True):
                g = B.piece(L - gap, 4)
                r = bytearray(g)
                marks = np.linspace(40, len(g) - 1, k + n + (1 if gap else 0) + 2)[1:-1].astype(int)
                order = B.rng.permutation(len(marks))
                cut = None
                for y, p in enumerate(marks[order]):
                    if y < k:
                        r[p] = B.other(bytes(r[p:p + 1]))[0]
                    elif y < k + n:
                        r[p] = ord("N")
                    else:
                        cut = int(p)
                r = bytes(r)
                if cut is not None:
                    ins = bytes([next(b for b in ACGT if b not in (g[cut - 1], g[cut]))]) * gap
                    r = r[:cut] + ins + r[cut:]
                B.add(r, "S2", rc)


# ---- S3 ------------------------------------------------------------------------------------------------------------------
def fam_lazy_f(B, sc, L=150):
    for W in (16, 8):
        seg = (L + W - 1) // W
        ks = [k for k in range(1, W) if 50 <= k * seg <= L - 60][:1] + [k for k in range(1, W) if 50 <= k * seg <= L - 60][-1:]
        for n in (1, seg - 1, seg, seg + 1, 2 * seg):
            for k in ks:
                for off in (-1, 0, 1):
                    p = k * seg + off
                    rc = bool((n + k + off) & 1)
                    # a gap in the read's rows: the read holds n bases the window does not
                    g = B.piece(L - n, 2)
                    ins = bytes([next(b for b in ACGT if b not in (g[p - 1], g[p]))]) * n
                    B.add(g[:p] + ins + g[p:], "S3", rc)
                    # and in the window's columns: the window holds n bases the read does not
                    g = B.piece(L + n, 2)
                    B.add(g[:p] + g[p + n:], "S3", not rc)


# ---- S4 ------------------------------------------------------------------------------------------------------------------
def fam_hang(B, sc, L, fam):
    """reads hanging off an entry's start or end by o bases; entries shorter than the read; starts at read 0 and window 0"""
    for o in (1, 2, 15, 16, 17, L - 47):
        for rc in (False, True):
            e = B.own(B.bases(L + 200 + (-(L + 200)) % 16))
            r = B.bases(o) + e[:L - o]                               # off the start: the seed is the entry's first 32-mer
            B.add(B.subs(r, 2, (0, o + 32)) if L - o >= 80 else r, fam, rc)
            e = B.own(B.bases(L + 200 + (-(L + 200)) % 16))
            r = e[len(e) - (L - o):] + B.bases(o)                    # off the end: W = L - o
            B.add(B.subs(r, 2, (0, 47)) if L - o >= 80 else r, fam, rc)
    for n in (47, 60, L // 2, L - 1):
        e = B.own(B.bases(n))
        pre = int(B.rng.integers(0, L - n + 1))
        B.add(B.bases(pre) + e + B.bases(L - n - pre), fam, bool(n & 1))
    for rc in (False, True):
        e = B.own(B.bases(L + 64))
        B.add(e[:L], fam, rc)                                        # begins at read 0 and at window 0
        B.add(B.subs(e[:L], 1, (0, 47)), fam, rc)


def fam_ties(B, sc, L, fam):
    """a tandem repeat of period 7 or 8 between unique flanks, the entry holding one unit more or less than the read: the
    best score occurs at two end columns or rows, and the forward and the reverse pass have to resolve the ties"""
    for P in (7, 8):
        for dn in (-1, 1):
            for rc in (False, True):
                unit = B.bases(P)
                nr = min((L - 110) // P, 12)
                a = L - 55 - nr * P
                fa, fb = B.bases(a), B.bases(55)
                B.place(fa + unit * (nr + dn) + fb, 3)
                B.add(fa + unit * nr + fb, fam, rc)


def fam_ends(B, sc):
    fam_hang(B, sc, 120, "S4")
    fam_ties(B, sc, 150, "S4")
    B.add(b"", "S4")
    B.add(B.piece(40)[:31], "S4")


# ---- S5 ------------------------------------------------------------------------------------------------------------------
def fam_ns(B, sc, L=128):
    for W in (16, 8):
        seg = (L + W - 1) // W
        for k in (48 // seg + 1, (L - 20) // seg - 1):
            for what in ("first", "last", "run", "both"):
                for in_read in (True, False):
                    for rc in (False, True):
                        lo = k * seg
                        span = {"first": (lo, lo + 1), "last": (lo + seg - 1, lo + seg), "run": (lo, lo + seg),
                                "both": (lo + seg - 1, lo + seg + 1)}[what]
                        g = B.bases(L)
                        r = g
                        if in_read:
                            r = g[:span[0]] + b"N" * (span[1] - span[0]) + g[span[1]:]
                        else:
                            g = g[:span[0]] + b"N" * (span[1] - span[0]) + g[span[1]:]
                        B.place(g, 1)
                        B.add(B.subs(r, 1, (0, span[1] + 2)), "S5", rc)


# ---- S6 / S9 -------------------------------------------------------------------------------------------------------------
def indel_read(B, g, L, n):
    """L bases of g with n short indels spread over the read, deletions and insertions in turn; g has L + 8 bases"""
    cuts = np.linspace(100, L - 100, n + 2)[1:-1].astype(int)
    r, at = b"", 0
    for x, c in enumerate(cuts):
        size = 1 + (x + n) % 3
        if x & 1:
            r += g[at:c] + bytes([next(b for b in ACGT if b not in (g[c - 1], g[c]))]) * size
            at = c
        else:
            r += g[at:c]
            at = c + size
    return (r + g[at:])[:L]


def fam_saturation(B, sc, L, fam, parts="ABC", n_indels=1):
    """A: a perfect read and one with 3 substitutions; B: 6 and 9 substitutions (one candidate each); C: a read with
    n_indels short indels (a candidate per diagonal that holds a seed: up to n_indels + 1)"""
    for k in ((0, 3) if "A" in parts else ()) + ((6, 9) if "B" in parts else ()):
        g = B.piece(L, 20 % 16)
        B.add(B.subs(g, k, (0, 48)), fam, bool(k & 1))
    if "C" in parts:
        g = B.piece(L + 8, 4)
        B.add(indel_read(B, g, L, n_indels), fam, n_indels == 2)


def fam_s6(B, sc):
    if sc == (127, 3, 5, 2):
        for L in (257, 258, 259):                  # 32 639, 32 766, and past saturation
            for rc in (False, True):
                B.add(B.piece(L, 5), "S6", rc)
        for k in (0, 3, 9):
            for rc in (False, True):
                g = B.piece(300, 7)
                B.add(B.subs(g, k, (0, 48)), "S6", rc)
        for rc in (False, True):
            g = B.piece(302, 9)
            B.add(g[:150] + g[152:], "S6", rc)     # a 2-base deletion
            g = B.piece(300, 9)
            B.add(g[:170] + bytes([next(b for b in ACGT if b not in (g[169], g[170]))]) * 2 + g[170:298], "S6", rc)
    else:
        for L in (327, 328, 400):                  # 32 700, and past saturation
            for rc in (False, True):
                B.add(B.piece(L, 11), "S6", rc)
                g = B.piece(L + 2, 11)
                B.add(g[:L // 2] + g[L // 2 + 2:], "S6", rc)


S9_GROUPS = (((31, 3, 5, 2), (1056, 1057, 1058)),
             ((7, 3, 5, 2), (4681, 4682)),            # 7 x 4681 = 32 767 exactly
             ((4, 3, 5, 2), (8191, 8192, 8193)),
             ((5, 3, 5, 2), (9000,)),
             ((8, 3, 5, 2), (9000,)),
             ((16, 10, 12, 4), (2100,)),
             ((31, 30, 20, 12), (1200,)))
S6_SCORINGS = ((127, 3, 5, 2), (100, 90, 3, 5))


# ---- S7 / S8 -------------------------------------------------------------------------------------------------------------
def short_reads(B, n, fam):
    for x in range(n):
        g = B.piece(151, 6)
        r = B.subs(g[:150], 2, (0, 48)) if x % 3 else g[:70] + g[71:151]
        B.add(r, fam, bool(x & 1))


def long_read(B, L, fam, rc=False, indel=True):
    g = B.piece(L + 1, 8)
    r = g[:L // 2] + g[L // 2 + 1:] if indel else g[:L]
    B.add(B.subs(r, 4, (0, 48)), fam, rc)


def fam_mixed(B, longs, fam, indel=True):
    """150-base reads with the long reads as class runs of length one at batch position 0, in the middle and last"""
    long_read(B, longs[0], fam, False, indel)
    short_reads(B, 6, fam)
    for x, L in enumerate(longs[1:-1]):
        long_read(B, L, fam, bool(x & 1), indel)
        short_reads(B, 3, fam)
    if len(longs) > 1:
        long_read(B, longs[-1], fam, True, indel)


def fam_around(B, L, fam):
    """one long read with 150-base reads around it"""
    short_reads(B, 8, fam)
    long_read(B, L, fam)
    short_reads(B, 8, fam)


# ---- S10 -----------------------------------------------------------------------------------------------------------------
S10_INDELS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 32, 63, 64, 65)


def fam_banded(B, sc, L=600):
    for n in S10_INDELS:
        for rc in (False, True):
            p = L // 2 + int(B.rng.integers(-40, 41))
            g = B.piece(L - n, 3)
            B.add(g[:p] + B.other(g[p:p + 1] * n) + g[p:], "S10 I%d" % n, rc)        # initial band n + 1
            g = B.piece(L + n, 3)
            B.add(g[:p] + g[p + n:], "S10 D%d" % n, rc)
    # an insertion and, 150 bases on, a deletion of as many bases: both spans equal, band 1 first, doubled until it holds n
    for n in (2, 3, 5, 9, 20):
        for rc in (False, True):
            g = B.piece(L, 3)
            B.add(g[:200] + B.other(g[200:201] * n) + g[200:350] + g[350 + n:], "S10 X%d" % n, rc)
    # a span its band covers (refLen <= 2 bw + 1, the sentinel write of ssw.c:655 on a live cell): an insertion of 17 and a
    # deletion of 2 give band 16 first, which cannot hold 17, then 32 over a span of 57 + d columns; the rest of the read is junk
    for d in (0, 4, 8):
        for rc in (False, True):
            g = B.own(B.bases(57 + d))
            pre = int(B.rng.integers(5, 200))
            body = g[:32] + B.other(g[32:33] * 17) + g[32:44] + g[46:]
            B.add(B.bases(pre) + body + B.bases(L - pre - len(body)), "S10 covered", rc)


def fam_long_cigar(B, sc, L=9000):
    """one indel every 40 bases, insertions and deletions in turn: a CIGAR far beyond the small temp slot"""
    g = B.piece(L + 200, 5)
    r, at = b"", 0
    for x, c in enumerate(range(60, L, 40)):
        if x & 1:
            r += g[at:c] + bytes([next(b for b in ACGT if b not in (g[c - 1], g[c]))])
            at = c
        else:
            r += g[at:c]
            at = c + 1
    B.add((r + g[at:])[:L], "S10 long")
    short_reads(B, 4, "S10 long")


# ---- the cases -----------------------------------------------------------------------------------------------------------
def _tag(sc):
    return "_".join(str(v) for v in sc)


CASES = {}          # name -> (seed, scoring, family group, builder function)


def _case(name, sc, group, fn):
    CASES[name] = (zlib.crc32(name.encode()), sc, group, fn)


for _sc in OUTSIDE:
    _case("S1-5 " + _tag(_sc), _sc, "S1-5",
          lambda B, sc: [f(B, sc) for f in (fam_seams, fam_handover, fam_lazy_f, fam_ends, fam_ns)])
for _sc in S6_SCORINGS:
    _case("S6 " + _tag(_sc), _sc, "S6", fam_s6)
_S7_EDGE = longest_below_opt_in(sw_striped_lds)          # 6528: from lcap 6544 on the kernel has to opt in
for _L in (_S7_EDGE - 16, _S7_EDGE, _S7_EDGE + 16, _S7_EDGE + 32, 9000):
    _case("S7 L%d" % _L, (2, 9, 5, 2), "S7", lambda B, sc, L=_L: fam_around(B, L, "S7"))
_S8_EDGE = longest_below_opt_in(sw_long_lds)
_case("S8 lcap", DEFAULT, "S8", lambda B, sc: fam_mixed(B, [512, 513, 527, 528, 529], "S8"))
_case("S8 opt-in", DEFAULT, "S8", lambda B, sc: fam_mixed(B, [_S8_EDGE, _S8_EDGE + 1, _S8_EDGE - 15], "S8"))
_case("S8 L9000", DEFAULT, "S8", lambda B, sc: fam_mixed(B, [9000], "S8"))
_case("S8 ties and hang-offs", DEFAULT, "S8", lambda B, sc: (fam_ties(B, sc, 600, "S8"), fam_hang(B, sc, 600, "S8")))
for _x, (_sc, _lens) in enumerate(S9_GROUPS):
    for _L in _lens:
        _n = 1 + (_x + _L) % 3
        if _L <= 2100:
            _case("S9 %s L%d" % (_tag(_sc), _L), _sc, "S9",
                  lambda B, sc, L=_L, n=_n: fam_saturation(B, sc, L, "S9", "ABC", n))
        else:                                   # at most four long candidates per case
            for _part in ("AB", "C"):
                _case("S9 %s L%d %s" % (_tag(_sc), _L, _part), _sc, "S9",
                      lambda B, sc, L=_L, n=_n, part=_part: fam_saturation(B, sc, L, "S9", part, n))
_case("S10 indels", DEFAULT, "S10", fam_banded)
_case("S10 long cigar", DEFAULT, "S10", fam_long_cigar)

# the S6 / S9 cases in which no candidate scores 32 767: the lengths just below the cut, and the indel reads whose match x
# length is a match or two above it (7 x 4682 = 32 774, 4 x 8193 = 32 772, less the gaps).  (The perfect read of
# "S9 7_3_5_2 L4681 AB" scores exactly 32 767 on the k_sw_long route.)  tests/test_sw_literal_cases.py holds the list to
# the oracle.
BELOW_SATURATION = ("S9 31_3_5_2 L1056", "S9 7_3_5_2 L4681 C", "S9 7_3_5_2 L4682 C", "S9 4_3_5_2 L8191 AB",
                    "S9 4_3_5_2 L8191 C", "S9 4_3_5_2 L8192 C", "S9 4_3_5_2 L8193 C")
_built = {}


def build(name):
    """the Builder of a case (made once)"""
    if name not in _built:
        seed, sc, group, fn = CASES[name]
        B = Builder(seed)
        fn(B, sc)
        _built[name] = B.close()
    return _built[name]


def names(group=None, scoring=None):
    return [n for n, (_, sc, g, _) in CASES.items() if (group is None or g == group) and (scoring is None or sc == scoring)]


def lowered(sc, B):
    """the scoring of a case with match lowered until no read of B can saturate (the k_sw_long route for the same reads)"""
    return (max(1, SAT // max(len(r) for r in B.reads)),) + tuple(sc[1:])
