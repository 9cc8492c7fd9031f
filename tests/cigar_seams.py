"""Closed-form read families for the banded CIGAR stage (k-slam_amd/csrc/cigar.hip), shared by
tests/test_cigar_plan_ref.py (CPU: the restatement against the oracle, and the preconditions) and
tests/test_gpu_cigar_seams.py (GPU: rows, CIGARs and the printed counts under four tunings).

Every read gets fresh random sequence of its own -- a stretch of the shared entry 0, between junk, or a short entry --
so that a candidate is one read against one place.  Every member is built for both strands.  Families:
  I / D  one insertion / deletion of h - 1 and h bases (bw0 = h and h + 1) for every bin edge h, in the first third, the
         middle and the last third of the read;
  X      an insertion of a bases and further on a deletion of b: bw0 = |a - b| + 1 but the path strays max(a, b)
         diagonals, so the band doubles from bw0 until it holds them;
  H      short local alignments -- a seed flank, an insertion, a short flank, junk around -- whose window is 2 bw0 + 1
         bases long, one shorter, one and two longer: the hand-over rule at equality;
  W      the aligned span's length over six consecutive values and the indel's row over twelve, per band (the six cells
         per direction word, by row and by turn);
  S      read lengths 150 / 151 mixed and junk prefixes of 0..16 bases: every 16-byte residue of both staged spans;
  C      alternating one-base insertions and deletions: CIGARs of 21..29 ops around the 24-op temp slot, some starting
         `1M 1I` (the traceback then ends on an indel), some with one 6-base indel (a systolic traceback overflows), some
         with four mismatches in a row that (10, 8, 6, 3) aligns as `4I 4D` (the even op counts);
  T      ungapped reads with mismatches in a row, and one-base rotations that a gap pair aligns better: sw_epilogue's
         inline <n>M rule at its edge;
  N      batches whose band-2 list holds exactly 1, 63, 64, 65, 127, 128 and 129 candidates;
  R      windows of 32 bases: entries that are one 32-mer which the k-mer coding matches and the SW coding does not (the
         read holds lower-case c / g / t where the entry holds A), so the local alignment is whatever the random rest of
         the read finds in 32 bases -- the only way to a window no longer than a register band (at most 15).  Not closed
         form: the family is sized so that the oracle finds each case often enough.
"""
import numpy as np

import cigar_plan_ref as P

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
EDGES = (1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128)
DEFAULT = (2, 3, 5, 2)
SC3 = (3, 2, 4, 1)
SC10 = (10, 8, 6, 3)


def revcomp(s):
    return s[::-1].translate(COMP)


def gap_cost(sc, n):
    return sc[2] + (n - 1) * sc[3]


def pays(sc, flank, n):
    """a flank of `flank` matching bases is worth crossing a gap of n bases for (with two points to spare)"""
    return sc[0] * flank >= gap_cost(sc, n) + 2


class Builder:
    def __init__(self, seed, L):
        self.rng = np.random.default_rng(seed)
        self.L = L
        self.reads, self.entries, self.fam = [], [b""], []

    def bases(self, n):
        return ACGT[self.rng.integers(0, 4, n)].tobytes()

    def other(self, s):
        """bases that differ from s position by position: junk that cannot extend an alignment along its diagonal"""
        a = np.frombuffer(bytes(s), dtype=np.uint8)
        idx = np.searchsorted(ACGT, a)
        return ACGT[(idx + self.rng.integers(1, 4, len(a))) % 4].tobytes()

    def piece(self, n, pre=0, post=0, res=0):
        """n fresh bases appended to the shared entry after junk, starting at res modulo 16 (res = 0: the entry's k-mer at
        the piece's first base is one of those the index samples).  Returns (piece, the pre bases before it, the post
        bases after it) -- what a read's junk must differ from."""
        e = self.entries[0] + self.bases(64 + max(pre, post))
        e += self.bases((res - len(e)) % 16)
        s = self.bases(n)
        before = e[len(e) - pre:] if pre else b""
        self.last_start = len(e)
        e += s
        after = self.bases(max(post, 64))
        self.entries[0] = e + after
        return s, before, after[:post]

    def patch(self, at, b):
        """overwrite the base at offset `at` of the piece made last"""
        e = bytearray(self.entries[0])
        e[self.last_start + at] = b
        self.entries[0] = bytes(e)

    def own(self, g, total):
        """g at the start of a short entry of its own, padded to `total` bases"""
        pad = self.bases(max(0, total - len(g)))
        self.entries.append(g + pad)
        return pad

    def add(self, read, fam, rc):
        assert len(read) == self.L, (fam, len(read), self.L)
        self.reads.append(revcomp(read) if rc else read)
        self.fam.append(fam + (" rc" if rc else " fw"))


def _strands():
    return (False, True)


# ---- I / D -------------------------------------------------------------------------------------------------------------
def fam_indel(B, sc, hs, kinds="ID"):
    L = B.L
    for h in hs:
        for s in (h - 1, h):
            if s < 1:
                continue
            for where, frac in (("first", 1 / 3), ("mid", 1 / 2), ("last", 2 / 3)):
                for kind in kinds:
                    body = L - s if kind == "I" else L            # read bases taken from the entry
                    p = int(round(body * frac))
                    if not pays(sc, min(p, body - p), s) or min(p, body - p) < 8:
                        continue
                    for rc in _strands():
                        if kind == "I":
                            g, _, _ = B.piece(L - s)
                            r = g[:p] + B.other(g[p:p + 1] * s if p < len(g) else b"A" * s) + g[p:]
                        else:
                            g, _, _ = B.piece(L + s)
                            r = g[:p] + g[p + s:]
                        B.add(r, "%s h=%d size=%d %s" % (kind, h, s, where), rc)


# ---- X -----------------------------------------------------------------------------------------------------------------
def chain_pairs(max_stray):
    """(a, b): a = b around every power of two (chains from band 1 to each later bin), and |a - b| + 1 in {3, 5, 6, 7}
    with max(a, b) just past half of every doubled width (the chain ends at 6, 12, 24, 48, 96, 10, 20, 40, 80, ...)."""
    out = []
    k = 1
    while (1 << k) - 1 <= max_stray:
        for a in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            if 1 <= a <= max_stray:
                out.append((a, a))
        k += 1
    out.append((1, 1))
    for bw0 in (3, 5, 6, 7):
        w = 2 * bw0
        while w // 2 + 1 <= max_stray:
            big = w // 2 + 1
            out.append((big, big - (bw0 - 1)))
            out.append((big - (bw0 - 1), big))
            w *= 2
    return sorted(set(out))


def fam_chain(B, sc, max_stray, extra=()):
    L = B.L
    for a, b in chain_pairs(max_stray) + list(extra):
        n1 = max(33, (L - a) // 3)                 # the first flank holds the seed
        n2 = (L - a - n1) // 2
        n3 = L - a - n1 - n2
        if not pays(sc, n2, max(a, b)) or n2 < 8:
            continue
        for rc in _strands():
            if max(a, b) > 128:                    # an entry of its own, no longer than the window span: no junk to stray into
                g = B.bases(n1 + n2 + b + n3)
                B.own(g, 0)
            else:
                g, _, _ = B.piece(n1 + n2 + b + n3)
            if sc == DEFAULT:
                ins = B.other(g[n1:n1 + 1] * a)
            else:                                  # cheap gaps: random bases would find partners in the deleted stretch
                ins = bytes([next(x for x in ACGT if x not in (g[n1 - 1], g[n1]))]) * a
            r = g[:n1] + ins + g[n1:n1 + n2] + g[n1 + n2 + b:]
            B.add(r, "X a=%d b=%d" % (a, b), rc)


# ---- I / D beyond half a read: class 8 asked for directly --------------------------------------------------------------
def fam_huge(B, sc):
    """Entries of their own, as long as the window span: an insertion of 255 / 256 bases in a read of 511 (refLen 256 /
    255), and a deletion of as many (readLen 256 / 255, the rest of the read junk)."""
    L = B.L
    for s in (255, 256):
        for rc in _strands() * 2:
            g = B.bases(L - s)
            B.own(g, 0)
            B.add(g[:128] + B.other(g[128:129] * s) + g[128:], "I huge size=%d" % s, rc)
            g = B.bases(L)
            B.own(g, 0)
            B.add(g[:128] + g[128 + s:] + B.bases(s), "D huge size=%d" % s, rc)


# ---- H -----------------------------------------------------------------------------------------------------------------
def fam_handover(B, sc, inserts, own_entry):
    """refLen = seed + f, readLen = seed + I + f, bw0 = I + 1: refLen - (2 bw0 + 1) = seed + f - 2 I - 3 = d"""
    L = B.L
    for I in inserts:
        for d in (-1, 0, 1, 2):
            for seed in (33, 36, 40):
                f = 2 * I + 3 + d - seed
                if f < 2 or not pays(sc, f, I) or not pays(sc, seed, I):
                    continue
                for rc in _strands():
                    pre = int(B.rng.integers(0, 12))
                    post = L - pre - seed - I - f
                    if own_entry:
                        g = B.bases(seed + f)
                        pad = B.own(g, max(47, seed + f + int(B.rng.integers(0, 4))))
                        before, after = B.bases(pre), (pad + B.bases(post))[:post]
                    else:
                        g, before, after = B.piece(seed + f, pre, min(post, 64))
                        after = after + B.bases(post - len(after))
                    ins = B.other(g[seed:seed + 1] * I)
                    r = B.other(before) + g[:seed] + ins + g[seed:] + B.other(after)
                    B.add(r, "H I=%d d=%d seed=%d%s" % (I, d, seed, " own" if own_entry else ""), rc)


# ---- W -----------------------------------------------------------------------------------------------------------------
def fam_words(B, sc, bands=(1, 2, 4, 7, 15)):
    """Per band: an indel of band - 1 bases (band 1: a one-base insertion and deletion 30 bases apart) at twelve
    consecutive rows, with junk of 0..3 bases in front and 0..5 behind: six consecutive span lengths."""
    L = B.L
    for bw in bands:
        for k in range(12):
            head, tail = (k // 6) * 2 + (k % 2), k % 6
            for kind in "ID":
                for rc in _strands():
                    body = L - head - tail                        # read bases between the junk
                    p = 50 + k                                    # the indel's row, before the head junk
                    if bw == 1:                                   # a one-base insertion and deletion: refLen == readLen
                        g, before, after = B.piece(body, head, tail)
                        q = p + 30
                        mid = g[:p] + B.other(g[p:p + 1]) + g[p:q] + g[q + 1:] if kind == "I" else \
                            g[:p] + g[p + 1:q] + B.other(g[q:q + 1]) + g[q:]
                    elif kind == "I":
                        s = bw - 1
                        g, before, after = B.piece(body - s, head, tail)
                        mid = g[:p] + B.other(g[p:p + 1] * s) + g[p:]
                    else:
                        s = bw - 1
                        g, before, after = B.piece(body + s, head, tail)
                        mid = g[:p] + g[p + s:]
                    r = B.other(before) + mid + B.other(after)
                    B.add(r, "W band=%d k=%d %s" % (bw, k, kind), rc)


# ---- S -----------------------------------------------------------------------------------------------------------------
def fam_staging(B, sc):
    """(B.L is 150; every third member has 151 bases, so the reads' offsets take every residue.)  A one-base insertion
    (odd j + t) or deletion in the middle, junk of j bases in front and t behind, and the entry's stretch starting at
    every residue modulo 16 on both strands."""
    n = 0
    for j in range(17):
        for t in (0, 1, 2, 5, 9):
            for rc in _strands():
                L = 150 + (n % 3 == 0)
                n += 1
                body = L - j - t
                p = body // 2
                if (j + t) & 1:
                    g, before, after = B.piece(body - 1, j, t, res=(7 * (n // 2) + 3 * (n & 1)) % 16)
                    mid = g[:p] + B.other(g[p:p + 1]) + g[p:]
                else:
                    g, before, after = B.piece(body + 1, j, t, res=(7 * (n // 2) + 3 * (n & 1)) % 16)
                    mid = g[:p] + g[p + 1:]
                B.L = L
                B.add(B.other(before) + mid + B.other(after), "S j=%d t=%d L=%d" % (j, t, L), rc)
    B.L = 150


# ---- C -----------------------------------------------------------------------------------------------------------------
def fam_cap(B, sc, lead_insertion=False):
    """k one-base indels, insertions and deletions in turn, every `step` bases: 2 k + 1 ops; with lead_insertion the
    read's second base is the first insertion (the CIGAR starts 1M 1I; the scoring must make one match worth a gap);
    `six`: one of them is 6 bases long (band 7: bin 3, the systolic kernel under the default tuning)."""
    L = B.L
    for k in range(10, 15):
        for six in (False, True):
            for rc in _strands() * (6 if lead_insertion else 2):
                # an exact stretch that holds a sampled 32-mer first: bases 0..32, or 1..48 behind a leading insertion
                if lead_insertion:
                    step = (L - 49 - 12) // (k - 1)
                    pos = [1] + [49 + step * x for x in range(k - 1)]
                else:
                    step = (L - 33 - 12) // k
                    pos = [33 + step * x for x in range(k)]
                if six and not pays(sc, step, 6):
                    continue
                g, _, _ = B.piece(L + 8)
                r, at = b"", 0
                for x, p in enumerate(pos):
                    n = 6 if six and x == k // 2 else 1
                    r += g[at:p]
                    if x % 2 == 0:
                        r += B.other(g[p:p + 1] * n)
                        at = p
                    else:
                        at = p + n
                r += g[at:]
                B.add(r[:L], "C k=%d%s%s" % (k, " six" if six else "", " lead" if lead_insertion else ""), rc)


def fam_cap_block(B, sc, lead_insertion=False):
    """fam_cap's members with four mismatches in a row 14 bases before the read's end, for a scoring where four
    mismatches cost more than an insertion and a deletion of four bases (4 mismatch > 2 gap_open + 6 gap_extend): the
    traceback leaves `4I 4D` (or `4D 4I`) with no match between them, three more ops: 2 k + 4, an EVEN count.  The read's
    block is AAAA and the entry holds no A from one base before the block to one behind it, so nothing else lines up."""
    assert 4 * sc[1] > 2 * sc[2] + 6 * sc[3]
    L = B.L
    for k in range(9, 13):
        for rc in _strands() * (6 if lead_insertion else 2):
            if lead_insertion:
                step = (L - 49 - 24) // (k - 1)
                pos = [1] + [49 + step * x for x in range(k - 1)]
            else:
                step = (L - 33 - 24) // k
                pos = [33 + step * x for x in range(k)]
            g = bytearray(B.piece(L + 8)[0])
            gmap, at = [], 0                      # per read base: its entry base, or -(p + 1) for a base inserted before p
            for x, p in enumerate(pos):
                gmap += range(at, p)
                if x % 2 == 0:
                    gmap.append(-(p + 1))
                    at = p
                else:
                    at = p + 1
            gmap += range(at, len(g))
            gmap = gmap[:L]
            bp = L - 14
            gi = gmap[bp]
            assert gmap[bp - 1:bp + 5] == list(range(gi - 1, gi + 5)), "the block lies in the last exact stretch"
            for z in range(gi - 1, gi + 5):
                g[z] = b"CGT"[int(B.rng.integers(0, 3))]
                B.patch(z, g[z])
            r = bytearray(B.other(bytes(g[-z - 1] for z in gmap if z < 0)))
            r = bytearray(g[z] if z >= 0 else r.pop(0) for z in gmap)
            r[bp:bp + 4] = b"AAAA"
            B.add(bytes(r), "C block k=%d%s" % (k, " lead" if lead_insertion else ""), rc)


# ---- T -----------------------------------------------------------------------------------------------------------------
def fam_ties(B, sc):
    """Ungapped reads with 2 and 3 mismatches in a row (inline <n>M as long as nothing beats the diagonal), and blocks
    of k + 1 bases where the read holds the entry's block rotated by one (entry x0 x1 .. xk, read x1 .. xk y): deleting
    x0 and inserting y gains k matches and k + 1 mismatches for two gap opens."""
    L = B.L
    for m in (2, 3):
        for at in (40, 75, 110):
            for rc in _strands():
                g, _, _ = B.piece(L)
                B.add(g[:at] + B.other(g[at:at + m]) + g[at + m:], "T mismatches=%d" % m, rc)
    if sc == DEFAULT:
        # entry a b N d, read b a N e (a != b, e != d): the diagonal pays two mismatches for the swap and one for e;
        # inserting b, matching a and deleting d pays two gap opens for one match -- one point more
        for at in (40, 52, 64, 76, 88, 100, 112):
            for rc in _strands():
                g, _, _ = B.piece(L)
                a, b = g[at:at + 1], g[at + 1:at + 2]
                if a == b:
                    b = B.other(a)
                    B.patch(at + 1, b[0])
                B.patch(at + 2, ord("N"))
                B.add(g[:at] + b + a + b"N" + B.other(g[at + 3:at + 4]) + g[at + 4:], "T swap", rc)
    for k in (1, 2, 3):
        for at in (40, 60, 75, 90, 110):
            for rc in _strands():
                g, _, _ = B.piece(L)
                blk = g[at + 1:at + 1 + k] + B.other(g[at + k:at + k + 1])
                B.add(g[:at] + blk + g[at + k + 1:], "T rotate k=%d" % k, rc)


# ---- N -----------------------------------------------------------------------------------------------------------------
def fam_lists(B, sc, n_gapped, n_plain=8):
    """n_gapped copies of one D member (a one-base deletion 20 bases before the read's end: one seed flank, so ONE
    candidate per read, band 2), and a few perfect reads."""
    L = B.L
    for x in range(n_gapped):
        g, _, _ = B.piece(L + 1)
        B.add(g[:L - 20] + g[L - 19:], "N D size=1", bool(x & 1))
    for x in range(n_plain):
        g, _, _ = B.piece(L)
        B.add(g, "N plain", bool(x & 1))


# ---- R -----------------------------------------------------------------------------------------------------------------
def fam_short_windows(B, sc, n):
    L = B.L
    for k in range(n):
        rc = bool(k & 1)
        fake = bytearray(B.bases(32))
        rd = bytearray(fake)
        for i in range(32):
            if i % 4 != 3:                       # (every fourth base is real: the all-A k-mer never joins)
                fake[i] = ord("A")
                rd[i] = b"cgt"[int(B.rng.integers(0, 3))]
        # the read's k-mer is the entry's on the forward strand, or its reverse complement
        B.entries.append(revcomp(bytes(fake)) if rc else bytes(fake))
        pre = int(B.rng.integers(0, 8))
        B.reads.append(B.bases(pre) + bytes(rd) + B.bases(L - 32 - pre))
        B.fam.append("R %d%s" % (k, " rc" if rc else " fw"))


# ---- cases -------------------------------------------------------------------------------------------------------------
def _edges(lo, hi):
    return [h for h in EDGES if lo <= h <= hi]


# name -> (seed, read length, scoring, [family calls], extra environment)
CASES = {
    "L150": (1, 150, DEFAULT, [lambda B, sc: fam_indel(B, sc, _edges(1, 32)), lambda B, sc: fam_chain(B, sc, 33)],
             {"KSLAM_SWEEP_ROOM": "0"}),
    "L150_words": (2, 150, DEFAULT, [fam_words], {"KSLAM_SWEEP_ROOM": "0"}),
    "L150_staging": (3, 150, DEFAULT, [fam_staging], {}),
    "L150_cap_ties": (4, 150, DEFAULT, [fam_cap, fam_ties], {}),
    "L150_sc3": (5, 150, SC3, [lambda B, sc: fam_chain(B, sc, 66),
                               lambda B, sc: fam_handover(B, sc, (19, 20, 21, 22), False),
                               lambda B, sc: fam_handover(B, sc, (19, 20, 21, 22), True), fam_ties], {}),
    "L160": (6, 160, DEFAULT, [lambda B, sc: fam_indel(B, sc, (1, 2, 7, 8, 31, 32)), lambda B, sc: fam_chain(B, sc, 17),
                               lambda B, sc: fam_words(B, sc, (2, 7))], {}),
    "L161": (7, 161, DEFAULT, [lambda B, sc: fam_indel(B, sc, (1, 2, 7, 8, 31, 32)), lambda B, sc: fam_chain(B, sc, 17),
                               lambda B, sc: fam_words(B, sc, (2, 7))], {}),
    "L256": (8, 256, DEFAULT, [lambda B, sc: fam_indel(B, sc, (1, 4, 15, 16, 32)), lambda B, sc: fam_chain(B, sc, 33),
                               lambda B, sc: fam_words(B, sc, (1, 15))], {}),
    "L257": (9, 257, DEFAULT, [lambda B, sc: fam_indel(B, sc, (1, 4, 15, 16, 32)), lambda B, sc: fam_chain(B, sc, 33),
                               lambda B, sc: fam_words(B, sc, (1, 15))], {}),
    "L400": (10, 400, DEFAULT, [lambda B, sc: fam_indel(B, sc, _edges(3, 64)), lambda B, sc: fam_chain(B, sc, 97)], {}),
    "L511_sc3": (11, 511, SC3, [lambda B, sc: fam_indel(B, sc, _edges(31, 128)),
                                lambda B, sc: fam_chain(B, sc, 130)], {}),
    "L511_sc10": (15, 511, SC10, [lambda B, sc: fam_indel(B, sc, _edges(63, 128)), fam_huge,
                                  lambda B, sc: fam_chain(B, sc, 130, [(131, 131), (135, 133), (140, 140), (145, 145), (150, 150), (160, 160)])], {}),
    "sc10": (12, 150, SC10, [fam_cap, lambda B, sc: fam_cap(B, sc, True), fam_ties,
                             lambda B, sc: fam_indel(B, sc, (2, 5, 16)),
                             lambda B, sc: fam_handover(B, sc, (19, 20, 21, 22), False),
                             lambda B, sc: fam_handover(B, sc, (19, 20, 21, 22), True)], {}),
    "sc10_short": (16, 150, SC10, [lambda B, sc: fam_short_windows(B, sc, 400)], {}),
    "sc10_even": (17, 150, SC10, [fam_cap_block, lambda B, sc: fam_cap_block(B, sc, True)], {}),
    "long512": (13, 512, DEFAULT, [lambda B, sc: fam_indel(B, sc, (2, 5, 8, 16, 32, 64)),
                                   lambda B, sc: fam_chain(B, sc, 33),
                                   lambda B, sc: fam_handover(B, sc, (40, 41), False)], {}),
    "one_gapped": (14, 150, DEFAULT, [lambda B, sc: fam_lists(B, sc, 1)], {}),
}
for _n in (63, 64, 65, 127, 128, 129):
    CASES["list%d" % _n] = (20 + _n, 150, DEFAULT, [lambda B, sc, n=_n: fam_lists(B, sc, n)], {})


class Case:
    pass


_cache = {}


def case(name, oracle):
    """The batch of a case, the oracle's answer for it and the restatement's candidates (computed once)."""
    if name not in _cache:
        seed, L, sc, fams, env = CASES[name]
        B = Builder(seed, L)
        for f in fams:
            f(B, sc)
        c = Case()
        c.name, c.sc, c.env, c.B = name, sc, dict(env), B
        c.reads, c.entries, c.fam = B.reads, B.entries, B.fam
        lens = np.array([len(r) for r in c.reads])
        cap = P.short_cap(sc)
        assert (lens <= cap).all() or (lens > cap).all(), "one class of reads per batch: one chunk"
        c.long_chunk = bool((lens > cap).all())
        c.lmax = int(lens.max())
        p = oracle.Params.default(match=sc[0], mismatch=sc[1], gap_open=sc[2], gap_extend=sc[3])
        c.rows, c.cig, _ = oracle.align_to_database(c.reads, c.entries, p)
        roff = np.concatenate([[0], np.cumsum(lens)])
        eoff = np.concatenate([[0], np.cumsum([len(e) for e in c.entries])])
        c.cand = P.candidates(c.rows, c.reads, c.entries, sc, roff, eoff)
        c.plans = {}
        _cache[name] = c
    return _cache[name]


def plan_of(c, tuning_name, **perturb):
    key = (tuning_name,) + tuple(sorted(perturb.items()))
    if key not in c.plans:
        tune = P.Tuning.of_env(P.TUNINGS[tuning_name], c.long_chunk)
        c.plans[key] = P.plan(c.cand, tune, c.lmax, **perturb)
    return c.plans[key]
