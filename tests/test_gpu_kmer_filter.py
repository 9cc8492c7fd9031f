"""k_extract_filter (k-slam_amd/csrc/filter.hip) survivor by survivor, at its edges.

The fused extraction + membership filter decides which read k-mers reach the sort and the join.  Alignment rows hide a
dropped survivor (a database read has ~7 k-mers on its true diagonal), so every case here asserts
  (a) timings()["n_kmers_kept"] == the survivor count of the CPU restatement (tests/filter_ref.py), exactly;
  (b) find_overlaps(): the raw count and the deduplicated (read, entry, rel, revcomp) list equal the oracle's
      findOverlaps on the FULL read k-mer list (a false negative of the filter loses overlaps);
  (c) for the edge batch, the phase-complete batch and the short_cap batch: align_batch rows and CIGARs equal the oracle.

The database: sixteen entries G[s:], s = 0..15, of one random genome G, so that every position of G is a sampled genome
k-mer (gap 16) -- every non-zero k-mer of a read cut from G is a genome key, whatever the hash -- plus two unrelated
entries large enough that the smallest filter (2^20 bits) gives false positives, a poly-A entry (k-mer 0) and an entry
of repeated keys.  G carries palindromic 32-mers (fwd == rc, which take the reverse-complement branch).
"""
import numpy as np
import pytest

import filter_ref as F

pytestmark = pytest.mark.gpu

DEFAULT_SHORT_CAP = 511      # api_align.hip:32 for the default scoring (2, 3, 5, 2): min(511, 8187 // 6)
JUNK = np.frombuffer(b"NnacgtRYU-", dtype=np.uint8)      # (bytes >= 128 are undefined in the reference)
JUNK_AT = (0, 15, 16, 31, 32, 63, 64, 127, 128, 143, 144, -1)
EDGE_LENGTHS = list(range(0, 81)) + list(range(120, 166)) + list(range(250, 261)) + list(range(490, 512))
LONG_LENGTHS = list(range(512, 521))
OV_FIELDS = ("read", "entry", "rel", "revcomp")
AL_FIELDS = ("read", "entry", "rel", "revcomp", "score", "ref_begin", "ref_end", "query_begin", "query_end", "cigar_len")


def short_cap_of(match, gap_extend):
    return min(511, 8187 // (match + 2 * gap_extend))    # api_align.hip:32 (inside the scoring envelope)


class Db:
    def __init__(self, synth):
        rng = np.random.default_rng(2024)
        G = synth.random_bases(rng, 4096)
        for p in range(40, 4000, 97):                     # palindromic 32-mers at every phase of the sampling
            h = synth.random_bases(rng, 16)
            G[p:p + 32] = np.concatenate([h, synth.revcomp(h)])
        U = [synth.random_bases(rng, 700000) for _ in range(2)]
        entries = [G[s:] for s in range(16)] + U + [np.frombuffer(b"A" * 500, dtype=np.uint8).copy(),
                                                    np.concatenate([U[0][1000:3000], U[1][500:900]])]
        self.G, self.U = G, U
        self.genomes = synth.to_bytes(entries)
        self.genome_recs = F.O.extract_kmers(self.genomes, True, 16)
        assert (F.O.extract_kmers([G.tobytes()], False, 1)["kmer"] != 0).all()   # no k-mer 0 in G: closed forms hold
        self._filters = {}

    def filt(self, fb):
        if fb not in self._filters:
            self._filters[fb] = F.build_filter(self.genome_recs["kmer"], fb)
        return self._filters[fb]


class Case:
    """One batch of reads and what the oracle says about it (computed once, compared under every configuration)."""

    def __init__(self, db, reads):
        self.db, self.reads = db, reads
        self.lens = np.array([len(r) for r in reads], dtype=np.int64)
        self.recs = F.O.extract_kmers(reads, False, 1)
        self.ov, self.raw = F.O.find_overlaps(F.O.sort_kmers(np.concatenate([self.recs, db.genome_recs])), self.lens)
        self._kept, self._al = {}, {}

    def kept_mask(self, filter_bits, short_cap):
        """filter_ref.expected_survivors on this case, with the database's filters cached"""
        key = (filter_bits, short_cap)
        if key not in self._kept:
            fb = F.auto_filter_bits(len(self.db.genome_recs)) if filter_bits is None else F.env_filter_bits(filter_bits)
            if fb == 0:
                m = np.ones(len(self.recs), dtype=bool)
            else:
                long_read = self.lens[F.read_index(self.recs)] > short_cap
                m = long_read | ((self.recs["kmer"] != 0) & F.is_member(self.db.filt(fb), self.recs["kmer"], fb))
            self._kept[key] = m
        return self._kept[key]

    def expected_kept(self, filter_bits=None, short_cap=DEFAULT_SHORT_CAP):
        return int(self.kept_mask(filter_bits, short_cap).sum())

    def alignments(self, params=None):
        key = None if params is None else tuple(getattr(params, f) for f, _ in params._fields_)
        if key not in self._al:
            exp, ecig, _ = F.O.align_to_database(self.reads, self.db.genomes, params)
            self._al[key] = (exp, ecig)
        return self._al[key]


def check_overlaps(ctx, case, filter_bits=None, short_cap=DEFAULT_SHORT_CAP, exact=None):
    """(a) and (b) on a fresh load of the case's reads; `exact`: a closed-form survivor count to assert as well"""
    ctx.load_reads(case.reads)
    got, raw = ctx.find_overlaps()
    t = ctx.timings()
    assert t["n_read_kmers"] == len(case.recs)
    exp_kept = case.expected_kept(filter_bits, short_cap)
    if exact is not None:
        assert exp_kept == exact, ("filter_ref disagrees with the closed form", exp_kept, exact)
    assert t["n_kmers_kept"] == exp_kept, ("n_kmers_kept", t["n_kmers_kept"], "expected", exp_kept)
    assert raw == case.raw, ("raw overlaps", raw, "expected", case.raw)
    assert len(got) == len(case.ov), ("deduplicated overlaps", len(got), "expected", len(case.ov))
    for f in OV_FIELDS:
        bad = np.nonzero(got[f] != case.ov[f])[0]
        assert len(bad) == 0, "%s differs at %s: got %s exp %s" % (f, bad[:5], got[bad[:5]], case.ov[bad[:5]])
    return t


def check_alignments(ctx, case, params=None):
    """(c)"""
    got, gcig = ctx.align_batch(case.reads)
    exp, ecig = case.alignments(params)
    assert len(got) == len(exp), ("alignments", len(got), "expected", len(exp))
    for f in AL_FIELDS:
        bad = np.nonzero(got[f] != exp[f])[0]
        assert len(bad) == 0, "%s differs at %s: got %s exp %s" % (f, bad[:5], got[bad[:5]], exp[bad[:5]])
    go, eo = got["cigar_off"].astype(np.int64), exp["cigar_off"].astype(np.int64)
    for i in range(len(got)):
        n = int(got["cigar_len"][i])
        assert (gcig[go[i]:go[i] + n] == ecig[eo[i]:eo[i] + n]).all(), "cigar %d" % i


# ---- reads ----

class Reads:
    def __init__(self, db, synth, seed):
        self.db, self.synth = db, synth
        self.rng = np.random.default_rng(seed)

    def _slice(self, src, L):
        a = int(self.rng.integers(0, len(src) - L + 1))
        return src[a:a + L].copy()

    def _subs(self, s, rate=0.01):
        return self.synth.mutate(self.rng, s, rate, 0.0)

    def _junk(self, s):
        s = s.copy()
        for p in JUNK_AT:
            if -len(s) <= p < len(s):
                s[p] = self.rng.choice(JUNK)
        return s

    def make(self, kind, L):
        r, syn = self.rng, self.synth
        u = self.db.U[int(r.integers(0, 2))]
        if kind == "u":                      # from the database, with substitutions
            s = self._subs(self._slice(u, L))
        elif kind == "u_rc":
            s = syn.revcomp(self._subs(self._slice(u, L)))
        elif kind == "g":                    # exact, from the phase-complete genome (palindromes included)
            s = self._slice(self.db.G, L)
        elif kind == "g_rc":
            s = syn.revcomp(self._slice(self.db.G, L))
        elif kind == "random":
            s = syn.random_bases(r, L)
        elif kind == "junk":                 # non-ACGT bytes at the kernel's word, row and register edges
            s = self._junk(self._slice(u, L))
        elif kind == "g_junk":
            s = self._junk(syn.revcomp(self._slice(self.db.G, L)))
        elif kind == "poly_a":
            s = np.frombuffer(b"A" * L, dtype=np.uint8)
        elif kind == "poly_a_u":             # k-mer 0 next to genome k-mers
            s = np.concatenate([np.frombuffer(b"A" * (L // 2), dtype=np.uint8), self._slice(u, L - L // 2)])
        else:
            raise ValueError(kind)
        assert len(s) == L
        return s.tobytes()

    def mixed(self, n, lo, hi, kinds=("u", "u_rc", "g", "random", "junk", "g_rc", "poly_a_u")):
        return [self.make(kinds[i % len(kinds)], int(self.rng.integers(lo, hi + 1))) for i in range(n)]


def edge_reads(db, synth):
    """Every length 0..80, 120..165, 250..260, 490..511 and 512..520 (long class), each at all four start residues of its
    byte offset mod 4, twice: a database read (forward / reverse complement, with substitutions, or exact from G) and one
    of random / non-ACGT bytes / poly-A / palindromes.  The long reads follow as one run (one chunk), short reads after."""
    R = Reads(db, synth, 77)
    reads, total = [], [0]

    def add(s):
        reads.append(s)
        total[0] += len(s)

    kinds_a = ("u", "u_rc", "g", "g_rc")
    kinds_b = ("random", "junk", "poly_a", "g_junk", "poly_a_u", "junk", "random", "u_rc")
    j = 0
    for lengths, is_long in ((EDGE_LENGTHS, False), (LONG_LENGTHS, True)):
        for L in lengths:
            for residue in range(4):
                for kinds in (kinds_a, kinds_b):
                    k = (residue - total[0]) % 4
                    if k:     # a pad read of the same class shifts the next start to `residue`
                        add(R.make("random", 512 + k) if is_long else b"C" * k)
                    assert total[0] % 4 == residue
                    add(R.make(kinds[(j + j // 4) % len(kinds)], L))   # (the kind moves against the residue from length to length)
                j += 1
    for L in (150, 33, 159, 287, 415, 511):
        add(R.make("g", L))
    return reads


@pytest.fixture(scope="module")
def db(synth):
    return Db(synth)


@pytest.fixture(scope="module")
def edge(db, synth):
    return Case(db, edge_reads(db, synth))


@pytest.fixture(scope="module")
def phase(db, synth):
    """128 reads of 511 bases from G (a whole workgroup of 8 waves x 16 reads, every one all survivors), then reads from G
    of every length up to 511 (forward and reverse complement)."""
    R = Reads(db, synth, 78)
    reads = [R.make("g" if i % 2 == 0 else "g_rc", 511) for i in range(128)]
    reads += [R.make("g" if L % 2 else "g_rc", L) for L in range(20, 512, 7)]
    case = Case(db, reads)
    case.closed_form = int(np.sum(np.maximum(case.lens - F.K + 1, 0)))
    return case


def test_phase_batch_overflows_the_stage(phase):
    """Precondition of the stage-overflow branch (filter.hip:325-339): with STAGE = 2048 slots (filter.hip:199), each of the
    16 trips of the first workgroup (reads w * 16 + i of waves w = 0..7) hands out 8 x 480 survivors -- which also leaves the
    stage more than half full at every trip boundary (the flush between trips, filter.hip:284-292)."""
    kept = phase.kept_mask(None, DEFAULT_SHORT_CAP)
    per_read = np.bincount(F.read_index(phase.recs)[kept], minlength=len(phase.reads))
    assert (per_read[:128] == 511 - F.K + 1).all()
    for i in range(F.RPW):
        assert per_read[[w * F.RPW + i for w in range(F.FW)]].sum() == 8 * 480 > F.STAGE


FILTER_CONFIGS = [(b, how) for b in ("20", "21", "24", None, "0") for how in ("blocks", "atomics", "no_digits")]


@pytest.mark.parametrize("bits,how", FILTER_CONFIGS)
def test_filter_configurations(kslam, db, edge, phase, monkeypatch, bits, how):
    """The edge batch and the phase-complete batch under KSLAM_FILTER_BITS 20 (line_bits 10) / 21 / 24 / automatic / 0,
    each with the block-by-block filter build, the atomic build and without the extraction's digit bytes."""
    if bits is not None:
        monkeypatch.setenv("KSLAM_FILTER_BITS", bits)
    if how == "atomics":
        monkeypatch.setenv("KSLAM_FILTER_BUILD", "atomics")
    if how == "no_digits":
        monkeypatch.setenv("KSLAM_SORT_DIGIT_BYTES", "0")
    c = kslam.Context()
    try:
        c.set_index(db.genomes)
        t = check_overlaps(c, edge, bits)
        if bits == "0":
            assert t["n_kmers_kept"] == t["n_read_kmers"]
        t = check_overlaps(c, phase, bits, exact=None if bits == "0" else phase.closed_form)
        if bits == "0":
            assert t["n_kmers_kept"] == t["n_read_kmers"]
        check_alignments(c, edge)
        check_alignments(c, phase)
    finally:
        c.close()


@pytest.fixture(scope="module")
def batches(db, synth):
    R = Reads(db, synth, 79)
    return {n: Case(db, R.mixed(n, 20, 511 if n < 1000 else 260)) for n in (1, 15, 16, 17, 127, 128, 129, 4100)}


def test_batch_sizes(kslam, db, batches):
    """1, 15, 16, 17, 127, 128, 129 and 4100 reads: around RPW = 16 reads per wave and FW * RPW = 128 per workgroup."""
    c = kslam.Context()
    try:
        c.set_index(db.genomes)
        for n in sorted(batches, reverse=True):
            check_overlaps(c, batches[n])
        for n in sorted(batches):
            check_overlaps(c, batches[n])
    finally:
        c.close()


def first_cap(kept_last, nk_all):
    """The extraction's first output capacity (api_align.hip:185-186)"""
    return min(max(kept_last + kept_last // 4, nk_all // 8) + 4096, nk_all)


@pytest.mark.parametrize("digits", ["1", "0"])
def test_capacity_rerun(kslam, db, synth, monkeypatch, digits):
    """The output-capacity re-run of the extraction (api_align.hip:185-198), with and without the digit bytes it writes:
    (i) the first batch of a context all survivors; (ii) one batch in two chunks (max_kmers_per_chunk), a low-survival one
    then an all-survivor one, so that the capacity guessed from the first is too small; (iii) a small batch after a big one."""
    monkeypatch.setenv("KSLAM_SORT_DIGIT_BYTES", digits)
    R = Reads(db, synth, 80)
    big = Case(db, [R.make("g" if i % 2 else "g_rc", 150) for i in range(300)])
    nk_big = 300 * (150 - F.K + 1)
    small = Case(db, R.mixed(17, 30, 300))
    c = kslam.Context()
    try:
        c.set_index(db.genomes)
        assert nk_big > first_cap(0, nk_big)                      # (i): the first attempt cannot hold the survivors
        check_overlaps(c, big, exact=nk_big)
        check_overlaps(c, small)                                  # (iii)
        check_overlaps(c, big, exact=nk_big)
    finally:
        c.close()
    per_chunk = 150 * (150 - F.K + 1)
    two = Case(db, [R.make("random", 150) for _ in range(150)] + [R.make("g_rc" if i % 2 else "g", 150) for i in range(150)])
    kept1 = int(two.kept_mask(None, DEFAULT_SHORT_CAP)[F.read_index(two.recs) < 150].sum())
    assert per_chunk > first_cap(kept1, per_chunk)               # (ii): the second chunk's first attempt is too small
    c = kslam.Context(max_kmers_per_chunk=per_chunk)
    try:
        c.set_index(db.genomes)
        t = check_overlaps(c, two, exact=kept1 + per_chunk)
        assert t["n_chunks"] == 2
        check_overlaps(c, small)
    finally:
        c.close()


def test_short_cap_boundary(kslam, db, synth, oracle):
    """Scoring (16, 10, 12, 4) is inside the envelope and gives short_cap = 341 (api_align.hip:32): reads of 340 and 341 bases
    take the filtered extraction, reads of 342 the unfiltered one (all their k-mers kept), in one batch."""
    match, mismatch, gap_open, gap_extend = 16, 10, 12, 4
    cap = short_cap_of(match, gap_extend)
    assert cap == 341
    R = Reads(db, synth, 81)
    reads = []
    for kind in ("g", "g_rc", "random", "u", "u_rc", "junk", "random", "g"):
        for L in (340, 341, 342, 150):
            reads.append(R.make(kind, L))
    case = Case(db, reads)
    # the boundary is crossed: the 342-base reads count whole, which a 511 cap would not
    assert case.expected_kept(None, cap) > case.expected_kept(None, DEFAULT_SHORT_CAP)
    c = kslam.Context(match=match, mismatch=mismatch, gap_open=gap_open, gap_extend=gap_extend)
    try:
        c.set_index(db.genomes)
        t = check_overlaps(c, case, short_cap=cap)
        assert t["n_chunks"] >= 3
        check_alignments(c, case, oracle.Params.default(match=match, mismatch=mismatch, gap_open=gap_open,
                                                        gap_extend=gap_extend))
    finally:
        c.close()
