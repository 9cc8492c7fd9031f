"""The CPU restatement of the read k-mer membership filter (tests/filter_ref.py) checked on its own: what
tests/test_gpu_kmer_filter.py holds the kernel to must itself be right.  No GPU."""
import numpy as np
import pytest

import filter_ref as F

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_JUNK = np.frombuffer(b"NnacgtRYU-", dtype=np.uint8)


def _random_read(rng, n, junk=0.0):
    s = _ACGT[rng.integers(0, 4, n)].copy()
    if junk and n:
        at = np.nonzero(rng.random(n) < junk)[0]
        s[at] = rng.choice(_JUNK, len(at))
    return s.tobytes()


def _naive_revcomp(kmer, width=32):
    out = 0
    for j in range(width):
        out = (out << 2) | (((kmer >> (2 * j)) & 3) ^ 2)
    return out


def _positions(recs, lens):
    """read position q of each record: forward records carry q, reverse-complement ones len - 32 - q"""
    rc = (recs["meta"] >> np.uint32(30)) & np.uint32(1)
    off = recs["offset"].astype(np.int64)
    L = lens[F.read_index(recs)]
    return np.where(rc == 1, L - F.K - off, off)


def test_revcomp_and_probe_are_strand_symmetric():
    rng = np.random.default_rng(5)
    k = rng.integers(0, 1 << 63, 4000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 4000, dtype=np.uint64)
    half = rng.integers(0, 1 << 32, 50, dtype=np.uint64)
    pal = (half << np.uint64(32)) | F.revcomp32(half)           # fwd == rc
    k = np.concatenate([k, pal, np.array([0, 0xFFFFFFFFFFFFFFFF, 0xAAAAAAAAAAAAAAAA], dtype=np.uint64)])
    rc = F.revcomp64(k)
    assert all(int(r) == _naive_revcomp(int(x)) for x, r in zip(k[:300], rc[:300]))
    assert all(int(r) == _naive_revcomp(int(x), 16) for x, r in zip(half, F.revcomp32(half)))
    assert (F.revcomp64(rc) == k).all()
    assert (F.revcomp64(pal) == pal).all()
    for line_bits in (10, 11, 14, 22):
        p1, b1 = F.probe(k, line_bits)
        p2, b2 = F.probe(rc, line_bits)
        assert (p1 == p2).all() and all((x == y).all() for x, y in zip(b1, b2))
        assert int(p1.max()) < (1 << (line_bits + 3))
    assert (F.canonical_minimizer(k) == F.canonical_minimizer(rc)).all()


def test_direct_minimizer_equals_the_kernels_sliding_derivation():
    """canonical_minimizer (17 windows of both 64-bit strands, as min_window16) against k_extract_filter's derivation
    restated (c(p) = min(F(p), R(p)) over the read's 16-mers, minimum over [q, q + 16]) on reads of every length 32..520;
    and the packing both assume (A 0 C 1 T 2 G 3, first base high) against the oracle's records."""
    rng = np.random.default_rng(17)
    reads = [_random_read(rng, n, junk=0.01 if n % 3 == 0 else 0.0) for n in range(32, 521)]
    reads += [b"A" * 40, b"ACGT" * 30, b"GATC" * 20]
    recs = F.O.extract_kmers(reads, False, 1)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    assert len(recs) == int(np.sum(lens - F.K + 1))
    q = _positions(recs, lens)
    rid = F.read_index(recs)
    direct = F.canonical_minimizer(recs["kmer"])
    sliding = np.empty(len(recs), dtype=np.uint64)
    packed = np.empty(len(recs), dtype=np.uint64)
    for i, r in enumerate(reads):
        sel = np.nonzero(rid == i)[0]
        sliding[sel] = F.sliding_minimizers(r)[q[sel]]
        packed[sel] = F.packed_window(F.encode(r), F.K)[q[sel]]
    assert (direct == sliding).all()
    assert (np.minimum(packed, F.revcomp64(packed)) == recs["kmer"]).all()
    # forward records are the packed value itself, everything else (palindromes included) its reverse complement
    is_rc = ((recs["meta"] >> np.uint32(30)) & np.uint32(1)) == 1
    assert (is_rc == (packed >= F.revcomp64(packed))).all()


def test_packing_agrees_with_the_reference_extraction():
    if not F.O.have_ref_kmer():
        pytest.skip("the reference's k-mer library is not built here")
    rng = np.random.default_rng(3)
    reads = [_random_read(rng, n, junk=0.02) for n in (32, 33, 64, 150, 250, 511)]
    got = F.O.ref_extract_kmers(reads, False, 1)
    exp = F.O.extract_kmers(reads, False, 1)
    assert len(got) == len(exp) and (got == exp).all()
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    q, rid = _positions(got, lens), F.read_index(got)
    packed = np.array([int(F.packed_window(F.encode(reads[i]), F.K)[j]) for i, j in zip(rid, q)], dtype=np.uint64)
    assert (np.minimum(packed, F.revcomp64(packed)) == got["kmer"]).all()


@pytest.mark.parametrize("bits", [20, 21, 24, None])
def test_every_genome_key_is_a_member(bits):
    rng = np.random.default_rng(40 + (bits or 0))
    genomes = [_random_read(rng, 60000), _random_read(rng, 3000, junk=0.01), b"A" * 300, b"ACGT" * 10, b""]
    keys = F.genome_keys(genomes)["kmer"]
    fb = F.auto_filter_bits(len(keys)) if bits is None else bits
    filt = F.build_filter(keys, fb)
    assert F.is_member(filt, keys[keys != 0], fb).all()
    # a filter is not everything: random k-mers mostly miss it
    other = rng.integers(0, 1 << 63, 20000, dtype=np.uint64)
    assert F.is_member(filt, other, fb).mean() < 0.05


def test_expected_survivors():
    rng = np.random.default_rng(8)
    g = _random_read(rng, 20000)
    # reads cut at the sampled offsets of the entry: their first k-mer is a genome key; long reads count whole
    reads = [g[16 * j:16 * j + 100] for j in range(40)] + [_random_read(rng, 100) for _ in range(40)]
    reads += [b"A" * 80, _random_read(rng, 400)]
    recs, n = F.expected_survivors(reads, [g], None, 341)
    assert n == len(recs)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    q, rid = _positions(recs, lens), F.read_index(recs)
    for j in range(40):
        assert (q[rid == j] % 16 == 0).sum() == 5
    assert (rid == 81).sum() == 400 - 31                       # the long read: every k-mer
    assert (rid == 80).sum() == 0                               # k-mer 0
    assert n < 40 * 69 // 4 + 400
    _, n0 = F.expected_survivors(reads, [g], 0, 341)
    assert n0 == len(F.O.extract_kmers(reads, False, 1))
    assert F.env_filter_bits(5) == 20 and F.env_filter_bits(40) == 36 and F.env_filter_bits(-1) == 0
