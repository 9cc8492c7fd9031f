"""CPU tests of tests/sort_ref.py, the host restatement tests/test_gpu_sort_scan.py holds the device sort, scans and
partition to: its digit against arbitrary-precision Python ints, its stable sort against sorted() on tuples and against
the oracle's sortKMers order, and the product's pass lists against the lists written out by hand."""
import numpy as np
import pytest

import sort_ref as R

HAND_WORDS = [0, 1, 0x7F, 0x80, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x01020304, 0xF0E0D0C0, 0x40000000, 0xC0000000, 0x3FFFFFFF]
SHIFTS = [0, 7, 20, 28, 31, 56]


def _py_digit(rec, p):
    """the same digit on Python ints, from the definition in include/kslam.h"""
    word, shift, invert, hi_shift, hi_bits = p
    if len(rec) == 2 and word == 2:
        return (((rec[1] << 32) | rec[0]) >> shift) % 256
    v = rec[word] ^ invert
    lo_bits = 8 - hi_bits
    lo = (v >> shift) % (1 << lo_bits)
    hi = (v >> hi_shift) % (1 << hi_bits)
    return lo + (hi << lo_bits)


def _records(rng, n, rw):
    r = rng.integers(0, 1 << 32, (n, rw), dtype=np.uint64).astype(np.uint32)
    k = min(n, len(HAND_WORDS))
    for c in range(rw):
        r[:k, c] = np.roll(np.array(HAND_WORDS, dtype=np.uint32), c)[:k]
    return r


@pytest.mark.parametrize("rw", [2, 4])
def test_digit_against_python_ints(rw):
    rng = np.random.default_rng(101 + rw)
    recs = _records(rng, 300, rw)
    rows = [[int(x) for x in r] for r in recs]
    passes = []
    for word in range(rw if rw == 2 else 3):
        for shift in SHIFTS:
            if shift >= 32:
                continue
            for invert in (0, 0xFFFFFFFF, 0x80000000):
                passes.append((word, shift, invert, 0, 0))
                for hi_bits in range(1, 8):
                    for hi_shift in (0, 8, 24, 30, 32 - hi_bits):
                        passes.append((word, shift, invert, hi_shift, hi_bits))
    if rw == 2:
        passes += [(2, sh, 0, 0, 0) for sh in SHIFTS + [24, 25, 31, 32, 33, 39, 55]]      # digits that straddle the two words among them
    for p in passes:
        got = R.digit(recs, p)
        assert got.dtype == np.uint64 and int(got.max()) < 256
        assert [int(x) for x in got] == [_py_digit(r, p) for r in rows], p


def test_digit_hand_cases():
    one = np.array([[0x89ABCDEF, 0x01234567]], dtype=np.uint32)
    assert int(R.digit(one, (0, 0, 0, 0, 0))[0]) == 0xEF
    assert int(R.digit(one, (0, 8, 0xFFFFFFFF, 0, 0))[0]) == 0x32          # ~0xCD
    assert int(R.digit(one, (0, 28, 0, 0, 0))[0]) == 0x8                    # nothing above the word
    assert int(R.digit(one, (2, 28, 0, 0, 0))[0]) == 0x78                   # the key 0x0123456789ABCDEF: bits 28 .. 35
    assert int(R.digit(one, (2, 56, 0, 0, 0))[0]) == 0x01
    assert int(R.digit(one, (2, 31, 0, 0, 0))[0]) == (0x0123456789ABCDEF >> 31) & 0xFF
    # the index build's top pass for 9 id bits: id bit 8 below the revComp bit, both inverted
    meta = np.array([[0, 0, 0x80000000 | (1 << 30) | 0x1A5, 0], [0, 0, 0x80000000 | 0x0A5, 0]], dtype=np.uint32)
    top = (2, 8, 0xFFFFFFFF, 30, 1)
    assert [int(x) for x in R.digit(meta, top)] == [(~1 & 0x7F) | (0 << 7), (~0 & 0x7F) | (1 << 7)]


@pytest.mark.parametrize("rw", [2, 4])
@pytest.mark.parametrize("n", [0, 1, 2, 7, 64, 300])
def test_stable_sort_equals_sorted_on_tuples(rw, n):
    rng = np.random.default_rng(5 * n + rw)
    recs = rng.integers(0, 4, (n, rw), dtype=np.uint64).astype(np.uint32) * np.uint32(0x40000081)   # many ties, bits at both ends
    recs[:, rw - 1] = np.arange(n)                                                                    # the original index
    lists = [[(0, 0, 0, 0, 0)], [(0, 0, 0, 0, 0), (0, 24, 0, 0, 0)], [(0, 24, 0x80000000, 0, 0)],
             [(0, 0, 0, 30, 1)], [(0, 0, 0, 0, 0), (0, 8, 0, 0, 0), (0, 16, 0, 0, 0), (0, 24, 0, 0, 0)]]
    if rw == 4:
        lists += [R.full_key_passes(), R.index_passes(300), R.kmer_passes()]
    else:
        lists += [[(2, 28, 0, 0, 0), (2, 36, 0, 0, 0)], R.signed_passes()]
    for pl in lists:
        rows = [tuple(int(x) for x in r) for r in recs]
        exp = sorted(rows, key=lambda r: tuple(_py_digit(r, p) for p in reversed(pl)))     # sorted() is stable
        got = R.stable_sort(recs, pl)
        assert [tuple(int(x) for x in r) for r in got] == exp, pl
        # the composite key and the pass-by-pass form agree
        step = recs
        for p in pl:
            step = step[np.argsort(R.digit(step, p), kind="stable")]
        assert (step == got).all()


def test_argsort_of_a_16_bit_key_is_the_stable_sort_of_its_two_byte_passes():
    """test_gpu_sort_scan.py's case above 256 chunks takes its expected order from a stable argsort of the 16-bit key and
    not from stable_sort's 64-bit composite key (67 million records): the two agree"""
    rng = np.random.default_rng(258)
    n = 300000
    k16 = rng.integers(0, 1 << 10, n, dtype=np.uint16) * np.uint16(61)
    recs = np.stack([k16.astype(np.uint32), np.arange(n, dtype=np.uint32)], axis=1)
    assert np.array_equal(recs[np.argsort(k16, kind="stable")], R.stable_sort(recs, R.entry_passes(0xFFFF)))


def test_full_key_order_is_the_oracles(oracle, kslam):
    rng = np.random.default_rng(77)
    n = 5000
    recs = np.zeros(n, dtype=kslam.KMER_DT)
    recs["kmer"] = rng.integers(0, 300, n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    recs["meta"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    recs["offset"] = np.arange(n)
    exp = oracle.sort_kmers(recs)
    got = R.stable_sort(recs.view(np.uint32).reshape(n, 4), R.full_key_passes()).reshape(-1).view(kslam.KMER_DT)
    assert (got["kmer"] == exp["kmer"]).all() and (got["meta"] == exp["meta"]).all()
    # sortKMers leaves the order of exact ties open (src/KMer.h:392-396); the stable passes keep the input order
    same = (got["kmer"][1:] == got["kmer"][:-1]) & (got["meta"][1:] == got["meta"][:-1])
    assert (got["offset"][1:][same] > got["offset"][:-1][same]).all()


def test_scan_and_partition():
    assert R.excl_scan([])[1] == 0 and len(R.excl_scan([])[0]) == 0
    out, tot = R.excl_scan([3, 0, 0xFFFFFFFF, 0xFFFFFFFF, 1])
    assert [int(x) for x in out] == [0, 3, 3, 3 + 0xFFFFFFFF, 3 + 2 * 0xFFFFFFFF] and tot == 4 + 2 * 0xFFFFFFFF
    big = np.full(3 * (1 << 20), 0xFFFFFFFF, dtype=np.uint32)
    out, tot = R.excl_scan(big)
    assert tot == len(big) * 0xFFFFFFFF and int(out[-1]) == (len(big) - 1) * 0xFFFFFFFF
    lists = R.partition([7, 0, 8, 0, 255, 3, 7])
    assert [list(map(int, l)) for l in lists] == [[1, 3], [], [], [5], [], [], [], [0, 6]]
    assert all(l.dtype == np.uint32 for l in lists)


# ---- the pass lists, written out by hand from the code ---------------------------------------------------------------
KMER = [(0, 0, 0, 0, 0), (0, 8, 0, 0, 0), (0, 16, 0, 0, 0), (0, 24, 0, 0, 0), (1, 0, 0, 0, 0), (1, 8, 0, 0, 0), (1, 16, 0, 0, 0), (1, 24, 0, 0, 0)]
INV = 0xFFFFFFFF


def test_kmer_and_full_key_lists():
    assert R.kmer_passes() == KMER                                                                      # api_index.hip: kmer_passes
    assert R.full_key_passes() == [(2, 0, INV, 0, 0), (2, 8, INV, 0, 0), (2, 16, INV, 0, 0), (2, 24, INV, 0, 0)] + KMER   # api_index.hip: full_key_passes
    assert R.read_kmer_passes(3) == KMER[5:] and R.read_kmer_passes(8) == KMER and R.read_kmer_passes(0) == []   # api_align.hip: kpasses
    assert R.read_kmer_passes(1) == [(1, 24, 0, 0, 0)]


@pytest.mark.parametrize("n_entries,n_passes", [(1, 9), (9, 9), (128, 9), (129, 10), (300, 10), (40000, 11)])
def test_index_list_has_the_passes_the_build_reports(n_entries, n_passes):
    """the counts tests/test_gpu_parity.py::test_index_build_stats_and_the_passes_of_the_one_time_sort asserts"""
    pl = R.index_passes(n_entries)
    assert len(pl) == n_passes and pl[-8:] == KMER


def test_index_lists_by_hand():
    # api_index.hip: build_index -- while (id_bits - at > 7) a whole byte; then {revComp, the remaining id bits}
    assert R.bits_for(0) == 1 and R.bits_for(1) == 1 and R.bits_for(127) == 7 and R.bits_for(128) == 8 and R.bits_for(39999) == 16
    assert R.index_passes(1) == [(2, 0, INV, 30, 1)] + KMER
    assert R.index_passes(128) == [(2, 0, INV, 30, 1)] + KMER
    assert R.index_passes(129) == [(2, 0, INV, 0, 0), (2, 8, INV, 30, 1)] + KMER
    assert R.index_passes(40000) == [(2, 0, INV, 0, 0), (2, 8, INV, 0, 0), (2, 16, INV, 30, 1)] + KMER
    assert R.index_passes_for_id_bits(0) == R.index_passes_for_id_bits(7) == [(2, 0, INV, 30, 1)] + KMER
    assert R.index_passes_for_id_bits(15) == [(2, 0, INV, 0, 0), (2, 8, INV, 30, 1)] + KMER
    assert R.index_passes_for_id_bits(23) == R.index_passes_for_id_bits(17) == [(2, 0, INV, 0, 0), (2, 8, INV, 0, 0), (2, 16, INV, 30, 1)] + KMER
    assert R.index_passes_for_id_bits(30) == [(2, 0, INV, 0, 0), (2, 8, INV, 0, 0), (2, 16, INV, 0, 0), (2, 24, INV, 30, 1)] + KMER
    assert R.index_passes(1 << 30) == R.index_passes_for_id_bits(30)          # the most entries the build takes
    # the order those passes give is sortKMers' on genome records: id and revComp descending inside a k-mer
    rng = np.random.default_rng(3)
    recs = np.zeros((2000, 4), dtype=np.uint32)
    recs[:, 0] = rng.integers(0, 40, 2000)
    recs[:, 2] = 0x80000000 | (rng.integers(0, 2, 2000) << 30) | rng.integers(0, 300, 2000)
    recs[:, 3] = np.arange(2000)
    assert (R.stable_sort(recs, R.index_passes(300)) == R.stable_sort(recs, R.full_key_passes())).all()


def test_filter_overlap_and_pair_lists_by_hand():
    # filter.hip: for (sh = 20 + FBLK_BITS; sh <= 20 + piece_bits; sh += 8), piece_bits = log2_bits - 10 + 3, FBLK_BITS = 11
    assert R.filter_passes(20) == [(2, 31, 0, 0, 0)]
    assert R.filter_passes(28) == [(2, 31, 0, 0, 0), (2, 39, 0, 0, 0)]
    assert R.filter_passes(32) == [(2, 31, 0, 0, 0), (2, 39, 0, 0, 0)]
    assert R.filter_passes(32, start=20) == [(2, 20, 0, 0, 0), (2, 28, 0, 0, 0), (2, 36, 0, 0, 0), (2, 44, 0, 0, 0)]
    assert R.filter_passes(32, start=28) == [(2, 28, 0, 0, 0), (2, 36, 0, 0, 0), (2, 44, 0, 0, 0)]
    # api_align.hip a-6: for (sh = low_bits; sh < key_bits; sh += 8) with low_bits = bits_rel + 1, or the key's bytes
    assert R.overlap_passes(17, 11, 20, True) == [(2, 21, 0, 0, 0), (2, 29, 0, 0, 0), (2, 37, 0, 0, 0), (2, 45, 0, 0, 0)]
    assert R.overlap_passes(17, 11, 20, False) == KMER[:7]
    assert R.overlap_passes(10, 1, 12, False) == KMER[:3]
    # pairs.hip: pseudo_on_records / max_allowed_insert_device / pseudo_route
    assert R.entry_passes(0) == R.entry_passes(255) == KMER[:1]
    assert R.entry_passes(256) == KMER[:2] and R.entry_passes(1 << 16) == KMER[:3] and R.entry_passes(0xFFFFFFFF) == KMER[:4]
    assert R.signed_passes() == [(0, 0, 0x80000000, 0, 0), (0, 8, 0x80000000, 0, 0), (0, 16, 0x80000000, 0, 0), (0, 24, 0x80000000, 0, 0)]
    assert R.route_passes() == [(0, 0, 0, 0, 0)]
    # signed order: negative numbers first
    v = np.array([5, -1, 0, -2**31, 2**31 - 1, -7], dtype=np.int32)
    recs = np.stack([v.view(np.uint32), np.arange(len(v), dtype=np.uint32)], axis=1)
    assert [int(x) for x in R.stable_sort(recs, R.signed_passes())[:, 0].view(np.int32)] == sorted(int(x) for x in v)
