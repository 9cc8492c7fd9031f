"""A plain numpy restatement of the three device primitives every stage stands on: the LSD radix sort
(k-slam_amd/csrc/radix_sort.hip), the exclusive scans and the 8-way partition by bin (k-slam_amd/csrc/scan.hip).

A radix pass is (word, shift, invert, hi_shift, hi_bits), as kslam_sort_pass in include/kslam.h.  The sort is stated as
what stable passes, least significant first, must produce -- one stable argsort by the composite key -- so that a test
can demand the device's output byte for byte, tie order included.  The pass lists the product builds are restated here
from the code, each with the line it comes from; tests/test_sort_ref.py pins them.

Test infrastructure only (CPU, numpy).
"""
import numpy as np

SORT_TILE = 4096        # common.h: records per workgroup of a pass
CHUNK_TILES = 64        # radix_sort.hip: tiles per first-level scan chunk
FBLK_BITS = 11          # filter.hip: log2 of the 16-byte pieces per filter block
U64 = np.uint64


def bits_for(max_value):
    """api_core.hip: bits_for -- bits needed for max_value, at least 1"""
    b = 1
    while b < 64 and (max_value >> b) != 0:
        b += 1
    return b


def digit(words, p):
    """The 8-bit digit of pass p of every record: words is uint32 [n, 2 or 4] (common.h: sort_pass_digit,
    radix_sort.hip: digit_of).  Returned as uint64."""
    word, shift, invert, hi_shift, hi_bits = (int(x) for x in p)
    w = np.asarray(words, dtype=np.uint32).astype(U64)
    if w.shape[1] == 2 and word == 2:        # the digit of the whole 64-bit key, whatever words it straddles
        key = (w[:, 1] << U64(32)) | w[:, 0]
        return (key >> U64(shift)) & U64(0xFF)
    v = w[:, word] ^ U64(invert)
    if hi_bits == 0:
        return (v >> U64(shift)) & U64(0xFF)
    lo_bits = 8 - hi_bits
    lo = (v >> U64(shift)) & U64((1 << lo_bits) - 1)
    hi = (v >> U64(hi_shift)) & U64((1 << hi_bits) - 1)
    return lo | (hi << U64(lo_bits))


def stable_sort(records, passes):
    """records (uint32 [n, 2 or 4]) after the stable passes, passes[0] least significant."""
    records = np.asarray(records, dtype=np.uint32)
    if len(passes) == 0 or len(records) == 0:
        return records.copy()
    if len(passes) <= 8:      # one composite key of at most 64 bits, the last pass on top
        key = np.zeros(len(records), dtype=U64)
        for p in reversed(passes):
            key = (key << U64(8)) | digit(records, p)
        return records[np.argsort(key, kind="stable")]
    out = records
    for p in passes:          # more than 64 bits of key: the stable passes themselves
        out = out[np.argsort(digit(out, p), kind="stable")]
    return out


def excl_scan(v):
    """(exclusive sums as uint64, total) of uint32 values: exact, the sums stay far below 2^64"""
    v = np.asarray(v, dtype=np.uint32).astype(U64)
    inc = np.cumsum(v, dtype=U64)
    out = np.zeros(len(v), dtype=U64)
    out[1:] = inc[:-1]
    return out, (int(inc[-1]) if len(v) else 0)


def partition(bins):
    """the 8 lists of partition_bins: the element numbers of each bin below 8, ascending"""
    bins = np.asarray(bins, dtype=np.uint8)
    return [np.flatnonzero(bins == k).astype(np.uint32) for k in range(8)]


# ---- the pass lists the product builds -------------------------------------------------------------------------------
def kmer_passes():
    """api_index.hip: kmer_passes -- the 8 bytes of the k-mer in words 0 and 1"""
    return [(w, 8 * b, 0, 0, 0) for w in range(2) for b in range(4)]


def full_key_passes():
    """api_index.hip: full_key_passes -- the 4 bytes of the inverted meta word, then the k-mer"""
    return [(2, 8 * b, 0xFFFFFFFF, 0, 0) for b in range(4)] + kmer_passes()


def index_passes_for_id_bits(id_bits):
    """api_index.hip: build_index -- whole id bytes while more than 7 id bits remain, then the rest below the revComp bit"""
    out, at = [], 0
    while id_bits - at > 7:
        out.append((2, at, 0xFFFFFFFF, 0, 0))
        at += 8
    out.append((2, at, 0xFFFFFFFF, 30, 1))
    return out + kmer_passes()


def index_passes(n_entries):
    """api_index.hip: build_index -- id_bits = bits_for(n - 1)"""
    return index_passes_for_id_bits(bits_for(n_entries - 1 if n_entries else 0))


def read_kmer_passes(nbytes):
    """api_align.hip: kpasses -- the top nbytes bytes of the k-mer"""
    return [(b // 4, 8 * (b % 4), 0, 0, 0) for b in range(8 - nbytes, 8)]


def filter_passes(log2_bits, start=20 + FBLK_BITS):
    """filter.hip: filter_build_sorted -- 64-bit key digits from bit 20 + FBLK_BITS up to bit 20 + piece_bits"""
    piece_bits = log2_bits - 10 + 3
    return [(2, sh, 0, 0, 0) for sh in range(start, 20 + piece_bits + 1, 8)]


def overlap_passes(bits_read, bits_entry, bits_rel, grouped):
    """api_align.hip: a-6 -- the key bits above rel and revComp (grouped), or every byte of the key"""
    key_bits = bits_read + bits_entry + bits_rel + 1
    if grouped:
        return [(2, sh, 0, 0, 0) for sh in range(bits_rel + 1, key_bits, 8)]
    return [(b // 4, 8 * (b % 4), 0, 0, 0) for b in range((key_bits + 7) // 8)]


def entry_passes(max_entry):
    """pairs.hip: pseudo_on_records -- the bytes of word 0 that the largest entry number needs (1 to 4 passes)"""
    bits = 1
    while bits < 32 and (max_entry >> bits):
        bits += 1
    return [(0, 8 * b, 0, 0, 0) for b in range((bits + 7) // 8)]


def signed_passes():
    """pairs.hip: max_allowed_insert_device -- word 0 as a signed number"""
    return [(0, 8 * b, 0x80000000, 0, 0) for b in range(4)]


def route_passes():
    """pairs.hip: pseudo_route -- one pass over the low byte of word 0"""
    return [(0, 0, 0, 0, 0)]
