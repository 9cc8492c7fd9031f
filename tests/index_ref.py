"""A plain numpy restatement of the one-time genome index build (k-slam_amd/csrc/api_index.hip: build_index).

Written from the definition -- the reference's src/KMer.h (getKMers_parallel :190-241, the base codes :246-268, the
canonical choice :173, sortKMers :388-398), src/SLAM.h:64 (gap k/2) and src/ssw_cpp.cpp:11-23 (the SSW base table) as the
kernels' comments cite them -- and not from the kernels: no segments, no digit bytes, no radix passes, no blocks.  What
kslam_debug_index_export (include/kslam.h) returns is compared with this, table by table and bit for bit
(tests/test_gpu_index_build.py); tests/test_index_ref.py holds this module to the oracle and to values written out by hand.

Only three things are restated from build_index itself, because they are choices of the build and not of the reference:
the bucket table's width (bucket_bits), the filter's size (filter_ref.auto_filter_bits / env_filter_bits) and the byte
code of g_codes.

Test infrastructure only (CPU, numpy).
"""
import numpy as np

import filter_ref as F
import join_ref as J

K = 32
GAP = K // 2                     # src/SLAM.h:64
U64 = np.uint64
KMER_DT = J.KMER_DT
FROM_GENBANK = 0x80000000        # src/KMer.h:65-67: meta = id | revComp << 30 | isFromGenbank << 31
REVCOMP = 0x40000000
BUCKET_BITS_MAX = 27             # common.h: Tuning::bucket_bits_max (KSLAM_BUCKET_BITS)

# A 0, C 1, T 2, G 3; anything else, lower case included, is 0 (src/KMer.h:246-268)
KMER_CODE = np.zeros(256, dtype=np.uint64)
for _ch, _v in ((b"A", 0), (b"C", 1), (b"T", 2), (b"G", 3)):
    KMER_CODE[_ch[0]] = _v

# g_codes (common.h: encode_bases): bits 0-2 the SSW code -- A 0, C 1, G 2, T 3, U 0, either case, anything else 4
# (src/ssw_cpp.cpp:11-23; bytes of 128 and above are outside the reference's table and are not used by any test) -- and
# bit 3 "inPlaceReverseComplement complements this base": upper-case A, C, G, T only (src/sequenceTools.h:98-116)
BASE_CODE = np.full(256, 4, dtype=np.uint8)
for _ch, _v in ((b"A", 0), (b"C", 1), (b"G", 2), (b"T", 3), (b"U", 0)):
    BASE_CODE[_ch[0]] = _v
    BASE_CODE[_ch.lower()[0]] = _v
for _ch in b"ACGT":
    BASE_CODE[_ch] |= 8


def offsets(entries):
    off = np.zeros(len(entries) + 1, dtype=np.uint64)
    if len(entries):
        np.cumsum([len(e) for e in entries], out=off[1:])
    return off


def base_codes(entries):
    """g_codes over [0, total bases)"""
    return BASE_CODE[np.frombuffer(b"".join(entries), dtype=np.uint8)]


def kmers_per_entry(entries):
    return np.array([(len(e) - K) // GAP + 1 if len(e) >= K else 0 for e in entries], dtype=np.int64)


def records(entries):
    """The genome k-mer records in extraction order: every 16th offset of every entry with at least 32 bases.
    fwd holds the first base in its highest bits; rc is the complement (code ^ 2) read backwards.  The canonical strand
    is forward iff fwd < rc -- a palindrome takes the rc branch and sets bit 30 -- and offset = pos on both strands."""
    nk = kmers_per_entry(entries)
    m = int(nk.sum())
    out = np.zeros(m, dtype=KMER_DT)
    if m == 0:
        return out
    cat = KMER_CODE[np.frombuffer(b"".join(entries), dtype=np.uint8)]
    off = offsets(entries).astype(np.int64)
    ident = np.repeat(np.arange(len(entries), dtype=np.int64), nk)
    first = np.cumsum(nk) - nk                                          # records before each entry
    pos = (np.arange(m, dtype=np.int64) - np.repeat(first, nk)) * GAP
    start = off[ident] + pos
    fwd = np.zeros(m, dtype=U64)
    rc = np.zeros(m, dtype=U64)
    for j in range(K):
        c = cat[start + j]
        fwd |= c << U64(2 * (K - 1 - j))
        rc |= (c ^ U64(2)) << U64(2 * j)
    is_fwd = fwd < rc
    out["kmer"] = np.where(is_fwd, fwd, rc)
    out["meta"] = (FROM_GENBANK | ident | np.where(is_fwd, 0, REVCOMP)).astype(np.uint32)
    out["offset"] = pos.astype(np.uint32)
    return out


def order(recs):
    """sortKMers' order made total: k-mer ascending, then meta descending; ties keep the extraction order, because every
    radix pass is stable.  Two stable sorts, the minor key first."""
    by_meta = np.argsort(~recs["meta"], kind="stable")
    return by_meta[np.argsort(recs["kmer"][by_meta], kind="stable")]


def bucket_bits(m, bits_max=BUCKET_BITS_MAX, exact=None):
    """build_index: start at 8, grow while m >> (bits + 2) is non-zero up to the tuning's maximum; or
    KSLAM_BUCKET_BITS_EXACT as read_tuning clamps it (8..28)"""
    if exact:
        return min(28, max(8, int(exact)))
    bits = 8
    while bits < bits_max and (m >> (bits + 2)) != 0:
        bits += 1
    return bits


def filter_bits(m, env=None):
    """env: None = the automatic size, otherwise what KSLAM_FILTER_BITS is set to"""
    return F.auto_filter_bits(m) if env is None else F.env_filter_bits(env)


def build(entries, bucket_exact=None, filter_env=None, sorted_recs=None):
    """Everything kslam_debug_index_export returns, by the same names.  sorted_recs: the records of an earlier build of the
    same entries (the columns do not depend on the two settings)."""
    if sorted_recs is None:
        recs = records(entries)
        sorted_recs = recs[order(recs)]
    s = sorted_recs
    m = len(s)
    bb = bucket_bits(m, exact=bucket_exact)
    fb = filter_bits(m, filter_env)
    return {"n_entries": len(entries), "n_genome_kmers": m, "n_bases": sum(len(e) for e in entries),
            "bucket_bits": bb, "filter_bits": fb, "offsets": offsets(entries), "codes": base_codes(entries),
            "keys": s["kmer"].copy(), "meta": s["meta"].copy(), "offset": s["offset"].copy(),
            "bucket": J.bucket_table(s["kmer"], bb),
            "filter": F.build_filter(s["kmer"], fb) if fb else np.zeros(0, dtype=np.uint32),
            "records": s}


TABLES = ("offsets", "codes", "keys", "meta", "offset", "bucket", "filter")
SCALARS = ("n_entries", "n_genome_kmers", "n_bases", "bucket_bits", "filter_bits")


def first_difference(got, exp):
    """None when the two exports agree, else (name of the first table or size that differs, position, got, expected)"""
    for k in SCALARS:
        if int(got[k]) != int(exp[k]):
            return (k, None, int(got[k]), int(exp[k]))
    for k in TABLES:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        if g.shape != e.shape:
            return (k, "length", g.shape, e.shape)
        bad = np.flatnonzero(g != e)
        if len(bad):
            i = int(bad[0])
            return (k, i, int(g[i]), int(e[i]), "%d positions differ" % len(bad))
    return None


# ---- what the families of tests/index_seams.py are asked to reach (tests/test_index_ref.py) ------------------------------
def key_groups(s):
    """(start, end) of every equal-k-mer group of the sorted records"""
    if len(s) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    cut = np.flatnonzero(s["kmer"][1:] != s["kmer"][:-1]) + 1
    return np.concatenate([[0], cut]), np.concatenate([cut, [len(s)]])


def groups_differing(s, values):
    """the number of equal-k-mer groups whose members do not all share values[i]"""
    lo, hi = key_groups(s)
    if len(lo) == 0:
        return 0
    v = np.asarray(values)
    change = np.concatenate([[0], np.cumsum(v[1:] != v[:-1])])        # changes of the value up to each record
    return int(np.sum(change[hi - 1] - change[lo] > 0))


def longest_equal_record_run(s):
    """the longest run of equal (kmer, meta), and whether its offsets ascend"""
    if len(s) == 0:
        return 0, True
    same = (s["kmer"][1:] == s["kmer"][:-1]) & (s["meta"][1:] == s["meta"][:-1])
    cut = np.concatenate([[0], np.flatnonzero(~same) + 1, [len(s)]])
    i = int(np.argmax(np.diff(cut)))
    a, b = int(cut[i]), int(cut[i + 1])
    return b - a, bool((np.diff(s["offset"][a:b].astype(np.int64)) > 0).all())


def longest_empty_bucket_run(table):
    """the longest run of consecutive empty buckets of a table of lower bounds"""
    empty = np.diff(table.astype(np.int64)) == 0
    edge = np.flatnonzero(np.diff(np.concatenate([[0], empty.astype(np.int8), [0]])))
    return int((edge[1::2] - edge[::2]).max()) if len(edge) else 0


def filter_block_words(keys, log2_bits):
    """the distinct non-zero keys each filter block of 2^11 pieces receives (filter.hip: one workgroup per block)"""
    k = np.unique(np.asarray(keys, dtype=np.uint64))
    k = k[k != 0]
    piece, _bits = F.probe(k, log2_bits - 10)
    n_blocks = 1 << (log2_bits - 10 + 3 - 11)
    return np.bincount((piece >> U64(11)).astype(np.int64), minlength=n_blocks)
