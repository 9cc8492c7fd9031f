"""A plain host restatement of the k-mer join and the overlap dedupe (numpy and Python loops, test infrastructure only).

Written from the reference's src/Overlap.h as k-slam_amd/csrc/join.hip's header cites it -- processPileUp (:153-199),
findOverlaps (:230-246), overlapSort / overlapEqual (:79-98) and the sort + std::unique of findOverlaps_parallel (:289-291)
-- and not from the kernels: no bucket shortcut, no piece, no run decomposition, no per-group walk.  What the hooks
kslam_debug_join / kslam_debug_overlap_unique (include/kslam.h) return is compared with this, exactly.

Records are KMER_DT = {kmer u8, meta u4, offset u4}, meta = id | revComp << 30 | isFromGenbank << 31 (src/KMer.h:65-67).
A layout is (bits_read, bits_entry, bits_rel, rel_bias); the packed key is
    read << (bits_entry + bits_rel + 1) | entry << (bits_rel + 1) | (rel + rel_bias) << 1 | revComp.
"""
import numpy as np

KMER_DT = np.dtype([("kmer", "<u8"), ("meta", "<u4"), ("offset", "<u4")])
OVERLAP_DT = np.dtype([("read", "<u4"), ("entry", "<u4"), ("rel", "<i4"), ("revcomp", "u1"), ("pad", "u1"), ("score", "<u2"),
                       ("ref_begin", "<i4"), ("ref_end", "<i4"), ("query_begin", "<i4"), ("query_end", "<i4"),
                       ("cigar_len", "<u4"), ("pad2", "<u4"), ("cigar_off", "<u8")])
assert OVERLAP_DT.itemsize == 48
K = 32
ID_MASK = 0x3FFFFFFF
SENTINEL = np.uint64(0xEEEEEEEEEEEEEEEE)           # kslam.h: KSLAM_DEBUG_SENTINEL_BYTE in every byte
SENTINEL32 = np.uint32(0xEEEEEEEE)


def bucket_table(keys, bits):
    """[2^bits + 1] lower bounds of the sorted keys by their top `bits` bits"""
    b = np.asarray(keys, dtype=np.uint64) >> np.uint64(64 - bits)
    return np.searchsorted(b, np.arange((1 << bits) + 1, dtype=np.uint64), side="left").astype(np.uint32)


def pack(read, entry, rel, revcomp, layout):
    """one packed key (Python ints)"""
    _br, be, bl, bias = layout
    relb = rel + bias
    assert 0 <= relb < (1 << bl) and 0 <= entry < (1 << be)
    return (read << (be + bl + 1)) | (entry << (bl + 1)) | (relb << 1) | int(revcomp)


def unpack(key, layout):
    """-> (read, entry, rel, revcomp) of one packed key"""
    _br, be, bl, bias = layout
    key = int(key)
    return key >> (be + bl + 1), (key >> (bl + 1)) & ((1 << be) - 1), ((key >> 1) & ((1 << bl) - 1)) - bias, key & 1


def genome_runs(genome):
    """key -> (first index, count) of the sorted genome records"""
    runs = {}
    for i, k in enumerate(genome["kmer"].tolist()):
        lo, c = runs.get(k, (i, 0))
        runs[k] = (lo, c + 1)
    return runs


def run_counts(genome, reads):
    """per read record: the number of genome records it meets (0 for k-mer 0, Overlap.h:236)"""
    runs = genome_runs(genome)
    return np.array([0 if k == 0 else runs.get(k, (0, 0))[1] for k in reads["kmer"].tolist()], dtype=np.int64)


def join(genome, reads, read_len, layout):
    """Every read record with k-mer != 0 (Overlap.h:236-239) against every genome record of the same k-mer
    (Overlap.h:175-197): the packed keys as a SORTED uint64 array -- the join's output is a multiset."""
    runs = genome_runs(genome)
    gid = (genome["meta"] & np.uint32(ID_MASK)).astype(np.int64)
    grc = ((genome["meta"] >> np.uint32(30)) & np.uint32(1)).astype(np.int64)
    goff = genome["offset"].astype(np.int64)
    _br, be, bl, bias = layout
    out = []
    for k, meta, roff in zip(reads["kmer"].tolist(), reads["meta"].tolist(), reads["offset"].tolist()):
        if k == 0 or k not in runs:
            continue
        lo, c = runs[k]
        rid, rrc = meta & ID_MASK, (meta >> 30) & 1
        L = int(read_len[rid])
        g_rc = grc[lo:lo + c]
        off = np.where(g_rc == 1, L - roff - K, roff)                               # Overlap.h:185-189
        rel = (goff[lo:lo + c] - off).astype(np.uint32).astype(np.int32).astype(np.int64)      # int32(g.offset - off), :192
        relb = rel + bias
        assert (relb >= 0).all() and (relb < (1 << bl)).all(), "the layout cannot hold this rel"
        rev = (g_rc != rrc).astype(np.uint64)                                       # !sameComp
        out.append((np.uint64(rid) << np.uint64(be + bl + 1)) | (gid[lo:lo + c].astype(np.uint64) << np.uint64(bl + 1)) |
                   (relb.astype(np.uint64) << np.uint64(1)) | rev)
    if not out:
        return np.zeros(0, dtype=np.uint64)
    return np.sort(np.concatenate(out))


def unique_flags(sorted_keys, layout):
    """std::unique with overlapEqual (Overlap.h:79-85, 290) over the fully sorted list: an element is dropped iff it has
    the read and entry of the last KEPT element and |rel - its rel| < 3.  -> bool keep flag per key.

    The list is sorted by the whole packed key, so revComp -- the least significant bit, false first -- breaks the tie of
    equal (read, entry, rel).  That tie order is this project's and not the reference's: overlapSort has no revComp in
    its key and the reference's sort is unstable there (DESIGN.md on the unstable tie)."""
    keep = np.zeros(len(sorted_keys), dtype=bool)
    last = None
    for i, k in enumerate(np.asarray(sorted_keys, dtype=np.uint64).tolist()):
        r, e, rel, _rc = unpack(k, layout)
        if last is not None and last[0] == r and last[1] == e and abs(rel - last[2]) < 3:
            continue
        keep[i] = True
        last = (r, e, rel)
    return keep


def has_big_group(keys, layout, cap=64):
    """True iff some (read, entry) holds more than `cap` keys"""
    if len(keys) == 0:
        return False
    hi = np.asarray(keys, dtype=np.uint64) >> np.uint64(layout[2] + 1)
    return bool(np.unique(hi, return_counts=True)[1].max() > cap)


def rows(kept_keys, layout, read_id_base):
    """the 48-byte rows of the kept keys: read + read_id_base, entry, rel, revcomp; every other field zero"""
    out = np.zeros(len(kept_keys), dtype=OVERLAP_DT)
    for i, k in enumerate(np.asarray(kept_keys, dtype=np.uint64).tolist()):
        r, e, rel, rc = unpack(k, layout)
        out[i]["read"], out[i]["entry"], out[i]["rel"], out[i]["revcomp"] = r + read_id_base, e, rel, rc
    return out


def unique_rows(keys, layout, read_id_base):
    """any order of keys -> (fully sorted keys, keep flags, rows)"""
    s = np.sort(np.asarray(keys, dtype=np.uint64))
    f = unique_flags(s, layout)
    return s, f, rows(s[f], layout, read_id_base)
