"""ctypes plumbing for include/kslam_alignqc.h: the alignment QC report (error rate by cycle and by base quality, substitution
spectrum, indel lengths, edit distance and identity per alignment, insert sizes) tallied per cycle on the GPU, its host twin, the
JSON writer and a parser for the file."""
import ctypes as C
import json

import numpy as np

from . import tail as _T
from . import variants as _V

# every symbol include/kslam_alignqc.h declares
EXPORTS = ["kslam_align_qc_add", "kslam_align_qc_kernel_ms", "kslam_align_qc_release", "kslam_align_qc_reset", "kslam_align_qc_take",
           "kslam_align_qc_write", "kslam_get_align_qc", "kslam_set_align_qc", "kslam_stream_get_align_qc", "kslam_stream_set_align_qc",
           "kslam_tail_align_qc", "kslam_tail_align_qc_free"]
DEFAULT_CYCLES, MAX_CYCLES = 512, 65536
QUAL_COLS, CYCLE_COLS, LEN_BINS, NM_BINS, IDENTITY_BINS, INSERT_BINS = 95, 4, 65, 65, 101, 1002
SCALARS = ("n_records", "n_reverse", "n_skipped", "n_without_quality", "m_columns", "compared", "mismatches", "ins_events", "ins_bases",
           "del_events", "del_bases", "unaligned_bases")
PAIR_SCALARS = ("n_read_pairs", "pairs_both", "pairs_r1_only", "pairs_r2_only", "insert_sum")
REPORT_WORDS = 6 + INSERT_BINS


def stream_words(cycles):
    """KSLAM_ALIGN_QC_STREAM_WORDS"""
    return len(SCALARS) + 16 + 2 * LEN_BINS + NM_BINS + IDENTITY_BINS + (cycles + 1) * (CYCLE_COLS + 2 * QUAL_COLS)


def words(cycles):
    """KSLAM_ALIGN_QC_WORDS: the block's 64-bit words for `cycles` per-cycle rows"""
    return REPORT_WORDS + 2 * stream_words(cycles)


def _stream_tables(cycles):
    return (("subst", 16), ("ins_len", LEN_BINS), ("del_len", LEN_BINS), ("nm", NM_BINS), ("identity", IDENTITY_BINS),
            ("cycle", (cycles + 1) * CYCLE_COLS), ("cq_compared", (cycles + 1) * QUAL_COLS), ("cq_mismatch", (cycles + 1) * QUAL_COLS))


class StreamView(C.Structure):
    """kslam_align_qc_stream"""
    _fields_ = [(n, C.c_uint64) for n in SCALARS] + [(n, C.c_void_p) for n in ("subst", "ins_len", "del_len", "nm", "identity", "cycle", "cq_compared",
                                                                                 "cq_mismatch")]


class Tables(C.Structure):
    """kslam_align_qc_tables"""
    _fields_ = [("max_cycles", C.c_uint32), ("paired", C.c_int32), ("n_words", C.c_uint64), ("block", C.c_void_p)] + \
               [(n, C.c_uint64) for n in PAIR_SCALARS] + [("insert", C.c_void_p), ("stream", StreamView * 2)]


_ready = False


def lib():
    global _ready
    L = _V.lib()
    if not _ready:
        vp, u64, u32, P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
        batch = [vp, u64, vp, u64, vp, vp, u64, vp, u64, vp, u64]   # overlaps, pool, read bases + offsets, read pairs, pairs
        L.kslam_set_align_qc.argtypes = [vp, C.c_int, u32]
        L.kslam_get_align_qc.argtypes = [vp, P(C.c_int), P(u32)]
        L.kslam_align_qc_reset.argtypes = [vp]
        L.kslam_align_qc_add.argtypes = [vp] + batch + [vp, C.c_int]
        L.kslam_align_qc_take.argtypes = [vp, P(Tables)]
        L.kslam_align_qc_release.argtypes = [vp, P(Tables)]
        L.kslam_align_qc_release.restype = None
        L.kslam_align_qc_kernel_ms.argtypes = [vp, P(C.c_double)]
        L.kslam_tail_align_qc.argtypes = [vp, vp, u64] + batch + [vp, C.c_int, u32, P(Tables)]
        L.kslam_tail_align_qc_free.argtypes = [P(Tables)]
        L.kslam_tail_align_qc_free.restype = None
        L.kslam_align_qc_write.argtypes = [P(Tables), C.c_int]
        L.kslam_stream_set_align_qc.argtypes = [vp, C.c_int, u32]
        L.kslam_stream_get_align_qc.argtypes = [vp, P(C.c_int), P(u32)]
        _ready = True
    return L


def unpack(block, cycles, paired):
    """a block of words(cycles) uint64 -> {"max_cycles", "paired", the pair counters, "insert", "streams": [dict, dict]}; every
    table a list of ints"""
    block = np.asarray(block, dtype=np.uint64)
    assert len(block) == words(cycles)
    out = {"max_cycles": int(cycles), "paired": bool(paired)}
    for k, name in enumerate(PAIR_SCALARS):
        out[name] = int(block[k])
    out["insert"] = block[6:REPORT_WORDS].tolist()
    out["streams"] = []
    for z in range(2):
        w = block[REPORT_WORDS + z * stream_words(cycles):REPORT_WORDS + (z + 1) * stream_words(cycles)]
        s = {name: int(w[k]) for k, name in enumerate(SCALARS)}
        at = len(SCALARS)
        for key, n in _stream_tables(cycles):
            s[key] = w[at:at + n].tolist()
            at += n
        out["streams"].append(s)
    return out


def pack(tables):
    """the inverse of unpack: -> (block as a uint64 array, cycles, paired)"""
    cycles = tables["max_cycles"]
    parts = [[tables[n] for n in PAIR_SCALARS] + [0] + list(tables["insert"])]
    for s in tables["streams"]:
        part = [s[n] for n in SCALARS]
        for key, _ in _stream_tables(cycles):
            part += list(s[key])
        parts.append(part)
    block = np.array([v for p in parts for v in p], dtype=np.uint64)
    assert len(block) == words(cycles)
    return block, cycles, bool(tables["paired"])


def _tables_out(t):
    block = _T.rows_at(t.block, int(t.n_words), np.dtype(np.uint64))
    return unpack(block, int(t.max_cycles), t.paired)


def _quality(read_quality, n_bytes):
    if read_quality is None:
        return None, None
    q = np.ascontiguousarray(np.frombuffer(read_quality, dtype=np.uint8) if isinstance(read_quality, (bytes, bytearray)) else read_quality, dtype=np.uint8)
    if len(q) != n_bytes:
        raise ValueError("the quality column has the layout of the bases")
    q = np.concatenate([q, np.zeros(1, dtype=np.uint8)])   # (an empty column still has an address)
    return q, q.ctypes.data


def set_align_qc(ctx, on=True, max_cycles=0):
    """kslam_set_align_qc: needs an index, ctx.set_pairing and a context with report_cigar; switching on zeroes the tables
    (max_cycles 0 = 512), off frees them"""
    ctx._chk(lib().kslam_set_align_qc(ctx._h, int(on), int(max_cycles)))


def get_align_qc(ctx):
    """-> (on, max_cycles as resolved; 0 when off)"""
    on, c = C.c_int(), C.c_uint32()
    ctx._chk(lib().kslam_get_align_qc(ctx._h, C.byref(on), C.byref(c)))
    return bool(on.value), int(c.value)


def reset(ctx):
    ctx._chk(lib().kslam_align_qc_reset(ctx._h))


def add(ctx, overlaps, cigar_pool, read_bases, read_offsets, read_pairs, pairs, read_quality=None, paired=False):
    """kslam_align_qc_add: one batch's arrays from the host (as kslam_amd.variants.add) with the quality column laid out like the
    bases (None: the batch has none)"""
    keep, args = _V._arrays(overlaps, cigar_pool, read_bases, read_offsets, read_pairs, pairs)
    q, qp = _quality(read_quality, len(keep[2]))
    ctx._chk(lib().kslam_align_qc_add(ctx._h, *args, qp, int(paired)))


def take(ctx):
    """kslam_align_qc_take -> the tables as unpack() gives them"""
    L = lib()
    t = Tables()
    ctx._chk(L.kslam_align_qc_take(ctx._h, C.byref(t)))
    try:
        return _tables_out(t)
    finally:
        L.kslam_align_qc_release(ctx._h, C.byref(t))


def kernel_ms(ctx):
    """device ms of the last kslam_align_qc_add's count pass"""
    ms = C.c_double()
    ctx._chk(lib().kslam_align_qc_kernel_ms(ctx._h, C.byref(ms)))
    return float(ms.value)


def tail_align_qc(entry_bases, entry_offsets, overlaps, cigar_pool, read_bases, read_offsets, read_pairs, pairs, read_quality=None, paired=False,
                  max_cycles=0):
    """kslam_tail_align_qc (host twin) -> the tables"""
    L = lib()
    gb = np.ascontiguousarray(np.frombuffer(entry_bases, dtype=np.uint8) if isinstance(entry_bases, (bytes, bytearray)) else entry_bases, dtype=np.uint8)
    go = np.ascontiguousarray(entry_offsets, dtype=np.uint64)
    keep, args = _V._arrays(overlaps, cigar_pool, read_bases, read_offsets, read_pairs, pairs)
    q, qp = _quality(read_quality, len(keep[2]))
    n_entries = max(len(go) - 1, 0)
    t = Tables()
    _T._chk(L.kslam_tail_align_qc(gb.ctypes.data if len(gb) else None, go.ctypes.data if n_entries else None, n_entries, *args, qp, int(paired),
                                  int(max_cycles), C.byref(t)))
    try:
        return _tables_out(t)
    finally:
        L.kslam_tail_align_qc_free(C.byref(t))


def write(tables, fd):
    """kslam_align_qc_write: tables as unpack() gives them"""
    block, cycles, paired = pack(tables)
    t = Tables()
    t.max_cycles, t.paired, t.n_words, t.block = cycles, int(paired), words(cycles), block.ctypes.data
    _T._chk(lib().kslam_align_qc_write(C.byref(t), int(fd)))


def report_bytes(tables):
    """the file as bytes (through a temporary descriptor)"""
    return _T.fd_bytes("kslam_align_qc", lambda fd: write(tables, fd))


def stream_set_align_qc(ctx, fd, max_cycles=0):
    """kslam_stream_set_align_qc: the descriptor the NEXT kslam_stream_classify on ctx writes its report to (-1: none)"""
    ctx._chk(lib().kslam_stream_set_align_qc(ctx._h, int(fd) if fd is not None else -1, int(max_cycles)))


def parse(text):
    """the file -> dict: json.loads with the ratio strings turned into floats (insert_size_median stays the string it is) and the
    keys of the count maps into ints (">64", "64+", ">1000" and "invalid" stay strings)"""
    if isinstance(text, bytes):
        text = text.decode()
    doc = json.loads(text)
    if doc.get("kslam_align_qc") != 1:
        raise ValueError("not an alignment QC report of format 1")

    def num_keys(d):
        return {(int(k) if k.isdigit() else k): v for k, v in d.items()}

    def ratios(d):
        for k, v in list(d.items()):
            if isinstance(v, str) and k != "insert_size_median":
                d[k] = float(v)
    ratios(doc["summary"])
    for name in ("read1", "read2"):
        if name not in doc:
            continue
        s = doc[name]
        ratios(s)
        s["mismatch_rate_by_cycle"] = [float(x) for x in s["mismatch_rate_by_cycle"]]
        s["by_quality"] = {k: [v[0], v[1], float(v[2])] for k, v in num_keys(s["by_quality"]).items()}
        for k in ("insertion_lengths", "deletion_lengths", "edit_distance_counts", "identity_counts"):
            s[k] = num_keys(s[k])
    doc["insert_size_counts"] = num_keys(doc["insert_size_counts"])
    return doc
