"""ctypes plumbing for include/kslam_readqc.h: the read QC report (reads and bases taken in, lengths, base content and quality
per cycle, mean quality per read, GC content) tallied per cycle on the GPU, its host twin, the JSON writer and a parser for the
file."""
import ctypes as C
import json

import numpy as np

from . import tail as _T

# every symbol include/kslam_readqc.h declares
EXPORTS = ["kslam_get_read_qc", "kslam_read_qc_add", "kslam_read_qc_kernel_ms", "kslam_read_qc_release", "kslam_read_qc_reset",
           "kslam_read_qc_take", "kslam_read_qc_write", "kslam_set_read_qc", "kslam_stream_get_read_qc", "kslam_stream_set_read_qc",
           "kslam_tail_read_qc", "kslam_tail_read_qc_free"]
DEFAULT_CYCLES, MAX_CYCLES = 512, 65536
BASE_COLS, QUAL_COLS, MEAN_BINS, GC_BINS = 6, 95, 94, 101


def words(cycles):
    """KSLAM_READ_QC_WORDS: a stream's 64-bit words for `cycles` per-cycle rows"""
    return 4 + (cycles + 2) + (cycles + 1) * (BASE_COLS + QUAL_COLS) + MEAN_BINS + GC_BINS


class StreamView(C.Structure):
    """kslam_read_qc_stream"""
    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("min_len", C.c_uint64), ("max_len", C.c_uint64),
                ("len_hist", C.c_void_p), ("base", C.c_void_p), ("qual", C.c_void_p), ("mean_q", C.c_void_p), ("gc", C.c_void_p)]


class Tables(C.Structure):
    """kslam_read_qc_tables"""
    _fields_ = [("max_cycles", C.c_uint32), ("paired", C.c_int32), ("words_per_stream", C.c_uint64), ("block", C.c_void_p),
                ("stream", StreamView * 2)]


_ready = False


def lib():
    global _ready
    L = _T.lib()
    if not _ready:
        vp, u64, u32, P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
        L.kslam_set_read_qc.argtypes = [vp, C.c_int, u32]
        L.kslam_get_read_qc.argtypes = [vp, P(C.c_int), P(u32)]
        L.kslam_read_qc_reset.argtypes = [vp]
        L.kslam_read_qc_add.argtypes = [vp, vp, vp, vp, u64, C.c_int]
        L.kslam_read_qc_take.argtypes = [vp, P(Tables)]
        L.kslam_read_qc_release.argtypes = [vp, P(Tables)]
        L.kslam_read_qc_release.restype = None
        L.kslam_read_qc_kernel_ms.argtypes = [vp, P(C.c_double), P(u64)]
        L.kslam_tail_read_qc.argtypes = [vp, vp, vp, vp, u64, C.c_int, u32, P(Tables)]
        L.kslam_tail_read_qc_free.argtypes = [P(Tables)]
        L.kslam_tail_read_qc_free.restype = None
        L.kslam_read_qc_write.argtypes = [P(Tables), C.c_int]
        L.kslam_stream_set_read_qc.argtypes = [vp, C.c_int, u32]
        L.kslam_stream_get_read_qc.argtypes = [vp, P(C.c_int), P(u32)]
        _ready = True
    return L


def unpack(block, cycles, paired):
    """a block of 2 * words(cycles) uint64 -> {"max_cycles", "paired", "streams": [dict, dict]}; every table a list of ints"""
    block = np.asarray(block, dtype=np.uint64)
    nw = words(cycles)
    assert len(block) == 2 * nw
    out = []
    for z in range(2):
        w = block[z * nw:(z + 1) * nw]
        at = 4
        s = {"n_reads": int(w[0]), "n_bases": int(w[1]), "min_len": int(w[2]), "max_len": int(w[3])}
        for key, n in (("len_hist", cycles + 2), ("base", (cycles + 1) * BASE_COLS), ("qual", (cycles + 1) * QUAL_COLS), ("mean_q", MEAN_BINS),
                       ("gc", GC_BINS)):
            s[key] = w[at:at + n].tolist()
            at += n
        out.append(s)
    return {"max_cycles": int(cycles), "paired": bool(paired), "streams": out}


def pack(tables):
    """the inverse of unpack: -> (block as a uint64 array, cycles, paired)"""
    cycles = tables["max_cycles"]
    parts = []
    for s in tables["streams"]:
        parts.append(np.array([s["n_reads"], s["n_bases"], s["min_len"], s["max_len"]] + list(s["len_hist"]) + list(s["base"]) + list(s["qual"]) +
                              list(s["mean_q"]) + list(s["gc"]), dtype=np.uint64))
    block = np.concatenate(parts)
    assert len(block) == 2 * words(cycles)
    return block, cycles, bool(tables["paired"])


def _tables_out(t):
    n = 2 * int(t.words_per_stream)
    block = _T.rows_at(t.block, n, np.dtype(np.uint64))
    return unpack(block, int(t.max_cycles), t.paired)


def _columns(bases, quality):
    """lists of bytes -> (concatenated bases, offsets, concatenated quality, offsets)"""
    def cat(items):
        off = np.zeros(len(items) + 1, dtype=np.uint64)
        if len(items):
            off[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
        return np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8), off
    b, bo = cat(bases)
    q, qo = cat(quality)
    return b, bo, q, qo


def set_read_qc(ctx, on=True, max_cycles=0):
    """kslam_set_read_qc: switching on zeroes the tables (max_cycles 0 = 512), off frees them"""
    ctx._chk(lib().kslam_set_read_qc(ctx._h, int(on), int(max_cycles)))


def get_read_qc(ctx):
    """-> (on, max_cycles as resolved; 0 when off)"""
    on, c = C.c_int(), C.c_uint32()
    ctx._chk(lib().kslam_get_read_qc(ctx._h, C.byref(on), C.byref(c)))
    return bool(on.value), int(c.value)


def reset(ctx):
    ctx._chk(lib().kslam_read_qc_reset(ctx._h))


def add(ctx, bases, quality, paired=False):
    """kslam_read_qc_add: one batch's reads (lists of bytes, equal lengths read by read; paired: [R1 | R2]) into the tables"""
    if any(len(b) != len(q) for b, q in zip(bases, quality)) or len(bases) != len(quality):
        raise ValueError("a read's bases and quality bytes have the same length")
    b, bo, q, _ = _columns(bases, quality)
    ctx._chk(lib().kslam_read_qc_add(ctx._h, b.ctypes.data, bo.ctypes.data, q.ctypes.data, len(bases), int(paired)))


def add_columns(ctx, bases, offsets, quality, paired=False):
    """kslam_read_qc_add on columns as they are: uint8 arrays of bases and quality bytes, uint64 offsets (n_reads + 1)"""
    b, q = np.ascontiguousarray(bases, dtype=np.uint8), np.ascontiguousarray(quality, dtype=np.uint8)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(b) != len(q) or len(off) < 1 or int(off[-1]) > len(b):
        raise ValueError("columns that do not hold together")
    ctx._chk(lib().kslam_read_qc_add(ctx._h, b.ctypes.data, off.ctypes.data, q.ctypes.data, len(off) - 1, int(paired)))


def take(ctx):
    """kslam_read_qc_take -> the tables as unpack() gives them"""
    L = lib()
    t = Tables()
    ctx._chk(L.kslam_read_qc_take(ctx._h, C.byref(t)))
    try:
        return _tables_out(t)
    finally:
        L.kslam_read_qc_release(ctx._h, C.byref(t))


def kernel_ms(ctx):
    """(device ms of the last kslam_read_qc_add's count pass, the bytes of bases + quality it read)"""
    ms, n = C.c_double(), C.c_uint64()
    ctx._chk(lib().kslam_read_qc_kernel_ms(ctx._h, C.byref(ms), C.byref(n)))
    return float(ms.value), int(n.value)


def tail_read_qc(bases, quality, paired=False, max_cycles=0):
    """kslam_tail_read_qc (host twin; lists of bytes) -> the tables"""
    L = lib()
    b, bo, q, qo = _columns(bases, quality)
    t = Tables()
    _T._chk(L.kslam_tail_read_qc(b.ctypes.data, bo.ctypes.data, q.ctypes.data, qo.ctypes.data, len(bases), int(paired), int(max_cycles), C.byref(t)))
    try:
        return _tables_out(t)
    finally:
        L.kslam_tail_read_qc_free(C.byref(t))


def write(tables, fd):
    """kslam_read_qc_write: tables as unpack() gives them"""
    block, cycles, paired = pack(tables)
    t = Tables()
    t.max_cycles, t.paired, t.words_per_stream, t.block = cycles, int(paired), words(cycles), block.ctypes.data
    _T._chk(lib().kslam_read_qc_write(C.byref(t), int(fd)))


def report_bytes(tables):
    """the file as bytes (through a temporary descriptor)"""
    return _T.fd_bytes("kslam_read_qc", lambda fd: write(tables, fd))


def stream_set_read_qc(ctx, fd, max_cycles=0):
    """kslam_stream_set_read_qc: the descriptor the NEXT kslam_stream_classify on ctx writes its report to (-1: none)"""
    ctx._chk(lib().kslam_stream_set_read_qc(ctx._h, int(fd) if fd is not None else -1, int(max_cycles)))


def parse(text):
    """the file -> dict: json.loads with the ratio strings turned into floats and the keys of the count maps into ints (">C" and
    "invalid" stay strings)"""
    if isinstance(text, bytes):
        text = text.decode()
    doc = json.loads(text)
    if doc.get("kslam_read_qc") != 1:
        raise ValueError("not a read QC report of format 1")

    def num_keys(d):
        return {(int(k) if k.isdigit() else k): v for k, v in d.items()}

    def ratios(d):
        for k, v in list(d.items()):
            if isinstance(v, str):
                d[k] = float(v)
    ratios(doc["summary"])
    for name in ("read1", "read2"):
        if name not in doc:
            continue
        s = doc[name]
        ratios(s)
        s["quality_mean"] = [float(x) for x in s["quality_mean"]]
        for k in ("length_counts", "quality_counts", "mean_quality_counts", "gc_counts"):
            s[k] = num_keys(s[k])
    return doc
