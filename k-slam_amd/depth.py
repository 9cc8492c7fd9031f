"""ctypes plumbing for include/kslam_depth.h: the depth along every entry accumulated on the GPU (one row per maximal run of equal
depth), its host twin, the bedGraph writer and a parser for the file."""
import ctypes as C

import numpy as np

from . import OVERLAP_DT
from . import tail as _T

# every symbol include/kslam_depth.h declares
EXPORTS = ["kslam_depth_add", "kslam_depth_kernel_ms", "kslam_depth_reset", "kslam_depth_set_compact_at", "kslam_depth_take",
           "kslam_depth_write", "kslam_get_depth", "kslam_set_depth", "kslam_stream_get_depth", "kslam_stream_set_depth", "kslam_tail_depth"]
ROW_DT = np.dtype([("entry", "<u4"), ("start", "<u4"), ("end", "<u4"), ("depth", "<u4")])
STAT_NAMES = ("n_records", "n_skipped", "n_intervals", "n_keys", "n_rows", "covered_bases", "max_depth")
_ready = False


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in STAT_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in STAT_NAMES}


def lib():
    global _ready
    L = _T.lib()
    if not _ready:
        vp, u64, u32, P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
        batch = [vp, u64, vp, u64, vp, u64, vp, u64, vp, u64]   # overlaps, pool, read offsets, read pairs, pairs
        L.kslam_set_depth.argtypes = [vp, C.c_int]
        L.kslam_get_depth.argtypes = [vp, P(C.c_int)]
        L.kslam_depth_reset.argtypes = [vp]
        L.kslam_depth_add.argtypes = [vp] + batch
        L.kslam_depth_take.argtypes = [vp, u32, P(vp), P(u64), P(Stats)]
        L.kslam_depth_kernel_ms.argtypes = [vp, P(C.c_double), P(C.c_double), P(C.c_double)]
        L.kslam_depth_set_compact_at.argtypes = [vp, u64]
        L.kslam_tail_depth.argtypes = [vp, u64] + batch + [u32, P(vp), P(u64), P(Stats)]
        L.kslam_depth_write.argtypes = [P(_T.IndexView), vp, u64, C.c_int]
        L.kslam_stream_set_depth.argtypes = [vp, C.c_int, u32]
        L.kslam_stream_get_depth.argtypes = [vp, P(C.c_int), P(u32)]
        L.kslam_free_pinned.argtypes = [vp, vp]
        L.kslam_free_pinned.restype = None
        L.kslam_free.argtypes = [vp]
        L.kslam_free.restype = None
        _ready = True
    return L


def _arrays(overlaps, cigar_pool, read_offsets, read_pairs, pairs):
    ov = np.ascontiguousarray(overlaps, dtype=OVERLAP_DT)
    cg = np.ascontiguousarray(cigar_pool, dtype=np.uint32)
    ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    rp = np.ascontiguousarray(read_pairs, dtype=_T.READ_PAIR_DT)
    pr = np.ascontiguousarray(pairs, dtype=_T.PAIRED_OVERLAP_DT)
    ptr = lambda a: a.ctypes.data if len(a) else None   # noqa: E731
    n_reads = max(len(ro) - 1, 0)
    return (ov, cg, ro, rp, pr), (ptr(ov), len(ov), ptr(cg), len(cg), ro.ctypes.data if n_reads else None, n_reads, ptr(rp), len(rp), ptr(pr), len(pr))


def set_depth(ctx, on=True):
    """kslam_set_depth: needs an index, ctx.set_pairing and a context with report_cigar; off frees the state"""
    ctx._chk(lib().kslam_set_depth(ctx._h, int(on)))


def get_depth(ctx):
    on = C.c_int()
    ctx._chk(lib().kslam_get_depth(ctx._h, C.byref(on)))
    return bool(on.value)


def reset(ctx):
    ctx._chk(lib().kslam_depth_reset(ctx._h))


def set_compact_at(ctx, n_keys=0):
    """kslam_depth_set_compact_at: the pending keys (two per interval) above which an add compacts; 0 = the default"""
    ctx._chk(lib().kslam_depth_set_compact_at(ctx._h, int(n_keys)))


def add(ctx, overlaps, cigar_pool, read_offsets, read_pairs, pairs):
    """kslam_depth_add: one batch's arrays from the host (OVERLAP_DT, uint32 pool, the reads' n + 1 offsets, READ_PAIR_DT,
    PAIRED_OVERLAP_DT)"""
    keep, args = _arrays(overlaps, cigar_pool, read_offsets, read_pairs, pairs)
    ctx._chk(lib().kslam_depth_add(ctx._h, *args))


def take(ctx, min_depth=1):
    """kslam_depth_take -> (rows: ROW_DT array, stats: dict)"""
    L = lib()
    rows, n, st = C.c_void_p(), C.c_uint64(), Stats()
    ctx._chk(L.kslam_depth_take(ctx._h, int(min_depth), C.byref(rows), C.byref(n), C.byref(st)))
    out = _T.rows_at(rows.value, n.value, ROW_DT)
    L.kslam_free_pinned(ctx._h, rows)
    return out, st.as_dict()


def kernel_ms(ctx):
    """(device ms of the last kslam_depth_add's emit passes, of the last compaction, of the last take without its compaction)"""
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    ctx._chk(lib().kslam_depth_kernel_ms(ctx._h, C.byref(a), C.byref(b), C.byref(c)))
    return float(a.value), float(b.value), float(c.value)


def tail_depth(entry_offsets, overlaps, cigar_pool, read_offsets, read_pairs, pairs, min_depth=1):
    """kslam_tail_depth (host twin) -> (rows, stats)"""
    L = lib()
    go = np.ascontiguousarray(entry_offsets, dtype=np.uint64)
    keep, args = _arrays(overlaps, cigar_pool, read_offsets, read_pairs, pairs)
    rows, n, st = C.c_void_p(), C.c_uint64(), Stats()
    n_entries = max(len(go) - 1, 0)
    _T._chk(L.kslam_tail_depth(go.ctypes.data if n_entries else None, n_entries, *args, int(min_depth), C.byref(rows), C.byref(n), C.byref(st)))
    out = _T.rows_at(rows.value, n.value, ROW_DT)
    L.kslam_free(rows)
    return out, st.as_dict()


def write(index, rows, fd):
    """kslam_depth_write: index a kslam_amd.tail index view (e.g. kslam_amd.db.Database), rows a ROW_DT array"""
    r = np.ascontiguousarray(rows, dtype=ROW_DT)
    _T._chk(lib().kslam_depth_write(C.byref(index.view), r.ctypes.data if len(r) else None, len(r), int(fd)))


def report_bytes(index, rows):
    """the bedGraph file as bytes (through a pipe-free temporary descriptor)"""
    return _T.fd_bytes("kslam_depth", lambda fd: write(index, rows, fd))


def stream_set_depth(ctx, fd, min_depth=1):
    """kslam_stream_set_depth: the descriptor the NEXT kslam_stream_classify on ctx writes its bedGraph file to (-1: none)"""
    ctx._chk(lib().kslam_stream_set_depth(ctx._h, int(fd) if fd is not None else -1, int(min_depth)))


def parse_bedgraph(text):
    """the file's lines -> list of (locus: str, start, end, depth); raises ValueError for a line of another kind"""
    if isinstance(text, bytes):
        text = text.decode()
    rows = []
    if text and not text.endswith("\n"):
        raise ValueError("the last line is not ended")
    for line in text.split("\n")[:-1]:
        f = line.split("\t")
        if len(f) != 4 or not f[0]:
            raise ValueError("a bedGraph line has %d fields" % len(f))
        rows.append((f[0], int(f[1]), int(f[2]), int(f[3])))
    return rows
