"""ctypes plumbing for include/kslam_coverage.h: the per-entry coverage table accumulated on the GPU (alignments, unique read
pairs, aligned and covered bases), its host twin, the report writer and a parser for the report."""
import ctypes as C

import numpy as np

from . import OVERLAP_DT
from . import tail as _T

# every symbol include/kslam_coverage.h declares
EXPORTS = ["kslam_coverage_add", "kslam_coverage_bitmap", "kslam_coverage_kernel_ms", "kslam_coverage_reset", "kslam_coverage_take",
           "kslam_coverage_write", "kslam_get_coverage", "kslam_set_coverage", "kslam_stream_get_coverage", "kslam_stream_set_coverage",
           "kslam_tail_coverage"]
ROW_DT = np.dtype([("alignments", "<u8"), ("unique_read_pairs", "<u8"), ("aligned_bases", "<u8"), ("covered_bases", "<u8")])
HEADER = b"#entry\tlocus\ttaxid\tlength\talignments\tunique_read_pairs\taligned_bases\tcovered_bases\tbreadth\tmean_depth\n"
_ready = False


def lib():
    global _ready
    L = _T.lib()
    if not _ready:
        vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
        L.kslam_set_coverage.argtypes = [vp, C.c_int]
        L.kslam_get_coverage.argtypes = [vp, P(C.c_int)]
        L.kslam_coverage_reset.argtypes = [vp]
        L.kslam_coverage_add.argtypes = [vp, vp, u64, vp, u64, vp, u64]
        L.kslam_coverage_take.argtypes = [vp, P(vp), P(u64), P(u64)]
        L.kslam_coverage_bitmap.argtypes = [vp, u64, vp, u64]
        L.kslam_coverage_kernel_ms.argtypes = [vp, P(C.c_double), P(C.c_double)]
        L.kslam_tail_coverage.argtypes = [vp, u64, vp, u64, vp, u64, vp, u64, vp, P(u64)]
        L.kslam_coverage_write.argtypes = [P(_T.IndexView), vp, u64, C.c_int]
        L.kslam_stream_set_coverage.argtypes = [vp, C.c_int]
        L.kslam_stream_get_coverage.argtypes = [vp, P(C.c_int)]
        L.kslam_free_pinned.argtypes = [vp, vp]
        L.kslam_free_pinned.restype = None
        _ready = True
    return L


def _arrays(overlaps, read_pairs, pairs):
    ov = np.ascontiguousarray(overlaps, dtype=OVERLAP_DT)
    rp = np.ascontiguousarray(read_pairs, dtype=_T.READ_PAIR_DT)
    pr = np.ascontiguousarray(pairs, dtype=_T.PAIRED_OVERLAP_DT)
    ptr = lambda a: a.ctypes.data if len(a) else None   # noqa: E731
    return (ov, rp, pr), (ptr(ov), len(ov), ptr(rp), len(rp), ptr(pr), len(pr))


def set_coverage(ctx, on=True):
    """kslam_set_coverage: needs an index and ctx.set_pairing first; switching on zeroes the table, off frees it"""
    ctx._chk(lib().kslam_set_coverage(ctx._h, int(on)))


def get_coverage(ctx):
    on = C.c_int()
    ctx._chk(lib().kslam_get_coverage(ctx._h, C.byref(on)))
    return bool(on.value)


def reset(ctx):
    ctx._chk(lib().kslam_coverage_reset(ctx._h))


def add(ctx, overlaps, read_pairs, pairs):
    """kslam_coverage_add: one batch's arrays (OVERLAP_DT, READ_PAIR_DT, PAIRED_OVERLAP_DT) from the host into the table"""
    keep, args = _arrays(overlaps, read_pairs, pairs)
    ctx._chk(lib().kslam_coverage_add(ctx._h, *args))


def take(ctx):
    """kslam_coverage_take -> (rows: ROW_DT array with one row per entry, n_skipped)"""
    L = lib()
    rows, n, skipped = C.c_void_p(), C.c_uint64(), C.c_uint64()
    ctx._chk(L.kslam_coverage_take(ctx._h, C.byref(rows), C.byref(n), C.byref(skipped)))
    out = _T.rows_at(rows.value, n.value, ROW_DT)
    L.kslam_free_pinned(ctx._h, rows)
    return out, int(skipped.value)


def bitmap(ctx, entry, length):
    """kslam_coverage_bitmap: the ceil(length / 64) words of one entry (uint64 array)"""
    words = np.zeros((int(length) + 63) // 64, dtype=np.uint64)
    ctx._chk(lib().kslam_coverage_bitmap(ctx._h, int(entry), words.ctypes.data if len(words) else None, len(words)))
    return words


def kernel_ms(ctx):
    """(device ms of the last kslam_coverage_add's mark passes, of the last take's count pass)"""
    a, b = C.c_double(), C.c_double()
    ctx._chk(lib().kslam_coverage_kernel_ms(ctx._h, C.byref(a), C.byref(b)))
    return float(a.value), float(b.value)


def tail_coverage(entry_lengths, overlaps, read_pairs, pairs):
    """kslam_tail_coverage (host twin) -> (rows, n_skipped)"""
    lens = np.ascontiguousarray(entry_lengths, dtype=np.uint64)
    keep, args = _arrays(overlaps, read_pairs, pairs)
    rows = np.zeros(len(lens), dtype=ROW_DT)
    skipped = C.c_uint64()
    _T._chk(lib().kslam_tail_coverage(lens.ctypes.data if len(lens) else None, len(lens), *args, rows.ctypes.data if len(rows) else None,
                                      C.byref(skipped)))
    return rows, int(skipped.value)


def write_report(index, rows, fd):
    """kslam_coverage_write: index a kslam_amd.tail index view (e.g. kslam_amd.db.Database), rows a ROW_DT array"""
    r = np.ascontiguousarray(rows, dtype=ROW_DT)
    _T._chk(lib().kslam_coverage_write(C.byref(index.view), r.ctypes.data if len(r) else None, len(r), int(fd)))


def report_bytes(index, rows):
    """the report as bytes (through a pipe-free temporary descriptor)"""
    return _T.fd_bytes("kslam_coverage", lambda fd: write_report(index, rows, fd))


def stream_set_coverage(ctx, fd):
    """kslam_stream_set_coverage: the descriptor the NEXT kslam_stream_classify on ctx writes its coverage report to (-1: none)"""
    ctx._chk(lib().kslam_stream_set_coverage(ctx._h, int(fd) if fd is not None else -1))


def parse_report(text):
    """the report's lines -> list of dicts (entry, locus, taxid, length, alignments, unique_read_pairs, aligned_bases,
    covered_bases as int; breadth, mean_depth as float); raises ValueError on another header"""
    if isinstance(text, str):
        text = text.encode()
    if not text.startswith(HEADER):
        raise ValueError("not a coverage report: the header line is missing")
    names = HEADER[1:-1].decode().split("\t")
    out = []
    for line in text[len(HEADER):].split(b"\n"):
        if not line:
            continue
        f = line.decode().split("\t")
        if len(f) != len(names):
            raise ValueError("a coverage line has %d fields" % len(f))
        row = {}
        for k, v in zip(names, f):
            row[k] = v if k == "locus" else float(v) if k in ("breadth", "mean_depth") else int(v)
        out.append(row)
    return out
