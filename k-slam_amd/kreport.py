"""ctypes plumbing for include/kslam_kreport.h: the Kraken-style report (percent, clade reads, direct reads, rank code, taxonomy
id, indented name) counted per taxon on the GPU, its host twin, the report writer and a parser for the report."""
import ctypes as C

import numpy as np

from . import tail as _T
from . import taxonomy as _X

# every symbol include/kslam_kreport.h declares
EXPORTS = ["kslam_get_kreport", "kslam_kreport_add", "kslam_kreport_kernel_ms", "kslam_kreport_reset", "kslam_kreport_take",
           "kslam_kreport_write", "kslam_set_kreport", "kslam_stream_get_kreport", "kslam_stream_set_kreport", "kslam_tail_kreport"]
ROW_DT = np.dtype([("tax_id", "<u4"), ("node", "<u4"), ("direct", "<u8"), ("clade", "<u8")])
NO_NODE = 0xFFFFFFFF


class Stats(C.Structure):
    """kslam_kreport_stats"""
    _fields_ = [("n_ids", C.c_uint64), ("n_unknown_ids", C.c_uint64), ("n_rows", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


_ready = False


def lib():
    global _ready
    L = _X.lib()
    if not _ready:
        vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
        L.kslam_set_kreport.argtypes = [vp, C.c_int]
        L.kslam_get_kreport.argtypes = [vp, P(C.c_int)]
        L.kslam_kreport_reset.argtypes = [vp]
        L.kslam_kreport_add.argtypes = [vp, vp, u64]
        L.kslam_kreport_take.argtypes = [vp, P(vp), P(u64), P(Stats)]
        L.kslam_kreport_kernel_ms.argtypes = [vp, P(C.c_double), P(C.c_double)]
        L.kslam_tail_kreport.argtypes = [vp, vp, u64, P(vp), P(u64), P(Stats)]
        L.kslam_kreport_write.argtypes = [vp, vp, u64, u64, C.c_int]
        L.kslam_stream_set_kreport.argtypes = [vp, C.c_int]
        L.kslam_stream_get_kreport.argtypes = [vp, P(C.c_int)]
        L.kslam_free_pinned.argtypes = [vp, vp]
        L.kslam_free_pinned.restype = None
        L.kslam_free.argtypes = [vp]
        L.kslam_free.restype = None
        _ready = True
    return L


def _rows(ptr, n):
    return _T.rows_at(ptr.value, n.value, ROW_DT)


def set_kreport(ctx, on=True):
    """kslam_set_kreport: needs kslam_amd.samtext.set_annotations with a taxdb first; switching on zeroes the state, off frees it"""
    ctx._chk(lib().kslam_set_kreport(ctx._h, int(on)))


def get_kreport(ctx):
    on = C.c_int()
    ctx._chk(lib().kslam_get_kreport(ctx._h, C.byref(on)))
    return bool(on.value)


def reset(ctx):
    ctx._chk(lib().kslam_kreport_reset(ctx._h))


def add(ctx, tax_ids):
    """kslam_kreport_add: one batch's taxonomy ids (uint32, one per read pair) from the host into the counters"""
    ids = np.ascontiguousarray(tax_ids, dtype=np.uint32)
    ctx._chk(lib().kslam_kreport_add(ctx._h, ids.ctypes.data if len(ids) else None, len(ids)))


def take(ctx):
    """kslam_kreport_take -> (rows: ROW_DT array, stats: dict)"""
    L = lib()
    rows, n, st = C.c_void_p(), C.c_uint64(), Stats()
    ctx._chk(L.kslam_kreport_take(ctx._h, C.byref(rows), C.byref(n), C.byref(st)))
    out = _rows(rows, n)
    L.kslam_free_pinned(ctx._h, rows)
    return out, st.as_dict()


def kernel_ms(ctx):
    """(device ms of the last kslam_kreport_add's count pass, of the last take's kernels)"""
    a, b = C.c_double(), C.c_double()
    ctx._chk(lib().kslam_kreport_kernel_ms(ctx._h, C.byref(a), C.byref(b)))
    return float(a.value), float(b.value)


def tail_kreport(taxdb, tax_ids):
    """kslam_tail_kreport (host twin; taxdb: kslam_amd.taxonomy.TaxDB) -> (rows, stats)"""
    L = lib()
    ids = np.ascontiguousarray(tax_ids, dtype=np.uint32)
    rows, n, st = C.c_void_p(), C.c_uint64(), Stats()
    _T._chk(L.kslam_tail_kreport(taxdb._h, ids.ctypes.data if len(ids) else None, len(ids), C.byref(rows), C.byref(n), C.byref(st)))
    out = _rows(rows, n)
    L.kslam_free(rows)
    return out, st.as_dict()


def write(taxdb, rows, total_read_pairs, fd):
    """kslam_kreport_write: rows a ROW_DT array, total_read_pairs the run's read pairs (the percentages' denominator)"""
    r = np.ascontiguousarray(rows, dtype=ROW_DT)
    _T._chk(lib().kslam_kreport_write(taxdb._h, r.ctypes.data if len(r) else None, len(r), int(total_read_pairs), int(fd)))


def report_bytes(taxdb, rows, total_read_pairs):
    """the report as bytes (through a pipe-free temporary descriptor)"""
    return _T.fd_bytes("kslam_kreport", lambda fd: write(taxdb, rows, total_read_pairs, fd))


def stream_set_kreport(ctx, fd):
    """kslam_stream_set_kreport: the descriptor the NEXT kslam_stream_classify on ctx writes its report to (-1: none)"""
    ctx._chk(lib().kslam_stream_set_kreport(ctx._h, int(fd) if fd is not None else -1))


def parse_report(text):
    """the report's lines -> list of dicts (percent as float; clade, direct, taxid, level as int; code, name as str)"""
    if isinstance(text, str):
        text = text.encode()
    out = []
    for line in text.split(b"\n"):
        if not line:
            continue
        f = line.decode().split("\t")
        if len(f) != 6:
            raise ValueError("a report line has %d fields" % len(f))
        name = f[5].lstrip(" ")
        indent = len(f[5]) - len(name)
        if indent % 2:
            raise ValueError("an indent of %d spaces" % indent)
        out.append({"percent": float(f[0]), "clade": int(f[1]), "direct": int(f[2]), "code": f[3], "taxid": int(f[4]), "level": indent // 2,
                    "name": name})
    return out
