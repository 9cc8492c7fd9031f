"""ctypes plumbing for include/kslam_readsplit.h: the classified / unclassified reads written back out as FASTQ, split on the GPU,
with a host twin."""
import ctypes as C

import numpy as np

from . import tail as _T

# every symbol include/kslam_readsplit.h declares
EXPORTS = ["kslam_collect_reads_out", "kslam_get_reads_out", "kslam_get_reads_out_bgzf", "kslam_reads_out_kernel_ms",
           "kslam_release_reads_out", "kslam_set_reads_out", "kslam_set_reads_out_bgzf", "kslam_split_reads_text",
           "kslam_stream_get_reads_out", "kslam_stream_set_reads_out", "kslam_tail_split_reads"]
CLASSIFIED, UNCLASSIFIED = 1, 2
FLAG_BGZF, FLAG_LEFT_TO_HOST, FLAG_HOST_MEMORY = 1, 2, 4
_ready = False


class ReadsOut(C.Structure):
    """kslam_reads_out"""
    _fields_ = [("data", C.c_void_p * 4), ("len", C.c_uint64 * 4), ("n_records", C.c_uint64 * 2), ("flags", C.c_uint32),
                ("pad_", C.c_uint32)]


def lib():
    global _ready
    L = _T.lib()
    if not _ready:
        vp, u64, u32, P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
        L.kslam_set_reads_out.argtypes = [vp, u32]
        L.kslam_get_reads_out.argtypes = [vp, P(u32)]
        L.kslam_set_reads_out_bgzf.argtypes = [vp, C.c_int]
        L.kslam_get_reads_out_bgzf.argtypes = [vp, P(C.c_int)]
        L.kslam_collect_reads_out.argtypes = [vp, u64, P(ReadsOut)]
        L.kslam_release_reads_out.argtypes = [vp, P(ReadsOut)]
        L.kslam_release_reads_out.restype = None
        L.kslam_tail_split_reads.argtypes = [vp, u64, vp, u64, u64, C.c_int, vp, u64, u32, P(ReadsOut)]
        L.kslam_split_reads_text.argtypes = [vp, vp, u64, vp, u64, u64, C.c_int, vp, u64, u32, P(ReadsOut)]
        L.kslam_stream_set_reads_out.argtypes = [vp, P(C.c_int * 4)]
        L.kslam_stream_get_reads_out.argtypes = [vp, P(C.c_int * 4)]
        L.kslam_reads_out_kernel_ms.argtypes = [vp, P(C.c_double), P(u64)]
        _ready = True
    return L


def set_reads_out(ctx, which):
    """kslam_set_reads_out: a mask of CLASSIFIED | UNCLASSIFIED, 0 = off; needs ctx.set_pairing first"""
    ctx._chk(lib().kslam_set_reads_out(ctx._h, int(which)))


def get_reads_out(ctx):
    w = C.c_uint32()
    ctx._chk(lib().kslam_get_reads_out(ctx._h, C.byref(w)))
    return int(w.value)


def set_reads_out_bgzf(ctx, on=True):
    ctx._chk(lib().kslam_set_reads_out_bgzf(ctx._h, int(on)))


def get_reads_out_bgzf(ctx):
    on = C.c_int()
    ctx._chk(lib().kslam_get_reads_out_bgzf(ctx._h, C.byref(on)))
    return bool(on.value)


def _take(ctx, ro):
    """the four blocks as bytes (None for a stream not asked for), the record counts and the flags; releases the blocks"""
    blocks = [C.string_at(ro.data[k], ro.len[k]) if ro.data[k] else None for k in range(4)]
    out = {"blocks": blocks, "n_records": (int(ro.n_records[0]), int(ro.n_records[1])), "flags": int(ro.flags)}
    lib().kslam_release_reads_out(ctx._h if ctx is not None else None, C.byref(ro))
    return out


def collect_reads_out(ctx, ticket):
    """kslam_collect_reads_out, after ctx.collect_batch(ticket) -> {"blocks": [c1, c2, u1, u2], "n_records", "flags"}"""
    ro = ReadsOut()
    ctx._chk(lib().kslam_collect_reads_out(ctx._h, ticket, C.byref(ro)))
    return _take(ctx, ro)


def _pairs(read_pairs):
    rp = np.ascontiguousarray(read_pairs, dtype=_T.READ_PAIR_DT)
    return rp, (rp.ctypes.data if len(rp) else None)


def tail_split_reads(r1, r2, read_pairs, which=3, max_pairs=0, at_eof=True):
    """kslam_tail_split_reads (host): r1 / r2 bytes (r2 None: single-end), read_pairs a READ_PAIR_DT array"""
    rp, prp = _pairs(read_pairs)
    ro = ReadsOut()
    _T._chk(lib().kslam_tail_split_reads(r1, len(r1), r2, len(r2) if r2 is not None else 0, max_pairs, int(at_eof), prp, len(rp),
                                         int(which), C.byref(ro)))
    return _take(None, ro)


def split_reads_text(ctx, r1, r2, read_pairs, which=3, max_pairs=0, at_eof=True):
    """kslam_split_reads_text (device, on ctx itself): the same arguments as tail_split_reads"""
    rp, prp = _pairs(read_pairs)
    ro = ReadsOut()
    ctx._chk(lib().kslam_split_reads_text(ctx._h, r1, len(r1), r2, len(r2) if r2 is not None else 0, max_pairs, int(at_eof), prp,
                                          len(rp), int(which), C.byref(ro)))
    return _take(ctx, ro)


def stream_set_reads_out(ctx, fds):
    """kslam_stream_set_reads_out: four descriptors (classified R1, R2, unclassified R1, R2; -1 = not wanted) for the NEXT
    kslam_stream_classify on ctx; None = none"""
    arr = (C.c_int * 4)(*[int(f) for f in fds]) if fds is not None else None
    ctx._chk(lib().kslam_stream_set_reads_out(ctx._h, C.byref(arr) if arr is not None else None))


def kernel_ms(ctx):
    """(device ms of the last batch's flag, scan and copy kernels on ctx, text bytes the copy read + wrote)"""
    ms, b = C.c_double(), C.c_uint64()
    ctx._chk(lib().kslam_reads_out_kernel_ms(ctx._h, C.byref(ms), C.byref(b)))
    return float(ms.value), int(b.value)
