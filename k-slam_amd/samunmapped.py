"""ctypes plumbing for include/kslam_samunmapped.h: FLAG-4 rows (text, BGZF or BAM) for the reads without alignment, written on the
GPU behind each batch's other rows, with a host twin."""
import ctypes as C

import numpy as np

from . import tail as _T

# every symbol include/kslam_samunmapped.h declares
EXPORTS = ["kslam_get_sam_unmapped", "kslam_sam_unmapped_kernel_ms", "kslam_set_sam_unmapped", "kslam_tail_sam_unmapped"]
TEXT_SAM_UNMAPPED = 64   # KSLAM_TEXT_SAM_UNMAPPED in kslam_batch_result.text_flags
_ready = False


def lib():
    global _ready
    L = _T.lib()
    if not _ready:
        vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
        L.kslam_set_sam_unmapped.argtypes = [vp, C.c_int]
        L.kslam_get_sam_unmapped.argtypes = [vp, P(C.c_int)]
        L.kslam_sam_unmapped_kernel_ms.argtypes = [vp, P(C.c_double), P(u64), P(u64)]
        L.kslam_tail_sam_unmapped.argtypes = [P(_T.TailParams), P(_T.ReadsView), vp, u64, u64, C.c_int, C.c_int, P(vp), P(u64)]
        _ready = True
    return L


def set_sam_unmapped(ctx, on=True):
    """kslam_set_sam_unmapped: every batch's rows are followed by one row per read that has none (lanes, kslam_sam_text /
    kslam_sam_bam, kslam_stream_classify)"""
    ctx._chk(lib().kslam_set_sam_unmapped(ctx._h, int(on)))


def get_sam_unmapped(ctx):
    on = C.c_int()
    ctx._chk(lib().kslam_get_sam_unmapped(ctx._h, C.byref(on)))
    return bool(on.value)


def kernel_ms(ctx):
    """(device ms of the new kernels of the last batch formatted on ctx or one of its lanes, bytes of the new rows, rows)"""
    ms, b, n = C.c_double(), C.c_uint64(), C.c_uint64()
    ctx._chk(lib().kslam_sam_unmapped_kernel_ms(ctx._h, C.byref(ms), C.byref(b), C.byref(n)))
    return float(ms.value), int(b.value), int(n.value)


def tail_sam_unmapped(params, reads, read_pairs, n_consumed_pairs, bam=False, seq=False):
    """kslam_tail_sam_unmapped (host): reads a tail.Reads (or samseq.without_qualities of one), read_pairs a READ_PAIR_DT array ->
    the rows as bytes"""
    rp = np.ascontiguousarray(read_pairs, dtype=_T.READ_PAIR_DT)
    out, n = C.c_void_p(), C.c_uint64()
    _T._chk(lib().kslam_tail_sam_unmapped(C.byref(params), C.byref(reads.view), rp.ctypes.data if len(rp) else None, len(rp),
                                          int(n_consumed_pairs), int(bam), int(seq), C.byref(out), C.byref(n)))
    return _T._text(out, n)
