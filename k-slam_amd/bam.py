"""ctypes plumbing for include/kslam_bam.h: the SAM file as BAM, records encoded and compressed on the GPU, with host twins."""
import ctypes as C

import numpy as np

from . import tail as _T

EXPORTS = ["kslam_bam_header", "kslam_get_sam_bam", "kslam_sam_bam", "kslam_set_sam_bam", "kslam_tail_finish_write_rows_bam",
           "kslam_tail_sam_bam"]
TEXT_SAM_BAM = 16   # KSLAM_TEXT_SAM_BAM
_ready = False


def lib():
    global _ready
    L = _T.lib()
    if not _ready:
        vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
        L.kslam_set_sam_bam.argtypes = [vp, C.c_int]
        L.kslam_get_sam_bam.argtypes = [vp, P(C.c_int)]
        L.kslam_bam_header.argtypes = [P(_T.IndexView), C.c_char_p, u64, P(vp), P(u64)]
        L.kslam_sam_bam.argtypes = [vp, C.c_int, C.c_uint32, C.c_int, P(vp), P(u64)]
        L.kslam_tail_sam_bam.argtypes = [P(_T.TailParams), P(_T.ReadsView), P(_T.IndexView), vp, u64, vp, u64, P(vp), P(u64),
                                         P(_T.TailStats)]
        L.kslam_tail_finish_write_rows_bam.argtypes = [P(_T.TailParams), P(_T.ReadsView), P(_T.IndexView), vp, u64, vp, u64,
                                                       vp, vp, u64, vp, u64, vp, u64, _T.WRITE_FN, vp, P(_T.TailStats)]
        _ready = True
    return L


def set_sam_bam(ctx, on=True):
    """kslam_set_sam_bam: the lanes (and kslam_stream_classify) write the SAM file as BAM"""
    ctx._chk(lib().kslam_set_sam_bam(ctx._h, int(on)))


def get_sam_bam(ctx):
    on = C.c_int()
    ctx._chk(lib().kslam_get_sam_bam(ctx._h, C.byref(on)))
    return bool(on.value)


def header(index, sam_header):
    """kslam_bam_header: the uncompressed BAM header around `sam_header` (normally tail.sam_header's text)"""
    L = lib()
    sam_header = bytes(sam_header)
    out, n = C.c_void_p(), C.c_uint64()
    _T._chk(L.kslam_bam_header(C.byref(index.view), sam_header, len(sam_header), C.byref(out), C.byref(n)))
    return _T._text(out, n)


def sam_bam(ctx, paired=True, num_alignments=10, sam_xa=False):
    """kslam_sam_bam on the context's resident batch -> the uncompressed BAM records"""
    L = lib()
    out, n = C.c_void_p(), C.c_uint64()
    ctx._chk(L.kslam_sam_bam(ctx._h, int(paired), num_alignments, int(sam_xa), C.byref(out), C.byref(n)))
    try:
        return bytes((C.c_char * n.value).from_address(out.value)) if n.value else b""
    finally:
        if out.value:
            L.kslam_free_pinned(ctx._h, out)


def tail_sam_bam(params, reads, index, overlaps, cigar_pool):
    """kslam_tail_sam_bam (host) -> (BAM records as bytes, stats)"""
    L = lib()
    ov, pov = _T._ov(overlaps)
    pool = np.ascontiguousarray(cigar_pool, dtype=np.uint32)
    out, n, st = C.c_void_p(), C.c_uint64(), _T.TailStats()
    _T._chk(L.kslam_tail_sam_bam(C.byref(params), C.byref(reads.view), C.byref(index.view), pov, len(ov),
                                 _T._p(pool) if len(pool) else None, len(pool), C.byref(out), C.byref(n), C.byref(st)))
    return _T._text(out, n), st


def tail_finish_rows_bam(params, reads, index, overlaps, cigar_pool, details, md_pool, read_pairs, pairs):
    """kslam_tail_finish_write_rows_bam (host): tail.tail_finish_rows writing BAM records -> (records as bytes, stats); read_pairs
    and pairs are MODIFIED in place, details / md_pool may be None"""
    L = lib()
    ov, pov = _T._ov(overlaps)
    pool = np.ascontiguousarray(cigar_pool, dtype=np.uint32)
    det = np.ascontiguousarray(details) if details is not None else None
    md = np.ascontiguousarray(md_pool, dtype=np.uint8) if md_pool is not None else np.zeros(0, dtype=np.uint8)
    assert read_pairs.dtype == _T.READ_PAIR_DT and pairs.dtype == _T.PAIRED_OVERLAP_DT
    assert read_pairs.flags["C_CONTIGUOUS"] and pairs.flags["C_CONTIGUOUS"]
    chunks = []

    def _cb(user, data, k):
        chunks.append(C.string_at(data, k))
        return 0

    cb = _T.WRITE_FN(_cb)
    st = _T.TailStats()
    _T._chk(L.kslam_tail_finish_write_rows_bam(
        C.byref(params), C.byref(reads.view), C.byref(index.view), pov, len(ov), _T._p(pool) if len(pool) else None, len(pool),
        _T._p(det) if det is not None and len(det) else None, _T._p(md) if len(md) else None, len(md),
        _T._p(read_pairs) if len(read_pairs) else None, len(read_pairs), _T._p(pairs) if len(pairs) else None, len(pairs),
        cb, None, C.byref(st)))
    return b"".join(chunks), st
