"""ctypes plumbing for include/kslam_samseq.h: SEQ and QUAL on the primary rows of the SAM file (text, BGZF or BAM), written on
the GPU, with host twins."""
import ctypes as C

import numpy as np

from . import tail as _T

# every symbol include/kslam_samseq.h declares
EXPORTS = ["kslam_get_sam_seq", "kslam_set_sam_seq", "kslam_tail_finish_write_rows_seq", "kslam_tail_sam_seq"]
_ready = False


def lib():
    global _ready
    L = _T.lib()
    if not _ready:
        vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
        L.kslam_set_sam_seq.argtypes = [vp, C.c_int]
        L.kslam_get_sam_seq.argtypes = [vp, P(C.c_int)]
        L.kslam_tail_sam_seq.argtypes = [P(_T.TailParams), P(_T.ReadsView), P(_T.IndexView), vp, u64, vp, u64, C.c_int, P(vp), P(u64),
                                         P(_T.TailStats)]
        L.kslam_tail_finish_write_rows_seq.argtypes = [P(_T.TailParams), P(_T.ReadsView), P(_T.IndexView), vp, u64, vp, u64,
                                                       vp, vp, u64, vp, u64, vp, u64, C.c_int, _T.WRITE_FN, vp, P(_T.TailStats)]
        _ready = True
    return L


def set_sam_seq(ctx, on=True):
    """kslam_set_sam_seq: rows without flag 0x100 carry SEQ and QUAL (lanes, kslam_sam_text / kslam_sam_bam, kslam_stream_classify)"""
    ctx._chk(lib().kslam_set_sam_seq(ctx._h, int(on)))


def get_sam_seq(ctx):
    on = C.c_int()
    ctx._chk(lib().kslam_get_sam_seq(ctx._h, C.byref(on)))
    return bool(on.value)


def without_qualities(reads):
    """a copy of a tail.Reads view that says "no qualities" (quality == NULL); it keeps `reads` alive"""
    v = _T.ReadsView(reads.view.n_reads, reads.view.bases, reads.view.bases_off, None, reads.view.quality_off, reads.view.ids,
                     reads.view.ids_off)

    class _View:
        pass

    out = _View()
    out.view, out._keep = v, reads
    return out


def tail_sam_seq(params, reads, index, overlaps, cigar_pool, bam=False):
    """kslam_tail_sam_seq (host) -> (SAM text or BAM records with SEQ / QUAL as bytes, stats)"""
    L = lib()
    ov, pov = _T._ov(overlaps)
    pool = np.ascontiguousarray(cigar_pool, dtype=np.uint32)
    out, n, st = C.c_void_p(), C.c_uint64(), _T.TailStats()
    _T._chk(L.kslam_tail_sam_seq(C.byref(params), C.byref(reads.view), C.byref(index.view), pov, len(ov),
                                 _T._p(pool) if len(pool) else None, len(pool), int(bam), C.byref(out), C.byref(n), C.byref(st)))
    return _T._text(out, n), st


def tail_finish_rows_seq(params, reads, index, overlaps, cigar_pool, details, md_pool, read_pairs, pairs, bam=False):
    """kslam_tail_finish_write_rows_seq (host) -> (bytes, stats); read_pairs and pairs are MODIFIED in place, details / md_pool
    may be None"""
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
    _T._chk(L.kslam_tail_finish_write_rows_seq(
        C.byref(params), C.byref(reads.view), C.byref(index.view), pov, len(ov), _T._p(pool) if len(pool) else None, len(pool),
        _T._p(det) if det is not None and len(det) else None, _T._p(md) if len(md) else None, len(md),
        _T._p(read_pairs) if len(read_pairs) else None, len(read_pairs), _T._p(pairs) if len(pairs) else None, len(pairs),
        int(bam), cb, None, C.byref(st)))
    return b"".join(chunks), st
