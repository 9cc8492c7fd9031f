"""ctypes plumbing for include/kslam_taxreads.h: the reads of chosen taxa written back out as FASTQ (KrakenTools'
extract_kraken_reads.py without a second pass), selected on the GPU, with a host twin."""
import ctypes as C

import numpy as np

from . import readsplit as _RS
from . import tail as _T
from . import taxonomy as _X

# every symbol include/kslam_taxreads.h declares
EXPORTS = ["kslam_collect_taxon_reads", "kslam_get_taxon_reads", "kslam_set_taxon_reads", "kslam_stream_get_taxon_reads",
           "kslam_stream_set_taxon_reads", "kslam_tail_taxon_reads", "kslam_taxon_reads_kernel_ms", "kslam_taxon_reads_mask",
           "kslam_taxon_reads_text"]
CHILDREN, PARENTS, EXCLUDE = 1, 2, 4
_ready = False


def lib():
    global _ready
    L = _RS.lib()
    _X.lib()
    if not _ready:
        vp, u64, u32, P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
        L.kslam_set_taxon_reads.argtypes = [vp, vp, u64, u32]
        L.kslam_get_taxon_reads.argtypes = [vp, P(vp), P(u64), P(u32)]
        L.kslam_collect_taxon_reads.argtypes = [vp, u64, P(_RS.ReadsOut)]
        L.kslam_tail_taxon_reads.argtypes = [vp, vp, u64, u32, vp, u64, vp, u64, u64, C.c_int, vp, vp, u64, P(_RS.ReadsOut)]
        L.kslam_taxon_reads_text.argtypes = [vp, vp, u64, vp, u64, u64, C.c_int, vp, vp, u64, P(_RS.ReadsOut)]
        L.kslam_taxon_reads_mask.argtypes = [vp, P(vp), P(u64), P(vp), P(u64), P(C.c_int)]
        L.kslam_taxon_reads_kernel_ms.argtypes = [vp, P(C.c_double), P(C.c_double), P(C.c_double), P(u64)]
        L.kslam_stream_set_taxon_reads.argtypes = [vp, P(C.c_int * 2)]
        L.kslam_stream_get_taxon_reads.argtypes = [vp, P(C.c_int * 2)]
        L.kslam_free.argtypes = [vp]
        L.kslam_free.restype = None
        _ready = True
    return L


def _ids(ids):
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    return a, (a.ctypes.data if len(a) else None)


def set_taxon_reads(ctx, ids, mode=0):
    """kslam_set_taxon_reads: the chosen taxonomy ids and a mask of CHILDREN | PARENTS | EXCLUDE; no ids = off.  Needs
    kslam_amd.samtext.set_annotations with a taxdb and ctx.set_pairing first."""
    a, p = _ids(ids)
    ctx._chk(lib().kslam_set_taxon_reads(ctx._h, p, len(a), int(mode)))


def get_taxon_reads(ctx):
    """-> (ids: uint32 array, mode); an empty array with the switch off"""
    L = lib()
    p, n, mode = C.c_void_p(), C.c_uint64(), C.c_uint32()
    ctx._chk(L.kslam_get_taxon_reads(ctx._h, C.byref(p), C.byref(n), C.byref(mode)))
    out = _T.rows_at(p.value, n.value, np.dtype(np.uint32))
    L.kslam_free(p)
    return out, int(mode.value)


def _take(ctx, ro):
    out = _RS._take(ctx, ro)
    return {"blocks": out["blocks"][:2], "n_records": out["n_records"], "flags": out["flags"]}


def collect_taxon_reads(ctx, ticket):
    """kslam_collect_taxon_reads, after ctx.collect_batch(ticket) -> {"blocks": [selected R1, selected R2], "n_records", "flags"}"""
    ro = _RS.ReadsOut()
    ctx._chk(lib().kslam_collect_taxon_reads(ctx._h, ticket, C.byref(ro)))
    return _take(ctx, ro)


def tail_taxon_reads(taxdb, ids, mode, r1, r2, read_pairs, pair_tax_ids, max_pairs=0, at_eof=True):
    """kslam_tail_taxon_reads (host; taxdb: kslam_amd.taxonomy.TaxDB): r1 / r2 bytes (r2 None: single-end), read_pairs a
    READ_PAIR_DT array, pair_tax_ids the taxonomy id of each of them"""
    a, p = _ids(ids)
    rp, prp = _RS._pairs(read_pairs)
    t, pt = _ids(pair_tax_ids)
    assert len(t) == len(rp)
    ro = _RS.ReadsOut()
    _T._chk(lib().kslam_tail_taxon_reads(taxdb._h, p, len(a), int(mode), r1, len(r1), r2, len(r2) if r2 is not None else 0, max_pairs,
                                         int(at_eof), prp, pt, len(rp), C.byref(ro)))
    return _take(None, ro)


def taxon_reads_text(ctx, r1, r2, read_pairs, pair_tax_ids, max_pairs=0, at_eof=True):
    """kslam_taxon_reads_text (device, on ctx itself, with the S of set_taxon_reads): the same texts and pairs as tail_taxon_reads"""
    rp, prp = _RS._pairs(read_pairs)
    t, pt = _ids(pair_tax_ids)
    assert len(t) == len(rp)
    ro = _RS.ReadsOut()
    ctx._chk(lib().kslam_taxon_reads_text(ctx._h, r1, len(r1), r2, len(r2) if r2 is not None else 0, max_pairs, int(at_eof), prp, pt,
                                          len(rp), C.byref(ro)))
    return _take(ctx, ro)


def mask(ctx):
    """kslam_taxon_reads_mask -> (mask: uint8 array, one byte per node; unknown ids: uint32 array; all_nonzero: bool)"""
    L = lib()
    m, n, u, nu, a = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64(), C.c_int()
    ctx._chk(L.kslam_taxon_reads_mask(ctx._h, C.byref(m), C.byref(n), C.byref(u), C.byref(nu), C.byref(a)))
    hm = _T.rows_at(m.value, n.value, np.dtype(np.uint8))
    hu = _T.rows_at(u.value, nu.value, np.dtype(np.uint32))
    L.kslam_free(m)
    L.kslam_free(u)
    return hm, hu, bool(a.value)


def kernel_ms(ctx):
    """(mask ms of the last set_taxon_reads; flag ms, lengths + scans + copy ms and text bytes moved of the last taxon_reads_text)"""
    a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint64()
    ctx._chk(lib().kslam_taxon_reads_kernel_ms(ctx._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
    return float(a.value), float(b.value), float(c.value), int(n.value)


def stream_set_taxon_reads(ctx, fds):
    """kslam_stream_set_taxon_reads: two descriptors (selected R1, R2; -1 = not wanted) for the NEXT kslam_stream_classify on ctx,
    which selects by the ids of set_taxon_reads; None = none"""
    arr = (C.c_int * 2)(*[int(f) for f in fds]) if fds is not None else None
    ctx._chk(lib().kslam_stream_set_taxon_reads(ctx._h, C.byref(arr) if arr is not None else None))
