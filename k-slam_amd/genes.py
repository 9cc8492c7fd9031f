"""ctypes plumbing for include/kslam_genes.h: the per-gene abundance table counted on the GPU (alignments, unique read pairs and
overlapping bases per annotated gene), its host twin, the table writer and a parser for the file."""
import ctypes as C

import numpy as np

from . import tail as _T

# every symbol include/kslam_genes.h declares
EXPORTS = ["kslam_genes_add", "kslam_genes_kernel_ms", "kslam_genes_lookup", "kslam_genes_reset", "kslam_genes_take", "kslam_genes_write",
           "kslam_get_genes", "kslam_set_genes", "kslam_stream_get_genes", "kslam_stream_set_genes", "kslam_tail_genes"]
ROW_DT = np.dtype([("gene", "<u8"), ("alignments", "<u8"), ("unique_read_pairs", "<u8"), ("overlap_bases", "<u8")])
HEADER = (b"#entry\tlocus\ttaxid\tgene\tstart\tstop\tlength\tname\tprotein_id\tproduct\talignments\tunique_read_pairs\toverlap_bases"
          b"\trpk\ttpm\n")
_TEXT = ("locus", "name", "protein_id", "product")
_FLOAT = ("rpk", "tpm")
_ready = False


class Stats(C.Structure):
    _fields_ = [("n_alignments", C.c_uint64), ("n_in_gene", C.c_uint64), ("n_no_gene", C.c_uint64), ("n_skipped", C.c_uint64),
                ("n_rows", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def lib():
    global _ready
    L = _T.lib()
    if not _ready:
        vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
        L.kslam_set_genes.argtypes = [vp, C.c_int]
        L.kslam_get_genes.argtypes = [vp, P(C.c_int)]
        L.kslam_genes_reset.argtypes = [vp]
        L.kslam_genes_add.argtypes = [vp, vp, u64, vp, u64]
        L.kslam_genes_take.argtypes = [vp, P(vp), P(u64), P(Stats)]
        L.kslam_genes_lookup.argtypes = [vp, vp, vp, vp, u64, vp, vp, C.c_int]
        L.kslam_genes_kernel_ms.argtypes = [vp, P(C.c_double), P(C.c_double), P(C.c_double)]
        L.kslam_tail_genes.argtypes = [P(_T.IndexView), vp, u64, vp, u64, P(vp), P(u64), P(Stats)]
        L.kslam_genes_write.argtypes = [P(_T.IndexView), vp, u64, C.c_int]
        L.kslam_stream_set_genes.argtypes = [vp, C.c_int]
        L.kslam_stream_get_genes.argtypes = [vp, P(C.c_int)]
        L.kslam_free_pinned.argtypes = [vp, vp]
        L.kslam_free_pinned.restype = None
        _ready = True
    return L


class GeneIndex:
    """An index view (.view, as kslam_amd.tail.Index) over gene columns that already are arrays: entry e owns the genes
    gene_first[e] .. gene_first[e + 1]; starts / stops are int32 and may be anything; names / protein_ids / products are lists of
    bytes (default: empty).  The entries themselves have no bases: entry_lengths only lays out bases_off."""

    def __init__(self, gene_first, starts, stops, names=None, protein_ids=None, products=None, locus_tags=None, taxonomy_ids=None,
                 entry_lengths=None):
        first = np.ascontiguousarray(gene_first, dtype=np.uint64)
        n, g = len(first) - 1, len(starts)
        gs, ge = np.ascontiguousarray(starts, dtype=np.int32), np.ascontiguousarray(stops, dtype=np.int32)
        lengths = np.zeros(n, dtype=np.uint64) if entry_lengths is None else np.asarray(entry_lengths, dtype=np.uint64)
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
        bases = np.zeros(int(off[-1]) + 1, dtype=np.uint8)
        tax = np.zeros(max(n, 1), dtype=np.uint32)
        if taxonomy_ids is not None:
            tax[:n] = taxonomy_ids
        lc = _T._column(locus_tags if locus_tags is not None else [b"entry%d" % i for i in range(n)])
        cols = [_T._column(list(c) if c is not None else [b""] * g) for c in (names, protein_ids, products)]
        self._keep = [first, gs, ge, off, bases, tax, lc, cols]
        self.gene_first, self.starts, self.stops = first, gs, ge
        p = _T._p
        v = _T.IndexView(n, p(bases), p(off), p(lc[0]), p(lc[1]), p(tax))
        v.n_genes = g
        v.gene_first, v.gene_start, v.gene_stop = p(first), p(gs), p(ge)
        v.gene_name, v.gene_name_off = p(cols[0][0]), p(cols[0][1])
        v.protein_id, v.protein_id_off = p(cols[1][0]), p(cols[1][1])
        v.product, v.product_off = p(cols[2][0]), p(cols[2][1])
        self.view = v


def _arrays(read_pairs, pairs):
    rp = np.ascontiguousarray(read_pairs, dtype=_T.READ_PAIR_DT)
    pr = np.ascontiguousarray(pairs, dtype=_T.PAIRED_OVERLAP_DT)
    ptr = lambda a: a.ctypes.data if len(a) else None   # noqa: E731
    return (rp, pr), (ptr(rp), len(rp), ptr(pr), len(pr))


def set_genes(ctx, on=True):
    """kslam_set_genes: needs an index, ctx.set_pairing and kslam_amd.samtext.set_annotations first; switching on builds the
    lookup index and zeroes the table, off frees it"""
    ctx._chk(lib().kslam_set_genes(ctx._h, int(on)))


def get_genes(ctx):
    on = C.c_int()
    ctx._chk(lib().kslam_get_genes(ctx._h, C.byref(on)))
    return bool(on.value)


def reset(ctx):
    ctx._chk(lib().kslam_genes_reset(ctx._h))


def add(ctx, read_pairs, pairs):
    """kslam_genes_add: one batch's arrays (READ_PAIR_DT, PAIRED_OVERLAP_DT) from the host into the table"""
    keep, args = _arrays(read_pairs, pairs)
    ctx._chk(lib().kslam_genes_add(ctx._h, *args))


def take(ctx):
    """kslam_genes_take -> (rows: ROW_DT array of the genes with alignments > 0 in gene order, statistics as a dict)"""
    L = lib()
    rows, n, st = C.c_void_p(), C.c_uint64(), Stats()
    ctx._chk(L.kslam_genes_take(ctx._h, C.byref(rows), C.byref(n), C.byref(st)))
    out = _T.rows_at(rows.value, n.value, ROW_DT)
    L.kslam_free_pinned(ctx._h, rows)
    return out, st.as_dict()


def lookup(ctx, entries, starts, stops, linear=False):
    """kslam_genes_lookup -> (genes: int64, -1 none, -2 entry outside; shared: int64)"""
    e = np.ascontiguousarray(entries, dtype=np.uint32)
    b, t = np.ascontiguousarray(starts, dtype=np.int32), np.ascontiguousarray(stops, dtype=np.int32)
    n = len(e)
    assert len(b) == n and len(t) == n
    genes, shared = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    ptr = lambda a: a.ctypes.data if len(a) else None   # noqa: E731
    ctx._chk(lib().kslam_genes_lookup(ctx._h, ptr(e), ptr(b), ptr(t), n, ptr(genes), ptr(shared), int(linear)))
    return genes, shared


def kernel_ms(ctx):
    """(device ms of the last switch-on's index build, of the last kslam_genes_add's count passes, of the last take)"""
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    ctx._chk(lib().kslam_genes_kernel_ms(ctx._h, C.byref(a), C.byref(b), C.byref(c)))
    return float(a.value), float(b.value), float(c.value)


def tail_genes(index, read_pairs, pairs):
    """kslam_tail_genes (host twin) -> (rows, statistics as a dict); index: anything with .view"""
    keep, args = _arrays(read_pairs, pairs)
    rows, n, st = C.c_void_p(), C.c_uint64(), Stats()
    _T._chk(lib().kslam_tail_genes(C.byref(index.view), *args, C.byref(rows), C.byref(n), C.byref(st)))
    return _T._take(rows, n.value, ROW_DT), st.as_dict()


def write(index, rows, fd):
    """kslam_genes_write: index anything with .view (its gene columns), rows a ROW_DT array"""
    r = np.ascontiguousarray(rows, dtype=ROW_DT)
    _T._chk(lib().kslam_genes_write(C.byref(index.view), r.ctypes.data if len(r) else None, len(r), int(fd)))


def table_bytes(index, rows):
    """the file as bytes (through a pipe-free temporary descriptor)"""
    return _T.fd_bytes("kslam_genes", lambda fd: write(index, rows, fd))


def stream_set_genes(ctx, fd):
    """kslam_stream_set_genes: the descriptor the NEXT kslam_stream_classify on ctx writes its gene table to (-1: none)"""
    ctx._chk(lib().kslam_stream_set_genes(ctx._h, int(fd) if fd is not None else -1))


def parse(text):
    """the file's lines -> list of dicts (locus, name, protein_id, product as str; rpk, tpm as float; the rest as int); raises
    ValueError on another header"""
    if isinstance(text, str):
        text = text.encode()
    if not text.startswith(HEADER):
        raise ValueError("not a gene table: the header line is missing")
    names = HEADER[1:-1].decode().split("\t")
    out = []
    for line in text[len(HEADER):].split(b"\n"):
        if not line:
            continue
        f = line.decode().split("\t")
        if len(f) != len(names):
            raise ValueError("a gene line has %d fields" % len(f))
        out.append({k: v if k in _TEXT else float(v) if k in _FLOAT else int(v) for k, v in zip(names, f)})
    return out
