"""ctypes plumbing for include/kslam_indels.h: the indel table piled up on the GPU (one row per entry, anchor, kind, length and
inserted bases, left-normalised, with its observations by strand and the depth at the anchor), its host twin, the VCF writer and
a parser for the file."""
import ctypes as C

import numpy as np

from . import tail as _T
from .variants import _arrays

# every symbol include/kslam_indels.h declares
EXPORTS = ["kslam_get_indels", "kslam_indels_add", "kslam_indels_kernel_ms", "kslam_indels_reset", "kslam_indels_take", "kslam_indels_write",
           "kslam_set_indels", "kslam_stream_get_indels", "kslam_stream_set_indels", "kslam_tail_indels"]
ROW_DT = np.dtype([("entry", "<u4"), ("pos", "<u4"), ("kind", "u1"), ("pad", "u1", (3,)), ("len", "<u4"), ("bases", "<u8"), ("alt_fwd", "<u4"),
                   ("alt_rev", "<u4"), ("depth", "<u4"), ("pad2", "<u4")])
STAT_NAMES = ("n_records", "n_skipped", "n_intervals", "n_deletions", "n_insertions", "n_unanchored", "n_long_del", "n_unrepresentable", "n_sites")
COLUMNS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
MAX_DEL, MAX_INS, DEL, INS = 65536, 32, 0, 1
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
        batch = [vp, u64, vp, u64, vp, vp, u64, vp, u64, vp, u64]   # overlaps, pool, read bases + offsets, read pairs, pairs
        L.kslam_set_indels.argtypes = [vp, C.c_int]
        L.kslam_get_indels.argtypes = [vp, P(C.c_int)]
        L.kslam_indels_reset.argtypes = [vp]
        L.kslam_indels_add.argtypes = [vp] + batch
        L.kslam_indels_take.argtypes = [vp, u32, u32, P(vp), P(u64), P(Stats)]
        L.kslam_indels_kernel_ms.argtypes = [vp, P(C.c_double), P(C.c_double)]
        L.kslam_tail_indels.argtypes = [vp, vp, u64] + batch + [u32, u32, P(vp), P(u64), P(Stats)]
        L.kslam_indels_write.argtypes = [P(_T.IndexView), vp, u64, P(Stats), C.c_int]
        L.kslam_stream_set_indels.argtypes = [vp, C.c_int, u32, u32]
        L.kslam_stream_get_indels.argtypes = [vp, P(C.c_int), P(u32), P(u32)]
        L.kslam_free_pinned.argtypes = [vp, vp]
        L.kslam_free_pinned.restype = None
        L.kslam_free.argtypes = [vp]
        L.kslam_free.restype = None
        _ready = True
    return L


def set_indels(ctx, on=True):
    """kslam_set_indels: needs an index, ctx.set_pairing and a context with report_cigar; off frees the state"""
    ctx._chk(lib().kslam_set_indels(ctx._h, int(on)))


def get_indels(ctx):
    on = C.c_int()
    ctx._chk(lib().kslam_get_indels(ctx._h, C.byref(on)))
    return bool(on.value)


def reset(ctx):
    ctx._chk(lib().kslam_indels_reset(ctx._h))


def add(ctx, overlaps, cigar_pool, read_bases, read_offsets, read_pairs, pairs):
    """kslam_indels_add: one batch's arrays from the host (as kslam_amd.variants.add)"""
    keep, args = _arrays(overlaps, cigar_pool, read_bases, read_offsets, read_pairs, pairs)
    ctx._chk(lib().kslam_indels_add(ctx._h, *args))


def take(ctx, min_alt=2, min_depth=1):
    """kslam_indels_take -> (rows: ROW_DT array, stats: dict)"""
    L = lib()
    rows, n, st = C.c_void_p(), C.c_uint64(), Stats()
    ctx._chk(L.kslam_indels_take(ctx._h, int(min_alt), int(min_depth), C.byref(rows), C.byref(n), C.byref(st)))
    out = _T.rows_at(rows.value, n.value, ROW_DT)
    L.kslam_free_pinned(ctx._h, rows)
    return out, st.as_dict()


def kernel_ms(ctx):
    """(device ms of the last kslam_indels_add's emit passes, of the last take)"""
    a, b = C.c_double(), C.c_double()
    ctx._chk(lib().kslam_indels_kernel_ms(ctx._h, C.byref(a), C.byref(b)))
    return float(a.value), float(b.value)


def tail_indels(entry_bases, entry_offsets, overlaps, cigar_pool, read_bases, read_offsets, read_pairs, pairs, min_alt=2, min_depth=1):
    """kslam_tail_indels (host twin) -> (rows, stats)"""
    L = lib()
    gb = np.ascontiguousarray(np.frombuffer(entry_bases, dtype=np.uint8) if isinstance(entry_bases, (bytes, bytearray)) else entry_bases, dtype=np.uint8)
    go = np.ascontiguousarray(entry_offsets, dtype=np.uint64)
    keep, args = _arrays(overlaps, cigar_pool, read_bases, read_offsets, read_pairs, pairs)
    rows, n, st = C.c_void_p(), C.c_uint64(), Stats()
    n_entries = max(len(go) - 1, 0)
    _T._chk(L.kslam_tail_indels(gb.ctypes.data if len(gb) else None, go.ctypes.data if n_entries else None, n_entries, *args, int(min_alt),
                                int(min_depth), C.byref(rows), C.byref(n), C.byref(st)))
    out = _T.rows_at(rows.value, n.value, ROW_DT)
    L.kslam_free(rows)
    return out, st.as_dict()


def write(index, rows, fd, stats=None):
    """kslam_indels_write: index a kslam_amd.tail index view (e.g. kslam_amd.db.Database), rows a ROW_DT array"""
    r = np.ascontiguousarray(rows, dtype=ROW_DT)
    st = None
    if stats is not None:
        st = Stats(*[int(stats[n]) for n in STAT_NAMES])
    _T._chk(lib().kslam_indels_write(C.byref(index.view), r.ctypes.data if len(r) else None, len(r), C.byref(st) if st is not None else None, int(fd)))


def report_bytes(index, rows, stats=None):
    """the VCF file as bytes (through a pipe-free temporary descriptor)"""
    return _T.fd_bytes("kslam_indels", lambda fd: write(index, rows, fd, stats))


def stream_set_indels(ctx, fd, min_alt=2, min_depth=1):
    """kslam_stream_set_indels: the descriptor the NEXT kslam_stream_classify on ctx writes its VCF file to (-1: none)"""
    ctx._chk(lib().kslam_stream_set_indels(ctx._h, int(fd) if fd is not None else -1, int(min_alt), int(min_depth)))


def bases_str(bases, length):
    """the inserted bases of a row as text"""
    return "".join("ACGT"[(int(bases) >> (2 * (length - 1 - j))) & 3] for j in range(length))


def parse(path):
    """the rows of a written file -> list of dicts: chrom, pos (1-based, the anchor), ref, alt, type ('del' / 'ins'), len, DP, AO, SAF,
    SAR as int, AF as float; raises ValueError for a file of another kind"""
    with open(path, "rb") as f:
        return parse_vcf(f.read())[1]


def parse_vcf(text):
    """the file's bytes -> (meta: the ## lines without the marker, rows as parse() gives them)"""
    if isinstance(text, bytes):
        text = text.decode()
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    meta, rows, seen_columns = [], [], False
    for line in lines:
        if line.startswith("##"):
            if seen_columns:
                raise ValueError("a ## line after the column line")
            meta.append(line[2:])
        elif line.startswith("#"):
            if line + "\n" != COLUMNS.decode() or seen_columns:
                raise ValueError("not the column line of a sites-only VCF file")
            seen_columns = True
        else:
            if not seen_columns:
                raise ValueError("a record before the column line")
            f = line.split("\t")
            if len(f) != 8:
                raise ValueError("a VCF line has %d fields" % len(f))
            info = dict(kv.split("=", 1) for kv in f[7].split(";"))
            if sorted(info) != ["AF", "AO", "DP", "LEN", "SAF", "SAR", "TYPE"] or f[2] != "." or f[5] != "." or f[6] != "." or info["TYPE"] not in ("del", "ins"):
                raise ValueError("a VCF line of another kind: " + line)
            rows.append({"chrom": f[0], "pos": int(f[1]), "ref": f[3], "alt": f[4], "type": info["TYPE"], "len": int(info["LEN"]), "DP": int(info["DP"]),
                         "AO": int(info["AO"]), "SAF": int(info["SAF"]), "SAR": int(info["SAR"]), "AF": float(info["AF"])})
    if not seen_columns or not meta or meta[0] != "fileformat=VCFv4.2":
        raise ValueError("not a VCF 4.2 file")
    return meta, rows
