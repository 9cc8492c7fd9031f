"""ctypes plumbing for include/kslam_bamsort.h: the SAM file as a coordinate-sorted BAM with its BAI index, the records held,
sorted, gathered, compressed and indexed on the GPU; the host twins, and a parser for the index."""
import ctypes as C
import struct

import numpy as np

from . import tail as _T

# every symbol include/kslam_bamsort.h declares
EXPORTS = ["kslam_bam_sort_add", "kslam_bam_sort_kernel_ms", "kslam_bam_sort_reset", "kslam_bam_sort_set_gather", "kslam_bam_sort_set_segment",
           "kslam_bam_sort_set_slice", "kslam_bam_sort_take", "kslam_get_bam_sort", "kslam_set_bam_sort", "kslam_stream_get_bam_sort",
           "kslam_stream_set_bam_sort", "kslam_tail_bai", "kslam_tail_bam_sort", "kslam_tail_bam_sort_header"]
STAT_NAMES = ("n_records", "n_no_coor", "record_bytes", "compressed_bytes", "n_members", "n_chunks", "bytes_held")
TEXT_SAM_HELD = 128
MEMBER_IN = 65280
DEFAULT_SLICE = 16448 * MEMBER_IN
PSEUDO_BIN = 37450
KERNEL_MS_NAMES = ("append", "sort", "gather", "compress", "index")
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
        L.kslam_set_bam_sort.argtypes = [vp, C.c_int]
        L.kslam_get_bam_sort.argtypes = [vp, P(C.c_int)]
        L.kslam_bam_sort_add.argtypes = [vp, u64, vp, u64]
        L.kslam_bam_sort_reset.argtypes = [vp]
        L.kslam_bam_sort_set_slice.argtypes = [vp, u64]
        L.kslam_bam_sort_set_segment.argtypes = [vp, u32]
        L.kslam_bam_sort_set_gather.argtypes = [vp, u32]
        L.kslam_bam_sort_kernel_ms.argtypes = [vp, P(C.c_double)]
        L.kslam_bam_sort_take.argtypes = [vp, vp, u64, _T.WRITE_FN, vp, _T.WRITE_FN, vp, P(Stats)]
        L.kslam_stream_set_bam_sort.argtypes = [vp, C.c_int, C.c_int]
        L.kslam_stream_get_bam_sort.argtypes = [vp, P(C.c_int), P(C.c_int)]
        L.kslam_tail_bam_sort_header.argtypes = [vp, u64, P(vp), P(u64)]
        L.kslam_tail_bam_sort.argtypes = [P(vp), P(u64), u64, P(vp), P(u64)]
        L.kslam_tail_bai.argtypes = [vp, u64, u32, vp, u64, u64, P(vp), P(u64)]
        L.kslam_free.argtypes = [vp]
        L.kslam_free.restype = None
        _ready = True
    return L


def set_bam_sort(ctx, on=True):
    """kslam_set_bam_sort: needs an index; the lanes then hold their BAM records on the device; off frees the store"""
    ctx._chk(lib().kslam_set_bam_sort(ctx._h, int(on)))


def get_bam_sort(ctx):
    on = C.c_int()
    ctx._chk(lib().kslam_get_bam_sort(ctx._h, C.byref(on)))
    return bool(on.value)


def add(ctx, seq, records):
    """kslam_bam_sort_add: one batch's BAM records (bytes) as ordinal seq"""
    b = bytes(records)
    ctx._chk(lib().kslam_bam_sort_add(ctx._h, int(seq), C.c_char_p(b) if b else None, len(b)))


def reset(ctx):
    ctx._chk(lib().kslam_bam_sort_reset(ctx._h))


def set_slice(ctx, nbytes=0):
    ctx._chk(lib().kslam_bam_sort_set_slice(ctx._h, int(nbytes)))


def set_segment(ctx, records=0):
    ctx._chk(lib().kslam_bam_sort_set_segment(ctx._h, int(records)))


def set_gather(ctx, lanes=0):
    ctx._chk(lib().kslam_bam_sort_set_gather(ctx._h, int(lanes)))


def kernel_ms(ctx):
    """device ms by KERNEL_MS_NAMES: the last append, then the last take's sort, gather, compress and index"""
    ms = (C.c_double * 5)()
    ctx._chk(lib().kslam_bam_sort_kernel_ms(ctx._h, ms))
    return dict(zip(KERNEL_MS_NAMES, (float(x) for x in ms)))


def _collector(chunks):
    def cb(user, data, n):
        chunks.append(bytes((C.c_char * n).from_address(data)) if n else b"")
        return 0
    return _T.WRITE_FN(cb)


def take(ctx, sam_header, index=True):
    """kslam_bam_sort_take -> (the BAM file, the BAI index or None, stats: dict)"""
    h = bytes(sam_header)
    bam, bai, st = [], [], Stats()
    cb_bam, cb_bai = _collector(bam), _collector(bai)
    ctx._chk(lib().kslam_bam_sort_take(ctx._h, C.c_char_p(h) if h else None, len(h), cb_bam, None, cb_bai if index else C.cast(None, _T.WRITE_FN), None, C.byref(st)))
    return b"".join(bam), (b"".join(bai) if index else None), st.as_dict()


def take_fd(ctx, sam_header, bam_fd, bai_fd=None):
    """kslam_bam_sort_take writing to descriptors (kslam_write_fd) -> stats: dict"""
    L = lib()
    h = bytes(sam_header)
    st = Stats()
    wr = C.cast(L.kslam_write_fd, _T.WRITE_FN)
    f1, f2 = C.c_int(int(bam_fd)), C.c_int(int(bai_fd) if bai_fd is not None else -1)
    ctx._chk(L.kslam_bam_sort_take(ctx._h, C.c_char_p(h) if h else None, len(h), wr, C.addressof(f1), wr if bai_fd is not None else C.cast(None, _T.WRITE_FN),
                                   C.addressof(f2), C.byref(st)))
    return st.as_dict()


def stream_set_bam_sort(ctx, on=True, bai_fd=None):
    """kslam_stream_set_bam_sort: the NEXT kslam_stream_classify on ctx writes its SAM file as a coordinate-sorted BAM, and the
    index to bai_fd (None: no index)"""
    ctx._chk(lib().kslam_stream_set_bam_sort(ctx._h, int(bool(on)), int(bai_fd) if bai_fd is not None else -1))


def stream_get_bam_sort(ctx):
    on, fd = C.c_int(), C.c_int()
    ctx._chk(lib().kslam_stream_get_bam_sort(ctx._h, C.byref(on), C.byref(fd)))
    return bool(on.value), int(fd.value)


def _taken(L, out, n):
    data = bytes((C.c_char * n.value).from_address(out.value)) if n.value else b""
    L.kslam_free(out)
    return data


def tail_bam_sort_header(sam_header):
    """kslam_tail_bam_sort_header: the sorted file's BAM header, uncompressed"""
    L = lib()
    h = bytes(sam_header)
    out, n = C.c_void_p(), C.c_uint64()
    _T._chk(L.kslam_tail_bam_sort_header(C.c_char_p(h) if h else None, len(h), C.byref(out), C.byref(n)))
    return _taken(L, out, n)


def tail_bam_sort(batches):
    """kslam_tail_bam_sort (host twin): the batches' bytes in seq order -> the sorted record stream"""
    L = lib()
    keep = [bytes(b) for b in batches]
    ptrs = (C.c_void_p * max(len(keep), 1))(*[C.cast(C.c_char_p(b), C.c_void_p) if b else None for b in keep])
    lens = (C.c_uint64 * max(len(keep), 1))(*[len(b) for b in keep])
    out, n = C.c_void_p(), C.c_uint64()
    _T._chk(L.kslam_tail_bam_sort(ptrs, lens, len(keep), C.byref(out), C.byref(n)))
    return _taken(L, out, n)


def tail_bai(stream, n_ref, member_sizes, header_compressed_len):
    """kslam_tail_bai (host twin): the sorted record stream and the compressed size of each of its members -> the BAI bytes"""
    L = lib()
    s = bytes(stream)
    m = np.ascontiguousarray(member_sizes, dtype=np.uint32)
    out, n = C.c_void_p(), C.c_uint64()
    _T._chk(L.kslam_tail_bai(C.c_char_p(s) if s else None, len(s), int(n_ref), m.ctypes.data if len(m) else None, len(m), int(header_compressed_len),
                             C.byref(out), C.byref(n)))
    return _taken(L, out, n)


def parse_bai(data):
    """the BAI bytes -> {"refs": [{"bins": {bin: [(beg, end), ...]}, "pseudo": (beg, end, n_mapped, n_unmapped) or None, "ioffset": [...]}],
    "n_no_coor": int}; bins in file order (dicts keep it).  Raises ValueError for another magic, a truncated or an over-long file, a
    bin listed twice or a pseudo-bin without its two chunks."""
    data = bytes(data)
    if data[:4] != b"BAI\x01":
        raise ValueError("not a BAI index")
    pos = 4

    def get(fmt):
        nonlocal pos
        k = struct.calcsize(fmt)
        if pos + k > len(data):
            raise ValueError("truncated BAI index")
        v = struct.unpack_from(fmt, data, pos)
        pos += k
        return v

    (n_ref,) = get("<i")
    refs = []
    for _ in range(n_ref):
        (n_bin,) = get("<i")
        bins, pseudo = {}, None
        for _ in range(n_bin):
            b, n_chunk = get("<Ii")
            chunks = [get("<QQ") for _ in range(n_chunk)]
            if b == PSEUDO_BIN:
                if n_chunk != 2 or pseudo is not None:
                    raise ValueError("a pseudo-bin without its two chunks")
                pseudo = chunks[0] + chunks[1]
            else:
                if b in bins:
                    raise ValueError("bin %d is listed twice" % b)
                bins[b] = chunks
        (n_intv,) = get("<i")
        refs.append({"bins": bins, "pseudo": pseudo, "ioffset": list(get("<%dQ" % n_intv))})
    n_no_coor = get("<Q")[0] if pos < len(data) else None
    if pos != len(data):
        raise ValueError("bytes behind the end of the BAI index")
    return {"refs": refs, "n_no_coor": n_no_coor}
