"""ctypes plumbing for include/kslam_gunzip.h: plain gzip input (.fastq.gz as gzip, pigz and the sequencers write it), inflated
in parallel on the GPU."""
import ctypes as C

from . import KslamError, lib as _base_lib

EXPORTS = ["kslam_gunzip_header", "kslam_gunzip_inflate", "kslam_gunzip_last_stats", "kslam_gunzip_set_chunk", "kslam_gunzip_set_round"]
DEFAULT_CHUNK = 32 * 1024           # include/kslam_gunzip.h: KSLAM_GUNZIP_CHUNK_DEFAULT -- compressed bytes per chunk
MIN_CHUNK = 1024                    # KSLAM_GUNZIP_CHUNK_MIN
DEFAULT_ROUND = 256 * 1024 * 1024   # KSLAM_GUNZIP_ROUND_DEFAULT -- symbols per round
WINDOW = 32768                      # csrc/gunzip.h: GUNZIP_WINDOW
# the kinds of error kslam_gunzip_inflate names besides those of kslam_bgzf_inflate (k-slam_amd/inflate.py: ERROR_KINDS)
HEADER, NOT_MEMBER = "gzip header", "not a gzip member"
_ready = False


class Stats(C.Structure):
    """kslam_gunzip_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("members", "chunks", "starts_found", "starts_live", "starts_dropped", "rounds", "text_len")] + \
               [(n, C.c_double) for n in ("find_ms", "count_ms", "decode_ms", "window_ms", "resolve_ms", "check_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def lib():
    global _ready
    L = _base_lib()
    if not _ready:
        vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
        L.kslam_gunzip_header.argtypes = [C.c_char_p, u64, P(u64)]
        L.kslam_gunzip_inflate.argtypes = [vp, C.c_char_p, u64, P(vp), P(u64)]
        L.kslam_gunzip_set_chunk.argtypes = [vp, u64]
        L.kslam_gunzip_set_round.argtypes = [vp, u64]
        L.kslam_gunzip_last_stats.argtypes = [vp, P(Stats)]
        L.kslam_tail_last_error.restype = C.c_char_p
        _ready = True
    return L


def header(blob):
    """kslam_gunzip_header: the offset of the first member's deflate data; host only, raises KslamError with its message"""
    L = lib()
    blob = bytes(blob)
    at = C.c_uint64()
    st = L.kslam_gunzip_header(blob, len(blob), C.byref(at))
    if st != 0:
        raise KslamError(st, L.kslam_tail_last_error().decode())
    return at.value


def inflate(ctx, blob):
    """kslam_gunzip_inflate: any gzip file -> the text of all its members"""
    L = lib()
    blob = bytes(blob)
    out, n = C.c_void_p(), C.c_uint64()
    ctx._chk(L.kslam_gunzip_inflate(ctx._h, blob, len(blob), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value) if n.value else b""
    finally:
        if out.value:
            L.kslam_free_pinned(ctx._h, out)


def set_chunk(ctx, n_bytes):
    """kslam_gunzip_set_chunk: compressed bytes per chunk (0: the default)"""
    ctx._chk(lib().kslam_gunzip_set_chunk(ctx._h, n_bytes))


def set_round(ctx, symbols):
    """kslam_gunzip_set_round: symbols of scratch per round (0: the default)"""
    ctx._chk(lib().kslam_gunzip_set_round(ctx._h, symbols))


def stats(ctx):
    """kslam_gunzip_last_stats as a dict"""
    s = Stats()
    ctx._chk(lib().kslam_gunzip_last_stats(ctx._h, C.byref(s)))
    return s.as_dict()
