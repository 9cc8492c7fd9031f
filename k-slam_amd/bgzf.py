"""ctypes plumbing for include/kslam_bgzf.h: the SAM file as BGZF (blocked gzip), compressed on the GPU."""
import ctypes as C

from . import lib as _base_lib

EXPORTS = ["kslam_bgzf_compress", "kslam_set_sam_bgzf", "kslam_get_sam_bgzf", "kslam_set_bgzf_deflate", "kslam_get_bgzf_deflate"]
DEFLATE_FIXED, DEFLATE_DYNAMIC = 0, 1   # KSLAM_BGZF_DEFLATE_*
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # KSLAM_BGZF_EOF: an empty member
_ready = False


def lib():
    global _ready
    L = _base_lib()
    if not _ready:
        vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
        L.kslam_bgzf_compress.argtypes = [vp, C.c_char_p, u64, P(vp), P(u64)]
        L.kslam_set_sam_bgzf.argtypes = [vp, C.c_int]
        L.kslam_get_sam_bgzf.argtypes = [vp, P(C.c_int)]
        L.kslam_set_bgzf_deflate.argtypes = [vp, C.c_int]
        L.kslam_get_bgzf_deflate.argtypes = [vp, P(C.c_int)]
        _ready = True
    return L


def compress(ctx, data):
    """kslam_bgzf_compress: bytes -> BGZF members (no EOF marker; b"" for empty input)"""
    L = lib()
    data = bytes(data)
    out, n = C.c_void_p(), C.c_uint64()
    ctx._chk(L.kslam_bgzf_compress(ctx._h, data, len(data), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value) if n.value else b""
    finally:
        if out.value:
            L.kslam_free_pinned(ctx._h, out)


def set_sam_bgzf(ctx, on=True):
    """kslam_set_sam_bgzf: the lanes (and kslam_stream_classify) write the SAM text as BGZF"""
    ctx._chk(lib().kslam_set_sam_bgzf(ctx._h, int(on)))


def set_deflate(ctx, mode):
    """kslam_set_bgzf_deflate: DEFLATE_FIXED or DEFLATE_DYNAMIC, for every member the context compresses from now on"""
    ctx._chk(lib().kslam_set_bgzf_deflate(ctx._h, int(mode)))


def get_deflate(ctx):
    """kslam_get_bgzf_deflate"""
    mode = C.c_int()
    ctx._chk(lib().kslam_get_bgzf_deflate(ctx._h, C.byref(mode)))
    return mode.value
