"""ctypes plumbing for include/kslam_inflate.h: BGZF-compressed input (.fastq.gz as bgzip writes it), inflated on the GPU."""
import ctypes as C

from . import KslamError, lib as _base_lib

EXPORTS = ["kslam_bgzf_inflate", "kslam_bgzf_inflate_kernel_ms", "kslam_bgzf_is_gzip", "kslam_bgzf_scan"]
WAVES_PER_WORKGROUP = 4    # csrc/inflate.h: INFLATE_WAVES -- members per workgroup, one wave each
DEFAULT_ROUND = 4096       # csrc/inflate.h: INFLATE_ROUND -- members per launch round unless KSLAM_INFLATE_ROUND says otherwise
# the kinds of member error kslam_bgzf_inflate names in kslam_last_error (csrc/inflate.hip: inflate_error_name)
ERROR_KINDS = ("bad block type", "stored length check", "code lengths over-subscribed", "code lengths incomplete", "invalid symbol",
               "distance too far back", "output overrun", "output underrun", "CRC mismatch", "deflate data length")
_ready = False


def lib():
    global _ready
    L = _base_lib()
    if not _ready:
        vp, u64, P = C.c_void_p, C.c_uint64, C.POINTER
        L.kslam_bgzf_is_gzip.argtypes = [C.c_char_p, u64]
        L.kslam_bgzf_is_gzip.restype = C.c_int
        L.kslam_bgzf_scan.argtypes = [C.c_char_p, u64, P(u64), P(u64)]
        L.kslam_bgzf_inflate.argtypes = [vp, C.c_char_p, u64, P(vp), P(u64)]
        L.kslam_bgzf_inflate_kernel_ms.argtypes = [vp, P(C.c_double)]
        L.kslam_tail_last_error.restype = C.c_char_p
        _ready = True
    return L


def is_gzip(blob):
    """kslam_bgzf_is_gzip: the two magic bytes"""
    blob = bytes(blob)
    return bool(lib().kslam_bgzf_is_gzip(blob, len(blob)))


def scan(blob):
    """kslam_bgzf_scan: (number of members, inflated length); host only, raises KslamError with the scan's message"""
    L = lib()
    blob = bytes(blob)
    n, t = C.c_uint64(), C.c_uint64()
    st = L.kslam_bgzf_scan(blob, len(blob), C.byref(n), C.byref(t))
    if st != 0:
        raise KslamError(st, L.kslam_tail_last_error().decode())
    return n.value, t.value


def inflate(ctx, blob):
    """kslam_bgzf_inflate: BGZF bytes -> the text (b"" for empty input or empty members only)"""
    L = lib()
    blob = bytes(blob)
    out, n = C.c_void_p(), C.c_uint64()
    ctx._chk(L.kslam_bgzf_inflate(ctx._h, blob, len(blob), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value) if n.value else b""
    finally:
        if out.value:
            L.kslam_free_pinned(ctx._h, out)


def kernel_ms(ctx):
    """kslam_bgzf_inflate_kernel_ms: device time of the last inflate()'s kernels on this context"""
    ms = C.c_double()
    ctx._chk(lib().kslam_bgzf_inflate_kernel_ms(ctx._h, C.byref(ms)))
    return ms.value
