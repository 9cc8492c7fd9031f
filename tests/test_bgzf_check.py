"""tests/bgzf_check.py, the validator the GPU tests of include/kslam_bgzf.h rely on: it accepts BGZF as Python's zlib
writes it (fixed Huffman) and rejects six corruptions."""
import gzip
import os
import struct
import zlib

import pytest

import bgzf_check as B


def _member(data, strategy=zlib.Z_FIXED):
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, strategy)
    body = c.compress(data) + c.flush()
    size = 18 + len(body) + 8
    head = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, ord("B"), ord("C"), 2, 0]) + struct.pack("<H", size - 1)
    return head + body + struct.pack("<II", zlib.crc32(data), len(data))


def _file(data, strategy=zlib.Z_FIXED):
    return b"".join(_member(data[i:i + B.MAX_INPUT], strategy) for i in range(0, len(data), B.MAX_INPUT)) + B.EOF_MARKER


@pytest.fixture(scope="module")
def text():
    import random
    rnd = random.Random(7)
    lines = [b"read%d\t%d\tNC_%04d\t%d\t60\t150M\t=\t%d\t300\t*\t*\tNM:i:0\tAS:i:%d\n" %
             (i, rnd.choice((99, 147, 83, 163)), rnd.randrange(20), rnd.randrange(10 ** 6), rnd.randrange(10 ** 6), rnd.randrange(300))
             for i in range(4000)]
    return b"".join(lines) + os.urandom(1000)


def test_accepts_fixed_huffman_bgzf(text):
    blob = _file(text)
    ms = B.members(blob)
    assert len(ms) == (len(text) + B.MAX_INPUT - 1) // B.MAX_INPUT + 1
    assert B.check(blob) == text
    assert gzip.decompress(blob) == text
    assert B.check(B.EOF_MARKER) == b""


def test_rejects_corruptions(text):
    good = _file(text)
    first = B.members(good)[0]
    bad = {}
    b = bytearray(good)                                      # BSIZE one too small
    struct.pack_into("<H", b, 16, first[1] - 2)
    bad["bsize"] = bytes(b)
    bad["no_eof"] = good[:-28]
    bad["early_empty"] = _member(text[:1000]) + B.EOF_MARKER + _member(text[1000:2000]) + B.EOF_MARKER
    b = bytearray(good)                                      # CRC32 of the first member
    b[first[1] - 8] ^= 1
    bad["crc"] = bytes(b)
    bad["plain_gzip"] = gzip.compress(text[:5000]) + B.EOF_MARKER
    b = bytearray(_file(text[:3000]))                         # BTYPE 10 (dynamic Huffman) in the first member
    b[18] = (b[18] & ~6) | 4
    bad["btype10"] = bytes(b)
    for name, blob in bad.items():
        with pytest.raises(B.BgzfError):
            B.members(blob)
            pytest.fail(name)


def test_library_exports_every_bgzf_symbol(kslam):
    """include/kslam_bgzf.h is in the same library, and k-slam_amd/bgzf.py binds every symbol it declares"""
    import ctypes
    import importlib
    import re
    Z = importlib.import_module("kslam_amd.bgzf")
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kslam_bgzf.h")).read()
    eof = re.search(r'#define KSLAM_BGZF_EOF\s*\\?\s*"([^"]*)"', h).group(1)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S))))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert declared == sorted(Z.EXPORTS) and all(hasattr(L, n) for n in declared)
    assert Z.EOF == B.EOF_MARKER == bytes(int(x, 16) for x in eof.split("\\x")[1:])
