"""include/kslam_gunzip.h without a GPU: the library exports what the header declares and k-slam_amd/gunzip.py lists, the
header is plain C, and the host's header walk, kslam_gunzip_header, on every header shape and at every truncation length."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest

import gunzip_cases as Gc
import gunzip_ref as G
import inflate_cases as Cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1


@pytest.fixture(scope="module")
def Z(kslam):
    return importlib.import_module("kslam_amd.gunzip")


def test_library_exports_every_gunzip_symbol(kslam, Z):
    h = open(os.path.join(ROOT, "include", "kslam_gunzip.h")).read()
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S))))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 5 and declared == sorted(Z.EXPORTS) and all(hasattr(L, n) for n in declared)
    needed = subprocess.run(["readelf", "-d", kslam.LIB_PATH], capture_output=True, text=True).stdout
    assert "libz" not in needed                                 # the inflater is ours
    assert ctypes.sizeof(Z.Stats) == 7 * 8 + 6 * 8
    assert (Z.DEFAULT_CHUNK, Z.MIN_CHUNK, Z.DEFAULT_ROUND) == tuple(
        eval(re.search(r"#define %s \(?([^)/\n]*)" % n, h).group(1).replace("u", "")) for n in
        ("KSLAM_GUNZIP_CHUNK_DEFAULT", "KSLAM_GUNZIP_CHUNK_MIN", "KSLAM_GUNZIP_ROUND_DEFAULT"))


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "kslam_gunzip.h"\nint main(void) { kslam_gunzip_stats s; s.members = 0; return (int)s.members; }\n')
    ran = 0
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        if not shutil.which(cc):
            continue
        r = subprocess.run([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", lang,
                            str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        ran += 1
    assert ran, "no C compiler to check the header with"


def _shapes():
    """every combination of FEXTRA / FNAME / FCOMMENT / FHCRC, with fields of several lengths"""
    text = Cs.fastq_text(300, seed=3)
    out = []
    for flags in range(0, 32, 2):
        for extra, name, comment in ((b"", b"", b""), (b"\x01\x02\x03", b"a.fq", b"c"), (bytes(300), b"n" * 70, b"lane 1, run 7")):
            out.append((flags, Gc.gz(text, flags=flags, extra=extra, name=name, comment=comment)))
    return out


def _refused(Z, kslam, blob):
    with pytest.raises(kslam.KslamError) as e:
        Z.header(blob)
    assert e.value.status == ERR_ARG and "member 0 (byte offset 0)" in str(e.value), str(e.value)
    return str(e.value).rsplit(": ", 1)[1]


def test_header_walk_on_every_shape_and_every_truncation(kslam, Z):
    shapes = _shapes()
    assert len(shapes) == 16 * 3
    for flags, blob in shapes:
        at = G.header(blob)
        assert Z.header(blob) == at and Z.header(blob[:at]) == at, flags       # the header alone is a whole header
        if not flags:
            assert at == 10
        for cut in range(at):                                                    # every shorter piece is refused, and for the reason the restatement gives
            with pytest.raises(G.GunzipError) as e:
                G.header(blob[:cut])
            assert _refused(Z, kslam, blob[:cut]) == e.value.kind, (flags, cut)
            assert e.value.kind == (G.NOT_MEMBER if cut < 2 else G.HEADER)


def test_header_walk_refuses_what_is_no_gzip_header(kslam, Z):
    blob = Gc.gz(b"text")
    assert _refused(Z, kslam, b"") == G.NOT_MEMBER
    assert _refused(Z, kslam, b"\x1f\x8c" + blob[2:]) == G.NOT_MEMBER
    assert _refused(Z, kslam, b"@r\nACGT\n+\nFFFF\n") == G.NOT_MEMBER
    assert _refused(Z, kslam, blob[:2] + b"\x07" + blob[3:]) == G.HEADER       # method 7
    for bit in (0x20, 0x40, 0x80):                                             # the reserved FLG bits
        assert _refused(Z, kslam, blob[:3] + bytes([bit]) + blob[4:]) == G.HEADER
    assert Z.header(Cs.EOF_MARKER) == 18                                       # a BGZF member is a gzip member with an FEXTRA field
