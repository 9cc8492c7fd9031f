"""tests/bam_check.py, the reader the tests of include/kslam_bam.h rely on: it decodes hand-built records (bins at their edges)
and rejects each kind of malformed input; and kslam_bam.h's symbols are the ones k-slam_amd/bam.py binds."""
import ctypes
import importlib
import os
import re
import struct
import zlib

import pytest

import bam_check as B
import bgzf_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = b"@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:chrA\tLN:100000\tSP:7\n@SQ\tSN:chrB\tLN:50\n@PG\tID:SLAM\tPN:SLAM\tVN:1.0\tCL:\"x\"\n"
REFS = [(b"chrA", 100000), (b"chrB", 50)]


def header(text=TEXT, refs=REFS):
    h = B.MAGIC + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        h += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", ln)
    return h


def record(name=b"r1", flag=99, ref=0, pos=99, mapq=50, cigar=((5, 4), (90, 0), (2, 2), (5, 1)), nref=0, npos=300, tlen=250,
           tags=b"", bin_=None, name_nul=True):
    ops = b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar)
    span = sum(n for n, op in cigar if op in (0, 2)) if cigar and not flag & 4 else 0
    if bin_ is None:
        bin_ = B.reg2bin(pos, pos + max(1, span))
    rn = name + (b"\0" if name_nul else b"")
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(rn), mapq, bin_, len(cigar), flag, 0, nref, npos, tlen) + rn + ops + tags
    return struct.pack("<i", len(body)) + body


def tag_i(t, v, typ=None):
    typ = typ or B.int_type(v)
    return t + typ.encode() + struct.pack(B.INT_TYPES[typ], v)


def tag_z(t, s):
    return t + b"Z" + s + b"\0"


def bgzf(data):
    out = b""
    for i in range(0, len(data), bgzf_check.MAX_INPUT):
        chunk = data[i:i + bgzf_check.MAX_INPUT]
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)   # (the one block type bgzf_check takes besides stored)
        body = c.compress(chunk) + c.flush()
        out += bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", 25 + len(body)) + body + \
            struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return out + bgzf_check.EOF_MARKER


def test_reg2bin_edges():
    assert B.reg2bin(-1, 0) == 4680
    assert B.reg2bin(0, 1) == 4681
    assert B.reg2bin(16383, 16384) == 4681
    assert B.reg2bin(16383, 16385) == 585          # crosses a 16 kb bin: one level up
    assert B.reg2bin(16384, 16385) == 4682


def test_decodes_hand_built_records():
    tags = tag_z(b"MD", b"90^AC5") + tag_i(b"AS", 180) + tag_i(b"XS", 300) + tag_i(b"NM", 2) + tag_i(b"X0", 1) + \
        tag_i(b"XT", 70000) + tag_z(b"XR", b'"a product"') + tag_i(b"zz", -5) + tag_i(b"zy", -200) + tag_i(b"zx", -40000)
    recs = [record(tags=tags),
            record(name=b"r1", flag=0x185, pos=-1, mapq=0, cigar=(), nref=0, npos=100, tlen=-250),    # unmapped, POS 0
            record(name=b"s", flag=0, pos=16380, cigar=((10, 0),), nref=-1, npos=-1, tlen=0),        # crosses 16384
            record(name=b"e", flag=0, ref=1, pos=0, cigar=(), nref=-1, npos=-1, tlen=0)]             # mapped, empty CIGAR
    text = B.check(bgzf(header() + b"".join(recs)))
    lines = text[len(TEXT):].split(b"\n")
    assert text.startswith(TEXT) and lines[-1] == b""
    assert lines[0] == b"r1\t99\tchrA\t100\t50\t5S90M2D5I\t=\t301\t250\t*\t*\tMD:Z:90^AC5\tAS:i:180\tXS:i:300\tNM:i:2\tX0:i:1\t" \
                       b"XT:i:70000\tXR:Z:\"a product\"\tzz:i:-5\tzy:i:-200\tzx:i:-40000"
    assert lines[1] == b"r1\t389\tchrA\t0\t0\t*\t=\t101\t-250\t*\t*"
    assert lines[2] == b"s\t0\tchrA\t16381\t50\t10M\t*\t0\t0\t*\t*"
    assert lines[3] == b"e\t0\tchrB\t1\t50\t*\t*\t0\t0\t*\t*"
    assert struct.unpack_from("<H", recs[1], 14)[0] == 4680 and struct.unpack_from("<H", recs[3], 14)[0] == 4681
    assert struct.unpack_from("<H", recs[2], 14)[0] == 585


@pytest.mark.parametrize("what", ["magic", "block_size", "nul", "bin", "width", "truncated", "sq", "trailing", "tagtype"])
def test_rejects(what):
    good = header() + record(tags=tag_i(b"AS", 10))
    B.decode(good)
    if what == "magic":
        bad = b"BAM\x02" + good[4:]
    elif what == "block_size":
        r = record(tags=tag_i(b"AS", 10))
        bad = header() + struct.pack("<i", struct.unpack_from("<i", r)[0] + 3) + r[4:] + b"\0\0\0"
    elif what == "nul":
        bad = header() + record(name_nul=False)
    elif what == "bin":
        bad = header() + record(bin_=4681 + 7)
    elif what == "width":
        bad = header() + record(tags=tag_i(b"AS", 10, "S"))
    elif what == "truncated":
        bad = good[:-1]
    elif what == "sq":
        bad = header(refs=[(b"chrA", 100000), (b"chrB", 51)])
    elif what == "trailing":
        bad = good + b"\0\0"
    else:
        bad = header() + record(tags=b"ASf" + struct.pack("<f", 1.0))
    with pytest.raises(B.BamError):
        B.decode(bad)


def _declared(header_name):
    h = open(os.path.join(ROOT, "include", header_name)).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    return sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))


def test_bam_header_symbols_are_bound_and_exported(kslam):
    M = importlib.import_module("kslam_amd.bam")
    L = ctypes.CDLL(kslam.LIB_PATH)
    declared = _declared("kslam_bam.h")
    assert sorted(M.EXPORTS) == declared and len(declared) == 6
    for name in declared:
        assert hasattr(L, name), "missing export " + name
    assert M.TEXT_SAM_BAM == 16
