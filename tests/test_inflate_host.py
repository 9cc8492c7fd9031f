"""include/kslam_inflate.h without a GPU: the yardstick itself (tests/inflate_ref.py equals zlib on every case of
tests/inflate_cases.py, every case holds the seam it is named for, every corrupt case is refused for the intended reason), and
the host's walk over the members, kslam_bgzf_scan, at its edges."""
import ctypes
import gzip
import importlib
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import inflate_cases as Cs
import inflate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def valid():
    return Cs.valid_cases()


@pytest.fixture(scope="module")
def reports(valid):
    """name -> (text by inflate_ref, [Report per member]), computed once"""
    return {k: R.inflate(blob) for k, (blob, _) in valid.items()}


@pytest.fixture(scope="module")
def Z(kslam):
    return importlib.import_module("kslam_amd.inflate")


def test_reference_inflater_equals_zlib(valid, reports):
    assert len(valid) == 3 * 8 + 1 + 5
    for name, (blob, text) in valid.items():
        assert gzip.decompress(blob) == text, name          # the case is what every other reader makes of it
        assert reports[name][0] == text, name


def test_every_case_holds_its_seam(valid, reports):
    def all_blocks(name):
        return [b for rep in reports[name][1] for b in rep.blocks]

    def agg(name, field):
        return max(getattr(rep, field) for rep in reports[name][1])

    for name, (blob, _) in valid.items():
        assert len(R.members(blob)) >= (3 if name.split("_")[0] in ("fastq", "random", "zeros") else 1), name
    for data in ("fastq", "random", "zeros"):
        assert {b[0] for b in all_blocks(data + "_level0")} == {0}
        # Z_FIXED: fixed Huffman blocks, except that zlib still stores what does not compress
        assert {b[0] for b in all_blocks(data + "_fixed")} == ({0} if data == "random" else {1})
        assert agg(data + "_huffman_only", "max_distance") == 0
    # random bytes at memLevel 1 do not fit a member of 65 280: the chunks were halved
    assert len(R.members(valid["random_mem1"][0])) > len(R.members(valid["random_level6"][0]))
    assert 2 in {b[0] for b in all_blocks("fastq_level6")} and 2 in {b[0] for b in all_blocks("fastq_huffman_only")}
    # memLevel 1 ends a block every 127 symbols or so: 91 dynamic blocks in a member of this text, each with tables of its own
    assert max(len(rep.blocks) for rep in reports["fastq_mem1"][1]) >= 64
    assert any({1, 2} <= set(rep.types) for rep in reports["fastq_mem1"][1])        # fixed and dynamic blocks mixed in one member
    assert agg("zeros_rle", "max_distance") == 1 and agg("fastq_rle", "max_distance") == 1
    assert agg("zeros_level6", "max_length") == 258 and agg("zeros_level6", "max_distance") == 1      # overlapping copies
    # codes longer than the kernel's direct tables (9 bits literal/length, 6 bits distance) take its canonical walk
    assert max(agg(k, "max_ll_len") for k in valid) > 9 and max(agg(k, "max_d_len") for k in valid) > 6
    assert agg("fastq_level9", "max_distance") > 16384
    flush = all_blocks("flushes")
    assert sum(1 for b in flush if b == (0, 0)) == 10 and len(reports["flushes"][1]) == 1
    far = reports["far_32768"][1][0]
    assert far.max_distance == 32768 and far.first_byte_match and far.types == [1]
    assert max(agg(k, "max_distance") for k in valid if k.split("_")[0] in ("fastq", "random", "zeros")) < 32768   # zlib stops short of it
    rle = reports["rle_258"][1][0]
    assert (rle.max_length, rle.max_distance, rle.first_byte_match) == (258, 1, True)
    assert reports["match_to_the_end"][1][0].max_length == 5 and len(valid["match_to_the_end"][1]) == 10
    assert valid["one_literal"][1] == b"x" and reports["one_literal"][1][0].max_length == 0
    assert reports["repeat_crossing"][1][0].repeat_crossed and reports["repeat_crossing"][1][0].types == [2]
    assert not any(rep.repeat_crossed for k in valid if k != "repeat_crossing" for rep in reports[k][1])       # zlib never does


def test_every_corrupt_case_is_refused_for_its_reason(Z):
    bad = Cs.corrupt_cases()
    assert len(bad) == 11 and R.KINDS == Z.ERROR_KINDS
    for name, (blob, index, kind) in bad.items():
        with pytest.raises(R.InflateError) as e:
            R.inflate(blob)
        assert (e.value.member, e.value.kind) == (index, kind), name
        assert len(R.members(blob)) == 3                     # the framing is intact: only inflating finds it
    # zlib refuses them too (whatever it calls the reason)
    for name, (blob, _, _) in bad.items():
        with pytest.raises((zlib.error, gzip.BadGzipFile, EOFError)):
            gzip.decompress(blob)
            pytest.fail(name)


def test_library_exports_every_inflate_symbol(kslam, Z):
    """the header/module pair as tests/test_abi_and_dist.py asks of the others"""
    h = open(os.path.join(ROOT, "include", "kslam_inflate.h")).read()
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S))))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 4 and declared == sorted(Z.EXPORTS) and all(hasattr(L, n) for n in declared)
    needed = subprocess.run(["readelf", "-d", kslam.LIB_PATH], capture_output=True, text=True).stdout
    assert "libz" not in needed                                 # the inflater is ours


def test_header_is_plain_c(tmp_path):
    import shutil
    src = tmp_path / "h.c"
    src.write_text('#include "kslam_inflate.h"\nint main(void) { return 0; }\n')
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        if not shutil.which(cc):
            pytest.skip(cc + " not available")
        r = subprocess.run([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", lang,
                            str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _refused(Z, kslam, blob, status):
    with pytest.raises(kslam.KslamError) as e:
        Z.scan(blob)
    assert e.value.status == status, str(e.value)
    return str(e.value)


def test_scan_counts_and_lengths(Z):
    text = Cs.fastq_text(1000, seed=9)
    one = Cs.member(Cs.deflate_raw(text), text)
    assert Z.scan(b"") == (0, 0)
    assert Z.scan(one) == (1, 1000)                                              # no EOF marker
    assert Z.scan(one + Cs.EOF_MARKER) == (2, 1000)
    assert Z.scan(one * 3 + Cs.EOF_MARKER) == (4, 3000)
    assert Z.scan(one + Cs.EOF_MARKER + one + Cs.EOF_MARKER) == (4, 2000)       # cat a.gz b.gz: an empty member in the middle
    assert Z.scan(Cs.EOF_MARKER) == (1, 0)
    assert Z.is_gzip(one) and Z.is_gzip(gzip.compress(text)) and not Z.is_gzip(text) and not Z.is_gzip(b"") and not Z.is_gzip(b"\x1f")
    blob, data = Cs.bgzf(Cs.fastq_text(3 * Cs.CHUNK + 5)), None
    assert Z.scan(blob) == (4, 3 * Cs.CHUNK + 5)


def test_scan_refuses_truncation_and_plain_gzip(Z, kslam):
    text = Cs.fastq_text(1000, seed=9)
    one = Cs.member(Cs.deflate_raw(text), text)
    for cut in (1, 8, len(one) - 18, len(one) - 17, len(one) - 3, len(one) - 1):   # inside the trailer, the data, the header
        msg = _refused(Z, kslam, one + one[:-cut], ERR_ARG)
        assert "member 1" in msg and "byte offset %d" % len(one) in msg, msg
    big = bytearray(one + one)                                                       # BSIZE past the end
    big[len(one) + 16:len(one) + 18] = (len(one) + 99).to_bytes(2, "little")
    msg = _refused(Z, kslam, bytes(big), ERR_ARG)
    assert "member 1" in msg and "byte offset %d" % len(one) in msg and "BSIZE" in msg
    msg = _refused(Z, kslam, gzip.compress(text), ERR_UNSUPPORTED)
    assert "bgzip" in msg and "plain gzip" in msg
    msg = _refused(Z, kslam, one + gzip.compress(text), ERR_UNSUPPORTED)
    assert "member 1" in msg and "bgzip" in msg
    _refused(Z, kslam, one + b"trailing text, not a member", ERR_ARG)


def test_scan_accepts_the_projects_own_bgzf_output(Z):
    """the bytes --sam-bgzf writes for the golden SAM text: Python's gzip stands in for the GPU writer's framing here (the GPU
    round trip is tests/test_gpu_inflate.py); what is scanned is BGZF exactly as csrc/bgzf.hip frames it"""
    sam = np.load(os.path.join(ROOT, "tests", "golden", "slam_loop.npz"))["a_sam"].tobytes()
    blob = Cs.bgzf(sam, level=1, strategy=zlib.Z_FIXED) + Cs.EOF_MARKER
    assert Z.scan(blob) == ((len(sam) + Cs.CHUNK - 1) // Cs.CHUNK + 1, len(sam))
