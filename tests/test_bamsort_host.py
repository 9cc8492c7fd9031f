"""The host twins of the coordinate-sorted BAM (kslam_tail_bam_sort, kslam_tail_bai, kslam_tail_bam_sort_header; include/
kslam_bamsort.h) byte for byte against the restatement (tests/bamsort_ref.py) on the seam cases, their refusals, the exported
symbols, and the twins under ASan + UBSan through a stand-alone program (tools/bamsort_check.cpp).  No GPU."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_check  # noqa: E402
import bamsort_cases as BC  # noqa: E402
import bamsort_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = BC.cases()


@pytest.fixture(scope="module")
def BS(kslam):
    return importlib.import_module("kslam_amd.bamsort")


def test_library_exports_every_bamsort_symbol(kslam, BS):
    h = open(os.path.join(ROOT, "include", "kslam_bamsort.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 14 and declared == sorted(BS.EXPORTS) and all(hasattr(L, n) for n in declared)
    assert ctypes.sizeof(BS.Stats) == 56 and BS.TEXT_SAM_HELD == 128 and "KSLAM_TEXT_SAM_HELD 128u" in h
    assert kslam.lib().kslam_abi_version() == 10             # additive: the version stays


@pytest.mark.parametrize("name", sorted(CASES))
def test_twins_against_the_restatement(BS, name):
    stream = BS.tail_bam_sort(CASES[name])
    assert stream == R.sort_batches(CASES[name])
    head = BC.zlib_members(BS.tail_bam_sort_header(BC.SAM_HEADER))
    body = BC.zlib_members(stream)
    sizes, hlen = [len(m) for m in body], sum(len(m) for m in head)
    bai = BS.tail_bai(stream, len(BC.REFS), sizes, hlen)
    assert bai == R.bai(stream, len(BC.REFS), sizes, hlen)
    bai_check.check(b"".join(head) + b"".join(body) + BC.EOF, bai)
    parsed = BS.parse_bai(bai)
    assert len(parsed["refs"]) == 3 and parsed["n_no_coor"] == sum(R.fields(r)["ref"] < 0 for r in R.split(stream))


def test_header_twin(BS, kslam):
    T = importlib.import_module("kslam_amd.tail")
    for text in (BC.SAM_HEADER, b"@HD\tVN:1.6\n" + BC.SAM_HEADER[23:], BC.SAM_HEADER[23:], b"@HD\tSO:queryname\tGO:none\n", b""):
        refs = BC.REFS if b"@SQ" in text else []
        assert BS.tail_bam_sort_header(text) == R.bam_header(R.coordinate_header(text), refs)
    with pytest.raises(kslam.KslamError, match="@SQ"):
        BS.tail_bam_sort_header(b"@SQ\tSN:x\n")
    # for the library's own header text these are kslam_bam_header's bytes over the rewritten text
    B = importlib.import_module("kslam_amd.bam")
    import numpy as np
    goff = np.concatenate([[0], np.cumsum([n for _, n in BC.REFS])]).astype(np.uint64)
    index = T.IndexArrays(np.zeros(int(goff[-1]) + 8, dtype=np.uint8)[:int(goff[-1])], goff, [n for n, _ in BC.REFS], np.arange(1, 4))
    text = T.sam_header(index, b"SLAM x")
    assert BS.tail_bam_sort_header(text) == B.header(index, R.coordinate_header(text))
    assert b"SO:coordinate" in R.coordinate_header(text).split(b"\n")[0]


def test_refusals(BS, kslam):
    good = BC.rec(0, 5)
    for bad, what in ((good[:-1], "chain"), (good + b"\x01\x00", "chain"), (b"\x10\x00\x00\x00" + bytes(16), "fixed part"),
                      (good[:4] + good[4:12] + b"\xff" + good[13:], "fixed part")):
        with pytest.raises(kslam.KslamError, match=what) as e:
            BS.tail_bam_sort([good, bad])
        assert e.value.status == 1
        with pytest.raises(kslam.KslamError, match=what):
            BS.tail_bai(bad, 3, [50], 10)
    with pytest.raises(kslam.KslamError, match="member sizes"):
        BS.tail_bai(good, 3, [50, 50], 10)
    with pytest.raises(kslam.KslamError, match="n_ref"):
        BS.tail_bai(BC.rec(3, 5), 3, [50], 10)
    with pytest.raises(kslam.KslamError, match="not sorted"):
        BS.tail_bai(BC.rec(0, 6) + BC.rec(0, 5), 3, [50], 10)
    with pytest.raises(ValueError):
        BS.parse_bai(b"BAM\x01")
    with pytest.raises(ValueError):
        BS.parse_bai(R.bai(good, 3, [50], 10)[:-1])


def test_twins_under_asan_and_ubsan(tmp_path):
    """A stand-alone program (its own main, never loaded into Python) built with the address and undefined-behaviour sanitizers:
    every batch is a heap block of exactly its size, so a walk that reads past one fails the run."""
    gxx = shutil.which("g++")
    assert gxx
    exe = str(tmp_path / "bamsort_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", os.path.join(ROOT, "tools", "bamsort_check.cpp"),
                           os.path.join(ROOT, "k-slam_amd", "host", "bamsort.cpp"), "-o", exe])
    r = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("bamsort_check ok"), r.stdout + r.stderr


def test_cli_refusals_and_the_help_text(kslam, tmp_path):
    slam = os.path.join(ROOT, "k-slam_amd", "SLAM")
    run = lambda args: subprocess.run([slam] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)   # noqa: E731
    r = run(["--db", "d", "--sam-file", "o.bam", "--sam-index", "o.bai", "r.fq"])
    assert r.returncode != 0 and b"option '--sam-index' needs '--sam-sorted'" in r.stderr
    r = run(["--db", "d", "--sam-sorted", "r.fq"])
    assert r.returncode != 0 and b"option '--sam-sorted' needs '--sam-file'" in r.stderr
    r = run(["--db", "d", "--sam-sorted", "--sam-index", "r.fq"])
    assert r.returncode != 0
    assert not list(tmp_path.iterdir()) or [p.name for p in tmp_path.iterdir()] == ["log.txt"]      # nothing was opened
    assert run(["--help"]).stdout == open(os.path.join(ROOT, "tests", "golden", "slam_help.txt"), "rb").read()
