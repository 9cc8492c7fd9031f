"""The host twin of the depth track (kslam_tail_depth) and the bedGraph writer (kslam_depth_write, include/kslam_depth.h) against
the plain-Python restatement (tests/depth_ref.py): the seam and tile cases the device is held to, the variants' case list and
seeded random cases, the file byte for byte against lines formatted here, and the refusals.  No GPU."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref as D  # noqa: E402
import variants_ref as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEAMS = D.seam_cases()
OTHERS = D.tile_cases() + [c for c in V.cases() if not c["name"].startswith(("walk-col", "run-", "distinct"))]


@pytest.fixture(scope="module")
def DP(kslam):
    return importlib.import_module("kslam_amd.depth")


@pytest.fixture(scope="module")
def T(kslam):
    return importlib.import_module("kslam_amd.tail")


def twin(DP, c, min_depth=1):
    return DP.tail_depth(c["goff"], c["ov"], c["pool"], c["roff"], c["rp"], c["pr"], min_depth)


def _check(DP, c, min_depth=1):
    rows, stats = D.table(c, min_depth)
    got, got_stats = twin(DP, c, min_depth)
    assert D.fields(got) == rows, c["name"]
    assert got_stats == stats, c["name"]
    return rows, stats


def test_library_exports_every_depth_symbol(kslam, DP):
    h = open(os.path.join(ROOT, "include", "kslam_depth.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 11 and declared == sorted(DP.EXPORTS) and all(hasattr(L, n) for n in declared)
    assert DP.ROW_DT.itemsize == 16 and DP.ROW_DT == D.ROW_DT and ctypes.sizeof(DP.Stats) == 56 and DP.STAT_NAMES == D.STAT_NAMES
    assert kslam.lib().kslam_abi_version() == 10             # additive: the version stays
    assert ctypes.sizeof(kslam.BatchResult) == 232


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_host_twin_on_the_seams(DP, name):
    case, expected, skipped = SEAMS[name]
    rows, stats = _check(DP, case)
    assert rows == expected and stats["n_skipped"] == skipped


@pytest.mark.parametrize("case", OTHERS, ids=[c["name"] for c in OTHERS])
def test_host_twin_matches_the_restatement(DP, case):
    _check(DP, case)


def test_filter(DP):
    c = D.filter_case()
    for m in (0, 1, 2, 3, 4):
        _check(DP, c, m)
    assert D.fields(twin(DP, c, 2)[0]) == [(0, 5, 10, 2), (0, 10, 20, 3), (0, 20, 25, 2)]


def test_40_random_cases(DP):
    for seed in range(40):
        _check(DP, V.random_case("random-%d" % seed, seed, 1 + 5 * seed, 1 + seed % 9, 1 + (37 * seed) % 300), 1 + seed % 3)


def _index(T, c, loci):
    return T.IndexArrays(c["gbases"], c["goff"], loci, np.arange(1, len(loci) + 1))


def test_the_file_byte_for_byte(DP, T):
    a, b, _ = D.random_cases()
    for c in (V.concat(a, b), SEAMS["seam-one-covered"][0], SEAMS["all-skipped"][0], SEAMS["identical-70001"][0]):
        n = len(c["goff"]) - 1
        loci = [b"LOCUS_%d.%d" % (e, e % 3) for e in range(n)]
        for m in (1, 2):
            rows, _ = twin(DP, c, m)
            text = DP.report_bytes(_index(T, c, loci), rows)
            assert text == b"".join(b"%s\t%d\t%d\t%d\n" % (loci[e], s, t, v) for e, s, t, v in D.fields(rows)), c["name"]
            assert DP.parse_bedgraph(text) == [(loci[e].decode(), s, t, v) for e, s, t, v in D.fields(rows)]
    assert DP.report_bytes(_index(T, c, loci), D.as_array([])) == b""
    big = D.as_array([(0, 0, 4294967295, 4294967295)])
    assert DP.report_bytes(_index(T, c, loci), big) == b"LOCUS_0.0\t0\t4294967295\t4294967295\n"
    with pytest.raises(ValueError):
        DP.parse_bedgraph(b"chr\t1\t2\n")


def test_refusals(DP, T):
    b = V.Builder("x", [b"ACGT" * 25, b"TTTT"])
    b.group([(0, b.aligned(0, 0, [(20, "M")], 0), b.aligned(0, 30, [(20, "M")], 1))])
    b.single(b.aligned(1, 0, [(4, "M")], 0))
    c = b.done()
    rows, _ = twin(DP, c)
    assert D.fields(rows) == [(0, 0, 20, 1), (0, 30, 50, 1), (1, 0, 4, 1)]
    args = lambda **kw: [kw.get(k, c[k]) for k in ("goff", "ov", "pool", "roff", "rp", "pr")]   # noqa: E731
    bad = c["pr"].copy()
    bad["r2"][0] = len(c["ov"])
    with pytest.raises(Exception, match="refers to overlap record"):
        DP.tail_depth(*args(pr=bad))
    rp = c["rp"].copy()
    rp["count"][1] = 2
    with pytest.raises(Exception, match="outside the pairs array"):
        DP.tail_depth(*args(rp=rp))
    rp = c["rp"].copy()
    rp["first"][1] = 0
    with pytest.raises(Exception, match="ascend"):
        DP.tail_depth(*args(rp=rp))
    ov = c["ov"].copy()
    ov["cigar_off"][1] = len(c["pool"])
    with pytest.raises(Exception, match="CIGAR slice lies outside the pool"):
        DP.tail_depth(*args(ov=ov))
    ov = c["ov"].copy()
    ov["read"][2] = len(c["roff"]) - 1
    with pytest.raises(Exception, match="refers to read"):
        DP.tail_depth(*args(ov=ov))
    roff = c["roff"].copy()
    roff[1] = roff[2] + 1
    with pytest.raises(Exception, match="read offsets must ascend"):
        DP.tail_depth(*args(roff=roff))
    # the writer: an entry with an empty locus is refused before anything is written; an entry outside the view too
    fd = os.memfd_create("bedgraph")
    try:
        with pytest.raises(Exception, match="empty locus"):
            DP.write(_index(T, c, [b"first", b""]), rows, fd)
        wrong = rows.copy()
        wrong["entry"][-1] = 2
        with pytest.raises(Exception, match="not of this index"):
            DP.write(_index(T, c, [b"first", b"second"]), wrong, fd)
        assert os.lseek(fd, 0, os.SEEK_END) == 0
    finally:
        os.close(fd)
