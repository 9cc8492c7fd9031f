"""The host twin of the indel table (kslam_tail_indels) and the VCF writer (kslam_indels_write, include/kslam_indels.h) against
the plain-Python restatement (tests/indels_ref.py): the case list the device is held to, field for field and statistics
included, the file byte for byte against the restatement's writer, the refusals.  No GPU."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import indels_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()


@pytest.fixture(scope="module")
def ID(kslam):
    return importlib.import_module("kslam_amd.indels")


@pytest.fixture(scope="module")
def T(kslam):
    return importlib.import_module("kslam_amd.tail")


def twin(ID, c, min_alt=1, min_depth=0):
    return ID.tail_indels(c["gbases"], c["goff"], c["ov"], c["pool"], c["rbases"], c["roff"], c["rp"], c["pr"], min_alt, min_depth)


def _check(ID, c, min_alt=1, min_depth=0):
    rows, stats = R.table(c, min_alt, min_depth)
    got, got_stats = twin(ID, c, min_alt, min_depth)
    assert R.fields(got) == rows, c["name"]
    assert got_stats == stats, c["name"]
    assert not got["pad"].any() and not got["pad2"].any()
    return got, stats


def test_library_exports_every_indels_symbol(kslam, ID):
    h = open(os.path.join(ROOT, "include", "kslam_indels.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 10 and declared == sorted(ID.EXPORTS) and all(hasattr(L, n) for n in declared)
    assert ID.ROW_DT.itemsize == 40 and ctypes.sizeof(ID.Stats) == 72 and ID.COLUMNS == R.COLUMNS
    assert (ID.MAX_DEL, ID.MAX_INS, ID.DEL, ID.INS) == (R.MAX_DEL, R.MAX_INS, R.DEL, R.INS)
    assert "#define KSLAM_INDEL_MAX_DEL 65536u" in h and "#define KSLAM_INDEL_MAX_INS 32u" in h
    assert kslam.lib().kslam_abi_version() == 10             # additive: the version stays


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_twin_matches_the_restatement(ID, case):
    _check(ID, case)


def test_filters(ID):
    c = [c for c in CASES if c["name"] == "depth"][0]
    seen = {}
    for min_alt in (1, 2, 3, 4):
        for min_depth in (0, 1, 2, 3, 99):
            rows, _ = _check(ID, c, min_alt, min_depth)
            seen[(min_alt, min_depth)] = [r[:5] for r in R.fields(rows)]
    far = (0, 100, R.DEL, 1, b"")     # AO 3, DP 2
    assert far in seen[(3, 2)] and far not in seen[(3, 3)] and far not in seen[(4, 0)]
    assert seen[(3, 3)] == [(0, 49, R.DEL, 2, b""), (0, 49, R.INS, 2, b"AT")] and seen[(3, 2)] == seen[(3, 3)] + [far] and seen[(1, 99)] == []


def test_40_random_cases(ID):
    for seed in range(40):
        _check(ID, R.random_case("random-%d" % seed, 1000 + seed, 5 + 7 * seed, (b"AC", b"ACGT", b"AAAC", b"A")[seed % 4], 1 + seed % 5, 30 + 5 * seed),
               1 + seed % 3, seed % 3)


def _index(T, c, loci):
    return T.IndexArrays(c["gbases"], c["goff"], loci, np.arange(1, len(loci) + 1))


def test_the_file_byte_for_byte(kslam, ID, T):
    source = kslam.lib().kslam_version().split()[0]
    for c in [c for c in CASES if c["name"] in ("alphabet", "depth", "after-same-repeat", "tandem-3", "strands", "limits", "random-ac")]:
        n = len(c["goff"]) - 1
        loci = [b"LOCUS_%d.%d" % (e, e % 3) for e in range(n)]
        for min_alt in (1, 2):
            rows, stats = twin(ID, c, min_alt, 0)
            text = ID.report_bytes(_index(T, c, loci), rows, stats)
            assert text == R.vcf_bytes(R.fields(rows), c, loci, source), c["name"]
            meta, parsed = ID.parse_vcf(text)
            assert meta[0] == "fileformat=VCFv4.2" and meta[1] == "source=" + source.decode()
            for p, (e, pos, kind, ln, s, fwd, rev, dp) in zip(parsed, R.fields(rows)):
                ref = R.entry_bytes(c, e)
                assert (loci.index(p["chrom"].encode()), p["pos"] - 1, p["type"], p["len"], p["SAF"], p["SAR"], p["DP"]) == \
                    (e, pos, "del" if kind == R.DEL else "ins", ln, fwd, rev, dp)
                assert p["ref"][0] == p["alt"][0] == chr(ref[pos]) and abs(len(p["ref"]) - len(p["alt"])) == ln
            assert len(parsed) == len(rows)
    with pytest.raises(ValueError):
        ID.parse_vcf(b"##fileformat=VCFv4.2\nchr\t1\n")


def test_parse_reads_a_written_file(ID, T, tmp_path):
    c = [c for c in CASES if c["name"] == "homopolymer"][0]
    rows, stats = twin(ID, c)
    name = str(tmp_path / "x.vcf")
    fd = os.open(name, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    ID.write(_index(T, c, [b"chr"]), rows, fd, stats)
    os.close(fd)
    a = len(R.LEFT)
    got = ID.parse(name)     # all 17 records cover the anchor, the flank's last base
    assert [(r["chrom"], r["pos"], r["ref"], r["alt"], r["type"], r["len"], r["AO"], r["DP"]) for r in got] == \
        [("chr", a, "CA", "C", "del", 1, 8, 17), ("chr", a, "C", "CA", "ins", 1, 9, 17)]
    assert all(r["SAF"] + r["SAR"] == r["AO"] and r["SAR"] > 0 and abs(r["AF"] - r["AO"] / 17) < 1e-6 for r in got)
    assert ID.bases_str(int(rows["bases"][1]), 1) == "A"


def test_refusals(ID, T):
    b = R.Builder("x", [b"ACGT" * 25, b"TTGTT"])
    b.group([(0, R.al(b, 0, 0, R.split_at(40, 20, "D", 2), single=False), R.al(b, 0, 30, R.split_at(40, 20, "I", 2), rc=1, fill=b"GG", single=False))])
    R.al(b, 1, 0, [(2, "M"), (1, "D"), (2, "M")])
    c = b.done()
    rows, _ = twin(ID, c)
    assert len(rows) == 3
    args = lambda **kw: [kw.get(k, c[k]) for k in ("gbases", "goff", "ov", "pool", "rbases", "roff", "rp", "pr")]   # noqa: E731
    bad = c["pr"].copy()
    bad["r2"][0] = len(c["ov"])
    with pytest.raises(Exception, match="refers to overlap record"):
        ID.tail_indels(*args(pr=bad))
    rp = c["rp"].copy()
    rp["count"][1] = 2
    with pytest.raises(Exception, match="outside the pairs array"):
        ID.tail_indels(*args(rp=rp))
    rp = c["rp"].copy()
    rp["first"][1] = 0
    with pytest.raises(Exception, match="ascend"):
        ID.tail_indels(*args(rp=rp))
    ov = c["ov"].copy()
    ov["cigar_off"][1] = len(c["pool"])
    with pytest.raises(Exception, match="CIGAR slice lies outside the pool"):
        ID.tail_indels(*args(ov=ov))
    ov = c["ov"].copy()
    ov["read"][2] = len(c["roff"]) - 1
    with pytest.raises(Exception, match="refers to read"):
        ID.tail_indels(*args(ov=ov))
    # the writer: nothing is written for rows that cannot become lines
    fd = os.memfd_create("vcf")
    try:
        with pytest.raises(Exception, match="empty locus"):
            ID.write(_index(T, c, [b"first", b""]), rows, fd)
        good = _index(T, c, [b"first", b"second"])
        wrong = rows.copy()
        wrong["entry"][-1] = 2
        with pytest.raises(Exception, match="not of this index"):
            ID.write(good, wrong, fd)
        wrong = rows.copy()
        assert wrong["entry"][-1] == 1 and wrong["kind"][-1] == R.DEL and wrong["pos"][-1] == 1
        wrong["len"][-1] = 4                         # anchor 1 + 4 deleted bases: one past the entry of 5
        with pytest.raises(Exception, match="runs past the entry"):
            ID.write(good, wrong, fd)
        wrong["len"][-1] = 3                         # ... up to its last base: written
        wrong["pos"][-1] = 5
        with pytest.raises(Exception, match="outside the entry"):
            ID.write(good, wrong, fd)
        wrong = rows.copy()
        wrong["kind"][0] = 2
        with pytest.raises(Exception, match="kind"):
            ID.write(good, wrong, fd)
        wrong = rows.copy()
        wrong["len"][0] = 0
        with pytest.raises(Exception, match="len"):
            ID.write(good, wrong, fd)
        assert os.lseek(fd, 0, os.SEEK_END) == 0
        wrong = rows.copy()
        wrong["len"][-1] = 3
        ID.write(good, wrong, fd)
        assert os.lseek(fd, 0, os.SEEK_END) > 0
    finally:
        os.close(fd)
