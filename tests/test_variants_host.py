"""The host twin of the SNV table (kslam_tail_variants) and the VCF writer (kslam_variants_write, include/kslam_variants.h)
against the plain-Python restatement (tests/variants_ref.py): the case list the device is held to and seeded random cases, the
file byte for byte against the restatement's writer, the refusals, and a planted-truth case.  No GPU."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import variants_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()


@pytest.fixture(scope="module")
def VR(kslam):
    return importlib.import_module("kslam_amd.variants")


@pytest.fixture(scope="module")
def T(kslam):
    return importlib.import_module("kslam_amd.tail")


def twin(VR, c, min_alt=1, min_depth=0):
    return VR.tail_variants(c["gbases"], c["goff"], c["ov"], c["pool"], c["rbases"], c["roff"], c["rp"], c["pr"], min_alt, min_depth)


def _check(VR, c, min_alt=1, min_depth=0):
    rows, stats = R.table(c, min_alt, min_depth)
    got, got_stats = twin(VR, c, min_alt, min_depth)
    assert R.fields(got) == R.fields(rows), c["name"]
    assert got_stats == stats, c["name"]
    return rows, stats


def test_the_restatement_itself():
    b = R.Builder("x", [b"ACGTACGTAC", b"GGGGG"])
    b.single(b.rec(b.read(b"ACCTAC"), 0, 0, b.cigar([(6, "M")])))                 # G -> C at 2
    b.single(b.rec(b.read(R.reverse_complement(b"CTACGT")), 0, 1, b.cigar([(2, "M"), (1, "D"), (4, "M")]), 1))   # G -> T at 2, pos 3 deleted
    b.single(b.rec(b.read(b"GGNgA"), 1, 0, b.cigar([(5, "M")])))                  # N and lower case: no event; G -> A at 4
    rows, stats = R.table(b.done())
    assert R.fields(rows) == [(0, 2, ord("G"), ord("C"), 1, 0, 2), (0, 2, ord("G"), ord("T"), 0, 1, 2), (1, 4, ord("G"), ord("A"), 1, 0, 1)]
    assert stats == {"n_records": 3, "n_skipped": 0, "n_intervals": 4, "n_events": 3, "n_sites": 3}
    text = R.vcf_bytes(rows, [b"one", b"two"], [10, 5], b"v1")
    assert text.endswith(b"two\t5\t.\tG\tA\t.\t.\tDP=1;AO=1;SAF=1;SAR=0;AF=1.000000\n") and b"##contig=<ID=one,length=10>\n" in text
    assert b"one\t3\t.\tG\tC\t.\t.\tDP=2;AO=1;SAF=1;SAR=0;AF=0.500000\n" in text
    assert R.read_vcf(text, [b"one", b"two"], [10, 5]) == R.fields(rows)


def test_library_exports_every_variants_symbol(kslam, VR):
    h = open(os.path.join(ROOT, "include", "kslam_variants.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 10 and declared == sorted(VR.EXPORTS) and all(hasattr(L, n) for n in declared)
    assert VR.ROW_DT.itemsize == 24 and VR.ROW_DT == R.ROW_DT and ctypes.sizeof(VR.Stats) == 40 and VR.COLUMNS == R.COLUMNS
    assert kslam.lib().kslam_abi_version() == 10             # additive: the version stays
    assert ctypes.sizeof(kslam.BatchResult) == 232           # kslam_batch_result keeps its size: callers allocate it


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_twin_matches_the_restatement(VR, case):
    _check(VR, case)


def test_what_the_cases_are_there_for(VR):
    by = {c["name"]: c for c in CASES}
    for col in R.WALK_COLUMNS:
        for strand in ("fwd", "rev"):
            rows, stats = _check(VR, by["walk-col%d-%s" % (col, strand)])
            assert [(r[1], r[4], r[5], r[6]) for r in R.fields(rows)] == [(50 + col, int(strand == "fwd"), int(strand == "rev"), 1)]
    rows, stats = _check(VR, by["walk-all-fwd"])
    assert stats["n_events"] == 21 and stats["n_sites"] == 18 and {r[1]: (r[4], r[5], r[6]) for r in R.fields(rows)}[50] == (1, 1, 2)
    rows, _ = _check(VR, by["cigar-split-fwd"])
    depth = {r[1]: r[6] for r in R.fields(rows)}
    assert depth[30 + 19] == 2 and depth[30 + 25] == 2 and {depth[p] for p in range(50, 55) if p in depth} == {1}   # the deleted positions: the plain read alone
    rows, _ = _check(VR, by["cigar-m-i-m-fwd"])
    depth = {r[1]: r[6] for r in R.fields(rows)}
    assert depth[39] == 2 and depth[40] == 2                  # adjacent intervals: no gap
    rows, stats = _check(VR, by["alphabet-fwd"])
    assert [r[1] for r in R.fields(rows)] == [20, 21, 35] and [r[6] for r in R.fields(rows)] == [2, 2, 2] and stats["n_events"] == 4
    rows, _ = _check(VR, by["entries-fwd"])
    got = {(r[0], r[1]): r[6] for r in R.fields(rows)}
    assert got[(0, 0)] == 1 and got[(1, 62)] == 2 and got[(2, 0)] == 2 and got[(1, 0)] == 1 and got[(3, 64)] == 2 and got[(2, 63)] == 1
    rows, _ = _check(VR, by["depth"])
    assert R.fields(rows) == [(0, 100, rows[0]["ref"], rows[0]["alt"], 1, 0, 4)]
    rows, stats = _check(VR, by["depth-20000"])
    assert [(r[4], r[6]) for r in R.fields(rows)] == [(20000, 20000)] and stats["n_intervals"] == 20000
    rows, stats = _check(VR, by["run-70001"])
    assert [(r[4], r[5], r[6]) for r in R.fields(rows)] == [(70001, 0, 70001)] and stats["n_sites"] == 1
    rows, stats = _check(VR, by["distinct-70001"])
    assert len(rows) == 70001 == stats["n_sites"] == stats["n_events"] and set(rows["depth"][:-2].tolist()) == {3} and rows["depth"][-2:].tolist() == [2, 2]
    rows, _ = _check(VR, by["alts"])
    assert [(r[1], r[4], r[5], r[6]) for r in R.fields(rows)] == [(22, 1, 2, 9)] * 3 and len(set(rows["alt"].tolist())) == 3
    rows, stats = _check(VR, by["contributing"])
    assert stats["n_records"] == 4 and 3 not in rows["entry"].tolist()
    assert {(r[0], r[1]): (r[4], r[5], r[6]) for r in R.fields(rows)}[(1, 34)] == (1, 1, 2)   # the reverse record is named by three live pairs and counts once; its mate adds the forward event
    rows, stats = _check(VR, by["skipped"])
    assert stats["n_skipped"] == 7 and stats["n_records"] == 10 and len(rows) == 3
    rows, stats = _check(VR, by["grid-70001"])
    assert stats["n_skipped"] >= 7 and stats["n_events"] > 20000
    rows, stats = _check(VR, by["grid-0"])
    assert len(rows) == 0 and stats == dict.fromkeys(R.STAT_NAMES, 0)


def test_filters(VR):
    c = R.filter_case()
    seen = {}
    for min_alt in (1, 2, 3):
        for min_depth in (4, 5, 6):
            rows, _ = _check(VR, c, min_alt, min_depth)
            seen[(min_alt, min_depth)] = [r[1] for r in R.fields(rows)]
    assert seen[(1, 5)] == [40, 45, 50] and seen[(2, 5)] == [40, 50] and seen[(3, 5)] == [50] and seen[(2, 4)] == [40, 50] and seen[(1, 6)] == []


def test_60_random_cases(VR):
    for seed in range(60):
        _check(VR, R.random_case("random-%d" % seed, seed, 1 + 5 * seed, 1 + seed % 9, 1 + (37 * seed) % 300), 1 + seed % 3, seed % 4)


def _index(T, c, loci):
    return T.IndexArrays(c["gbases"], c["goff"], loci, np.arange(1, len(loci) + 1))


def test_the_file_byte_for_byte(kslam, VR, T):
    source = kslam.lib().kslam_version().split()[0]
    for c in [c for c in CASES if c["name"] in ("alts", "contributing", "entries-rev", "skipped", "grid-70001", "grid-0", "alphabet-fwd")]:
        n = len(c["goff"]) - 1
        loci = [b"LOCUS_%d.%d" % (e, e % 3) for e in range(n)]
        lengths = np.diff(c["goff"].astype(np.int64))
        for min_alt in (1, 2):
            rows, stats = twin(VR, c, min_alt, 1)
            text = VR.report_bytes(_index(T, c, loci), rows, stats)
            assert text == R.vcf_bytes(rows, loci, lengths, source), c["name"]
            assert R.read_vcf(text, loci, lengths) == R.fields(rows)
            meta, parsed = VR.parse_vcf(text)
            assert meta[0] == "fileformat=VCFv4.2" and meta[1] == "source=" + source.decode()
            assert [(loci.index(r["chrom"].encode()), r["pos"] - 1, r["ref"], r["alt"], r["SAF"], r["SAR"], r["DP"]) for r in parsed] == \
                [(e, p, chr(a), chr(b), f, v, d) for e, p, a, b, f, v, d in R.fields(rows)]
    with pytest.raises(ValueError):
        VR.parse_vcf(b"##fileformat=VCFv4.2\nchr\t1\n")
    # DP == 0 is written as AF 0.000000 (no row of the table has it: the writer's own rule)
    row = np.zeros(1, dtype=VR.ROW_DT)
    row["ref"], row["alt"], row["alt_fwd"] = ord("A"), ord("C"), 1
    assert VR.report_bytes(_index(T, c, loci), row).endswith(b"\t1\t.\tA\tC\t.\t.\tDP=0;AO=1;SAF=1;SAR=0;AF=0.000000\n")


def test_refusals(VR, T):
    b = R.Builder("x", [b"ACGT" * 25, b"TTTT"])
    b.group([(0, b.aligned(0, 0, [(20, "M")], 0, mismatch_at=(3,)), b.aligned(0, 30, [(20, "M")], 1, mismatch_at=(3,)))])
    b.single(b.aligned(1, 0, [(4, "M")], 0, mismatch_at=(0,)))
    c = b.done()
    rows, _ = twin(VR, c)
    assert len(rows) == 3
    args = lambda **kw: [kw.get(k, c[k]) for k in ("gbases", "goff", "ov", "pool", "rbases", "roff", "rp", "pr")]   # noqa: E731
    bad = c["pr"].copy()
    bad["r2"][0] = len(c["ov"])
    with pytest.raises(Exception, match="refers to overlap record"):
        VR.tail_variants(*args(pr=bad))
    rp = c["rp"].copy()
    rp["count"][1] = 2
    with pytest.raises(Exception, match="outside the pairs array"):
        VR.tail_variants(*args(rp=rp))
    rp = c["rp"].copy()
    rp["first"][1] = 0
    with pytest.raises(Exception, match="ascend"):
        VR.tail_variants(*args(rp=rp))
    ov = c["ov"].copy()
    ov["cigar_off"][1] = len(c["pool"])
    with pytest.raises(Exception, match="CIGAR slice lies outside the pool"):
        VR.tail_variants(*args(ov=ov))
    ov = c["ov"].copy()
    ov["read"][2] = len(c["roff"]) - 1
    with pytest.raises(Exception, match="refers to read"):
        VR.tail_variants(*args(ov=ov))
    # the writer: an entry with an empty locus is refused before anything is written; an entry outside the view too
    fd = os.memfd_create("vcf")
    try:
        with pytest.raises(Exception, match="empty locus"):
            VR.write(_index(T, c, [b"first", b""]), rows, fd)
        wrong = rows.copy()
        wrong["entry"][-1] = 2
        with pytest.raises(Exception, match="not of this index"):
            VR.write(_index(T, c, [b"first", b"second"]), wrong, fd)
        assert os.lseek(fd, 0, os.SEEK_END) == 0
    finally:
        os.close(fd)


# ---- planted truth

def test_planted_truth(VR):
    entry, sites, reads = R.planted()
    positions = sorted(sites)
    assert len(positions) == 100 and min(np.diff(positions)) >= 200
    c = R.planted_case(entry, reads)
    rows, stats = _check(VR, c, 1, 0)
    over = {p: sum(1 for _, at, _ in reads if at <= p < at + 100) for p in positions}
    assert [(r[1], r[3]) for r in R.fields(rows)] == [(p, sites[p]) for p in positions]          # exactly the planted sites, the planted base
    assert all(r[4] + r[5] == r[6] == over[r[1]] for r in R.fields(rows))
    assert sum(r[4] for r in R.fields(rows)) > 300 and sum(r[5] for r in R.fields(rows)) > 300   # reads of both strands
    assert stats["n_skipped"] == 0 and stats["n_records"] == len(reads) == stats["n_intervals"]
    # what the aligner's test (tests/test_gpu_variants.py) leans on: every planted site has at least 4 reads whose copy of it
    # lies 3 or more bases from both read ends, so clipped read ends cannot take a site below min_alt = 2
    inner = {p: sum(1 for _, at, _ in reads if at + 3 <= p < at + 100 - 3) for p in positions}
    assert min(inner.values()) >= 4
