"""The host twin of the per-gene abundance table (kslam_tail_genes) and the table writer (kslam_genes_write, include/kslam_genes.h)
against the plain-Python restatement (tests/genes_ref.py): the case list the device is held to and 150 seeded random cases; the
file byte for byte against the restatement's formatter and against a fixture worked out by hand.  No GPU."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genes_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()


@pytest.fixture(scope="module")
def GN(kslam):
    return importlib.import_module("kslam_amd.genes")


def _index(GN, c, **columns):
    return GN.GeneIndex(c["first"], c["starts"], c["stops"], **columns)


def test_the_restatement_itself():
    first, starts, stops = R.genes_of([[(100, 300), (50, 250)], [], [(0, 10)]])
    assert R.gene_of(first, starts, stops, 0, 100, 250) == (0, 150)     # both share 150: file order decides
    assert R.gene_of(first, starts, stops, 0, 60, 90) == (1, 30)
    assert R.gene_of(first, starts, stops, 0, 300, 400) == (R.NONE, 0)  # begins where the gene stops
    assert R.gene_of(first, starts, stops, 1, 0, 1000) == (R.NONE, 0) and R.gene_of(first, starts, stops, 3, 0, 5) == (R.SKIPPED, 0)
    assert R.gene_of(first, starts, stops, 2, 5, 3) == (R.NONE, 0)      # ref_end <= ref_start
    c, _, _, _ = R.small()
    rows, st = R.table(c)
    assert rows.tolist() == R.SMALL_ROWS and st == R.SMALL_STATS


def test_library_exports_every_genes_symbol(kslam, GN):
    h = open(os.path.join(ROOT, "include", "kslam_genes.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 11 and declared == sorted(GN.EXPORTS) and all(hasattr(L, n) for n in declared)
    assert GN.ROW_DT.itemsize == 32 and ctypes.sizeof(GN.Stats) == 40 and GN.HEADER == R.HEADER
    assert GN.ROW_DT == R.ROW_DT
    assert ctypes.sizeof(kslam.BatchResult) == 232   # kslam_batch_result keeps its size: callers allocate it
    assert L.kslam_abi_version() == 10


def _check(GN, c):
    rows, st = R.table(c)
    got, got_st = GN.tail_genes(_index(GN, c), c["rp"], c["pr"])
    assert got.tolist() == rows.tolist(), c["name"]
    assert got_st == st, c["name"]
    assert st["n_in_gene"] + st["n_no_gene"] + st["n_skipped"] == st["n_alignments"] and st["n_rows"] == len(rows)
    assert int(rows["alignments"].sum()) == st["n_in_gene"]
    return rows, st


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_twin_matches_the_restatement(GN, case):
    _check(GN, case)


def test_what_the_cases_are_there_for(GN):
    by = {c["name"]: c for c in CASES}
    rows, st = _check(GN, by["big-group"])
    assert rows.tolist() == [(0, 3000, 1, sum(min(260 + k % 200, 400) - (100 + k % 200) for k in range(3000)))]
    rows, st = _check(GN, by["big-group-gap"])
    assert rows[0]["alignments"] == 2999 and rows[0]["unique_read_pairs"] == 0 and st["n_no_gene"] == 1
    rows, st = _check(GN, by["dead"])
    assert rows.tolist() == [(0, 2, 2, 300), (1, 2, 1, 200)]            # gene 2 is named by dead records alone: no row
    rows, st = _check(GN, by["only-gene-less"])
    assert len(rows) == 0 and st["n_no_gene"] == 3
    rows, st = _check(GN, by["skipped"])
    assert st["n_skipped"] == 2 and rows.tolist() == [(0, 2, 1, 300)]
    rows, st = _check(GN, by["two-genes"])
    assert rows["unique_read_pairs"].tolist() == [0, 1, 0] and rows["alignments"].tolist() == [2, 3, 1]
    rows, st = _check(GN, by["wave-alternating"])
    assert rows.tolist() == [(0, 32, 32, 32 * 150), (1, 32, 32, 32 * 100)]
    rows, st = _check(GN, by["no-read-pairs"])
    assert len(rows) == 0 and st["n_alignments"] == 0
    rows, st = _check(GN, by["no-genes"])
    assert len(rows) == 0 and st["n_no_gene"] == 2 and st["n_skipped"] == 1


def test_150_random_cases(GN):
    for seed in range(150):
        _check(GN, R.random_case("random-%d" % seed, seed, 1 + 3 * seed, 1 + seed % 9, seed % 14))


def test_the_file_byte_for_byte(GN):
    rng = np.random.default_rng(5)
    for c in [R.random_case("file-%d" % k, 900 + k, 400, 6, 10) for k in range(4)] + [c for c in CASES if c["name"] in ("dead", "no-pairs", "no-genes")]:
        n, g = len(c["first"]) - 1, len(c["starts"])
        loci = [b"LOCUS_%d.%d" % (e, e % 3) for e in range(n)]
        tax = rng.integers(0, 1 << 31, n)
        names = [b"gene%d" % k if k % 4 else b"" for k in range(g)]
        prots = [b"NP_%06d.1" % k if k % 3 else b"" for k in range(g)]
        prods = [b"product of %d, with spaces" % k if k % 5 else b"" for k in range(g)]
        index = _index(GN, c, names=names, protein_ids=prots, products=prods, locus_tags=loci, taxonomy_ids=tax)
        rows, _ = GN.tail_genes(index, c["rp"], c["pr"])
        got = GN.table_bytes(index, rows)
        assert got == R.text(rows, c["first"], c["starts"], c["stops"], loci, tax, names, prots, prods), c["name"]
        parsed = GN.parse(got)
        assert [r["gene"] for r in parsed] == rows["gene"].tolist()
        assert all(r["length"] == r["stop"] - r["start"] and r["name"] == names[r["gene"]].decode() for r in parsed)
        if len(parsed):
            assert abs(sum(r["tpm"] for r in parsed) - 1e6) < 1.0       # (the printed values are rounded to 1e-4 each)
    with pytest.raises(ValueError):
        GN.parse(b"entry\tlocus\n")


def test_the_small_fixture(GN):
    """tests/golden/genes_small.tsv: ten genes over three entries, the rows and the file worked out by hand"""
    c, names, prots, prods = R.small()
    index = _index(GN, c, names=names, protein_ids=prots, products=prods, locus_tags=R.SMALL_LOCI, taxonomy_ids=R.SMALL_TAX)
    rows, st = GN.tail_genes(index, c["rp"], c["pr"])
    assert rows.tolist() == R.SMALL_ROWS and st == R.SMALL_STATS
    every = np.array(sorted(R.SMALL_ROWS + [R.SMALL_EXTRA_ROW]), dtype=GN.ROW_DT)   # with a row for the gene of length -100
    golden = open(os.path.join(ROOT, "tests", "golden", "genes_small.tsv"), "rb").read()
    assert GN.table_bytes(index, every) == golden
    assert R.text(every, c["first"], c["starts"], c["stops"], R.SMALL_LOCI, R.SMALL_TAX, names, prots, prods) == golden
    lines = GN.parse(golden)
    assert lines[1]["name"] == "" and lines[2]["length"] == -100 and lines[2]["rpk"] == 0.0 and lines[2]["tpm"] == 0.0
    only_nil = np.array([(8, 4, 4, 0)], dtype=GN.ROW_DT)                 # a lone row of length 0: S == 0, tpm 0
    assert GN.table_bytes(index, only_nil).endswith(b"\t4\t4\t0\t0.0000\t0.0000\n")


def test_writer_refusals(GN):
    c, names, prots, prods = R.small()
    index = _index(GN, c, names=names, protein_ids=prots, products=prods)
    bad = np.array([(0, 1, 1, 10), (10, 1, 0, 5)], dtype=GN.ROW_DT)      # the view has genes 0 .. 9
    fd = os.memfd_create("refused")
    try:
        with pytest.raises(Exception, match="not one of the index view's"):
            GN.write(index, bad, fd)
        assert os.lseek(fd, 0, os.SEEK_END) == 0                         # nothing was written
    finally:
        os.close(fd)
    with pytest.raises(Exception, match="writing the gene table failed"):
        GN.write(index, bad[:1], 10 ** 6)
    L = GN.lib()
    assert L.kslam_genes_write(None, bad.ctypes.data, 1, 1) == 1 and L.kslam_genes_write(ctypes.byref(index.view), None, 1, 1) == 1


def test_twin_refusals(GN):
    c = R.build("x", [[(0, 100)]], [([(0, 0, 9)], []), ([(0, 1, 2)], [])])
    index = _index(GN, c)
    rp = c["rp"].copy()
    rp["count"][1] = 2
    with pytest.raises(Exception, match="outside the pairs array"):
        GN.tail_genes(index, rp, c["pr"])
    rp = c["rp"].copy()
    rp["first"][1] = 0
    with pytest.raises(Exception, match="ascend"):
        GN.tail_genes(index, rp, c["pr"])
    broken = GN.GeneIndex([0, 2], [0], [100])                            # gene_first names two genes, the view has one
    with pytest.raises(Exception, match="gene_first"):
        GN.tail_genes(broken, c["rp"], c["pr"])
    L = GN.lib()
    rows, n, st = ctypes.c_void_p(), ctypes.c_uint64(), GN.Stats()
    assert L.kslam_tail_genes(ctypes.byref(index.view), None, 1, None, 0, ctypes.byref(rows), ctypes.byref(n), ctypes.byref(st)) == 1
    assert L.kslam_tail_genes(None, None, 0, None, 0, ctypes.byref(rows), ctypes.byref(n), ctypes.byref(st)) == 1
    assert L.kslam_tail_genes(ctypes.byref(index.view), None, 0, None, 0, None, ctypes.byref(n), ctypes.byref(st)) == 1
