"""The reads of chosen taxa on the host (kslam_tail_taxon_reads, host/taxreads.cpp; include/kslam_taxreads.h) against the
plain-Python restatement (tests/taxreads_ref.py), byte for byte: chains, stars, forests, phantom parents, trees with and without
a node for id 1; the chosen-id edge list; all eight modes; paired and single-end texts in every line-ending form; the partition;
the refusals.  No GPU."""
import importlib
import json
import os

import numpy as np
import pytest

import kreport_ref as K
import readsplit_ref as RS
import taxreads_ref as R

ERR_ARG = 1   # include/kslam.h: kslam_status
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "taxreads_small.json")
TREES = R.trees(40)
TREES["chain_deep"] = R.chain(300)   # depth N: the walks past 64 and 256 levels


@pytest.fixture(scope="module")
def TR(kslam):
    return importlib.import_module("kslam_amd.taxreads")


@pytest.fixture(scope="module")
def X(kslam):
    return importlib.import_module("kslam_amd.taxonomy")


def _pairs(n_records, n_pairs, seed, paired=True):
    records = np.sort(np.random.default_rng(seed).permutation(n_records)[:n_pairs])
    return records, RS.read_pairs(records, n_records, paired)


def _both(TR, db, tax, ids, mode, r1, r2, records, rp, pair_ids, max_pairs=0, at_eof=True):
    exp, n_exp = R.select(tax, ids, mode, r1, r2, records, pair_ids, max_pairs, at_eof)
    got = TR.tail_taxon_reads(db, ids, mode, r1, r2, rp, pair_ids, max_pairs, at_eof)
    assert got["blocks"] == exp and got["n_records"] == n_exp and got["flags"] == 4   # KSLAM_READS_OUT_HOST_MEMORY
    return got["blocks"], n_exp


def test_worked_example_byte_for_byte(TR, X):
    g = json.load(open(GOLDEN))
    db = X.TaxDB(g["taxdb"].encode())
    rp = RS.read_pairs(g["pair_records"], 10)
    for r in g["rows"]:
        got = TR.tail_taxon_reads(db, r["chosen"], r["mode"], g["r1"].encode(), g["r2"].encode(), rp, g["pair_ids"])
        assert got["blocks"] == [r["r1"].encode(), r["r2"].encode()], r
        assert got["n_records"] == (r["n_selected"], 10 - r["n_selected"])


@pytest.mark.parametrize("tree", sorted(TREES))
def test_trees_chosen_ids_and_modes(TR, X, tree):
    recs = TREES[tree]
    tax = K.tax_text(recs)
    db = X.TaxDB(tax)
    n = 50
    r1, r2 = RS.text_of(n, n_bases=11), RS.text_of(n, b"\r\n", n_bases=9, mate=2)
    records, rp = _pairs(n, 37, 3)
    pair_ids = R.pair_ids_for(recs, len(rp), 17)
    counts = set()
    for name, ids in R.chosen_lists(recs).items():
        for mode in R.MODES:
            blocks, n_exp = _both(TR, db, tax, ids, mode, r1, r2, records, rp, pair_ids)
            counts.add(n_exp[0])
            if mode & R.EXCLUDE:   # the partition: with and without EXCLUDE merged by record number are the consumed records
                sel = R.selected_records(tax, ids, mode, records, pair_ids, n)
                other, _ = R.select(tax, ids, mode ^ R.EXCLUDE, r1, r2, records, pair_ids)
                for k, text in enumerate((r1, r2)):
                    assert R.merge(blocks[k], other[k], sel, n) == b"".join(RS.records(text)), (name, mode)
    assert len(counts) > 3   # the cases do select differently


FORMATS = [c for c in RS.cases() if c[0] in ("crlf", "cr", "mixed", "unterminated", "unterminated_crlf", "completed_by_eof", "max_pairs_mid",
                                             "not_eof_trailing_cr", "single_end", "single_end_mixed", "empty")]


@pytest.mark.parametrize("case", FORMATS, ids=[c[0] for c in FORMATS])
def test_texts(TR, X, case):
    name, r1, r2, max_pairs, at_eof = case
    tax = K.tax_text(R.with_root(R.forest(12)))
    db = X.TaxDB(tax)
    n = len(RS.records(r1, max_pairs, at_eof))
    records = np.arange(n)
    rp = RS.read_pairs(records, n, paired=r2 is not None)
    tree = K.Tree(tax)
    pair_ids = np.array([(tree.order[(3 * k) % len(tree.order)], 0, 999)[k % 3] for k in range(n)], dtype=np.uint32)
    for ids, mode in (([100], R.CHILDREN), ([100], R.CHILDREN | R.EXCLUDE), ([999], 0), ([999, 100], R.PARENTS | R.EXCLUDE),
                      ([1], R.CHILDREN), ([1], R.CHILDREN | R.EXCLUDE), ([4242], 0), ([4242], R.EXCLUDE)):
        blocks, n_exp = _both(TR, db, tax, ids, mode, r1, r2, records, rp, pair_ids, max_pairs, at_eof)
        if ids == [4242]:      # an empty selection, and everything selected
            assert n_exp == ((n, 0) if mode & R.EXCLUDE else (0, n))
            assert blocks[0] == (b"".join(RS.records(r1, max_pairs, at_eof)) if mode & R.EXCLUDE else b"")


def test_refusals(TR, X, kslam):
    L = TR.lib()
    RSm = importlib.import_module("kslam_amd.readsplit")
    tax = K.tax_text(R.forest(5))
    db = X.TaxDB(tax)
    r1 = RS.text_of(3)
    rp = RS.read_pairs([0, 2], 3, paired=False)
    t = np.array([100, 102], dtype=np.uint32)
    ro = RSm.ReadsOut()

    def call(ids, mode):
        a = np.asarray(ids, dtype=np.uint32)
        import ctypes as C
        return L.kslam_tail_taxon_reads(db._h, a.ctypes.data if len(a) else None, len(a), mode, r1, len(r1), None, 0, 0, 1, rp.ctypes.data,
                                        t.ctypes.data, 2, C.byref(ro))

    assert call([100, 0], 0) == ERR_ARG      # id 0 cannot be chosen
    assert call([100], 8) == ERR_ARG         # mode bits above 7
    assert call([], 0) == ERR_ARG            # the twin has no "off": n >= 1
    assert ro.data[0] is None and ro.len[0] == 0
    assert call([100], 7) == 0
    assert ro.n_records[0] + ro.n_records[1] == 3
    L.kslam_release_reads_out(None, ro)
