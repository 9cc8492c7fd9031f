"""The reads of chosen taxa, restated (tests/taxreads_ref.py, include/kslam_taxreads.h): the restatement reproduces every row of
the header's worked example byte for byte (tests/golden/taxreads_small.json, written by hand from the table), and on random
trees the CHILDREN count of every id equals its clade count in the Kraken-style report's restatement (tests/kreport_ref.py).
No GPU, no library."""
import json
import os

import numpy as np
import pytest

import kreport_ref as K
import taxreads_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "taxreads_small.json")


def _golden():
    return json.load(open(GOLDEN))


def test_golden_is_the_headers_example():
    g = _golden()
    assert g["taxdb"].encode() == K.tax_text(R.SMALL) and g["pair_ids"] == R.SMALL_IDS
    assert [(r["chosen"], r["mode"], r["n_selected"]) for r in g["rows"]] == [(c, m, n) for c, m, n in R.SMALL_ROWS]
    assert g["r1"].count("\n") == g["r2"].count("\n") == 40


@pytest.mark.parametrize("row", range(len(R.SMALL_ROWS)))
def test_worked_example_byte_for_byte(row):
    g = _golden()
    r = g["rows"][row]
    tax, r1, r2 = g["taxdb"].encode(), g["r1"].encode(), g["r2"].encode()
    assert R.selected_records(tax, r["chosen"], r["mode"], g["pair_records"], g["pair_ids"], 10) == r["selected"]
    out, counts = R.select(tax, r["chosen"], r["mode"], r1, r2, g["pair_records"], g["pair_ids"])
    assert out == [r["r1"].encode(), r["r2"].encode()] and counts == (r["n_selected"], 10 - r["n_selected"])
    single, counts1 = R.select(tax, r["chosen"], r["mode"], r1, None, g["pair_records"], g["pair_ids"])
    assert single == [r["r1"].encode(), None] and counts1 == counts


def test_the_parents_set_of_the_example():
    s, all_nonzero = R.chosen_set(K.Tree(K.tax_text(R.SMALL)), [562], R.PARENTS)
    assert s == {562, 1224, 2, 131567, 1} and not all_nonzero
    assert R.chosen_set(K.Tree(K.tax_text(R.SMALL)), [1], R.CHILDREN)[1]
    assert R.chosen_set(K.Tree(K.tax_text(R.SMALL)), [424242], R.CHILDREN | R.PARENTS) == ({424242, 1}, False)


def _random_tree(rng, n):
    ids = rng.choice(np.arange(2, 50 * n + 50), n, replace=False).tolist()
    recs = []
    for k, i in enumerate(ids):
        r = rng.random()
        parent = 1 if (k == 0 or r < 0.15) else (90000 + int(rng.integers(3)) if r < 0.2 else ids[int(rng.integers(k))])
        recs.append((i, parent, "n%d" % i, "no rank"))
    if rng.random() < 0.5:
        recs.insert(int(rng.integers(len(recs) + 1)), (1, 1, "root", "no rank"))
    return recs


@pytest.mark.parametrize("seed", range(12))
def test_children_count_equals_the_clade_count(seed):
    rng = np.random.default_rng(400 + seed)
    recs = _random_tree(rng, int(rng.integers(1, 120)))
    tax = K.tax_text(recs)
    tree = K.Tree(tax)
    pool = np.array(sorted(tree.node) + [0, 0, 1, 77777, 0xFFFFFFFF], dtype=np.uint32)
    pair_ids = rng.choice(pool, 500)
    rows, stats = K.rows(tax, pair_ids)
    assert len(rows) > 0
    seen = 0
    for row in rows.tolist():
        tax_id, _, _, clade = row
        if tax_id == 1:
            continue   # the tree's own node for id 1 is folded into the synthetic root row
        assert sum(R.matched(tax, [tax_id], R.CHILDREN, pair_ids)) == clade > 0
        seen += 1
    assert seen > 0
    # the synthetic root: every non-zero id
    assert sum(R.matched(tax, [1], R.CHILDREN, pair_ids)) == stats["n_ids"] == int(np.count_nonzero(pair_ids))
    # an id with clade 0 selects nothing
    absent = [i for i in tree.order if i != 1 and i not in set(rows["tax_id"].tolist())]
    for i in absent[:5]:
        assert sum(R.matched(tax, [i], R.CHILDREN, pair_ids)) == 0


@pytest.mark.parametrize("seed", range(6))
def test_exclude_is_the_complement(seed):
    rng = np.random.default_rng(900 + seed)
    recs = _random_tree(rng, 40)
    tax = K.tax_text(recs)
    pair_ids = rng.choice(np.array(sorted(K.Tree(tax).node) + [0, 5], dtype=np.uint32), 60)
    records = rng.permutation(100)[:60]
    chosen = [int(x) for x in rng.choice(pair_ids[pair_ids != 0], 3)]
    for mode in (0, 1, 2, 3):
        a = R.selected_records(tax, chosen, mode, records, pair_ids, 100)
        b = R.selected_records(tax, chosen, mode | R.EXCLUDE, records, pair_ids, 100)
        assert sorted(a + b) == list(range(100)) and not set(a) & set(b)
