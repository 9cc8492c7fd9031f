"""A plain-Python restatement of include/kslam_taxreads.h: the set S of the chosen taxa over a dict tree (a walk down the
children for CHILDREN, a walk up the parents for PARENTS), the matched read pairs, the selected record numbers and -- through
the record rule of tests/readsplit_ref.py -- the bytes of the two streams.  No code shared with the host twin (host/taxreads.cpp)
or the kernels (csrc/taxreads.hip).  Also the trees, chosen-id lists and texts the host and the device tests both run."""
import numpy as np

import kreport_ref as K
import readsplit_ref as RS

CHILDREN, PARENTS, EXCLUDE = 1, 2, 4
MODES = list(range(8))


def chosen_set(tree, ids, mode):
    """-> (S as a set of taxonomy ids, all_nonzero): all_nonzero stands for "every non-zero id", known to the tree or not"""
    ids = [int(i) for i in ids]
    assert ids and all(i != 0 for i in ids) and 0 <= mode < 8
    s = set(ids)
    if mode & CHILDREN:
        todo = [i for i in ids if i in tree.node]   # (a walk down with a list of its own: a chain may be deeper than Python's stack)
        while todo:
            i = todo.pop()
            s.add(i)
            todo.extend(k for k in tree.kids[i] if k not in s)
    if mode & PARENTS:
        for i in ids:
            p = tree.parent.get(i, 1)
            while p not in (0, 1) and p in tree.parent:   # `up` stops below the root
                s.add(p)
                p = tree.parent[p]
        s.add(1)                                           # by rule
    return s, bool(mode & CHILDREN) and 1 in ids


def matched(tax, ids, mode, pair_ids):
    """-> one bool per read pair"""
    s, all_nonzero = chosen_set(K.Tree(tax), ids, mode)
    return [int(t) != 0 and (all_nonzero or int(t) in s) for t in np.asarray(pair_ids).tolist()]


def mask(tax, ids, mode, tree=None):
    """S as kslam_taxon_reads_mask gives it: (one byte per node, the ids of S the tree does not know ascending, all_nonzero)"""
    tree = tree or K.Tree(tax)
    s, all_nonzero = chosen_set(tree, ids, mode)
    m = np.array([1 if i in s else 0 for i in tree.order], dtype=np.uint8)
    return m, sorted(i for i in s if i not in tree.node), all_nonzero


def selected_records(tax, ids, mode, pair_records, pair_ids, n_records):
    """the record numbers selected out of n_records: pair_records[g] is the R1 record number of read pair g"""
    hit = set(int(r) for r, m in zip(pair_records, matched(tax, ids, mode, pair_ids)) if m)
    return [r for r in range(n_records) if (r in hit) != bool(mode & EXCLUDE)]


def select(tax, ids, mode, r1, r2, pair_records, pair_ids, max_pairs=0, at_eof=True):
    """-> ([selected R1, selected R2 or None], (n selected, n others)); r2 None: single-end"""
    streams = [RS.records(r1, max_pairs, at_eof)] + ([RS.records(r2, max_pairs, at_eof)] if r2 is not None else [])
    n = len(streams[0])
    assert all(len(x) == n for x in streams)
    sel = selected_records(tax, ids, mode, pair_records, pair_ids, n)
    out = [b"".join(x[r] for r in sel) for x in streams] + [None] * (2 - len(streams))
    return out, (len(sel), n - len(sel))


def merge(selected_block, other_block, selected, n):
    """the partition: the selected and the excluded stream of one case merged back by record number"""
    return RS.merge(selected_block, other_block, selected, n)


# ---- trees (records as kreport_ref.tax_text takes them) ----

def chain(n, first=1000):
    return [(first + k, 1 if k == 0 else first + k - 1, "link%d" % k, "no rank") for k in range(n)]


def star(n, hub=500):
    return [(hub, 1, "hub", "genus")] + [(hub + 1 + k, hub, "ray%d" % k, "species") for k in range(n - 1)]


def forest(n, first=100):
    """several tops: every seventh node starts a tree of its own; the others hang one, two or three back"""
    return [(first + 2 * k, 1 if k % 7 == 0 else first + 2 * (k - 1 - (k % 3 if k % 7 > 2 else 0)), "w%d" % k, "no rank") for k in range(n)]


def phantom(n, first=100):
    """a forest whose tops hang under parents the file never defines (nodes past kslam_taxdb_size)"""
    base = forest(n - 2, first)
    return [(i, 7000 + (i % 2) if p == 1 else p, name, rank) for i, p, name, rank in base]


def with_root(records):
    return [(1, 1, "root", "no rank")] + list(records)


def trees(n):
    """name -> records with n nodes (phantom: n with its two undefined parents)"""
    out = {"chain": chain(n), "star": star(n), "forest": forest(n), "with_id_1": with_root(forest(n - 1)) if n > 1 else with_root([])}
    if n > 3:
        out["phantom"] = phantom(n)
    return out


def chosen_lists(records):
    """the chosen-id edge list for a tree: name -> ids"""
    tree = K.Tree(K.tax_text(records))
    keys = sorted(tree.node)
    lo, hi = keys[0], keys[-1]
    leaf = next(i for i in reversed(tree.order) if not tree.kids[i])
    deep = max(tree.order, key=lambda i: _depth(tree, i))
    top = deep
    while not tree.top(top):
        top = tree.parent[top]
    gap = next((k + 1 for k in keys if k + 1 not in tree.node and k + 1 < hi), hi + 5)
    out = {"smallest": [lo], "largest": [hi], "below_smallest": [lo - 1] if lo > 2 else [hi + 9], "above_largest": [hi + 1, 0xFFFFFFFF], "between": [gap],
           "duplicates": [hi, lo, hi, hi], "ancestor_and_descendant": [top, deep], "leaf": [leaf], "id_1": [1],
           "known_and_unknown": [deep, hi + 3, lo, hi + 3]}
    return out


def _depth(tree, i):
    d = 0
    while not tree.top(i):
        i = tree.parent[i]
        d += 1
    return d


def pair_ids_for(records, n, seed, extra=()):
    """n taxonomy ids drawn from the tree's ids, 0, and ids the tree does not know"""
    tree = K.Tree(K.tax_text(records))
    keys = sorted(tree.node)
    pool = np.array(keys + [0, 0, 1, keys[-1] + 1, keys[-1] + 3, 0xFFFFFFFF] + list(extra), dtype=np.uint32)
    return np.random.default_rng(seed).choice(pool, n)


# ---- the worked example of include/kslam_taxreads.h (tests/golden/taxreads_small.json) ----
SMALL, SMALL_IDS = K.SMALL, K.SMALL_IDS
SMALL_ROWS = [([562], 0, 3), ([562], CHILDREN, 5), ([562], PARENTS, 4), ([562], CHILDREN | PARENTS, 6), ([2], CHILDREN, 6), ([10239], CHILDREN, 1),
              ([999999], CHILDREN, 1), ([1], CHILDREN, 8), ([562], CHILDREN | EXCLUDE, 5)]
