"""The Kraken-style report on the host (include/kslam_kreport.h): the plain-Python restatement (tests/kreport_ref.py) and the host
twin with the writer (kslam_tail_kreport + kslam_kreport_write, host/kreport.cpp) reproduce the worked example byte for byte,
agree on every seam case, and keep the format's invariants.  No GPU."""
import importlib
import json
import os

import numpy as np
import pytest

import kreport_ref as R

CASES = R.cases()
ERR_ARG = 1   # include/kslam.h: kslam_status
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kreport_small.json")


@pytest.fixture(scope="module")
def KR(kslam):
    return importlib.import_module("kslam_amd.kreport")


@pytest.fixture(scope="module")
def X(kslam):
    return importlib.import_module("kslam_amd.taxonomy")


def test_worked_example_byte_for_byte(KR, X):
    g = json.load(open(GOLDEN))
    tax, ids, total, report = g["taxdb"].encode(), g["ids"], g["total"], g["report"].encode()
    assert tax == R.tax_text(R.SMALL) and ids == R.SMALL_IDS
    assert R.text(tax, ids, total) == report
    db = X.TaxDB(tax)
    rows, stats = KR.tail_kreport(db, ids)
    assert KR.report_bytes(db, rows, total) == report
    assert stats == {"n_ids": 8, "n_unknown_ids": 1, "n_rows": 8}   # (the tree's node for id 1 has no reads of its own: no row)
    assert report.endswith(b"\t999999\t  \n")   # the unknown id: its indent and an empty name
    assert [r["code"] for r in KR.parse_report(report)] == ["U", "R", "R1", "D", "P", "S", "S1", "D", "S", "R1"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_equals_restatement(KR, X, case):
    db = X.TaxDB(case["tax"])
    rows, stats = KR.tail_kreport(db, case["ids"])
    exp_rows, exp_stats = R.rows(case["tax"], case["ids"])
    assert rows.tolist() == exp_rows.tolist() and stats == exp_stats
    for total in (len(case["ids"]), int(stats["n_ids"]), 3 * len(case["ids"]) + 7):
        assert KR.report_bytes(db, rows, total) == R.text(case["tax"], case["ids"], total), total


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_invariants(KR, X, case):
    ids = case["ids"]
    tree = R.Tree(case["tax"])
    rows, stats = R.rows(case["tax"], ids)
    nonzero = int(np.count_nonzero(ids))
    assert int(rows["direct"].sum()) == nonzero == stats["n_ids"]
    lines = KR.parse_report(R.text(case["tax"], ids, len(ids)))
    root = [x for x in lines if x["code"] == "R"]
    assert (root[0]["clade"] == nonzero and root[0]["taxid"] == 1 and root[0]["level"] == 0) if nonzero else not root
    unclassified = [x for x in lines if x["code"] == "U"]
    assert (unclassified[0]["clade"] == len(ids) - nonzero) if len(ids) > nonzero else not unclassified   # omitted when its count is 0
    # every node's clade is its direct count plus its children's clades (children: the lines one level deeper, up to the next
    # line at this level or above)
    body = [x for x in lines if x["code"] != "U"]
    for k, x in enumerate(body):
        kids, j = 0, k + 1
        while j < len(body) and body[j]["level"] > x["level"]:
            if body[j]["level"] == x["level"] + 1:
                kids += body[j]["clade"]
            j += 1
        assert x["clade"] == x["direct"] + kids and x["clade"] > 0, x
    by_node = {int(r["node"]): r for r in rows if r["node"] != R.NO_NODE}
    for node, r in by_node.items():
        below = sum(int(q["clade"]) for n2, q in by_node.items() if tree.parent[tree.order[n2]] == tree.order[node] and not tree.top(tree.order[n2]))
        assert int(r["clade"]) == int(r["direct"]) + below


def test_total_below_the_ids_is_refused(KR, X):
    db = X.TaxDB(R.tax_text(R.SMALL))
    rows, _ = KR.tail_kreport(db, R.SMALL_IDS)
    fd = os.memfd_create("refused")
    try:
        assert KR.lib().kslam_kreport_write(db._h, rows.ctypes.data, len(rows), 7, fd) == ERR_ARG
        assert os.lseek(fd, 0, os.SEEK_END) == 0   # nothing was written
        assert b"7 read pairs" in KR.lib().kslam_tail_last_error()
    finally:
        os.close(fd)
    with pytest.raises(ValueError):
        R.text(R.tax_text(R.SMALL), R.SMALL_IDS, 7)
    assert not KR.report_bytes(db, rows, 8).startswith(b"  0.00")   # total == the ids counted: no unclassified line
    assert KR.report_bytes(db, rows, 8).startswith(b"100.00\t8\t0\tR\t1\troot\n")
    assert KR.report_bytes(db, rows[:0], 0) == b"" == R.text(R.tax_text(R.SMALL), [], 0)
    bad = rows.copy()
    bad["node"][0] = 1000
    assert KR.lib().kslam_kreport_write(db._h, bad.ctypes.data, len(bad), 10, -1) == ERR_ARG   # not a row of this tree


def test_library_exports_every_declared_symbol(kslam, KR):
    import ctypes
    import re
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kslam_kreport.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 10 and sorted(KR.EXPORTS) == declared
    for name in declared:
        assert hasattr(L, name), "missing export " + name
    assert KR.ROW_DT.itemsize == 24 and ctypes.sizeof(KR.Stats) == 24
