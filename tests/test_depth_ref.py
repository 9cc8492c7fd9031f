"""The plain-Python restatement of the depth track (tests/depth_ref.py) against rows written by hand: the walk, the entry seams
and the runs.  No GPU, no library."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref as D  # noqa: E402
import variants_ref as V  # noqa: E402

SEAMS = D.seam_cases()


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_restatement_against_hand_written_rows(name):
    case, expected, skipped = SEAMS[name]
    rows, stats = D.table(case)
    assert rows == expected
    assert stats["n_skipped"] == skipped and stats["n_rows"] == len(expected)
    assert stats["covered_bases"] == sum(t - s for _, s, t, _ in expected)
    assert stats["max_depth"] == max([v for *_, v in expected], default=0)


def test_stats_and_keys():
    case, _, _ = SEAMS["abutting"]
    assert D.table(case)[1] == {"n_records": 2, "n_skipped": 0, "n_intervals": 2, "n_keys": 2, "n_rows": 1, "covered_bases": 20, "max_depth": 1}
    case, _, _ = SEAMS["seam"]
    assert D.table(case)[1]["n_keys"] == 4          # the end of entry 0 and the start of entry 1 are two boundaries
    case, _, _ = SEAMS["identical-70001"]
    assert D.table(case)[1]["n_keys"] == 2 and D.table(case)[1]["n_intervals"] == 70001
    for t in (255, 256, 1023, 1025, 4097):
        assert D.table(D.boundaries("b", t))[1]["n_keys"] == t


def test_filter_drops_and_never_merges():
    c = D.filter_case()
    assert D.table(c, 0)[0] == D.table(c, 1)[0] and len(D.table(c, 1)[0]) == 5
    assert D.table(c, 2)[0] == [(0, 5, 10, 2), (0, 10, 20, 3), (0, 20, 25, 2)]      # three rows, not (5, 25)
    assert D.table(c, 3)[0] == [(0, 10, 20, 3)] and D.table(c, 4)[0] == []
    assert D.table(c, 3)[1] == D.table(c, 1)[1]                                       # the stats are taken before the filter


def test_same_counts_as_the_variants_restatement():
    for seed in range(8):
        c = V.random_case("r%d" % seed, seed, 40 + 30 * seed, 1 + seed % 5, 200)
        _, vs = V.table(c)
        _, ds = D.table(c)
        assert [ds[k] for k in ("n_records", "n_skipped", "n_intervals")] == [vs[k] for k in ("n_records", "n_skipped", "n_intervals")]
        depth, _ = D.profile(c)
        for r in V.table(c, 1, 0)[0]:
            assert int(depth[int(r["entry"])][int(r["pos"])]) == int(r["depth"])
    assert D.bedgraph_bytes([(1, 0, 4, 2)], [b"a", b"b.1"]) == b"b.1\t0\t4\t2\n"
