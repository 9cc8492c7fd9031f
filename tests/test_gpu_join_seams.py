"""The k-mer join, the group ordering and the dedupe, each alone, at every seam (GPU).

k-slam_amd/csrc/join.hip decides which (read, entry, diagonal) candidates exist at all, and the other tests reach it
through whole pipelines on DNA.  Here the two test hooks of include/kslam.h (kslam_debug_join, kslam_debug_overlap_unique)
run it on synthetic keys that place every seam on purpose (tests/join_seams.py; tests/test_join_ref.py shows without a GPU
that each seam is where its case says): a bucket of 16 and of 17 keys, a block total of 4096 and of 4097, a sixty-fifth
long run in one tile, a run that starts two keys before a piece boundary, a 64-key group that starts in lane 255, a last
key of all ones.  Every join case runs on both routes -- the probe and the merge -- and each result is compared with the
host restatement tests/join_ref.py and with the other route's.  No tolerances: exact equality everywhere.
"""
import numpy as np
import pytest

import join_ref as R
import join_seams as S
from join_cases import make_join_case

pytestmark = pytest.mark.gpu

PROBE, MERGE = 0, 1
ROUTES = {"probe": PROBE, "merge": MERGE}


@pytest.fixture(scope="module")
def ctx(kslam):
    c = kslam.Context()
    yield c
    c.close()


_REF = {}


def _ref(c):
    """the restatement's multiset (sorted) and bucket table of a case, computed once"""
    if c["name"] not in _REF:
        _REF[c["name"]] = (R.join(c["genome"], c["reads"], c["read_len"], c["layout"]),
                           R.bucket_table(c["genome"]["kmer"], c["bucket_bits"]))
    return _REF[c["name"]]


def _run(ctx, c, route, cap, want_table=False):
    return ctx.debug_join(c["genome"], c["bucket_bits"], c["reads"], c["sorted_top_bits"], c["read_len"], c["layout"], route, cap,
                          want_table=want_table)


def _check_whole(ctx, c):
    """both routes with cap = raw: the cursor, the multiset, the guard words, the table; and the two routes agree"""
    exp, table = _ref(c)
    raw = len(exp)
    got = {}
    for rname, route in ROUTES.items():
        tag = "%s [%s]" % (c["name"], rname)
        cur, out, tab = _run(ctx, c, route, raw, want_table=True)
        assert cur == raw, (tag, cur, raw)
        assert len(out) == raw + 64 and (out[raw:] == R.SENTINEL).all(), tag
        got[rname] = np.sort(out[:raw])
        bad = np.flatnonzero(got[rname] != exp)
        assert len(bad) == 0, (tag, len(bad), [R.unpack(exp[i], c["layout"]) for i in bad[:3]], [R.unpack(got[rname][i], c["layout"]) for i in bad[:3]])
        assert np.array_equal(tab, table), tag
    assert np.array_equal(got["probe"], got["merge"]), c["name"]
    return raw


def _ids(cases):
    return [c["name"] for c in cases]


JOIN_CASES = S.join_cases()
MERGE_CASES = S.merge_cases()


@pytest.mark.parametrize("case", JOIN_CASES, ids=_ids(JOIN_CASES))
def test_join_case_on_both_routes(ctx, case):
    raw = _check_whole(ctx, case)
    if case.get("no_hit") or case["name"] == "n_g=0":
        assert raw == 0, case["name"]
    elif case["name"] != "n_r=1":
        assert raw > 0, case["name"]


@pytest.mark.parametrize("case", MERGE_CASES, ids=_ids(MERGE_CASES))
def test_merge_case_on_both_routes(ctx, case):
    raw = _check_whole(ctx, case)
    assert raw > 0 or case.get("range_len") == 0, case["name"]


CAP_CASES = [c for c in JOIN_CASES if c["name"] in ("n_r=2049", "run_lengths", "block_total/flat_4096", "block_total/queue_overflow",
                                                    "block_total/one_run_of_5000", "strand_offset")]


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", CAP_CASES, ids=_ids(CAP_CASES))
def test_nothing_is_written_beyond_cap_and_the_cursor_is_the_total(ctx, case, route):
    exp, _table = _ref(case)
    raw = len(exp)
    assert raw > 2
    vals, counts = np.unique(exp, return_counts=True)
    for cap in (raw, raw - 1, raw // 2, 0):
        tag = "%s [%s] cap=%d of %d" % (case["name"], route, cap, raw)
        cur, out, _t = _run(ctx, case, ROUTES[route], cap)
        assert cur == raw, (tag, cur)
        assert len(out) == cap + 64 and (out[cap:] == R.SENTINEL).all(), tag
        written = out[:cap][out[:cap] != R.SENTINEL]
        if cap == raw:
            assert np.array_equal(np.sort(out[:raw]), exp), tag
            continue
        # a workgroup whose range does not fit writes nothing: what is there is part of the multiset, no value too often
        assert len(written) < raw, tag
        wv, wc = np.unique(written, return_counts=True)
        at = np.searchsorted(vals, wv)
        assert (at < len(vals)).all() and (vals[np.minimum(at, len(vals) - 1)] == wv).all(), tag
        assert (wc <= counts[at]).all(), tag


# ---- unique ---------------------------------------------------------------------------------------------------------------
SORTED_CASES = S.unique_sorted_cases()
GROUPED_CASES = S.unique_grouped_cases()
BASE = 1000003          # read_id_base


def _check_route0(ctx, name, lay, keys, base=BASE):
    exp_keys, exp_flags, exp_rows = R.unique_rows(keys, lay, base)
    assert np.array_equal(exp_keys, keys), name                              # (route 0 takes fully sorted keys)
    got = ctx.debug_overlap_unique(keys, lay, base, 0)
    assert got["big"] == 0, name
    assert not (got["flags"] == R.SENTINEL32).any(), (name, "a flag slot was never written")
    assert np.array_equal(got["flags"], exp_flags.astype(np.uint32)), (name, np.flatnonzero(got["flags"] != exp_flags)[:5])
    assert np.array_equal(got["keys_after"], keys) and np.array_equal(got["ordered"], keys), name
    assert got["rows"].tobytes() == exp_rows.tobytes(), name
    return got["rows"]


@pytest.mark.parametrize("case", SORTED_CASES, ids=[n for n, _l, _k in SORTED_CASES])
def test_dedupe_of_sorted_keys(ctx, case):
    name, lay, keys = case
    _check_route0(ctx, name, lay, keys)


@pytest.mark.parametrize("case", GROUPED_CASES, ids=[n for n, _l, _k in GROUPED_CASES])
def test_group_order_then_dedupe(ctx, case):
    name, lay, keys = case
    exp_keys, exp_flags, exp_rows = R.unique_rows(keys, lay, BASE)
    got = ctx.debug_overlap_unique(keys, lay, BASE, 1)
    assert got["big"] == int(R.has_big_group(keys, lay, S.GROUP_CAP)), name
    assert np.array_equal(got["keys_after"], keys), (name, "group_order only reads its input")
    if got["big"]:
        assert len(got["rows"]) == 0, name
    else:
        assert not (got["ordered"] == R.SENTINEL).any() and not (got["flags"] == R.SENTINEL32).any(), (name, "a slot was never written")
        assert np.array_equal(got["ordered"], exp_keys), name
        assert np.array_equal(got["flags"], exp_flags.astype(np.uint32)), (name, np.flatnonzero(got["flags"] != exp_flags)[:5])
        assert got["rows"].tobytes() == exp_rows.tobytes(), name
    # the long way on the same keys: the restatement again, and the same rows as the grouped route wherever that finished
    rows0 = _check_route0(ctx, name + " [sorted]", lay, np.sort(keys))
    if not got["big"]:
        assert rows0.tobytes() == got["rows"].tobytes(), name


def test_sorted_cases_through_the_grouped_route_too(ctx):
    """fully sorted keys are ordered by their high bits as well: both routes, identical rows whenever big stayed 0"""
    checked = 0
    for name, lay, keys in SORTED_CASES:
        if R.has_big_group(keys, lay, S.GROUP_CAP):
            got = ctx.debug_overlap_unique(keys, lay, 7, 1)
            assert got["big"] == 1 and len(got["rows"]) == 0 and np.array_equal(got["keys_after"], keys), name
            continue
        a, b = ctx.debug_overlap_unique(keys, lay, 7, 0), ctx.debug_overlap_unique(keys, lay, 7, 1)
        assert b["big"] == 0 and a["rows"].tobytes() == b["rows"].tobytes() and np.array_equal(a["flags"], b["flags"]), name
        checked += 1
    assert checked >= 10


def test_empty_inputs(ctx):
    got = ctx.debug_overlap_unique(np.zeros(0, dtype=np.uint64), (4, 4, 15, 0), 0, 0)
    assert got["big"] == 0 and len(got["rows"]) == 0 and len(got["flags"]) == 0
    c = S.join_case("empty", np.array([5, 6], dtype=np.uint64), np.zeros(0, dtype=np.uint64), 1)
    for route in ROUTES.values():
        cur, out, _t = _run(ctx, c, route, 0)
        assert cur == 0 and (out == R.SENTINEL).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _rec(rows):
    return np.array(rows, dtype=R.KMER_DT)


def _join_refusals():
    lay = (4, 4, 12, 100)
    G = 0x80000000
    g = _rec([(5 << 56, G | 1, 200), (9 << 56, G | 2, 300)])
    r = _rec([(5 << 56, 3, 10), (9 << 56, 4, 0)])
    rl = np.full(16, 100, dtype=np.uint32)
    ok = dict(genome=g, bucket_bits=8, reads=r, sorted_top_bits=8, read_len=rl, layout=lay, route=1, cap=16)
    return ok, {
        "genome keys not ascending": dict(genome=g[::-1].copy()),
        "bucket_bits below 8": dict(bucket_bits=7),
        "bucket_bits above 16": dict(bucket_bits=17),
        "a route that does not exist": dict(route=2),
        "read id outside the length array": dict(read_len=rl[:4]),
        "read k-mer beyond its read": dict(reads=_rec([(5 << 56, 3, 69)])),
        "read id beyond bits_read": dict(layout=(2, 4, 12, 100)),
        "genome id beyond bits_entry": dict(layout=(4, 1, 12, 100)),
        "rel below the field": dict(genome=_rec([(5 << 56, G | 1, 20)]), layout=(4, 4, 12, 10)),
        "rel above the field": dict(genome=_rec([(5 << 56, G | 1, 4090)])),
        "rel_bias beyond bits_rel": dict(layout=(4, 4, 6, 100)),
        "key wider than 63 bits": dict(layout=(31, 30, 20, 100)),
        "merge: reads out of order": dict(reads=r[::-1].copy()),
        "merge: no sorted bits": dict(sorted_top_bits=0),
        "cap beyond 2^28": dict(cap=1 << 28),
    }


def _unique_refusals():
    lay = (4, 4, 12, 100)
    k = np.array([R.pack(1, 1, 5, 0, lay), R.pack(1, 1, 3, 1, lay), R.pack(2, 0, 0, 0, lay)], dtype=np.uint64)    # low bits descend
    return {
        "route 0: keys not sorted": (k, lay, 0, 0),
        "route 1: high bits not ordered": (k[::-1].copy(), lay, 0, 1),
        "a route that does not exist": (np.sort(k), lay, 0, 2),
        "a key wider than the layout": (np.array([1 << 40], dtype=np.uint64), lay, 0, 0),
        "read + read_id_base beyond 32 bits": (np.sort(k), lay, 0xFFFFFFFF, 0),
        "bits_rel of 0": (np.sort(k), (4, 4, 0, 0), 0, 0),
        "key wider than 63 bits": (np.sort(k), (31, 30, 20, 0), 0, 0),
    }


def test_refusals_come_before_any_kernel_and_leave_the_context_usable(kslam):
    reads, genomes = make_join_case(11, n_reads=24)
    want_ov, want_cig = kslam.align_to_database(reads, genomes)
    assert len(want_ov) > 20
    c = kslam.Context()
    c.set_index(genomes)

    def still_fine(what):
        ov, cig = c.align_batch(reads)
        assert ov.tobytes() == want_ov.tobytes() and np.array_equal(cig, want_cig), what

    ok, bad = _join_refusals()
    cur, out, _t = c.debug_join(**ok)                         # the arguments every refusal below changes one of
    assert cur == 2 and (out[2:] == R.SENTINEL).all()
    still_fine("after a hook that ran")
    for what, change in bad.items():
        with pytest.raises(kslam.KslamError) as e:
            c.debug_join(**dict(ok, **change))
        assert e.value.status == kslam.KSLAM_ERR_ARG, (what, str(e.value))
        still_fine(what)
    assert c.debug_join(**dict(ok, route=0, reads=ok["reads"][::-1].copy(), sorted_top_bits=0))[0] == 2      # the probe takes any order
    for what, (keys, lay, base, route) in _unique_refusals().items():
        with pytest.raises(kslam.KslamError) as e:
            c.debug_overlap_unique(keys, lay, base, route)
        assert e.value.status == kslam.KSLAM_ERR_ARG, (what, str(e.value))
        still_fine(what)
    c.close()
