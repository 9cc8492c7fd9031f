"""The one-time genome index build, table by table, at every seam (GPU).

Every batch stands on what kslam_set_index / kslam_set_index_device leave on the device (k-slam_amd/csrc/api_index.hip:
build_index): the encoded bases, the sorted key column and the {meta, offset} column, the bucket table and the membership
filter.  The other tests see them only through alignments, where a read's other seeds hide one wrong bucket entry, one
k-mer missing at a segment seam or one lost filter word.  Here kslam_debug_index_export (include/kslam.h) reads the built
index back and every table is compared on its own with the numpy restatement tests/index_ref.py, bit for bit -- there is
no tolerance anywhere -- so that a failure names the table and the first position that differs.

The indexes (tests/index_seams.py; tests/test_index_ref.py shows without a GPU that each reaches the seam it is named
for) place entry lengths around one k-mer, one segment and 64 segments; record counts around a block of k_split_tables
and a tile of the sort; entry counts around each shape of the meta passes, with equal-key groups across those ids on both
strands; the two ratio switches; k-mer 0, N, lower case, palindromes, a doubled entry and a run of 4 200 equal records;
and the empty indexes.  Each runs the default build and, where it changes a kernel, the atomic filter build, the sort
without digit bytes, KSLAM_FILTER_BITS 0 / 20 / 21 / 28, KSLAM_BUCKET_BITS_EXACT 8 / 12 / 20 and kslam_set_index_device.
Every table comparison comes before find_overlaps, which ties the exported index to the one the join uses: a wrong build
is reported before the join could trip over it.
"""
import numpy as np
import pytest

import index_ref as R
import index_seams as S
import sort_ref as SR

pytestmark = pytest.mark.gpu

OV_FIELDS = ("read", "entry", "rel", "revcomp")
_EXPORTS = {}            # (index, route) -> the export of a fresh context, kept for the comparisons between routes


def _build(kslam, monkeypatch, name, route, ctx=None):
    """build index `name` on route `route` (on a fresh context unless one is given) -> (context, export)"""
    env, _bucket, _filter, through_device = S.ROUTES[route]
    for k in ("KSLAM_FILTER_BUILD", "KSLAM_SORT_DIGIT_BYTES", "KSLAM_FILTER_BITS", "KSLAM_BUCKET_BITS_EXACT", "KSLAM_BUCKET_BITS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    entries = list(S.index(name))
    c = ctx or kslam.Context()            # (the switches are read at kslam_create)
    try:
        if through_device:
            import torch
            off = R.offsets(entries) + np.uint64(S.DEVICE_FIRST_OFFSET)
            host = np.frombuffer(b"#" * S.DEVICE_FIRST_OFFSET + b"".join(entries) + b"#" * 9, dtype=np.uint8)
            dev = torch.from_numpy(host.copy()).to("cuda:0")
            torch.cuda.synchronize()
            c.set_index_device(len(entries), dev.data_ptr(), off)
            del dev
        else:
            c.set_index(entries)
        return c, c.debug_index_export()
    except BaseException:
        if ctx is None:
            c.close()
        raise


def _compare(got, exp, tag):
    diff = R.first_difference(got, exp)
    assert diff is None, (tag,) + diff


def _check_join(oracle, c, name, got, tag):
    """find_overlaps on a few reads cut from the entries == the oracle's findOverlaps over the EXPORTED records"""
    reads = S.reads_of(name)
    recs = np.zeros(len(got["keys"]), dtype=R.KMER_DT)
    recs["kmer"], recs["meta"], recs["offset"] = got["keys"], got["meta"], got["offset"]
    read_recs = oracle.extract_kmers(reads, False, 1)
    exp, raw = oracle.find_overlaps(oracle.sort_kmers(np.concatenate([read_recs, recs])), [len(r) for r in reads])
    c.load_reads(reads)
    ov, got_raw = c.find_overlaps()
    assert got_raw == raw and len(ov) == len(exp), (tag, "overlaps", got_raw, raw, len(ov), len(exp))
    for f in OV_FIELDS:
        bad = np.flatnonzero(ov[f] != exp[f])
        assert len(bad) == 0, (tag, f, bad[:5], ov[bad[:5]], exp[bad[:5]])
    return raw


@pytest.mark.parametrize("name,route", S.CASES, ids=["%s-%s" % c for c in S.CASES])
def test_index_tables(kslam, oracle, monkeypatch, name, route):
    tag = "%s [%s]" % (name, route)
    exp = S.expected(name, route)
    c, got = _build(kslam, monkeypatch, name, route)
    try:
        _EXPORTS[(name, route)] = got
        _compare(got, exp, tag)
        st = c.index_build_stats()
        assert st["n_genome_kmers"] == exp["n_genome_kmers"] and st["n_entries"] == exp["n_entries"], tag
        assert st["sort_passes"] == len(SR.index_passes(exp["n_entries"])), tag
        raw = _check_join(oracle, c, name, got, tag)
        assert (raw > 0) == (exp["n_genome_kmers"] > 0), (tag, raw)
        _compare(c.debug_index_export(), exp, tag + " after the join")          # a batch leaves the index as it was
    finally:
        c.close()


@pytest.mark.parametrize("name", [n for n in S.NAMES if len(S.routes_of(n)) > 1])
def test_all_routes_export_identical_tables(kslam, monkeypatch, name):
    """over one index: the same columns and bases on every route, the same bucket table wherever bucket_bits agree and the
    same filter wherever filter_bits agree"""
    def export(route):
        if (name, route) not in _EXPORTS:
            c, got = _build(kslam, monkeypatch, name, route)
            c.close()
            _EXPORTS[(name, route)] = got
        return _EXPORTS[(name, route)]
    base = export("default")
    for route in S.routes_of(name)[1:]:
        got = export(route)
        for t in ("offsets", "codes", "keys", "meta", "offset"):
            assert np.array_equal(got[t], base[t]), (name, route, t)
        if got["bucket_bits"] == base["bucket_bits"]:
            assert np.array_equal(got["bucket"], base["bucket"]), (name, route, "bucket")
        if got["filter_bits"] == base["filter_bits"]:
            assert np.array_equal(got["filter"], base["filter"]), (name, route, "filter")
    by_fb = {}
    for route in S.routes_of(name):
        by_fb.setdefault(export(route)["filter_bits"], []).append(route)
    for fb, routes in by_fb.items():
        for route in routes[1:]:
            assert np.array_equal(export(route)["filter"], export(routes[0])["filter"]), (name, route, routes[0], "filter")


@pytest.mark.parametrize("route", ["default", "no_digit_bytes", "atomics"])
def test_reuse_of_one_context(kslam, oracle, monkeypatch, route):
    """a large index, a small one, the large one again on ONE context: every export equals the restatement, which is what a
    fresh context exports (test_index_tables) -- stale record buffers, released digit bytes and a filter that shrinks from
    2^21 to 2^20 bits and grows again leave nothing behind.  Then the empty indexes and the large one once more."""
    c = None
    try:
        for step, name in enumerate(("ids/32769", "m/255", "ids/32769", "empty/short_only", "lengths", "empty/no_entries", "ids/32769")):
            tag = "%s [%s] step %d" % (name, route, step)
            c, got = _build(kslam, monkeypatch, name, route, ctx=c)
            _compare(got, S.expected(name, route), tag)
            if (name, route) in _EXPORTS:
                _compare(got, _EXPORTS[(name, route)], tag + " against a fresh context")
            if step in (2, 3, 4):
                _check_join(oracle, c, name, got, tag)
    finally:
        if c is not None:
            c.close()


def test_export_hook_refusals(kslam, monkeypatch):
    import ctypes as C
    L = kslam.lib()
    c = kslam.Context()
    try:
        x = kslam.IndexExport()
        assert L.kslam_debug_index_export(None, C.byref(x)) == kslam.KSLAM_ERR_ARG
        assert L.kslam_debug_index_export(c._h, None) == kslam.KSLAM_ERR_ARG
        assert kslam.STATUS[L.kslam_debug_index_export(c._h, C.byref(x))] == "ERR_STATE"          # no index yet
        with pytest.raises(kslam.KslamError) as e:
            c.debug_index_export()
        assert kslam.STATUS[e.value.status] == "ERR_STATE"
        c.set_index(list(S.index("m/257")))
        exp = S.expected("m/257", "default")
        assert L.kslam_debug_index_export(c._h, C.byref(x)) == 0                                  # the sizes alone
        assert (x.n_entries, x.n_genome_kmers, x.n_bases, x.bucket_bits, x.filter_bits, x.n_filter_bytes) == \
            (3, 257, exp["n_bases"], exp["bucket_bits"], 20, 1 << 17)
        # too little room in ONE buffer, or one buffer missing: refused, and no buffer is written at all
        need = {"offsets": 4 * 8, "codes": exp["n_bases"], "keys": 257 * 8, "meta": 257 * 8, "bucket": 257 * 4, "filter": 1 << 17}
        caps = {"cap_offsets": 4, "cap_codes": exp["n_bases"], "cap_records": 257, "cap_bucket": 257, "cap_filter": 1 << 17}
        for short in list(caps) + list(need):
            bufs = {k: np.full(v, kslam.DEBUG_SENTINEL_BYTE, dtype=np.uint8) for k, v in need.items()}
            y = kslam.IndexExport()
            for k in need:
                setattr(y, k, bufs[k].ctypes.data)
            for k, v in caps.items():
                setattr(y, k, v)
            if short in caps:
                setattr(y, short, caps[short] - 1)
            else:
                setattr(y, short, None)
            assert L.kslam_debug_index_export(c._h, C.byref(y)) == kslam.KSLAM_ERR_ARG, short
            assert all((b == kslam.DEBUG_SENTINEL_BYTE).all() for b in bufs.values()), short
        _compare(c.debug_index_export(), exp, "after the refusals")                               # and the context is as it was
    finally:
        c.close()
