"""The depth track on the GPU (csrc/depth.hip, include/kslam_depth.h): the device's rows and statistics against the host twin
(kslam_tail_depth) AND the plain-Python restatement (tests/depth_ref.py), exactly -- the walk, the entry seams, the runs, every
tile of the kernels, the filter, compaction at every threshold around a piece's key count, accumulation, the SNV table's depth as
a cross-check, the refusals, and real batches through kslam_stream_classify with one lane, three lanes, the host's SAM text and
pseudo-assembly left to the host."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import depth_ref as D
import variants_ref as V
from test_gpu_readsplit import _host_text, _indexed_context, world  # noqa: F401  (the fixture and its helpers)

pytestmark = pytest.mark.gpu
SEAMS = D.seam_cases()
TILE_CASES = D.tile_cases()
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = 1, 4, 5   # include/kslam.h: kslam_status
EMPTY = dict.fromkeys(D.STAT_NAMES, 0)


@pytest.fixture(scope="module")
def DP(kslam):
    return importlib.import_module("kslam_amd.depth")


@pytest.fixture(scope="module")
def VR(kslam):
    return importlib.import_module("kslam_amd.variants")


class _Bench:
    """one context; the index is rebuilt when a case brings other entries (kslam_set_index drops the state)"""

    def __init__(self, kslam, DP):
        self.c, self.DP, self.entries = kslam.Context(), DP, None

    def on(self, case):
        key = (case["gbases"].tobytes(), case["goff"].tobytes())
        if key != self.entries:
            self.keep = np.concatenate([case["gbases"], np.zeros(64, dtype=np.uint8)])
            self.c.set_index_arrays(self.keep, case["goff"])
            assert not self.DP.get_depth(self.c)   # a new index frees the state
            self.entries = key
            self.c.set_pairing(stages=3)
            self.DP.set_depth(self.c, True)
        else:
            self.DP.reset(self.c)
        self.DP.set_compact_at(self.c, 0)
        return self.c


@pytest.fixture(scope="module")
def bench(kslam, DP):
    b = _Bench(kslam, DP)
    yield b
    b.c.set_pairing(stages=0)
    b.c.close()


def twin(DP, c, min_depth=1):
    return DP.tail_depth(c["goff"], c["ov"], c["pool"], c["roff"], c["rp"], c["pr"], min_depth)


def _add(DP, ctx, c):
    DP.add(ctx, c["ov"], c["pool"], c["roff"], c["rp"], c["pr"])


def _expect(DP, c, min_depth=1):
    rows, stats = D.table(c, min_depth)
    got, got_stats = twin(DP, c, min_depth)
    assert D.fields(got) == rows and got_stats == stats
    return rows, stats


def _device_equals(DP, ctx, c, rows, stats, min_depth=1):
    got, got_stats = DP.take(ctx, min_depth)
    assert got_stats == stats, c["name"]
    assert D.fields(got) == rows, c["name"]


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_walk_entry_seams_and_runs(DP, bench, name):
    case, expected, skipped = SEAMS[name]
    ctx = bench.on(case)
    rows, stats = _expect(DP, case)
    assert rows == expected and stats["n_skipped"] == skipped     # the hand-written rows (tests/test_depth_ref.py)
    _add(DP, ctx, case)
    _device_equals(DP, ctx, case, rows, stats)


@pytest.mark.parametrize("case", TILE_CASES, ids=[c["name"] for c in TILE_CASES])
def test_tiles(DP, bench, case):
    ctx = bench.on(case)
    rows, stats = _expect(DP, case)
    kind, n = case["name"].split("-")
    assert stats["n_records" if kind == "records" else "n_keys"] == int(n)
    _add(DP, ctx, case)
    _device_equals(DP, ctx, case, rows, stats)


def test_filter(DP, bench):
    c = D.filter_case()
    ctx = bench.on(c)
    _add(DP, ctx, c)
    for m in (1, 2, 3, 0):
        rows, stats = _expect(DP, c, m)
        _device_equals(DP, ctx, c, rows, stats, m)
    assert D.fields(DP.take(ctx, 2)[0]) == [(0, 5, 10, 2), (0, 10, 20, 3), (0, 20, 25, 2)]     # dropped, never merged
    assert D.fields(DP.take(ctx, 0)[0]) == D.fields(DP.take(ctx, 1)[0])


@pytest.fixture(scope="module")
def pieces():
    """concat(a, b) of two random cases over the same entries, each of them two pieces: four adds"""
    _, _, ents = D.random_cases()
    parts = [V.random_case("p%d" % k, 78 + k, n, 7, entries=ents) for k, n in enumerate((500, 900, 700, 700))]
    a, b = V.concat(parts[0], parts[1]), V.concat(parts[2], parts[3])
    return parts, V.concat(a, b)


def test_compaction_changes_no_row(DP, bench, pieces):
    parts, whole = pieces
    rows, stats = _expect(DP, whole)
    first_keys = 2 * D.table(parts[0])[1]["n_intervals"]
    assert first_keys > 200 and stats["n_keys"] < 2 * stats["n_intervals"]      # boundaries do coincide: there is something to compact
    ctx = bench.on(whole)
    for compact_at, after_first in ((1, True), (first_keys, False), (first_keys - 1, True), (first_keys + 1, False), (0, False)):
        DP.reset(ctx)
        DP.set_compact_at(ctx, compact_at)
        for k, p in enumerate(parts):
            _add(DP, ctx, p)
            if k == 0:
                assert (DP.kernel_ms(ctx)[1] > 0) == after_first, compact_at     # a compaction ran exactly when the keys EXCEEDED the threshold
        _device_equals(DP, ctx, whole, rows, stats)
        emit_ms, compact_ms, take_ms = DP.kernel_ms(ctx)
        assert emit_ms > 0 and compact_ms > 0 and take_ms > 0
        _device_equals(DP, ctx, whole, rows, stats)                              # again: nothing is pending
        assert DP.kernel_ms(ctx)[1] == compact_ms                                # ... so no compaction ran
    DP.set_compact_at(ctx, 0)


def test_accumulation_reset_growth_and_switch(DP, bench):
    a, b, _ = D.random_cases()
    both, other = V.concat(a, b), V.concat(b, a)
    rows, stats = _expect(DP, both)
    assert _expect(DP, other) == (rows, stats) and stats["n_intervals"] > 3 * D.table(a)[1]["n_intervals"] > 0
    ctx = bench.on(a)
    _add(DP, ctx, a)
    first = D.table(a)
    _device_equals(DP, ctx, a, *first)
    _add(DP, ctx, b)                                           # an add after a take
    _device_equals(DP, ctx, both, rows, stats)
    _device_equals(DP, ctx, both, rows, stats)                 # take twice: the same rows
    _device_equals(DP, ctx, both, *D.table(both, 3), 3)        # and with another threshold
    DP.reset(ctx)
    _add(DP, ctx, both)                                        # one add of the concatenation
    _device_equals(DP, ctx, both, rows, stats)
    DP.reset(ctx)
    _add(DP, ctx, b)                                           # the order of the batches does not matter
    _add(DP, ctx, a)
    _device_equals(DP, ctx, both, rows, stats)
    DP.reset(ctx)
    got, got_stats = DP.take(ctx, 1)
    assert len(got) == 0 and got_stats == EMPTY
    _add(DP, ctx, a)
    DP.set_depth(ctx, False)
    assert not DP.get_depth(ctx)
    DP.set_depth(ctx, True)                                    # off and on again starts from nothing
    got, got_stats = DP.take(ctx, 1)
    assert len(got) == 0 and got_stats == EMPTY
    _add(DP, ctx, a)
    _device_equals(DP, ctx, a, *first)
    # kslam_set_index frees the state too
    bench.entries = None
    ctx = bench.on(a)
    got, got_stats = DP.take(ctx, 1)
    assert len(got) == 0 and got_stats == EMPTY


def test_cross_check_against_the_snv_table(DP, VR, bench):
    """the scan-based depth here against the search-based one of csrc/variants.hip, both switches on"""
    a, b, _ = D.random_cases()
    for c in (a, b, V.concat(a, b)):
        ctx = bench.on(c)
        VR.set_variants(ctx, True)
        VR.reset(ctx)
        _add(DP, ctx, c)
        VR.add(ctx, c["ov"], c["pool"], c["rbases"], c["roff"], c["rp"], c["pr"])
        sites, vs = VR.take(ctx, 1, 0)
        rows, ds = DP.take(ctx, 1)
        assert [ds[k] for k in ("n_records", "n_skipped", "n_intervals")] == [vs[k] for k in ("n_records", "n_skipped", "n_intervals")]
        track = [np.zeros(int(c["goff"][e + 1] - c["goff"][e]), dtype=np.int64) for e in range(len(c["goff"]) - 1)]
        for e, s, t, v in D.fields(rows):
            track[e][s:t] = v
        assert len(sites) > 100
        for r in sites:
            assert int(r["depth"]) == int(track[int(r["entry"])][int(r["pos"])])      # 0 where no row covers the position
        VR.set_variants(ctx, False)


def test_refusals(kslam, DP):
    L = DP.lib()
    bld = V.Builder("x", [b"ACGT" * 25])
    bld.group([(0, bld.aligned(0, 0, [(20, "M")], 0), bld.aligned(0, 30, [(20, "M")], 1))])
    bld.single(bld.aligned(0, 50, [(4, "M")], 0))
    case = bld.done()
    keep = np.concatenate([case["gbases"], np.zeros(64, dtype=np.uint8)])

    def args(**kw):
        a = {k: kw.get(k, case[k]) for k in ("ov", "pool", "roff", "rp", "pr")}
        return (a["ov"].ctypes.data, len(a["ov"]), a["pool"].ctypes.data, len(a["pool"]), a["roff"].ctypes.data, len(a["roff"]) - 1,
                a["rp"].ctypes.data, len(a["rp"]), a["pr"].ctypes.data, len(a["pr"]))

    rows, n, st = C.c_void_p(), C.c_uint64(), DP.Stats()
    c = kslam.Context()
    try:
        c.set_pairing(stages=3)
        assert L.kslam_set_depth(c._h, 1) == ERR_STATE                    # no index
        assert b"kslam_set_index" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=0)
        c.set_index_arrays(keep, case["goff"])
        assert L.kslam_set_depth(c._h, 1) == ERR_STATE                    # the pairing is off
        assert b"kslam_set_pairing" in c._L.kslam_last_error(c._h)
        for call in (lambda: L.kslam_depth_reset(c._h), lambda: L.kslam_depth_add(c._h, *args()),
                     lambda: L.kslam_depth_take(c._h, 1, C.byref(rows), C.byref(n), C.byref(st))):
            assert call() == ERR_STATE and b"kslam_set_depth" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=3)
        DP.set_depth(c, True)
        for field, kw, message in (("pr", ("r1", 1, len(case["ov"])), b"refers to overlap record"), ("rp", ("count", 1, 2), b"outside the pairs array"),
                                   ("rp", ("first", 1, 0), b"ascend"), ("ov", ("cigar_off", 1, len(case["pool"])), b"outside the pool"),
                                   ("ov", ("read", 2, len(case["roff"]) - 1), b"refers to read")):
            bad = case[field].copy()
            bad[kw[0]][kw[1]] = kw[2]
            assert L.kslam_depth_add(c._h, *args(**{field: bad})) == ERR_ARG
            assert message in c._L.kslam_last_error(c._h)
        roff = case["roff"].copy()
        roff[1] = roff[2] + 1
        assert L.kslam_depth_add(c._h, *args(roff=roff)) == ERR_ARG and b"read offsets must ascend" in c._L.kslam_last_error(c._h)
        got, stats = DP.take(c, 1)
        assert len(got) == 0 and stats == EMPTY                           # nothing was added
        _add(DP, c, case)
        assert D.fields(DP.take(c, 1)[0]) == D.table(case)[0] == [(0, 0, 20, 1), (0, 30, 54, 1)]
        DP.set_depth(c, False)
    finally:
        c.set_pairing(stages=0)
        c.close()
    c = kslam.Context(report_cigar=False)
    try:
        c.set_index_arrays(keep, case["goff"])
        c.set_pairing(stages=3)
        assert L.kslam_set_depth(c._h, 1) == ERR_STATE and b"report_cigar" in c._L.kslam_last_error(c._h)
    finally:
        c.set_pairing(stages=0)
        c.close()
    m = kslam.MultiContext([0])
    try:
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)   # (tests/test_gpu_readsplit.py: the first context)
        assert L.kslam_set_depth(h, 1) == ERR_UNSUPPORTED
        assert L.kslam_stream_set_depth(h, 1, 1) == ERR_UNSUPPORTED
    finally:
        m.close()


# ---- real batches through the lanes: the world of tests/test_gpu_readsplit.py ----

def _stream_files(kslam, DP, world, tmp, tag, lanes, env=None, depth=True):
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    env = dict(env or {}, KSLAM_LANES=str(lanes))
    os.environ.update(env)
    try:
        c = _indexed_context(kslam, world)
        h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
        tax = X.TaxDB(world["case"]["taxdb"])
        names = {k: str(tmp / (tag + "." + k)) for k in ("bg", "per_read", "sam")}
        fds = {k: os.open(p, os.O_RDWR | os.O_CREAT | os.O_TRUNC) for k, p in names.items()}
        st = S.classify_stream_native(c, world["db"], h1.ptr, len(r1), h2.ptr, len(r2), 300, T.TailParams.default(paired=True), taxdb=tax,
                                      sam_fd=fds["sam"], per_read_fd=fds["per_read"], depth=3, depth_fd=fds["bg"] if depth else None, depth_min=1)
        assert not DP.get_depth(c)   # the call switched it off again
        for fd in fds.values():
            os.close(fd)
        c.close()
        h1.close()
        h2.close()
    finally:
        for k in env:
            del os.environ[k]
    return {k: open(p, "rb").read() for k, p in names.items()}, st


def _twin_file(kslam, DP, world):
    """the same batches through the Python loop: the final arrays of every batch with its CIGAR pool and its reads' offsets,
    concatenated, through the host twin and the bedGraph writer"""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    got = []
    try:
        S.classify_stream(c, world["db"], h1.ptr, len(r1), h2.ptr, len(r2), 300, T.TailParams.default(paired=True), depth=3,
                          on_batch=lambda rec, ov, cg, rp, pr, reads: got.append((np.array(ov), np.array(cg), np.array(rp), np.array(pr), np.array(reads.bases_off))))
    finally:
        c.close()
        h1.close()
        h2.close()
    assert len(got) == 3
    ents = [bytes(e["bases"]) for e in world["case"]["entries"]]
    gbases = np.frombuffer(b"".join(ents), dtype=np.uint8)
    goff = np.concatenate([[0], np.cumsum([len(e) for e in ents])]).astype(np.uint64)
    whole = None
    for ov, cg, rp, pr, bases_off in got:
        roff = (bases_off - bases_off[0]).astype(np.uint64)
        part = {"name": "batch", "gbases": gbases, "goff": goff, "rbases": np.zeros(int(roff[-1]), dtype=np.uint8), "roff": roff,
                "pool": cg.astype(np.uint32), "ov": ov.astype(V.OVERLAP_DT), "rp": rp.astype(V.READ_PAIR_DT), "pr": pr.astype(V.PAIRED_OVERLAP_DT)}
        whole = part if whole is None else V.concat(whole, part)
    rows, stats = twin(DP, whole, 1)
    ref_rows, ref_stats = D.table(whole, 1)
    assert D.fields(rows) == ref_rows and stats == ref_stats and stats["n_skipped"] == 0 and stats["n_intervals"] > 500
    return DP.report_bytes(world["db"], rows), rows


def test_three_batches_through_the_stream(kslam, DP, world, tmp_path):
    exp, rows = _twin_file(kslam, DP, world)
    plain, _ = _stream_files(kslam, DP, world, tmp_path, "plain", 1, depth=False)
    assert plain["bg"] == b""
    files, st = _stream_files(kslam, DP, world, tmp_path, "l1", 1)
    assert files["bg"] == exp and st["batches_pseudo_on_host"] == 0 and len(exp) > 1000
    assert files["sam"] == plain["sam"] and files["per_read"] == plain["per_read"] and len(plain["sam"]) > 10000   # nothing else moves
    assert _stream_files(kslam, DP, world, tmp_path, "l3", 3)[0]["bg"] == exp
    assert _stream_files(kslam, DP, world, tmp_path, "host", 2, env={"KSLAM_HOST_SAM_TEXT": "1"})[0]["bg"] == exp
    # pseudo-assembly left to the host for every batch: the keys come in through kslam_depth_add on the host stage's thread
    left, st = _stream_files(kslam, DP, world, tmp_path, "cap", 2, env={"KSLAM_PSEUDO_CAP": "3"})
    assert st["batches_pseudo_on_host"] == 3 and left["bg"] == exp
    loci = [bytes(e["locusTag"]).decode() for e in world["case"]["entries"]]
    assert DP.parse_bedgraph(exp) == [(loci[e], s, t, v) for e, s, t, v in D.fields(rows)]
