"""The indel table on the GPU (csrc/indels.hip, include/kslam_indels.h): the device's rows and statistics through
kslam_indels_add against the host twin (kslam_tail_indels) AND the plain-Python restatement (tests/indels_ref.py), field for
field -- the grid seams, homopolymers and tandem repeats at every phase, the entry's start, the alphabet, the limits, a shift of
5 000 steps inside a wave of records without one, both strands, depth and the filters, the rows' order, accumulation and the
refusals."""
import ctypes as C
import importlib

import numpy as np
import pytest

import indels_ref as R

pytestmark = pytest.mark.gpu
CASES = R.cases()
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = 1, 4, 5   # include/kslam.h: kslam_status


@pytest.fixture(scope="module")
def ID(kslam):
    return importlib.import_module("kslam_amd.indels")


class _Bench:
    """one context; the index is rebuilt when a case brings other entries (kslam_set_index drops the state)"""

    def __init__(self, kslam, ID):
        self.c, self.ID, self.entries = kslam.Context(), ID, None

    def on(self, case):
        key = (case["gbases"].tobytes(), case["goff"].tobytes())
        if key != self.entries:
            self.keep = np.concatenate([case["gbases"], np.zeros(64, dtype=np.uint8)])
            self.c.set_index_arrays(self.keep, case["goff"])
            assert not self.ID.get_indels(self.c)   # a new index frees the state
            self.entries = key
            self.c.set_pairing(stages=3)
            self.ID.set_indels(self.c, True)
        else:
            self.ID.reset(self.c)
        return self.c


@pytest.fixture(scope="module")
def bench(kslam, ID):
    b = _Bench(kslam, ID)
    yield b
    b.c.set_pairing(stages=0)
    b.c.close()


def twin(ID, c, min_alt=1, min_depth=0):
    return ID.tail_indels(c["gbases"], c["goff"], c["ov"], c["pool"], c["rbases"], c["roff"], c["rp"], c["pr"], min_alt, min_depth)


def _add(ID, ctx, c):
    ID.add(ctx, c["ov"], c["pool"], c["rbases"], c["roff"], c["rp"], c["pr"])


def _expect(ID, c, min_alt=1, min_depth=0):
    rows, stats = R.table(c, min_alt, min_depth)
    got, got_stats = twin(ID, c, min_alt, min_depth)
    assert R.fields(got) == rows and got_stats == stats
    return rows, stats


def _device_equals(ID, ctx, c, rows, stats, min_alt=1, min_depth=0):
    got, got_stats = ID.take(ctx, min_alt, min_depth)
    assert got_stats == stats, c["name"]
    assert R.fields(got) == rows, c["name"]
    assert not got["pad"].any() and not got["pad2"].any()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_rows_equal_twin_and_restatement(ID, bench, case):
    ctx = bench.on(case)
    rows, stats = _expect(ID, case)
    assert stats["n_deletions"] + stats["n_insertions"] > 0
    _add(ID, ctx, case)
    _device_equals(ID, ctx, case, rows, stats)


def test_one_row_per_haplotype_change(ID, bench):
    """what the repeats are there for, on the device's own rows"""
    by = {c["name"]: c for c in CASES}
    a = len(R.LEFT) - 1
    for name, expect in (("homopolymer", [(0, a, R.DEL, 1, b"", 8), (0, a, R.INS, 1, b"A", 9)]),
                         ("tandem-2", [(0, a, R.DEL, 2, b"", 11), (0, a, R.INS, 2, b"CA", 13)]),
                         ("entry-start", [(0, 0, R.DEL, 1, b"", 7), (0, 0, R.INS, 1, b"A", 8)]),
                         ("after-same-base", [(1, 0, R.DEL, 1, b"", 7), (1, 0, R.INS, 1, b"A", 8)])):
        ctx = bench.on(by[name])
        _add(ID, ctx, by[name])
        got = R.fields(ID.take(ctx, 1, 0)[0])
        assert [r[:5] + (r[5] + r[6],) for r in got] == expect, name
        assert all(r[5] > 0 and r[6] > 0 for r in got)
    ctx = bench.on(by["long-shift"])
    _add(ID, ctx, by["long-shift"])
    got = [r for r in R.fields(ID.take(ctx, 1, 0)[0]) if r[1] == a]
    assert [r[:7] for r in got] == [(0, a, R.DEL, 1, b"", 1, 0), (0, a, R.INS, 1, b"A", 0, 1)]


def test_filters_and_more_alt_than_depth(ID, bench):
    c = [c for c in CASES if c["name"] == "depth"][0]
    ctx = bench.on(c)
    _add(ID, ctx, c)
    for min_alt in (1, 2, 3, 4):
        for min_depth in (0, 1, 2, 3, 99):
            rows, stats = _expect(ID, c, min_alt, min_depth)
            _device_equals(ID, ctx, c, rows, stats, min_alt, min_depth)
    got = R.fields(ID.take(ctx, 3, 2)[0])
    assert [r[:5] for r in got] == [(0, 49, R.DEL, 2, b""), (0, 49, R.INS, 2, b"AT"), (0, 100, R.DEL, 1, b"")]
    assert got[2][5:] == (3, 0, 2)     # AO 3 over DP 2: reported as counted


def test_accumulation_reset_growth_and_switch(ID, bench):
    a = R.random_case("a", 71, 200, n_entries=5)
    ents = [R.entry_bytes(a, e) for e in range(5)]
    rng = np.random.default_rng(72)
    bb = R.Builder("b", ents)                                    # ten times a's records: the buffers grow and keep a's keys
    for k in range(2000):
        e = int(rng.integers(0, 5))
        n = len(ents[e])
        at = int(rng.integers(1, n - 3))
        R.al(bb, e, 0, R.split_at(n, at, "DI"[k & 1], 1 + k % 3), rc=(k >> 1) & 1, fill=b"ACCA")
    b = bb.done()
    both, other = R.concat_cases(a, b), R.concat_cases(b, a)
    rows, stats = _expect(ID, both)
    assert _expect(ID, other) == (rows, stats) and stats["n_deletions"] > 1000 and stats["n_insertions"] > 1000
    ctx = bench.on(a)
    _add(ID, ctx, a)
    first = R.table(a)
    _device_equals(ID, ctx, a, *first)
    _add(ID, ctx, b)                                             # an add after a take
    _device_equals(ID, ctx, both, rows, stats)
    _device_equals(ID, ctx, both, rows, stats)                   # take twice: the same rows
    _device_equals(ID, ctx, both, *R.table(both, 2, 3), 2, 3)    # and with other thresholds
    ID.reset(ctx)
    _add(ID, ctx, both)                                          # one add of the concatenation
    _device_equals(ID, ctx, both, rows, stats)
    ID.reset(ctx)
    _add(ID, ctx, b)                                             # the order of the batches does not matter
    _add(ID, ctx, a)
    _device_equals(ID, ctx, both, rows, stats)
    empty = dict.fromkeys(R.STAT_NAMES, 0)
    ID.reset(ctx)
    got, got_stats = ID.take(ctx, 1, 0)
    assert len(got) == 0 and got_stats == empty
    _add(ID, ctx, a)
    ID.set_indels(ctx, False)
    assert not ID.get_indels(ctx)
    ID.set_indels(ctx, True)                                     # off and on again starts from nothing
    got, got_stats = ID.take(ctx, 1, 0)
    assert len(got) == 0 and got_stats == empty
    _add(ID, ctx, a)
    _device_equals(ID, ctx, a, *first)
    assert ID.kernel_ms(ctx)[0] > 0 and ID.kernel_ms(ctx)[1] > 0
    bench.entries = None                                         # kslam_set_index frees the state too
    ctx = bench.on(a)
    got, got_stats = ID.take(ctx, 1, 0)
    assert len(got) == 0 and got_stats == empty


def test_the_variants_switch_is_not_needed_and_not_disturbed(kslam, ID, bench):
    VR = importlib.import_module("kslam_amd.variants")
    c = [c for c in CASES if c["name"] == "strands"][0]
    ctx = bench.on(c)
    assert not VR.get_variants(ctx)
    _add(ID, ctx, c)
    VR.set_variants(ctx, True)
    VR.add(ctx, c["ov"], c["pool"], c["rbases"], c["roff"], c["rp"], c["pr"])
    _device_equals(ID, ctx, c, *R.table(c))
    assert VR.take(ctx, 1, 0)[1]["n_intervals"] == R.table(c)[1]["n_intervals"]
    VR.set_variants(ctx, False)
    _device_equals(ID, ctx, c, *R.table(c))


def test_refusals(kslam, ID):
    L = ID.lib()
    bld = R.Builder("x", [b"ACGT" * 25])
    bld.group([(0, R.al(bld, 0, 0, R.split_at(40, 20, "D", 2), single=False), R.al(bld, 0, 30, R.split_at(40, 20, "I", 2), rc=1, fill=b"GG", single=False))])
    R.al(bld, 0, 50, [(4, "M"), (1, "D"), (4, "M")])
    case = bld.done()
    keep = np.concatenate([case["gbases"], np.zeros(64, dtype=np.uint8)])

    def args(**kw):
        a = {k: kw.get(k, case[k]) for k in ("ov", "pool", "rbases", "roff", "rp", "pr")}
        return (a["ov"].ctypes.data, len(a["ov"]), a["pool"].ctypes.data, len(a["pool"]), a["rbases"].ctypes.data, a["roff"].ctypes.data,
                len(a["roff"]) - 1, a["rp"].ctypes.data, len(a["rp"]), a["pr"].ctypes.data, len(a["pr"]))

    c = kslam.Context()
    try:
        c.set_pairing(stages=3)
        assert L.kslam_set_indels(c._h, 1) == ERR_STATE                   # no index
        assert b"kslam_set_index" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=0)
        c.set_index_arrays(keep, case["goff"])
        assert L.kslam_set_indels(c._h, 1) == ERR_STATE                   # the pairing is off
        assert b"kslam_set_pairing" in c._L.kslam_last_error(c._h)
        for call in (lambda: L.kslam_indels_reset(c._h), lambda: L.kslam_indels_add(c._h, *args())):
            assert call() == ERR_STATE and b"kslam_set_indels" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=3)
        ID.set_indels(c, True)
        for field, kw, message in (("pr", ("r1", 1, len(case["ov"])), b"refers to overlap record"), ("rp", ("count", 1, 2), b"outside the pairs array"),
                                   ("rp", ("first", 1, 0), b"ascend"), ("ov", ("cigar_off", 1, len(case["pool"])), b"outside the pool"),
                                   ("ov", ("read", 2, len(case["roff"]) - 1), b"refers to read")):
            bad = case[field].copy()
            bad[kw[0]][kw[1]] = kw[2]
            assert L.kslam_indels_add(c._h, *args(**{field: bad})) == ERR_ARG
            assert message in c._L.kslam_last_error(c._h)
        got, stats = ID.take(c, 1, 0)
        assert len(got) == 0 and stats == dict.fromkeys(R.STAT_NAMES, 0)   # nothing was added
        _add(ID, c, case)
        assert R.fields(ID.take(c, 1, 0)[0]) == R.table(case)[0] and len(R.table(case)[0]) == 3
        ID.set_indels(c, False)
    finally:
        c.set_pairing(stages=0)
        c.close()
    c = kslam.Context(report_cigar=False)
    try:
        c.set_index_arrays(keep, case["goff"])
        c.set_pairing(stages=3)
        assert L.kslam_set_indels(c._h, 1) == ERR_STATE and b"report_cigar" in c._L.kslam_last_error(c._h)
    finally:
        c.set_pairing(stages=0)
        c.close()
    m = kslam.MultiContext([0])
    try:
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)   # (tests/test_gpu_readsplit.py: the first context)
        assert L.kslam_set_indels(h, 1) == ERR_UNSUPPORTED
        assert L.kslam_stream_set_indels(h, 1, 2, 1) == ERR_UNSUPPORTED
    finally:
        m.close()
