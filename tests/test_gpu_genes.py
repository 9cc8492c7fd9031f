"""The per-gene abundance table on the GPU (csrc/genes.hip, include/kslam_genes.h): the indexed lookup against the linear walk
AND the plain-Python restatement (tests/genes_ref.py), gene and shared, at its seams; the counted rows against the host twin
(kslam_tail_genes) and the restatement at the count and take seams; accumulation, the switch, the refusals; and real batches
through kslam_stream_classify with one lane, three lanes and pseudo-assembly left to the host."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import genes_ref as R
from test_gpu_readsplit import _host_text, _indexed_context, world  # noqa: F401  (the fixture and its helpers)

pytestmark = pytest.mark.gpu
CASES = R.cases()
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = 1, 4, 5   # include/kslam.h: kslam_status
SORT_TILE, SCAN_TILE = 4096, 4096               # csrc/common.h, csrc/scan.hip


@pytest.fixture(scope="module")
def GN(kslam):
    return importlib.import_module("kslam_amd.genes")


@pytest.fixture(scope="module")
def ST(kslam):
    return importlib.import_module("kslam_amd.samtext")


def _set_entries(ctx, n):
    """an index of n entries of 40 bases: the gene table asks the index for the number of entries alone"""
    ctx.set_index_arrays(np.frombuffer(b"ACGTTGCAAC" * (4 * n), dtype=np.uint8), np.arange(n + 1, dtype=np.uint64) * 40)


class _Bench:
    """one context; the index is rebuilt when a case brings another number of entries, the annotations and the table when it
    brings other genes (kslam_set_index and kslam_set_sam_annotations drop the table)"""

    def __init__(self, kslam, GN, ST):
        self.c, self.GN, self.ST, self.n, self.key, self.index = kslam.Context(), GN, ST, None, None, None

    def on(self, first, starts, stops):
        key = (np.asarray(first).tobytes(), np.asarray(starts).tobytes(), np.asarray(stops).tobytes())
        if key != self.key:
            if len(first) - 1 != self.n:
                _set_entries(self.c, len(first) - 1)
                self.n = len(first) - 1
                self.c.set_pairing(stages=3)
            self.index = self.GN.GeneIndex(first, starts, stops)
            self.ST.set_annotations(self.c, self.index)
            assert not self.GN.get_genes(self.c)   # new annotations free the table
            self.GN.set_genes(self.c, True)
            self.key = key
        else:
            self.GN.reset(self.c)
        return self.c


@pytest.fixture(scope="module")
def bench(kslam, GN, ST):
    b = _Bench(kslam, GN, ST)
    yield b
    b.c.set_pairing(stages=0)
    b.c.close()


# ---- the lookup ----

def _lookup_three_ways(GN, bench, per_entry, queries):
    first, starts, stops = R.genes_of(per_entry)
    ctx = bench.on(first, starts, stops)
    e, b, t = (np.array([q[k] for q in queries], dtype=np.int64) for k in range(3))
    exp_g, exp_s = R.lookups(first, starts, stops, e, b, t)
    for linear in (False, True):
        g, s = GN.lookup(ctx, e, b, t, linear=linear)
        assert g.tolist() == exp_g.tolist(), ("linear" if linear else "indexed")
        assert s.tolist() == exp_s.tolist(), ("linear" if linear else "indexed")
    return exp_g.tolist(), exp_s.tolist()


def test_lookup_seams_of_one_gene(GN, bench):
    per_entry = [[], [(100, 400)], [(7, 9)]]             # an entry without genes first; the last entry has one too
    q = [(0, 0, 1000),                                   # the entry with 0 genes
         (1, 0, 100), (1, 0, 101),                       # ends exactly at gene_start: nothing shared; one base further
         (1, 400, 500), (1, 399, 500),                   # starts at gene_stop; one base before
         (1, 150, 150), (1, 200, 150), (1, 100, 400), (1, 0, 1000),   # ref_end <= ref_start; the gene itself; around it
         (2, 0, 8), (2, 8, 100), (2, 9, 100),            # the last entry
         (3, 100, 200), (0xFFFFFFFF, 0, 10)]             # entry >= n_entries
    g, s = _lookup_three_ways(GN, bench, per_entry, q)
    assert g == [-1, -1, 0, -1, 0, -1, -1, 0, 0, 1, 1, -1, -2, -2]   # (gene 0 is entry 1's, gene 1 entry 2's)
    assert s == [0, 0, 1, 0, 1, 0, 0, 300, 300, 1, 1, 0, 0, 0]


def test_lookup_ties_nesting_and_odd_genes(GN, bench):
    per_entry = [
        [(100, 300), (50, 250)],                         # 0: the lower file index sorts LATER by start
        [(10, 90), (10, 50), (10, 90)],                  # 1: equal starts, identical duplicates
        [(0, 10000), (400, 450), (5000, 5100)],          # 2: short genes nested in a long one that starts first
        [(500, 100), (200, 300)],                        # 3: a gene with stop < start
        [(-80, 40), (-10, 5)],                           # 4: negative starts
        [(100000, 100500), (30, 60)],                    # 5: a gene past the entry's end
        [(900, 950), (600, 700), (300, 400), (0, 100)]]  # 6: file order descending by start
    q = [(0, 100, 250), (0, 60, 120), (0, 240, 300), (0, 50, 300),
         (1, 0, 100), (1, 20, 40), (1, 60, 80), (1, 50, 50),
         (2, 300, 460), (2, 420, 440), (2, 6000, 6100), (2, 4990, 5200), (2, 9999, 20000), (2, 10000, 20000),
         (3, 100, 500), (3, 250, 260), (3, 0, 1000),
         (4, -100, 0), (4, -5, 100), (4, -2147483648, 2147483647), (4, 2147483647, -2147483648),
         (5, 0, 1000), (5, 99000, 200000), (5, 60, 100000),
         (6, 0, 1000), (6, 650, 940), (6, 100, 300), (6, 390, 610)]
    g, s = _lookup_three_ways(GN, bench, per_entry, q)
    assert g[0] == 0 and s[0] == 150                     # genes 0 and 1 both share 150: gene 0 wins
    assert g[4:7] == [2, 2, 2] and s[4:7] == [80, 20, 20]   # (genes 2 .. 4 are entry 1's; the first of the equals)
    assert g[8:12] == [5, 5, 5, 5]                       # the long gene, found although a later start lies before the interval
    assert g[14:17] == [9, 9, 9]                         # never the gene whose stop lies before its start


def _genes_of_size(rng, n, long_first=False):
    """n genes: random places, some nested, duplicate or stop < start; long_first: gene 0 spans everything"""
    out = R.random_genes(rng, 1, 0)[0]
    while len(out) < n:
        out += [g for g in R.random_genes(rng, 1, 40)[0]]
    out = out[:n]
    if long_first and n:
        out[0] = (-50, 100000)
    return out


def test_lookup_across_the_wavefront_the_sort_tile_and_the_entry_seams(GN, bench):
    """entries of 0, 64, 65, SORT_TILE and SORT_TILE + 1 genes side by side (8 000 genes: two sort tiles, 33 workgroups of the
    max-scan, every entry seam inside a workgroup); the long first gene of the largest entry is found from positions 16
    workgroups behind it"""
    rng = np.random.default_rng(77)
    sizes = [0, 64, 65, 0, SORT_TILE, SORT_TILE + 1, 1, 3]
    per_entry = [_genes_of_size(rng, n, long_first=(n == SORT_TILE + 1)) for n in sizes]
    q = []
    for e in range(len(sizes)):
        for _ in range(24):
            b = int(rng.integers(-100, 5400))
            q.append((e, b, b + int(rng.integers(-3, 300))))
    q += [(5, 60000, 60100), (5, 5500, 99999), (4, 60000, 60100), (len(sizes), 0, 10)]
    g, s = _lookup_three_ways(GN, bench, per_entry, q)
    first = R.genes_of(per_entry)[0]
    assert g[-4:] == [first[5], first[5], -1, -2] and s[-4:-2] == [100, 99999 - 5500]
    assert sum(1 for x in g if x >= 0) >= 80             # (the intervals do find genes: 100 of the 196 with this seed)


def test_lookup_never_crosses_into_the_neighbouring_entry(GN, bench):
    """two neighbouring entries with identical genes, between entries without any: an interval is answered from its own entry's
    slice -- the same position in it -- and an entry whose genes all stop early is not kept open by the neighbour's long gene"""
    twin = [(0, 50000), (100, 200), (100, 200), (300, 250), (400, 500)]
    per_entry = [[], list(twin), list(twin), [(10, 20), (30, 40)], [(0, 90000)], []]
    q = []
    for e in range(6):
        q += [(e, 0, 100000), (e, 120, 180), (e, 390, 520), (e, 45000, 60000), (e, 15, 35), (e, 60, 70)]
    g, s = _lookup_three_ways(GN, bench, per_entry, q)
    assert g[6:12] == [0, 0, 0, 0, 0, 0] and g[12:18] == [5, 5, 5, 5, 5, 5]   # the same genes, each in its own entry
    assert g[18:24] == [10, -1, -1, -1, 10, -1]          # entry 3 between two long genes
    assert g[0:6] == [-1] * 6 and g[30:36] == [-1] * 6


# ---- the count passes ----

def _expect(GN, c):
    rows, st = R.table(c)
    twin, twin_st = GN.tail_genes(GN.GeneIndex(c["first"], c["starts"], c["stops"]), c["rp"], c["pr"])
    assert twin.tolist() == rows.tolist() and twin_st == st
    return rows, st


def _device_equals(GN, ctx, c, rows, st):
    got, got_st = GN.take(ctx)
    assert got.tolist() == rows.tolist(), c["name"]
    assert got_st == st, c["name"]
    assert got_st["n_in_gene"] + got_st["n_no_gene"] + got_st["n_skipped"] == got_st["n_alignments"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_rows_equal_twin_and_restatement(GN, bench, case):
    ctx = bench.on(case["first"], case["starts"], case["stops"])
    rows, st = _expect(GN, case)
    GN.add(ctx, case["rp"], case["pr"])
    _device_equals(GN, ctx, case, rows, st)


def test_the_linear_count_pass_gives_the_same_rows(GN, bench):
    case = R.random_case("linear", 31, 5000, 9, 25)
    ctx = bench.on(case["first"], case["starts"], case["stops"])
    rows, st = _expect(GN, case)
    os.environ["KSLAM_GENES_LOOKUP"] = "linear"
    try:
        GN.add(ctx, case["rp"], case["pr"])
    finally:
        del os.environ["KSLAM_GENES_LOOKUP"]
    _device_equals(GN, ctx, case, rows, st)


def test_take_seams(GN, bench):
    """9 000 disjoint genes over 90 entries: every gene counted, then every third (the compacted rows leave their flags' scan
    tile: row 1 366 is gene 4 098), then none"""
    per_entry = [[(10 * k, 10 * k + 8) for k in range(100)] for _ in range(90)]
    every = [([(g // 100, 10 * (g % 100) + 1, 10 * (g % 100) + 7)], []) for g in range(9000)]
    c = R.build("every-gene", per_entry, every)
    ctx = bench.on(c["first"], c["starts"], c["stops"])
    rows, st = _expect(GN, c)
    assert rows["gene"].tolist() == list(range(9000)) and len(rows) > 2 * SCAN_TILE
    GN.add(ctx, c["rp"], c["pr"])
    _device_equals(GN, ctx, c, rows, st)
    third = R.build("every-third", per_entry, every[::3])
    ctx = bench.on(c["first"], c["starts"], c["stops"])
    rows, st = _expect(GN, third)
    assert rows["gene"].tolist() == list(range(0, 9000, 3)) and rows["gene"][SCAN_TILE // 3 + 1] == SCAN_TILE + 2
    GN.add(ctx, third["rp"], third["pr"])
    _device_equals(GN, ctx, third, rows, st)
    GN.reset(ctx)
    got, got_st = GN.take(ctx)
    assert len(got) == 0 and got_st == dict.fromkeys(got_st, 0)


# ---- state ----

def test_accumulation_reset_and_switch(GN, ST, bench):
    a = R.random_case("a", 71, 3000, 7, 20)
    per_entry = [[(int(a["starts"][g]), int(a["stops"][g])) for g in range(int(a["first"][e]), int(a["first"][e + 1]))] for e in range(7)]
    b = R.random_case("b", 72, 2500, 7, 20, per_entry=per_entry)
    both = R.concat(a, b)
    rows, st = _expect(GN, both)
    ctx = bench.on(a["first"], a["starts"], a["stops"])
    GN.add(ctx, a["rp"], a["pr"])
    GN.add(ctx, b["rp"], b["pr"])
    _device_equals(GN, ctx, both, rows, st)
    _device_equals(GN, ctx, both, rows, st)                   # take twice: the same rows
    GN.reset(ctx)
    GN.add(ctx, both["rp"], both["pr"])                       # one add of the concatenation
    _device_equals(GN, ctx, both, rows, st)
    GN.reset(ctx)
    GN.add(ctx, b["rp"], b["pr"])                             # the order of the batches does not matter
    GN.add(ctx, a["rp"], a["pr"])
    _device_equals(GN, ctx, both, rows, st)
    half, half_st = _expect(GN, a)
    GN.reset(ctx)
    GN.add(ctx, a["rp"], a["pr"])
    _device_equals(GN, ctx, a, half, half_st)                 # a take ...
    GN.add(ctx, b["rp"], b["pr"])
    _device_equals(GN, ctx, both, rows, st)                   # ... and more batches behind it
    zero = dict.fromkeys(st, 0)
    GN.set_genes(ctx, False)
    assert not GN.get_genes(ctx)
    GN.set_genes(ctx, True)                                   # off and on again starts from zero
    got, got_st = GN.take(ctx)
    assert len(got) == 0 and got_st == zero
    build_ms, count_ms, take_ms = GN.kernel_ms(ctx)
    assert build_ms > 0 and take_ms > 0
    GN.add(ctx, a["rp"], a["pr"])
    assert GN.kernel_ms(ctx)[1] > 0
    # the annotations, then the index, free the state
    ST.set_annotations(ctx, bench.index)
    assert not GN.get_genes(ctx)
    GN.set_genes(ctx, True)
    _set_entries(ctx, 7)
    assert not GN.get_genes(ctx)
    bench.key = bench.n = None                                # (the next case lays everything out again)


def test_refusals(kslam, GN, ST):
    L = GN.lib()
    c = kslam.Context()
    case = R.build("x", [[(0, 100)]], [([(0, 0, 9)], []), ([(0, 1, 2)], [])])
    index = GN.GeneIndex(case["first"], case["starts"], case["stops"])
    args = lambda rp, pr: (rp.ctypes.data, len(rp), pr.ctypes.data, len(pr))   # noqa: E731
    err = lambda: c._L.kslam_last_error(c._h)   # noqa: E731
    rows, n, st = C.c_void_p(), C.c_uint64(), GN.Stats()
    one = np.zeros(1, dtype=np.int64)
    try:
        c.set_pairing(stages=3)
        assert L.kslam_set_genes(c._h, 1) == ERR_STATE and b"kslam_set_index" in err()            # no index
        c.set_pairing(stages=0)
        _set_entries(c, 1)
        assert L.kslam_set_genes(c._h, 1) == ERR_STATE and b"kslam_set_pairing" in err()          # the pairing is off
        c.set_pairing(stages=3)
        assert L.kslam_set_genes(c._h, 1) == ERR_STATE and b"kslam_set_sam_annotations" in err()  # no annotations
        for call in (lambda: L.kslam_genes_reset(c._h), lambda: L.kslam_genes_add(c._h, *args(case["rp"], case["pr"])),
                     lambda: L.kslam_genes_take(c._h, C.byref(rows), C.byref(n), C.byref(st)),
                     lambda: L.kslam_genes_lookup(c._h, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, one.ctypes.data, None, 0)):
            assert call() == ERR_STATE and b"kslam_set_genes" in err()
        broken = GN.GeneIndex([0, 1], [0, 5, 9], [10, 20, 30])              # three genes, gene_first ends at one
        ST.set_annotations(c, broken)
        assert L.kslam_set_genes(c._h, 1) == ERR_ARG and b"gene_first" in err() and not GN.get_genes(c)
        ST.set_annotations(c, index)
        GN.set_genes(c, True)
        GN.set_genes(c, True)                                               # on when already on: nothing happens
        rp = case["rp"].copy()
        rp["count"][1] = 2
        assert L.kslam_genes_add(c._h, *args(rp, case["pr"])) == ERR_ARG and b"outside the pairs array" in err()
        rp = case["rp"].copy()
        rp["first"][1] = 0
        assert L.kslam_genes_add(c._h, *args(rp, case["pr"])) == ERR_ARG and b"ascend" in err()
        assert L.kslam_genes_add(c._h, None, 2, case["pr"].ctypes.data, 2) == ERR_ARG
        assert L.kslam_genes_take(c._h, None, C.byref(n), C.byref(st)) == ERR_ARG
        assert L.kslam_genes_lookup(c._h, None, one.ctypes.data, one.ctypes.data, 1, one.ctypes.data, None, 0) == ERR_ARG
        got, got_st = GN.take(c)
        assert len(got) == 0 and got_st["n_alignments"] == 0                # nothing was counted
        g, s = GN.lookup(c, [], [], [])
        assert len(g) == 0
        fd = C.c_int(5)
        assert L.kslam_stream_set_genes(c._h, 7) == 0 and L.kslam_stream_get_genes(c._h, C.byref(fd)) == 0 and fd.value == 7
        assert L.kslam_stream_set_genes(c._h, -3) == 0 and L.kslam_stream_get_genes(c._h, C.byref(fd)) == 0 and fd.value == -1
        GN.set_genes(c, False)
    finally:
        c.set_pairing(stages=0)
        c.close()
    m = kslam.MultiContext([0])
    try:
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)   # (tests/test_gpu_readsplit.py: the first context)
        assert L.kslam_set_genes(h, 1) == ERR_UNSUPPORTED
        assert L.kslam_stream_set_genes(h, 1) == ERR_UNSUPPORTED
    finally:
        m.close()


# ---- real batches through the lanes: the world of tests/test_gpu_readsplit.py ----

def _stream_table(kslam, GN, world, tmp, tag, lanes, env=None, single=False, genes=True):
    """-> (the gene table, the SAM file, the per-read file, the statistics)"""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    env = dict(env or {}, KSLAM_LANES=str(lanes))
    os.environ.update(env)
    names = [str(tmp / (tag + ext)) for ext in (".genes", ".sam", ".per_read")]
    try:
        c = _indexed_context(kslam, world)
        h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
        tax = X.TaxDB(world["case"]["taxdb"])
        fds = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC) for p in names]
        P = T.TailParams.default(paired=not single)
        st = S.classify_stream_native(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), 300, P, taxdb=tax,
                                      sam_fd=fds[1], per_read_fd=fds[2], sam_header=T.sam_header(world["db"], b"SLAM"), depth=3,
                                      genes_fd=fds[0] if genes else -1)
        assert not GN.get_genes(c)   # the call switched it off again
        for fd in fds:
            os.close(fd)
        c.close()
        h1.close()
        h2.close()
    finally:
        for k in env:
            del os.environ[k]
    return [open(p, "rb").read() for p in names] + [st]


def _twin_table(kslam, GN, world, single=False):
    """the same batches through the Python loop: the final arrays of every batch, concatenated, through the host twin, the
    restatement and the writer"""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    got = []
    try:
        S.classify_stream(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), 300,
                          T.TailParams.default(paired=not single), depth=3,
                          on_batch=lambda rec, ov, cg, rp, pr, reads: got.append((np.array(rp), np.array(pr))))
    finally:
        c.close()
        h1.close()
        h2.close()
    assert len(got) == 3
    rp, at = [], 0
    for r, p in got:
        r = r.astype(R.READ_PAIR_DT)
        r["first"] += at
        at += len(p)
        rp.append(r)
    rp, pr = np.concatenate(rp), np.concatenate([p.astype(R.PAIRED_OVERLAP_DT) for _, p in got])
    db = world["db"]
    rows, st = GN.tail_genes(db, rp, pr)
    v = db.view
    col = lambda p, dt, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), shape=(max(int(n), 1),))[:int(n)].copy()   # noqa: E731
    case = {"first": col(v.gene_first, C.c_uint64, v.n_entries + 1), "starts": col(v.gene_start, C.c_int32, v.n_genes),
            "stops": col(v.gene_stop, C.c_int32, v.n_genes), "rp": rp, "pr": pr}
    ref_rows, ref_st = R.table(case)
    assert rows.tolist() == ref_rows.tolist() and st == ref_st and st["n_skipped"] == 0
    return GN.table_bytes(db, rows), rows, st


def test_three_batches_through_the_stream(kslam, GN, world, tmp_path):
    assert world["db"].view.n_genes > 0
    exp, rows, st = _twin_table(kslam, GN, world)
    assert len(rows) > 0 and st["n_in_gene"] > 0 and exp.startswith(GN.HEADER) and exp.count(b"\n") == 1 + len(rows)
    one, sam, per_read, stats = _stream_table(kslam, GN, world, tmp_path, "l1", 1)
    assert one == exp and stats["batches_pseudo_on_host"] == 0
    assert _stream_table(kslam, GN, world, tmp_path, "l3", 3)[0] == exp
    # pseudo-assembly left to the host for every batch: the rows come in through kslam_genes_add on the host stage's thread
    left, _, _, stats = _stream_table(kslam, GN, world, tmp_path, "cap", 2, env={"KSLAM_PSEUDO_CAP": "3"})
    assert stats["batches_pseudo_on_host"] == 3 and left == exp
    # the switch moves nothing else
    none, sam_off, per_read_off, _ = _stream_table(kslam, GN, world, tmp_path, "off", 1, genes=False)
    assert none == b"" and len(sam) > 1000 and sam == sam_off and per_read == per_read_off
    parsed = GN.parse(one)
    assert [r["gene"] for r in parsed] == rows["gene"].tolist() and all(r["alignments"] >= r["unique_read_pairs"] for r in parsed)


def test_single_end_through_the_stream(kslam, GN, world, tmp_path):
    exp, rows, st = _twin_table(kslam, GN, world, single=True)
    assert rows["alignments"].sum() > 0
    assert _stream_table(kslam, GN, world, tmp_path, "se", 2, single=True)[0] == exp
