"""The coverage table on the GPU (csrc/coverage.hip, include/kslam_coverage.h): the device's rows and every entry's bitmap words
against the host twin (kslam_tail_coverage) AND the plain-Python restatement (tests/coverage_ref.py), exactly -- the bit, entry,
contention, dead-record, mate, unique, skip, long-interval and grid seams, accumulation, the refusals, and real batches through
kslam_stream_classify with one lane, three lanes, the host's SAM text and pseudo-assembly left to the host."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import coverage_ref as R
from test_gpu_readsplit import _host_text, _indexed_context, world  # noqa: F401  (the fixture and its helpers)

pytestmark = pytest.mark.gpu
CASES = R.cases()
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = 1, 4, 5   # include/kslam.h: kslam_status


@pytest.fixture(scope="module")
def CV(kslam):
    return importlib.import_module("kslam_amd.coverage")


class _Bench:
    """one context; the index is rebuilt when a case brings other entry lengths (kslam_set_index drops the table)"""

    def __init__(self, kslam, CV):
        self.c, self.CV, self.lengths = kslam.Context(), CV, None

    def on(self, lengths):
        lengths = [int(x) for x in lengths]
        if lengths != self.lengths:
            rng = np.random.default_rng(len(lengths) + sum(lengths))
            off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
            self.c.set_index_arrays(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(off[-1])), off)
            assert not self.CV.get_coverage(self.c)   # a new index frees the table
            self.lengths = lengths
            self.c.set_pairing(stages=3)
            self.CV.set_coverage(self.c, True)
        else:
            self.CV.reset(self.c)
        return self.c


@pytest.fixture(scope="module")
def bench(kslam, CV):
    b = _Bench(kslam, CV)
    yield b
    b.c.set_pairing(stages=0)
    b.c.close()


def _expect(CV, c):
    rows, skipped, covered = R.table(c["lengths"], c["ov"], c["rp"], c["pr"])
    twin, twin_skipped = CV.tail_coverage(c["lengths"], c["ov"], c["rp"], c["pr"])
    assert twin.tolist() == rows.tolist() and twin_skipped == skipped
    return rows, skipped, covered


def _device_equals(CV, ctx, c, rows, skipped, covered):
    got, got_skipped = CV.take(ctx)
    assert got.tolist() == rows.tolist(), c["name"]
    assert got_skipped == skipped, c["name"]
    for e, length in enumerate(c["lengths"]):
        assert CV.bitmap(ctx, e, length).tolist() == R.words(covered[e]).tolist(), (c["name"], e)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_rows_and_bitmaps_equal_twin_and_restatement(CV, bench, case):
    ctx = bench.on(case["lengths"])
    rows, skipped, covered = _expect(CV, case)
    CV.add(ctx, case["ov"], case["rp"], case["pr"])
    _device_equals(CV, ctx, case, rows, skipped, covered)


def test_accumulation_reset_and_switch(CV, bench):
    a = R.random_case("a", 71, 3000, 7, 900)
    b = R.random_case("b", 72, 2500, 7, 900, lengths=a["lengths"])
    both = R.concat(a, b)
    rows, skipped, covered = _expect(CV, both)
    ctx = bench.on(a["lengths"])
    CV.add(ctx, a["ov"], a["rp"], a["pr"])
    CV.add(ctx, b["ov"], b["rp"], b["pr"])
    _device_equals(CV, ctx, both, rows, skipped, covered)
    again, again_skipped = CV.take(ctx)                       # take recounts from the bitmap: twice the same
    assert again.tolist() == rows.tolist() and again_skipped == skipped
    CV.reset(ctx)
    CV.add(ctx, both["ov"], both["rp"], both["pr"])           # one add of the concatenation
    _device_equals(CV, ctx, both, rows, skipped, covered)
    CV.add(ctx, b["ov"], b["rp"], b["pr"])                    # the order of the batches does not matter
    CV.reset(ctx)
    CV.add(ctx, b["ov"], b["rp"], b["pr"])
    CV.add(ctx, a["ov"], a["rp"], a["pr"])
    _device_equals(CV, ctx, both, rows, skipped, covered)
    zero = R.arrays("zero", a["lengths"], [], [], [])
    CV.reset(ctx)
    _device_equals(CV, ctx, zero, *R.table(a["lengths"], zero["ov"], zero["rp"], zero["pr"]))
    CV.add(ctx, a["ov"], a["rp"], a["pr"])
    CV.set_coverage(ctx, False)
    assert not CV.get_coverage(ctx)
    CV.set_coverage(ctx, True)                                # off and on again starts from zero
    _device_equals(CV, ctx, zero, *R.table(a["lengths"], zero["ov"], zero["rp"], zero["pr"]))
    assert CV.kernel_ms(ctx)[1] > 0


def test_refusals(kslam, CV):
    L = CV.lib()
    c = kslam.Context()
    case = R.build("x", [100], [([(0, (0, 0, 9), (0, 5, 20))], []), ([(0, (0, 1, 2), None)], [])])
    args = lambda ov, rp, pr: (ov.ctypes.data, len(ov), rp.ctypes.data, len(rp), pr.ctypes.data, len(pr))   # noqa: E731
    try:
        c.set_pairing(stages=3)
        assert L.kslam_set_coverage(c._h, 1) == ERR_STATE                 # no index
        assert b"kslam_set_index" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=0)
        c.set_index_arrays(np.frombuffer(b"ACGT" * 25, dtype=np.uint8), np.array([0, 100], dtype=np.uint64))
        assert L.kslam_set_coverage(c._h, 1) == ERR_STATE                 # the pairing is off
        assert b"kslam_set_pairing" in c._L.kslam_last_error(c._h)
        for call in (lambda: L.kslam_coverage_reset(c._h), lambda: L.kslam_coverage_add(c._h, *args(case["ov"], case["rp"], case["pr"]))):
            assert call() == ERR_STATE and b"kslam_set_coverage" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=3)
        CV.set_coverage(c, True)
        rows0 = CV.take(c)
        bad = case["pr"].copy()
        bad["r1"][1] = len(case["ov"])
        assert L.kslam_coverage_add(c._h, *args(case["ov"], case["rp"], bad)) == ERR_ARG
        assert b"refers to overlap record" in c._L.kslam_last_error(c._h)
        rp = case["rp"].copy()
        rp["count"][1] = 2
        assert L.kslam_coverage_add(c._h, *args(case["ov"], rp, case["pr"])) == ERR_ARG
        assert b"outside the pairs array" in c._L.kslam_last_error(c._h)
        words = np.zeros(3, dtype=np.uint64)
        assert L.kslam_coverage_bitmap(c._h, 0, words.ctypes.data, 3) == ERR_ARG   # the entry has two words
        assert L.kslam_coverage_bitmap(c._h, 1, words.ctypes.data, 2) == ERR_ARG   # no such entry
        got = CV.take(c)
        assert got[0].tolist() == rows0[0].tolist() == [(0, 0, 0, 0)] and got[1] == 0   # nothing was marked
        CV.set_coverage(c, False)
    finally:
        c.set_pairing(stages=0)
        c.close()
    m = kslam.MultiContext([0])
    try:
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)   # (tests/test_gpu_readsplit.py: the first context)
        assert L.kslam_set_coverage(h, 1) == ERR_UNSUPPORTED
        assert L.kslam_stream_set_coverage(h, 1) == ERR_UNSUPPORTED
    finally:
        m.close()


# ---- real batches through the lanes: the world of tests/test_gpu_readsplit.py ----

def _stream_report(kslam, CV, world, tmp, tag, lanes, env=None, single=False):
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
        name = str(tmp / (tag + ".cov"))
        fd = os.open(name, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        pr_fd = os.open(str(tmp / (tag + ".per_read")), os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        P = T.TailParams.default(paired=not single)
        st = S.classify_stream_native(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), 300, P, taxdb=tax,
                                      per_read_fd=pr_fd, depth=3, coverage_fd=fd)
        assert not CV.get_coverage(c)   # the call switched it off again
        os.close(fd)
        os.close(pr_fd)
        c.close()
        h1.close()
        h2.close()
    finally:
        for k in env:
            del os.environ[k]
    return open(name, "rb").read(), st


def _twin_report(kslam, CV, world, single=False):
    """the same batches through the Python loop, which leaves the SAM text to the host: the final arrays of every batch,
    concatenated, through the host twin and the report writer"""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    got = []
    try:
        S.classify_stream(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), 300,
                          T.TailParams.default(paired=not single), depth=3,
                          on_batch=lambda rec, ov, cg, rp, pr, reads: got.append((np.array(ov), np.array(rp), np.array(pr))))
    finally:
        c.close()
        h1.close()
        h2.close()
    assert len(got) == 3
    lengths = [len(e["bases"]) for e in world["case"]["entries"]]
    whole = None
    for ov, rp, pr in got:
        part = {"name": "batch", "lengths": np.asarray(lengths, dtype=np.uint64), "ov": ov.astype(R.OVERLAP_DT), "rp": rp.astype(R.READ_PAIR_DT),
                "pr": pr.astype(R.PAIRED_OVERLAP_DT)}
        whole = part if whole is None else R.concat(whole, part)
    rows, skipped = CV.tail_coverage(lengths, whole["ov"], whole["rp"], whole["pr"])
    ref_rows, ref_skipped, _ = R.table(whole["lengths"], whole["ov"], whole["rp"], whole["pr"])
    assert rows.tolist() == ref_rows.tolist() and skipped == ref_skipped == 0
    return CV.report_bytes(world["db"], rows), rows


def test_three_batches_through_the_stream(kslam, synth, CV, world, tmp_path):
    exp, rows = _twin_report(kslam, CV, world)
    report, st = _stream_report(kslam, CV, world, tmp_path, "l1", 1)
    assert report == exp and st["batches_pseudo_on_host"] == 0
    assert _stream_report(kslam, CV, world, tmp_path, "l3", 3)[0] == exp
    assert _stream_report(kslam, CV, world, tmp_path, "host", 2, env={"KSLAM_HOST_SAM_TEXT": "1"})[0] == exp
    # pseudo-assembly left to the host for every batch: the rows come in through kslam_coverage_add on the host stage's thread
    left, st = _stream_report(kslam, CV, world, tmp_path, "cap", 2, env={"KSLAM_PSEUDO_CAP": "3"})
    assert st["batches_pseudo_on_host"] == 3 and left == exp
    # the entries the fixture planted reads on, and no others, are covered
    case, n = world["case"], world["n"]
    genomes = synth.make_genomes(7311 % 1000, 3, 3, 14000, strain_sub=0.02, strain_indel=0.001, shared_segment=1800)
    _, truth = synth.make_paired_reads(7311 % 1000 + 1, genomes, n, read_len=110, frag_mean=300, frag_sd=45, sub_rate=0.015, indel_rate=0.003,
                                       n_rate=0.001, edge_frac=0.05, unmapped_frac=0.05)
    assert [bytes(g) for g in synth.to_bytes(genomes)] == [bytes(e["bases"]) for e in case["entries"]]
    planted = sorted({t[0] for i, t in enumerate(truth) if i % 2 == 0 and t[0] >= 0})
    parsed = CV.parse_report(report)
    assert planted == [r["entry"] for r in parsed if r["covered_bases"] > 0] == [e for e in range(len(rows)) if rows[e]["covered_bases"]]
    assert all(0 < r["breadth"] <= 1 and r["aligned_bases"] >= r["covered_bases"] and r["alignments"] >= r["unique_read_pairs"] for r in parsed)


def test_single_end_through_the_stream(kslam, CV, world, tmp_path):
    exp, rows = _twin_report(kslam, CV, world, single=True)
    assert rows["alignments"].sum() > 0
    assert _stream_report(kslam, CV, world, tmp_path, "se", 2, single=True)[0] == exp
