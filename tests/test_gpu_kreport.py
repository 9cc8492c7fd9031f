"""The Kraken-style report's counts on the GPU (csrc/kreport.hip, include/kslam_kreport.h): the device's rows and statistics
against the host twin (kslam_tail_kreport) AND the plain-Python restatement (tests/kreport_ref.py), exactly -- the wave, block and
grid seams, the wave combining, both ends of the binary search, unknown ids, deep chains, phantom and repeated nodes,
accumulation, the refusals, and real batches through kslam_stream_classify with one lane, three lanes, the host's text and
pseudo-assembly left to the host."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import kreport_ref as R
from test_gpu_readsplit import _host_text, _indexed_context, world  # noqa: F401  (the fixture and its helpers)

pytestmark = pytest.mark.gpu
CASES = R.cases()
ERR_UNSUPPORTED, ERR_STATE = 4, 5   # include/kslam.h: kslam_status


@pytest.fixture(scope="module")
def KR(kslam):
    return importlib.import_module("kslam_amd.kreport")


class _Bench:
    """one context over a one-entry index; the annotations are set again when a case brings another tree (which drops the state)"""

    def __init__(self, kslam, KR):
        self.KR, self.tax_text, self.tax = KR, None, None
        self.ST = importlib.import_module("kslam_amd.samtext")
        self.T = importlib.import_module("kslam_amd.tail")
        self.X = importlib.import_module("kslam_amd.taxonomy")
        self.c = kslam.Context()
        bases, off = np.frombuffer(b"ACGT" * 25, dtype=np.uint8), np.array([0, 100], dtype=np.uint64)
        self.c.set_index_arrays(bases, off)
        self.index = self.T.IndexArrays(bases, off, taxonomy_ids=[10])

    def on(self, tax_text):
        if tax_text != self.tax_text:
            self.tax = self.X.TaxDB(tax_text)
            self.ST.set_annotations(self.c, self.index, self.tax)
            assert not self.KR.get_kreport(self.c)   # new annotations free the state
            self.tax_text = tax_text
            self.KR.set_kreport(self.c, True)
        else:
            self.KR.reset(self.c)
        return self.c, self.tax


@pytest.fixture(scope="module")
def bench(kslam, KR):
    b = _Bench(kslam, KR)
    yield b
    b.c.close()


def _expect(KR, tax, tax_text, ids):
    rows, stats = R.rows(tax_text, ids)
    twin, twin_stats = KR.tail_kreport(tax, ids)
    assert twin.tolist() == rows.tolist() and twin_stats == stats
    return rows, stats


def _device_equals(KR, ctx, rows, stats, name=""):
    got, got_stats = KR.take(ctx)
    assert got.tolist() == rows.tolist(), name
    assert got_stats == stats, name


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_rows_equal_twin_and_restatement(KR, bench, case):
    ctx, tax = bench.on(case["tax"])
    rows, stats = _expect(KR, tax, case["tax"], case["ids"])
    KR.add(ctx, case["ids"])
    _device_equals(KR, ctx, rows, stats, case["name"])
    assert KR.report_bytes(tax, KR.take(ctx)[0], len(case["ids"])) == R.text(case["tax"], case["ids"], len(case["ids"]))


def test_accumulation_reset_and_switch(KR, bench):
    tax_text = R.tax_text(R.FIVE)
    rng = np.random.default_rng(31)
    pool = np.array([10, 20, 30, 40, 50, 0, 7, 0xFFFFFFFF], dtype=np.uint32)
    a, b = rng.choice(pool, 700), rng.choice(pool, 333)
    both = np.concatenate([a, b])
    ctx, tax = bench.on(tax_text)
    rows, stats = _expect(KR, tax, tax_text, both)
    KR.add(ctx, a)
    rows_a, stats_a = _expect(KR, tax, tax_text, a)
    _device_equals(KR, ctx, rows_a, stats_a)                  # take, and more batches follow it
    KR.add(ctx, b)
    _device_equals(KR, ctx, rows, stats)
    _device_equals(KR, ctx, rows, stats)                      # take twice gives the same
    KR.reset(ctx)
    KR.add(ctx, both)                                         # one add of the concatenation
    _device_equals(KR, ctx, rows, stats)
    KR.reset(ctx)
    KR.add(ctx, b)                                            # the order of the batches does not matter
    KR.add(ctx, a)
    _device_equals(KR, ctx, rows, stats)
    zero = R.rows(tax_text, [])
    KR.reset(ctx)
    _device_equals(KR, ctx, *zero)
    KR.add(ctx, a)
    KR.set_kreport(ctx, False)
    assert not KR.get_kreport(ctx)
    KR.set_kreport(ctx, True)                                 # off and on again starts from zero
    _device_equals(KR, ctx, *zero)
    KR.add(ctx, a)
    add_ms, take_ms = KR.kernel_ms(ctx)
    assert add_ms > 0 and take_ms > 0
    bench.ST.set_annotations(ctx, bench.index, tax)           # new annotations drop the state, even with the same tree
    assert not KR.get_kreport(ctx)
    bench.tax_text = None


def test_refusals(kslam, KR):
    L = KR.lib()
    ST = importlib.import_module("kslam_amd.samtext")
    T = importlib.import_module("kslam_amd.tail")
    c = kslam.Context()
    ids = np.array([10, 20], dtype=np.uint32)
    rows, n, st = C.c_void_p(), C.c_uint64(), KR.Stats()
    try:
        assert L.kslam_set_kreport(c._h, 1) == ERR_STATE                      # no annotations at all
        assert b"kslam_set_sam_annotations" in c._L.kslam_last_error(c._h)
        bases, off = np.frombuffer(b"ACGT" * 25, dtype=np.uint8), np.array([0, 100], dtype=np.uint64)
        c.set_index_arrays(bases, off)
        index = T.IndexArrays(bases, off, taxonomy_ids=[10])
        ST.set_annotations(c, index, None)
        assert L.kslam_set_kreport(c._h, 1) == ERR_STATE                      # annotations without a tree
        assert b"taxonomy tree" in c._L.kslam_last_error(c._h)
        for call in (lambda: L.kslam_kreport_reset(c._h), lambda: L.kslam_kreport_add(c._h, ids.ctypes.data, len(ids)),
                     lambda: L.kslam_kreport_take(c._h, C.byref(rows), C.byref(n), C.byref(st))):
            assert call() == ERR_STATE and b"kslam_set_kreport" in c._L.kslam_last_error(c._h)   # the switch is off
        assert not KR.get_kreport(c)
    finally:
        c.close()
    m = kslam.MultiContext([0])
    try:
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)   # (tests/test_gpu_readsplit.py: the first context)
        assert L.kslam_set_kreport(h, 1) == ERR_UNSUPPORTED
        assert L.kslam_stream_set_kreport(h, 1) == ERR_UNSUPPORTED
    finally:
        m.close()


# ---- real batches through the lanes: the world of tests/test_gpu_readsplit.py ----

def _stream(kslam, KR, world, tmp, tag, lanes, env=None, report=True):
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    env = dict(env or {}, KSLAM_LANES=str(lanes))
    os.environ.update(env)
    names = {k: str(tmp / (tag + "." + k)) for k in ("kreport", "sam", "per_read")}
    try:
        c = _indexed_context(kslam, world)
        h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
        tax = X.TaxDB(world["case"]["taxdb"])
        fds = {k: os.open(p, os.O_RDWR | os.O_CREAT | os.O_TRUNC) for k, p in names.items()}
        st = S.classify_stream_native(c, world["db"], h1.ptr, len(r1), h2.ptr, len(r2), 300, T.TailParams.default(paired=True), taxdb=tax,
                                      sam_fd=fds["sam"], per_read_fd=fds["per_read"], sam_header=b"@HD\tVN:1.0\n", depth=3,
                                      kreport_fd=fds["kreport"] if report else -1)
        assert not KR.get_kreport(c)   # the call switched it off again
        for fd in fds.values():
            os.close(fd)
        c.close()
        h1.close()
        h2.close()
        st["abbreviated"] = tax.summary(st["tax_ids"], st["n_pairs"])
    finally:
        for k in env:
            del os.environ[k]
    return {k: open(p, "rb").read() for k, p in names.items()}, st


def test_three_batches_through_the_stream(kslam, KR, world, tmp_path):
    tax_text = world["case"]["taxdb"]
    files, st = _stream(kslam, KR, world, tmp_path, "l1", 1)
    ids = st["tax_ids"]
    assert st["n_batches"] == 3 and st["batches_pseudo_on_host"] == 0 and st["n_pairs"] == world["n"] and np.count_nonzero(ids) > 100
    exp = R.text(tax_text, ids, st["n_pairs"])
    assert files["kreport"] == exp
    lines = KR.parse_report(files["kreport"])
    got = sorted((x["taxid"], x["direct"]) for x in lines if x["direct"] and x["code"] != "U")
    values, counts = np.unique(ids[ids != 0], return_counts=True)
    assert got == sorted(zip(values.tolist(), counts.tolist()))
    assert lines[0]["code"] == "U" and lines[0]["clade"] == st["n_pairs"] - np.count_nonzero(ids)
    # the switch off: no report, and the SAM, _PerRead and _abbreviated bytes are those of the run with it on
    off, st_off = _stream(kslam, KR, world, tmp_path, "off", 1, report=False)
    assert off["kreport"] == b"" and off["sam"] == files["sam"] and off["per_read"] == files["per_read"] and len(files["sam"]) > 1000
    assert st_off["abbreviated"] == st["abbreviated"] and st_off["tax_ids"].tolist() == ids.tolist()
    # three lanes count into one state
    assert _stream(kslam, KR, world, tmp_path, "l3", 3)[0]["kreport"] == exp
    # every batch formatted and classified on the host: all ids come in through kslam_kreport_add
    assert _stream(kslam, KR, world, tmp_path, "host", 2, env={"KSLAM_HOST_SAM_TEXT": "1"})[0]["kreport"] == exp
    # pseudo-assembly left to the host for every batch: no lane made the ids
    left, st_left = _stream(kslam, KR, world, tmp_path, "cap", 2, env={"KSLAM_PSEUDO_CAP": "3"})
    assert st_left["batches_pseudo_on_host"] == 3 and left["kreport"] == exp


def test_the_stream_needs_a_tree(kslam, KR, world, tmp_path):
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    fd = os.open(str(tmp_path / "none.kreport"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    try:
        with pytest.raises(kslam.KslamError) as e:
            S.classify_stream_native(c, world["db"], h1.ptr, len(r1), h2.ptr, len(r2), 300, T.TailParams.default(paired=True), kreport_fd=fd)
        assert e.value.status == ERR_STATE
        assert os.fstat(fd).st_size == 0
    finally:
        os.close(fd)
        c.close()
        h1.close()
        h2.close()
