"""The read QC report's tables on the GPU (csrc/readqc.hip, include/kslam_readqc.h): kslam_read_qc_add + take against the host
twin (kslam_tail_read_qc; tests/test_readqc_host.py holds the twin to the plain-Python restatement on the same cases), field for
field -- the wave, tile and workgroup seams, the pooled row, one very long read, every byte value, counters past 16 bits, both
stream layouts -- accumulation, reset, the switch, the refusals, and real batches through kslam_stream_classify with one lane and
three, from LF, CRLF and BGZF input, paired and single-end."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import readqc_ref as R
from test_cli import _fixture_case
from test_gpu_readsplit import _host_text

pytestmark = pytest.mark.gpu
CASES = R.cases()
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = 1, 4, 5   # include/kslam.h: kslam_status


@pytest.fixture(scope="module")
def RQ(kslam):
    return importlib.import_module("kslam_amd.readqc")


@pytest.fixture(scope="module")
def ctx(kslam):
    c = kslam.Context()   # no index, no pairing: the report needs neither
    yield c
    c.close()


def _on(RQ, ctx, cycles):
    """the switch on with `cycles` rows and zeroed tables"""
    on, now = RQ.get_read_qc(ctx)
    want = cycles or RQ.DEFAULT_CYCLES
    if on and now != want:
        RQ.set_read_qc(ctx, False)
        on = False
    if on:
        RQ.reset(ctx)
    else:
        RQ.set_read_qc(ctx, True, cycles)
    assert RQ.get_read_qc(ctx) == (True, want)


def _same(got, exp, name=""):
    assert got["max_cycles"] == exp["max_cycles"] and got["paired"] == exp["paired"], name
    for z in range(2):
        for key, want in exp["streams"][z].items():
            assert got["streams"][z][key] == want, (name, z, key)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_tables_equal_the_twin(RQ, ctx, case):
    exp = RQ.tail_read_qc(case["bases"], case["quality"], case["paired"], case["cycles"])
    _on(RQ, ctx, case["cycles"])
    RQ.add(ctx, case["bases"], case["quality"], case["paired"])
    got = RQ.take(ctx)
    _same(got, exp, case["name"])
    assert RQ.report_bytes(got) == RQ.report_bytes(exp)


def test_the_cases_cover_the_kernels_workgroup(RQ):
    """the case set is built around the kernel's reads per workgroup (common.h: RQ_READS)"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "k-slam_amd", "csrc", "common.h")).read()
    assert "constexpr uint64_t RQ_READS = 256;" in src
    assert {"reads_255", "reads_256", "reads_257"} <= {c["name"] for c in CASES}


def test_accumulation_reset_and_switch(RQ, ctx):
    a_b, a_q = R._reads([5, 64, 65, 130, 0, 7], 41)
    b_b, b_q = R._reads([300, 1, 64, 9], 42)
    _on(RQ, ctx, 100)
    both = RQ.tail_read_qc(a_b + b_b, a_q + b_q, False, 100)
    only_a = RQ.tail_read_qc(a_b, a_q, False, 100)
    RQ.add(ctx, a_b, a_q)
    _same(RQ.take(ctx), only_a)                    # take, and more batches follow it
    RQ.add(ctx, b_b, b_q)
    _same(RQ.take(ctx), both)                      # two adds equal one add of the concatenation
    _same(RQ.take(ctx), both)                      # take twice gives the same
    RQ.reset(ctx)
    RQ.add(ctx, b_b, b_q)                          # the order of the batches does not matter
    RQ.add(ctx, a_b, a_q)
    _same(RQ.take(ctx), both)
    zero = RQ.tail_read_qc([], [], False, 100)
    RQ.reset(ctx)
    _same(RQ.take(ctx), zero)                      # reset zeroes the tables, the minimum included
    # a paired add makes the tables paired until the next reset; the streams add up separately
    RQ.add(ctx, a_b, a_q, paired=True)
    RQ.add(ctx, a_b, a_q, paired=True)
    twice = RQ.tail_read_qc(a_b[:3] * 2 + a_b[3:] * 2, a_q[:3] * 2 + a_q[3:] * 2, True, 100)
    _same(RQ.take(ctx), twice)
    ms, nbytes = RQ.kernel_ms(ctx)
    assert ms > 0 and nbytes == 2 * sum(len(x) for x in a_b)
    # off, and on with another C
    L = RQ.lib()
    assert L.kslam_set_read_qc(ctx._h, 1, 7) == ERR_STATE and b"switch it off" in ctx._L.kslam_last_error(ctx._h)
    RQ.set_read_qc(ctx, True, 100)                 # the same C again: nothing happens, the counts stay
    _same(RQ.take(ctx), twice)
    RQ.set_read_qc(ctx, False)
    assert RQ.get_read_qc(ctx) == (False, 0)
    RQ.set_read_qc(ctx, True, 7)
    assert RQ.get_read_qc(ctx) == (True, 7)
    _same(RQ.take(ctx), RQ.tail_read_qc([], [], False, 7))
    RQ.add(ctx, a_b, a_q)
    _same(RQ.take(ctx), RQ.tail_read_qc(a_b, a_q, False, 7))
    RQ.set_read_qc(ctx, False)


def test_refusals(kslam, RQ):
    L = RQ.lib()
    c = kslam.Context()
    bases, quality = np.frombuffer(b"ACGTAC", dtype=np.uint8), np.frombuffer(b"IIIIII", dtype=np.uint8)
    good, t = np.array([0, 3, 6], dtype=np.uint64), RQ.Tables()
    add = lambda off, n, paired: L.kslam_read_qc_add(c._h, bases.ctypes.data, off.ctypes.data, quality.ctypes.data, n, paired)   # noqa: E731
    try:
        for call in (lambda: L.kslam_read_qc_reset(c._h), lambda: add(good, 2, 0), lambda: L.kslam_read_qc_take(c._h, C.byref(t))):
            assert call() == ERR_STATE and b"kslam_set_read_qc" in c._L.kslam_last_error(c._h)   # the switch is off
        assert L.kslam_set_read_qc(c._h, 1, 65537) == ERR_ARG and RQ.get_read_qc(c) == (False, 0)
        RQ.set_read_qc(c, True, 65536)             # the largest table: 53 MB per stream
        assert RQ.get_read_qc(c) == (True, 65536)
        RQ.set_read_qc(c, False)
        RQ.set_read_qc(c, True)
        assert add(np.array([0, 4, 3], dtype=np.uint64), 2, 0) == ERR_ARG and b"ascend" in c._L.kslam_last_error(c._h)
        assert add(np.array([0, 2, 4, 6], dtype=np.uint64), 3, 1) == ERR_ARG and b"even" in c._L.kslam_last_error(c._h)
        assert L.kslam_read_qc_add(c._h, None, None, None, 1, 0) == ERR_ARG
        assert RQ.take(c)["streams"][0]["n_reads"] == 0   # nothing of that was counted
        assert add(good, 2, 0) == 0 and RQ.take(c)["streams"][0]["n_reads"] == 2
        assert L.kslam_stream_set_read_qc(c._h, 1, 65537) == ERR_ARG
    finally:
        c.close()
    m = kslam.MultiContext([0])
    try:
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)   # (tests/test_gpu_readsplit.py: the first context)
        assert L.kslam_set_read_qc(h, 1, 0) == ERR_UNSUPPORTED
        assert L.kslam_stream_set_read_qc(h, 1, 0) == ERR_UNSUPPORTED
    finally:
        m.close()


# ---- real batches through the lanes: the recorded case of tests/test_cli_kreport.py, 420 pairs in batches of 150 ----

@pytest.fixture(scope="module")
def world(kslam, tmp_path_factory):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    tmp = tmp_path_factory.mktemp("readqc")
    z, case = _fixture_case("a")
    RL.write_case(case, tmp, D)
    db = D.Database.load(os.path.join(str(tmp), "db", "database"))
    r1, r2 = case["r1"], case["r2"]
    return {"case": case, "db": db, "per_batch": int(z["a_per_batch"]), "n": case["n_pairs"],
            "paired": R.text(R.of_fastq(r1, r2)), "single": R.text(R.of_fastq(r1))}


def _stream(kslam, RQ, world, tmp, tag, lanes, r1, r2, qc=True, cycles=0):
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    env = {"KSLAM_LANES": str(lanes)}
    os.environ.update(env)
    names = {k: str(tmp / (tag + "." + k)) for k in ("qc", "sam", "per_read")}
    try:
        c = kslam.Context()
        bases_pp, lens_p = world["db"].entry_pointers()
        c._chk(c._L.kslam_set_index(c._h, world["db"].n_entries, C.cast(bases_pp, C.c_void_p), C.cast(lens_p, C.c_void_p)))
        h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2) if r2 is not None else None
        tax = X.TaxDB(world["case"]["taxdb"])
        fds = {k: os.open(p, os.O_RDWR | os.O_CREAT | os.O_TRUNC) for k, p in names.items()}
        st = S.classify_stream_native(c, world["db"], h1.ptr, len(r1), h2.ptr if h2 else None, len(r2) if h2 else 0, world["per_batch"],
                                      T.TailParams.default(paired=h2 is not None), taxdb=tax, sam_fd=fds["sam"], per_read_fd=fds["per_read"],
                                      sam_header=b"@HD\tVN:1.0\n", depth=3, read_qc_fd=fds["qc"] if qc else -1, read_qc_max_cycles=cycles)
        assert RQ.get_read_qc(c) == (False, 0)   # the call switched it off again
        fd_now, cyc_now = C.c_int(), C.c_uint32()
        assert RQ.lib().kslam_stream_get_read_qc(c._h, C.byref(fd_now), C.byref(cyc_now)) == 0 and fd_now.value == -1   # (and forgot the descriptor)
        for fd in fds.values():
            os.close(fd)
        c.close()
        h1.close()
        if h2:
            h2.close()
    finally:
        for k in env:
            del os.environ[k]
    return {k: open(p, "rb").read() for k, p in names.items()}, st


def test_three_batches_through_the_stream(kslam, RQ, world, tmp_path):
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    files, st = _stream(kslam, RQ, world, tmp_path, "l1", 1, r1, r2)
    assert st["n_batches"] >= 3 and st["n_pairs"] == world["n"]
    assert files["qc"] == world["paired"]
    doc = RQ.parse(files["qc"])
    assert doc["summary"]["total_reads"] == 2 * world["n"] and doc["read1"]["total_reads"] == world["n"] and doc["paired"] is True
    # the switch off: no report, and the SAM and _PerRead bytes are those of the run with it on
    off, st_off = _stream(kslam, RQ, world, tmp_path, "off", 1, r1, r2, qc=False)
    assert off["qc"] == b"" and off["sam"] == files["sam"] and off["per_read"] == files["per_read"] and len(files["sam"]) > 1000
    assert st_off["tax_ids"].tolist() == st["tax_ids"].tolist()
    # three lanes count into one state
    l3, _ = _stream(kslam, RQ, world, tmp_path, "l3", 3, r1, r2)
    assert l3["qc"] == world["paired"] and l3["sam"] == files["sam"] and l3["per_read"] == files["per_read"]


def test_crlf_bgzf_and_single_end_through_the_stream(kslam, RQ, world, tmp_path):
    B = importlib.import_module("kslam_amd.bgzf")
    Z = importlib.import_module("kslam_amd.inflate")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    c1, c2 = r1.replace(b"\n", b"\r\n"), r2.replace(b"\n", b"\r\n")
    assert len(c1) > len(r1)
    assert _stream(kslam, RQ, world, tmp_path, "crlf", 3, c1, c2)[0]["qc"] == world["paired"]
    # BGZF copies: the members are inflated on the device and the text goes the same way
    c = kslam.Context()
    try:
        eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
        z1, z2 = B.compress(c, r1) + eof, B.compress(c, r2) + eof
        assert Z.is_gzip(z1) and len(z1) < len(r1)
        t1, t2 = Z.inflate(c, z1), Z.inflate(c, z2)
    finally:
        c.close()
    assert _stream(kslam, RQ, world, tmp_path, "bgzf", 1, t1, t2)[0]["qc"] == world["paired"]
    files, st = _stream(kslam, RQ, world, tmp_path, "se", 3, r1, None)
    assert st["n_batches"] >= 3 and files["qc"] == world["single"]
    assert b'"read2"' not in world["single"]
