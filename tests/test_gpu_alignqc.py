"""The alignment QC report on the GPU (csrc/alignqc.hip, include/kslam_alignqc.h): the device's tables against the host twin
(kslam_tail_align_qc) AND the plain-Python restatement (tests/alignqc_ref.py), word for word, on every case at both numbers of
cycle rows and with both instantiations of the walk; accumulation, reset and the switch; the refusals; real batches through
kslam_stream_classify with one lane and three, paired and single-end, plain and BGZF input; and planted errors found again through
the aligner."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import alignqc_ref as R
import variants_ref as V
from test_alignqc_host import twin
from test_gpu_readsplit import _host_text, _indexed_context, world  # noqa: F401  (the fixture and its helpers)

pytestmark = pytest.mark.gpu
CASES = R.cases()
BY_NAME = {c["name"]: c for c in CASES}
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = 1, 4, 5   # include/kslam.h: kslam_status


@pytest.fixture(scope="module")
def AQ(kslam):
    return importlib.import_module("kslam_amd.alignqc")


class _Bench:
    """one context; the index is rebuilt when a case brings other entries (kslam_set_index drops the state)"""

    def __init__(self, kslam, AQ):
        self.c, self.AQ, self.entries = kslam.Context(), AQ, None

    def on(self, case, cycles):
        b = case["batches"][0]
        key = (b["gbases"].tobytes(), b["goff"].tobytes())
        if key != self.entries:
            self.keep = np.concatenate([b["gbases"], np.zeros(64, dtype=np.uint8)])
            self.c.set_index_arrays(self.keep, b["goff"])
            assert self.AQ.get_align_qc(self.c) == (False, 0)   # a new index frees the state
            self.entries = key
            self.c.set_pairing(stages=3)
        self.AQ.set_align_qc(self.c, False)
        self.AQ.set_align_qc(self.c, True, cycles)                # off and on: zeroed, with this number of rows
        return self.c


@pytest.fixture(scope="module")
def bench(kslam, AQ):
    b = _Bench(kslam, AQ)
    yield b
    b.c.set_pairing(stages=0)
    b.c.close()


def _add(AQ, ctx, case):
    for b in case["batches"]:
        AQ.add(ctx, b["ov"], b["pool"], b["rbases"], b["roff"], b["rp"], b["pr"], b["rqual"], b["paired"])


def _equal(AQ, got, exp, what):
    assert AQ.pack(got)[0].tolist() == AQ.pack(exp)[0].tolist() and got == exp, what


@pytest.mark.parametrize("C", R.CYCLES)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_tables_equal_twin_and_restatement(AQ, bench, case, C):
    exp = R.tables(case, C)
    _equal(AQ, twin(AQ, case, C), exp, "twin")
    ctx = bench.on(case, C)
    _add(AQ, ctx, case)
    _equal(AQ, AQ.take(ctx), exp, case["name"])


@pytest.mark.parametrize("name,C", [("long-300", 4), ("long-300", 512), ("quality-bytes", 4), ("contributing", 512), ("random-20000", 512)])
def test_thread_per_record_baseline_counts_the_same(AQ, bench, name, C):
    """the instantiation that is kept to be measured against"""
    case = BY_NAME[name]
    ctx = bench.on(case, C)
    os.environ["KSLAM_ALIGNQC_WALK"] = "thread"
    try:
        _add(AQ, ctx, case)
    finally:
        del os.environ["KSLAM_ALIGNQC_WALK"]
    _equal(AQ, AQ.take(ctx), R.tables(case, C), name)


def test_accumulation_reset_and_switch(AQ, bench):
    a = R.random_batch("a", 81, 900, 7)
    ents = [a["gbases"][int(a["goff"][e]):int(a["goff"][e + 1])].tobytes() for e in range(7)]
    rng = np.random.default_rng(5)
    b = V.random_case("b", 82, 3000, 7, entries=ents)          # three times a's records over the same entries
    if (len(b["roff"]) - 1) & 1:
        b["roff"] = np.concatenate([b["roff"], b["roff"][-1:]])
    b["rqual"] = rng.integers(33, 75, len(b["rbases"])).astype(np.uint8)
    b["pr"]["insert_size"] = rng.integers(0, 1100, len(b["pr"]))
    b["paired"] = True
    C_ = 512
    ta, tb = R.batch_tables(a, C_), R.batch_tables(b, C_)
    both = R.add_tables(ta, tb)
    # the twin on the concatenation equals the sum -- but a concatenation changes which reads are stream 1, so the sum is taken per
    # batch here and the concatenation is checked on a single-end copy below
    ctx = bench.on(R.case_of("a", a), C_)
    AQ.add(ctx, a["ov"], a["pool"], a["rbases"], a["roff"], a["rp"], a["pr"], a["rqual"], True)
    _equal(AQ, AQ.take(ctx), ta, "a")
    AQ.add(ctx, b["ov"], b["pool"], b["rbases"], b["roff"], b["rp"], b["pr"], b["rqual"], True)     # an add after a take
    _equal(AQ, AQ.take(ctx), both, "a + b")
    _equal(AQ, AQ.take(ctx), both, "take twice")
    AQ.reset(ctx)
    _equal(AQ, AQ.take(ctx), R.empty(C_), "reset")
    AQ.add(ctx, b["ov"], b["pool"], b["rbases"], b["roff"], b["rp"], b["pr"], b["rqual"], True)     # the order does not matter
    AQ.add(ctx, a["ov"], a["pool"], a["rbases"], a["roff"], a["rp"], a["pr"], a["rqual"], True)
    _equal(AQ, AQ.take(ctx), both, "b + a")
    assert AQ.kernel_ms(ctx) > 0
    # two single-end adds equal the twin on the concatenation
    AQ.reset(ctx)
    sa, sb = dict(a, paired=False), dict(b, paired=False)
    for s in (sa, sb):
        s.pop("_aq", None)
        AQ.add(ctx, s["ov"], s["pool"], s["rbases"], s["roff"], s["rp"], s["pr"], s["rqual"], False)
    whole = V.concat(sa, sb)
    whole.update(rqual=np.concatenate([sa["rqual"], sb["rqual"]]), paired=False)
    exp = twin(AQ, R.case_of("whole", whole), C_)
    _equal(AQ, exp, R.batch_tables(whole, C_), "twin on the concatenation")
    _equal(AQ, AQ.take(ctx), exp, "two adds")
    # another C while on; off then on zeroes
    assert AQ.lib().kslam_set_align_qc(ctx._h, 1, 4) == ERR_STATE and b"switch it off" in ctx._L.kslam_last_error(ctx._h)
    AQ.set_align_qc(ctx, True, C_)                              # the same C: nothing happens
    _equal(AQ, AQ.take(ctx), exp, "on again")
    assert AQ.get_align_qc(ctx) == (True, 512)
    AQ.set_align_qc(ctx, False)
    assert AQ.get_align_qc(ctx) == (False, 0)
    AQ.set_align_qc(ctx, True, 0)                               # 0 means 512
    _equal(AQ, AQ.take(ctx), R.empty(512), "off and on")


def test_refusals(kslam, AQ):
    L = AQ.lib()
    Vm = importlib.import_module("kslam_amd.variants")
    case = R.header_example()["batches"][0]
    keep = np.concatenate([case["gbases"], np.zeros(64, dtype=np.uint8)])

    def args(paired=0, **kw):
        a = {k: kw.get(k, case[k]) for k in ("ov", "pool", "rbases", "roff", "rp", "pr")}
        hold, out = Vm._arrays(a["ov"], a["pool"], a["rbases"], a["roff"], a["rp"], a["pr"])
        args.hold = hold
        return out + (case["rqual"].ctypes.data, paired)

    c = kslam.Context()
    try:
        c.set_pairing(stages=3)
        assert L.kslam_set_align_qc(c._h, 1, 0) == ERR_STATE and b"kslam_set_index" in c._L.kslam_last_error(c._h)      # no index
        c.set_pairing(stages=0)
        c.set_index_arrays(keep, case["goff"])
        assert L.kslam_set_align_qc(c._h, 1, 0) == ERR_STATE and b"kslam_set_pairing" in c._L.kslam_last_error(c._h)    # the pairing is off
        t = AQ.Tables()
        for call in (lambda: L.kslam_align_qc_reset(c._h), lambda: L.kslam_align_qc_add(c._h, *args()), lambda: L.kslam_align_qc_take(c._h, C.byref(t))):
            assert call() == ERR_STATE and b"kslam_set_align_qc" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=3)
        assert L.kslam_set_align_qc(c._h, 1, 65537) == ERR_ARG and AQ.get_align_qc(c) == (False, 0)
        AQ.set_align_qc(c, True, 4)
        two = np.concatenate([case["rp"], case["rp"]])
        for kw, message in (({"pr": ("r1", 0, len(case["ov"]))}, b"refers to overlap record"), ({"rp": ("count", 0, 2)}, b"outside the pairs array"),
                            ({"ov": ("cigar_off", 1, len(case["pool"]))}, b"outside the pool"), ({"ov": ("read", 0, len(case["roff"]) - 1)}, b"refers to read"),
                            ({"rp": two}, b"ascend"), ({"roff": np.array([0, 6, 5], dtype=np.uint64)}, b"offsets must ascend"),
                            ({"roff": np.array([0, 6, 10, 10], dtype=np.uint64), "paired": 1}, b"even number")):
            bad = {}
            for field, change in kw.items():
                if isinstance(change, tuple):
                    bad[field] = case[field].copy()
                    bad[field][change[0]][change[1]] = change[2]
                else:
                    bad[field] = change
            assert L.kslam_align_qc_add(c._h, *args(**bad)) == ERR_ARG and message in c._L.kslam_last_error(c._h), message
        assert AQ.take(c) == R.empty(4)                                     # nothing was added
        AQ.add(c, case["ov"], case["pool"], case["rbases"], case["roff"], case["rp"], case["pr"], case["rqual"], False)
        assert AQ.take(c) == R.tables(R.header_example(), 4)
        AQ.set_align_qc(c, False)
    finally:
        c.set_pairing(stages=0)
        c.close()
    c = kslam.Context(report_cigar=False)
    try:
        c.set_index_arrays(keep, case["goff"])
        c.set_pairing(stages=3)
        assert L.kslam_set_align_qc(c._h, 1, 0) == ERR_STATE and b"report_cigar" in c._L.kslam_last_error(c._h)
    finally:
        c.set_pairing(stages=0)
        c.close()
    m = kslam.MultiContext([0])
    try:
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)   # (tests/test_gpu_readsplit.py: the first context)
        assert L.kslam_set_align_qc(h, 1, 0) == ERR_UNSUPPORTED
        assert L.kslam_stream_set_align_qc(h, 1, 0) == ERR_UNSUPPORTED
    finally:
        m.close()


# ---- real batches through the lanes: the world of tests/test_gpu_readsplit.py ----

def _fastq_column(text, k):
    return [line.rstrip(b"\r") for line in text.split(b"\n")[k::4]]


def _stream_files(kslam, AQ, world, tmp, tag, lanes, single=False, align_qc=True, bgzf=False, cycles=0, env=None):
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    B = importlib.import_module("kslam_amd.bgzf")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    env = dict(env or {}, KSLAM_LANES=str(lanes))
    os.environ.update(env)
    try:
        c = _indexed_context(kslam, world)
        if bgzf:      # BGZF copies: the members are inflated on the device and the text goes the same way
            Z = importlib.import_module("kslam_amd.inflate")
            eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
            z1, z2 = B.compress(c, r1) + eof, B.compress(c, r2) + eof
            assert Z.is_gzip(z1) and len(z1) < len(r1)
            r1, r2 = Z.inflate(c, z1), Z.inflate(c, z2)
        h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
        tax = X.TaxDB(world["case"]["taxdb"])
        names = {k: str(tmp / (tag + "." + k)) for k in ("json", "per_read", "sam")}
        fds = {k: os.open(p, os.O_RDWR | os.O_CREAT | os.O_TRUNC) for k, p in names.items()}
        P = T.TailParams.default(paired=not single)
        st = S.classify_stream_native(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), 300, P, taxdb=tax,
                                      sam_fd=fds["sam"], per_read_fd=fds["per_read"], depth=3, align_qc_fd=fds["json"] if align_qc else -1,
                                      align_qc_max_cycles=cycles)
        assert AQ.get_align_qc(c) == (False, 0)   # the call switched it off again
        for fd in fds.values():
            os.close(fd)
        c.close()
        h1.close()
        h2.close()
    finally:
        for k in env:
            del os.environ[k]
    return {k: open(p, "rb").read() for k, p in names.items()}, st


def _twin_file(kslam, AQ, world, single=False, cycles=512):
    """the same batches through the Python loop, which leaves the SAM text to the host: the final arrays of every batch with its
    CIGAR pool, its reads and their quality column, through the restatement batch by batch and through the host twin"""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    b1, b2, q1, q2 = _fastq_column(r1, 1), _fastq_column(r2, 1), _fastq_column(r1, 3), _fastq_column(r2, 3)
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    got = []
    try:
        S.classify_stream(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), 300,
                          T.TailParams.default(paired=not single), depth=3,
                          on_batch=lambda rec, ov, cg, rp, pr, reads: got.append((np.array(ov), np.array(cg), np.array(rp), np.array(pr), np.array(reads.bases_off))))
    finally:
        c.close()
        h1.close()
        h2.close()
    assert len(got) == 3
    ents = [bytes(e["bases"]) for e in world["case"]["entries"]]
    gbases = np.frombuffer(b"".join(ents), dtype=np.uint8)
    goff = np.concatenate([[0], np.cumsum([len(e) for e in ents])]).astype(np.uint64)
    parts = []
    for k, (ov, cg, rp, pr, bases_off) in enumerate(got):
        sl = slice(300 * k, 300 * k + 300)
        reads, quals = b1[sl] + ([] if single else b2[sl]), q1[sl] + ([] if single else q2[sl])   # a batch is [R1 block | R2 block]
        roff = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
        assert roff.tolist() == (bases_off - bases_off[0]).tolist()
        parts.append({"name": "batch", "gbases": gbases, "goff": goff, "rbases": np.frombuffer(b"".join(reads), dtype=np.uint8), "roff": roff,
                      "rqual": np.frombuffer(b"".join(quals), dtype=np.uint8), "paired": not single, "pool": cg.astype(np.uint32),
                      "ov": ov.astype(R.OVERLAP_DT), "rp": rp.astype(R.READ_PAIR_DT), "pr": pr.astype(R.PAIRED_OVERLAP_DT)})
    case = R.case_of("stream-%s-%d" % ("se" if single else "pe", cycles), *parts)
    exp = R.tables(case, cycles)
    _equal(AQ, twin(AQ, case, cycles), exp, "twin")
    exp = dict(exp, paired=not single)
    n = exp["streams"][0]["n_records"] + exp["streams"][1]["n_records"]
    assert n > 500 and exp["streams"][0]["n_skipped"] + exp["streams"][1]["n_skipped"] == 0 and exp["streams"][0]["mismatches"] > 100
    return R.text(exp), exp


def test_three_batches_through_the_stream(kslam, AQ, world, tmp_path):
    want, exp = _twin_file(kslam, AQ, world)
    assert exp["pairs_both"] > 100 and exp["streams"][1]["n_records"] > 100
    plain, _ = _stream_files(kslam, AQ, world, tmp_path, "plain", 1, align_qc=False)
    assert plain["json"] == b""
    files, st = _stream_files(kslam, AQ, world, tmp_path, "l1", 1)
    assert files["json"] == want
    assert files["sam"] == plain["sam"] and files["per_read"] == plain["per_read"] and len(plain["sam"]) > 10000   # nothing else moves
    assert _stream_files(kslam, AQ, world, tmp_path, "l3", 3)[0]["json"] == want
    assert _stream_files(kslam, AQ, world, tmp_path, "gz", 3, bgzf=True)[0]["json"] == want
    # pseudo-assembly left to the host for every batch: the tables come in through kslam_align_qc_add on the host stage's thread,
    # with the columns parsed from the batch's text
    left, st = _stream_files(kslam, AQ, world, tmp_path, "cap", 2, env={"KSLAM_PSEUDO_CAP": "3"})
    assert st["batches_pseudo_on_host"] == 3 and left["json"] == want
    doc = AQ.parse(want)
    assert doc["paired"] is True and doc["max_cycles"] == 512 and doc["summary"]["records"] == doc["read1"]["records"] + doc["read2"]["records"]


def test_planted_errors_are_found_through_the_aligner(kslam, AQ, tmp_path):
    """tests/alignqc_ref.py's planted reads as FASTQ through kslam_stream_classify: the report's mismatch cycles, quality rows,
    substitution cells, indel length bins and insert-size bins are the planted ones.  tests/test_alignqc_host.py checks on the CPU
    that the oracle chain places enough of these pairs."""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    entries, t1, t2, want = R.planted()
    n_pairs = want["read1"]["n"]
    goff = np.concatenate([[0], np.cumsum([len(e) for e in entries])]).astype(np.uint64)
    gbases = np.frombuffer(b"".join(entries) + bytes(64), dtype=np.uint8)
    c = kslam.Context()
    h1, h2 = _host_text(kslam, t1), _host_text(kslam, t2)
    name = str(tmp_path / "planted.json")
    fd = os.open(name, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    try:
        c.set_index_arrays(gbases, goff)
        S.classify_stream_native(c, T.IndexArrays(gbases[:int(goff[-1])], goff, [b"planted.1", b"decoy.1", b"decoy.2"], [1, 2, 3]), h1.ptr, len(t1),
                                 h2.ptr, len(t2), n_pairs, T.TailParams.default(paired=True), align_qc_fd=fd)
    finally:
        os.close(fd)
        c.close()
        h1.close()
        h2.close()
    R.check_planted(AQ.parse(open(name, "rb").read()), want, n_pairs)


def test_single_end_through_the_stream(kslam, AQ, world, tmp_path):
    want, exp = _twin_file(kslam, AQ, world, single=True, cycles=90)
    assert b'"read2"' not in want and exp["pairs_both"] == 0
    assert _stream_files(kslam, AQ, world, tmp_path, "se1", 1, single=True, cycles=90)[0]["json"] == want
    assert _stream_files(kslam, AQ, world, tmp_path, "se3", 3, single=True, cycles=90, bgzf=True)[0]["json"] == want
