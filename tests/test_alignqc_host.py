"""The host side of the alignment QC report (host/alignqc.cpp, include/kslam_alignqc.h): kslam_tail_align_qc equals the
plain-Python restatement (tests/alignqc_ref.py) word for word on the case set the device is held to, kslam_align_qc_write equals
the restatement's bytes and the header's example, every argument refusal is KSLAM_ERR_ARG and writes nothing, the library exports
what the header declares.  No GPU."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import alignqc_ref as R
from test_alignqc_ref import HEADER_EXAMPLE

ERR_ARG = 1   # include/kslam.h: kslam_status
CASES = R.cases()


@pytest.fixture(scope="module")
def AQ(kslam):
    return importlib.import_module("kslam_amd.alignqc")


def twin(AQ, case, cycles):
    """the host twin on every batch of the case, summed (a batch without a quality column cannot be concatenated with one with)"""
    t = None
    for b in case["batches"]:
        p = AQ.tail_align_qc(b["gbases"], b["goff"], b["ov"], b["pool"], b["rbases"], b["roff"], b["rp"], b["pr"], b["rqual"], b["paired"], cycles)
        t = p if t is None else R.add_tables(t, p)
    return t


@pytest.mark.parametrize("C", R.CYCLES)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_equals_restatement(AQ, case, C):
    exp = R.tables(case, C)
    got = twin(AQ, case, C)
    assert AQ.pack(got)[0].tolist() == AQ.pack(exp)[0].tolist() and got == exp, case["name"]     # word for word, and the two flags
    text = AQ.report_bytes(got)
    assert text == R.text(exp)
    doc = AQ.parse(text)
    assert doc["max_cycles"] == C and isinstance(doc["summary"]["error_rate"], float) and isinstance(doc["summary"]["insert_size_median"], str)
    assert doc["summary"]["records"] == exp["streams"][0]["n_records"] + exp["streams"][1]["n_records"]


def test_the_headers_example_and_the_parser(AQ):
    t = twin(AQ, R.header_example(), 4)
    assert AQ.report_bytes(t) == HEADER_EXAMPLE
    doc = AQ.parse(HEADER_EXAMPLE)
    assert doc["read1"]["by_quality"] == {2: [1, 0, 0.0], 20: [4, 3, 1.249387], 40: [4, 1, 6.0206]} and doc["insert_size_counts"] == {9: 1}
    assert doc["read1"]["mismatch_rate_by_cycle"] == [0.5, 0.5, 0.0, 1.0] and doc["summary"]["mean_identity"] == pytest.approx(5 / 11, abs=1e-6)
    with pytest.raises(ValueError):
        AQ.parse(b'{"kslam_align_qc": 2}')
    assert AQ.unpack(*AQ.pack(t)) == t
    # a rate of 1 prints no minus sign
    b = R.Builder("all-wrong", [b"ACGTACGTAC"])
    b.single(b.aligned(0, 0, [(10, "M")], 0, mismatch_at=range(10)))
    assert b'"40": [10, 10, "0.000000"]' in AQ.report_bytes(twin(AQ, R.case_of("all-wrong", b.done()), 4))


def test_planted_reads_through_the_oracle_chain(kslam, AQ):
    """The planted reads of tests/alignqc_ref.py through the oracle chain (the reference's aligner and pairing on the CPU) and the
    host twin: the chain places enough of the pairs for the GPU test's cap of 5 %, and the report holds what was planted."""
    import oracle
    T = importlib.import_module("kslam_amd.tail")
    entries, t1, t2, want = R.planted()
    col = lambda t, k: t.split(b"\n")[k::4]   # noqa: E731
    reads, quals = col(t1, 1) + col(t2, 1), col(t1, 3) + col(t2, 3)
    n = want["read1"]["n"]
    assert len(reads) == 2 * n and want["ins"] == want["del"] == n // 4
    eal, ecig, _ = oracle.align_to_database(reads, entries)
    view = T.Reads(reads, quals, [b"p%d" % (i % n) for i in range(2 * n)])
    erp, epr = oracle.tail_pairs(T.TailParams.default(paired=True), view.view, eal)
    offsets = lambda items: np.concatenate([[0], np.cumsum([len(x) for x in items])]).astype(np.uint64)   # noqa: E731
    t = AQ.tail_align_qc(np.frombuffer(b"".join(entries), dtype=np.uint8), offsets(entries), eal.astype(R.OVERLAP_DT), ecig.astype(np.uint32),
                         np.frombuffer(b"".join(reads), dtype=np.uint8), offsets(reads), erp.astype(R.READ_PAIR_DT), epr.astype(R.PAIRED_OVERLAP_DT),
                         np.frombuffer(b"".join(quals), dtype=np.uint8), True, 512)
    R.check_planted(AQ.parse(AQ.report_bytes(t)), want, n)
    assert t["pairs_both"] >= n - n // 40      # (inside the cap with room to spare: the device's ties may fall otherwise)


def test_argument_errors(kslam, AQ):
    L = AQ.lib()
    T = importlib.import_module("kslam_amd.tail")
    V = importlib.import_module("kslam_amd.variants")
    case = R.header_example()["batches"][0]

    def call(cycles=0, paired=0, t=None, quality=True, **kw):
        a = {k: kw.get(k, case[k]) for k in ("ov", "pool", "rbases", "roff", "rp", "pr")}
        keep, args = V._arrays(a["ov"], a["pool"], a["rbases"], a["roff"], a["rp"], a["pr"])
        t = t if t is not None else AQ.Tables()
        rc = L.kslam_tail_align_qc(case["gbases"].ctypes.data, case["goff"].ctypes.data, len(case["goff"]) - 1, *args,
                                   case["rqual"].ctypes.data if quality else None, paired, cycles, C.byref(t))
        if rc == 0:
            L.kslam_tail_align_qc_free(C.byref(t))
        else:
            assert not t.block and not t.n_words
        return rc

    assert call() == 0 and call(quality=False) == 0 and call(cycles=65536) == 0 and call(paired=1) == 0
    assert call(cycles=65537) == ERR_ARG and b"max_cycles" in T.lib().kslam_tail_last_error()
    for field, (key, at, value), message in (("pr", ("r1", 0, len(case["ov"])), b"refers to overlap record"), ("rp", ("count", 0, 2), b"outside the pairs array"),
                                             ("ov", ("cigar_off", 1, len(case["pool"])), b"outside the pool"),
                                             ("ov", ("read", 0, len(case["roff"]) - 1), b"refers to read")):
        bad = case[field].copy()
        bad[key][at] = value
        assert call(**{field: bad}) == ERR_ARG and message in T.lib().kslam_tail_last_error(), field
    two = np.concatenate([case["rp"], case["rp"]])          # two groups over the same slice
    assert call(rp=two) == ERR_ARG and b"ascend" in T.lib().kslam_tail_last_error()
    assert call(roff=np.array([0, 6, 5], dtype=np.uint64)) == ERR_ARG and b"offsets must ascend" in T.lib().kslam_tail_last_error()
    assert call(roff=np.array([0, 6, 10, 10], dtype=np.uint64), paired=1) == ERR_ARG and b"even number" in T.lib().kslam_tail_last_error()
    assert L.kslam_tail_align_qc(None, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, 0, None, 0, 0, None) == ERR_ARG
    assert L.kslam_tail_align_qc(None, None, 0, None, 1, None, 0, None, None, 0, None, 0, None, 0, None, 0, 0, C.byref(AQ.Tables())) == ERR_ARG
    # the writer: tables nobody laid out write nothing
    fd = os.memfd_create("nothing")
    try:
        t = AQ.Tables()
        assert L.kslam_align_qc_write(C.byref(t), fd) == ERR_ARG and L.kslam_align_qc_write(None, fd) == ERR_ARG
        block = np.zeros(AQ.words(4), dtype=np.uint64)
        t.max_cycles, t.n_words, t.block = 4, AQ.words(4) + 1, block.ctypes.data
        assert L.kslam_align_qc_write(C.byref(t), fd) == ERR_ARG
        t.max_cycles, t.n_words = 0, AQ.words(4)
        assert L.kslam_align_qc_write(C.byref(t), fd) == ERR_ARG
        assert os.lseek(fd, 0, os.SEEK_END) == 0
        t.max_cycles = 4
        assert L.kslam_align_qc_write(C.byref(t), -1) == ERR_ARG and b"writing the alignment QC report failed" in T.lib().kslam_tail_last_error()
        assert L.kslam_align_qc_write(C.byref(t), fd) == 0 and os.lseek(fd, 0, os.SEEK_END) > 0
    finally:
        os.close(fd)
    with pytest.raises(ValueError):
        AQ.tail_align_qc(case["gbases"], case["goff"], case["ov"], case["pool"], case["rbases"], case["roff"], case["rp"], case["pr"], b"II")


def test_library_exports_every_declared_symbol(kslam, AQ):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "kslam_alignqc.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = C.CDLL(kslam.LIB_PATH)
    assert len(declared) == 12 and sorted(AQ.EXPORTS) == declared
    for name in declared:
        assert hasattr(L, name), "missing export " + name
    assert L.kslam_abi_version() == 10
    assert C.sizeof(AQ.StreamView) == 12 * 8 + 8 * 8 and C.sizeof(AQ.Tables) == 24 + 5 * 8 + 8 + 2 * C.sizeof(AQ.StreamView)
    assert AQ.words(512) == 1008 + 2 * (324 + 513 * 194) and 8 * AQ.words(512) < 1.7e6
    for n, m in (("QUAL_COLS", "QUAL_COLS"), ("INSERT_BINS", "INSERT_BINS"), ("NM_BINS", "NM_BINS")):
        assert getattr(AQ, n) == getattr(R, m)
