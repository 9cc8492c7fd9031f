"""The consensus caller on the GPU (csrc/consensus.hip, include/kslam_consensus.h): the device's rows, sequences and statistics
against the host twin (kslam_tail_consensus) AND the plain-Python restatement (tests/consensus_ref.py), exactly -- the walk,
alphabet, entry, call and grid seams under every parameter set, the slice seams, accumulation and the refusals, real batches
through kslam_stream_classify with one lane, three lanes and pseudo-assembly left to the host, paired and single-end, and planted
substitutions, a deletion and an insertion found again through the aligner."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import consensus_ref as R
from test_gpu_readsplit import _host_text, _indexed_context, world  # noqa: F401  (the fixture and its helpers)

pytestmark = pytest.mark.gpu
CASES = R.cases()
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = 1, 4, 5   # include/kslam.h: kslam_status
_EXPECTED = {}


@pytest.fixture(scope="module")
def CN(kslam):
    return importlib.import_module("kslam_amd.consensus")


class _Bench:
    """one context; the index is rebuilt when a case brings other entries (kslam_set_index drops the state)"""

    def __init__(self, kslam, CN):
        self.c, self.CN, self.entries = kslam.Context(), CN, None

    def on(self, case):
        key = (case["gbases"].tobytes(), case["goff"].tobytes())
        if key != self.entries:
            self.keep = np.concatenate([case["gbases"], np.zeros(64, dtype=np.uint8)])
            self.c.set_index_arrays(self.keep, case["goff"])
            assert not self.CN.get_consensus(self.c)   # a new index frees the state
            self.entries = key
            self.c.set_pairing(stages=3)
            self.CN.set_consensus(self.c, True)
        else:
            self.CN.reset(self.c)
            self.CN.set_slice(self.c, 0)
        return self.c


@pytest.fixture(scope="module")
def bench(kslam, CN):
    b = _Bench(kslam, CN)
    yield b
    b.c.set_pairing(stages=0)
    b.c.close()


def twin(CN, c, params=R.DEFAULTS):
    return CN.tail_consensus(c["gbases"], c["goff"], c["ov"], c["pool"], c["rbases"], c["roff"], c["rp"], c["pr"], *params)


def _add(CN, ctx, c):
    CN.add(ctx, c["ov"], c["pool"], c["rbases"], c["roff"], c["rp"], c["pr"])


def _expect(CN, c, params=R.DEFAULTS):
    """the restatement's answer, which the twin must give too (computed once per case and parameter set)"""
    key = (c["name"], params)
    if key not in _EXPECTED:
        rows, seqs, stats = R.consensus(c, *params)
        got, seq, got_stats = twin(CN, c, params)
        assert R.fields(got) == R.fields(rows) and R.split(got, seq) == seqs and got_stats == stats, key
        _EXPECTED[key] = (R.fields(rows), seqs, stats)
    return _EXPECTED[key]


def _device_equals(CN, ctx, c, params=R.DEFAULTS):
    rows, seqs, stats = _expect(CN, c, params)
    got, seq, got_stats = CN.take(ctx, *params)
    assert got_stats == stats, (c["name"], params)
    assert R.fields(got) == rows, (c["name"], params)
    assert R.split(got, seq) == seqs and len(seq) == sum(len(s) for s in seqs), (c["name"], params)
    assert not got["pad"].any()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_twin_and_restatement(CN, bench, case):
    ctx = bench.on(case)
    _add(CN, ctx, case)
    for params in R.PARAMS:
        _device_equals(CN, ctx, case, params)


def test_slices(CN, bench):
    by = {c["name"]: c for c in CASES}
    for name in ("entries", "random-900"):
        c = by[name]
        ctx = bench.on(c)
        _add(CN, ctx, c)
        rows, _, stats = _expect(CN, c)
        assert stats["n_entries_touched"] >= 5
        lens = np.diff(c["goff"].astype(np.int64))
        total = int(sum(lens[r[0]] for r in rows))   # (every touched entry has a covered position at depth 1: the rows are the touched entries)
        assert len(rows) == stats["n_entries_touched"]
        for s in (total, total - 1, total + 1, 1, int(lens.max()), 0):
            CN.set_slice(ctx, s)
            for params in R.PARAMS[:3]:
                _device_equals(CN, ctx, c, params)


def test_accumulation_reset_growth_and_switch(CN, bench):
    a = R.random_case("a", 71, 300, 7, 300)
    ents = [a["gbases"][int(a["goff"][e]):int(a["goff"][e + 1])].tobytes() for e in range(7)]
    b = R.random_case("b", 72, 3000, 7, entries=ents)          # ten times a's keys: the buffers grow and keep a's keys
    both, other = R.concat(a, b), R.concat(b, a)
    both["name"], other["name"] = "a+b", "b+a"
    stats = _expect(CN, both)[2]
    assert _expect(CN, other) == _expect(CN, both) and stats["n_events"] > 5 * _expect(CN, a)[2]["n_events"] > 0 and stats["n_insertions"] > 50
    ctx = bench.on(a)
    _add(CN, ctx, a)
    _device_equals(CN, ctx, a)
    _add(CN, ctx, b)                                           # an add after a take
    _device_equals(CN, ctx, both)
    _device_equals(CN, ctx, both)                              # take twice: the same
    _device_equals(CN, ctx, both, R.PARAMS[2])                 # and with other parameters
    CN.reset(ctx)
    _add(CN, ctx, both)                                        # one add of the concatenation
    _device_equals(CN, ctx, both)
    CN.reset(ctx)
    _add(CN, ctx, b)                                           # the order of the batches does not matter
    _add(CN, ctx, a)
    _device_equals(CN, ctx, both)
    empty = dict.fromkeys(R.STAT_NAMES, 0)
    CN.reset(ctx)
    got, seq, got_stats = CN.take(ctx)
    assert len(got) == 0 and seq == b"" and got_stats == empty
    _add(CN, ctx, a)
    CN.set_consensus(ctx, False)
    assert not CN.get_consensus(ctx)
    CN.set_consensus(ctx, True)                                # off and on again starts from nothing
    got, seq, got_stats = CN.take(ctx)
    assert len(got) == 0 and got_stats == empty
    _add(CN, ctx, a)
    _device_equals(CN, ctx, a)
    assert CN.kernel_ms(ctx)[0] > 0 and CN.kernel_ms(ctx)[1] > 0
    # kslam_set_index frees the state too
    bench.entries = None
    ctx = bench.on(a)
    got, seq, got_stats = CN.take(ctx)
    assert len(got) == 0 and got_stats == empty


def test_refusals(kslam, CN):
    L = CN.lib()
    bld = R.CB("x", [b"ACGT" * 25])
    bld.group([(0, bld.gapped(0, 0, [(20, "M")], 0, mismatch_at=(3,)), bld.gapped(0, 30, [(10, "M"), (2, "I"), (10, "M")], 1, ins=[b"GG"]))])
    bld.single(bld.gapped(0, 50, [(4, "M")], 0, mismatch_at=(0,)))
    case = bld.done()
    keep = np.concatenate([case["gbases"], np.zeros(64, dtype=np.uint8)])

    def args(**kw):
        a = {k: kw.get(k, case[k]) for k in ("ov", "pool", "rbases", "roff", "rp", "pr")}
        return (a["ov"].ctypes.data, len(a["ov"]), a["pool"].ctypes.data, len(a["pool"]), a["rbases"].ctypes.data, a["roff"].ctypes.data,
                len(a["roff"]) - 1, a["rp"].ctypes.data, len(a["rp"]), a["pr"].ctypes.data, len(a["pr"]))

    c = kslam.Context()
    try:
        c.set_pairing(stages=3)
        assert L.kslam_set_consensus(c._h, 1) == ERR_STATE                 # no index
        assert b"kslam_set_index" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=0)
        c.set_index_arrays(keep, case["goff"])
        assert L.kslam_set_consensus(c._h, 1) == ERR_STATE                 # the pairing is off
        assert b"kslam_set_pairing" in c._L.kslam_last_error(c._h)
        for call in (lambda: L.kslam_consensus_reset(c._h), lambda: L.kslam_consensus_add(c._h, *args()), lambda: L.kslam_consensus_set_slice(c._h, 5)):
            assert call() == ERR_STATE and b"kslam_set_consensus" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=3)
        CN.set_consensus(c, True)
        CN.add(c, case["ov"], case["pool"], case["rbases"], case["roff"], case["rp"], case["pr"])
        before = CN.take(c)
        for field, kw, message in (("pr", ("r1", 1, len(case["ov"])), b"refers to overlap record"), ("rp", ("count", 1, 2), b"outside the pairs array"),
                                   ("rp", ("first", 1, 0), b"ascend"), ("ov", ("cigar_off", 1, len(case["pool"])), b"outside the pool"),
                                   ("ov", ("read", 2, len(case["roff"]) - 1), b"refers to read")):
            bad = case[field].copy()
            bad[kw[0]][kw[1]] = kw[2]
            assert L.kslam_consensus_add(c._h, *args(**{field: bad})) == ERR_ARG
            assert message in c._L.kslam_last_error(c._h)
            got = CN.take(c)                                             # the state is as it was
            assert R.fields(got[0]) == R.fields(before[0]) and got[1:] == before[1:]
        assert R.fields(before[0]) == R.fields(R.consensus(case)[0]) and before[2] == R.consensus(case)[2]
        for bad in ((0, 500, 0, 1), (1, 499, 0, 1), (1, 1000, 0, 1), (1, 500, 2, 1)):
            p = CN.params(*bad)
            rows, n, seq, st = C.c_void_p(), C.c_uint64(), C.c_void_p(), CN.Stats()
            assert L.kslam_consensus_take(c._h, C.byref(p), C.byref(rows), C.byref(n), C.byref(seq), C.byref(st)) == ERR_ARG
            assert L.kslam_stream_set_consensus(c._h, 1, C.byref(p)) == ERR_ARG
        CN.set_consensus(c, False)
    finally:
        c.set_pairing(stages=0)
        c.close()
    c = kslam.Context(report_cigar=False)
    try:
        c.set_index_arrays(keep, case["goff"])
        c.set_pairing(stages=3)
        assert L.kslam_set_consensus(c._h, 1) == ERR_STATE and b"report_cigar" in c._L.kslam_last_error(c._h)
    finally:
        c.set_pairing(stages=0)
        c.close()
    m = kslam.MultiContext([0])
    try:
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)   # (tests/test_gpu_readsplit.py: the first context)
        assert L.kslam_set_consensus(h, 1) == ERR_UNSUPPORTED
        assert L.kslam_stream_set_consensus(h, 1, None) == ERR_UNSUPPORTED
    finally:
        m.close()


# ---- real batches through the lanes: the world of tests/test_gpu_readsplit.py ----

def _fastq_bases(text):
    return [line.rstrip(b"\r") for line in text.split(b"\n")[1::4]]


def stream_file(kslam, CN, world, name, lanes, per_batch=300, env=None, single=False, params=None, taxdb=True):
    """kslam_stream_classify with kslam_stream_set_consensus -> (the file's bytes, the call's statistics)"""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    env = dict(env or {}, KSLAM_LANES=str(lanes))
    os.environ.update(env)
    try:
        c = _indexed_context(kslam, world)
        h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
        fd = os.open(name, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
        try:
            st = S.classify_stream_native(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), per_batch,
                                          T.TailParams.default(paired=not single), taxdb=X.TaxDB(world["case"]["taxdb"]) if taxdb else None, depth=3,
                                          consensus_fd=fd, consensus_params=params)
            assert not CN.get_consensus(c)   # the call switched it off again
        finally:
            os.close(fd)
            c.close()
            h1.close()
            h2.close()
    finally:
        for k in env:
            del os.environ[k]
    return open(name, "rb").read(), st


def twin_file(kslam, CN, world, per_batch=300, single=False, params=R.DEFAULTS):
    """the same batches through the Python loop: the final arrays of every batch with its CIGAR pool and its reads, concatenated,
    through the host twin (which must agree with the restatement) and the FASTA writer -> (the file's bytes, rows, sequences)"""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    b1, b2 = _fastq_bases(r1), _fastq_bases(r2)
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    got = []
    try:
        S.classify_stream(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), per_batch,
                          T.TailParams.default(paired=not single), depth=3,
                          on_batch=lambda rec, ov, cg, rp, pr, reads: got.append((np.array(ov), np.array(cg), np.array(rp), np.array(pr), np.array(reads.bases_off))))
    finally:
        c.close()
        h1.close()
        h2.close()
    ents = [bytes(e["bases"]) for e in world["case"]["entries"]]
    gbases = np.frombuffer(b"".join(ents), dtype=np.uint8)
    goff = np.concatenate([[0], np.cumsum([len(e) for e in ents])]).astype(np.uint64)
    whole = None
    for k, (ov, cg, rp, pr, bases_off) in enumerate(got):
        reads = b1[per_batch * k:per_batch * (k + 1)] + ([] if single else b2[per_batch * k:per_batch * (k + 1)])   # a batch is [R1 block | R2 block]
        roff = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
        assert roff.tolist() == (bases_off - bases_off[0]).tolist()
        part = {"name": "batch", "gbases": gbases, "goff": goff, "rbases": np.frombuffer(b"".join(reads), dtype=np.uint8), "roff": roff,
                "pool": cg.astype(np.uint32), "ov": ov.astype(R.OVERLAP_DT), "rp": rp.astype(R.READ_PAIR_DT), "pr": pr.astype(R.PAIRED_OVERLAP_DT)}
        whole = part if whole is None else R.concat(whole, part)
    rows, seq, stats = twin(CN, whole, params)
    ref_rows, ref_seqs, ref_stats = R.consensus(whole, *params)
    assert R.fields(rows) == R.fields(ref_rows) and R.split(rows, seq) == ref_seqs and stats == ref_stats and stats["n_skipped"] == 0
    return CN.report_bytes(world["db"], rows, seq), rows, ref_seqs, stats, len(got)


def test_three_batches_through_the_stream(kslam, CN, world, tmp_path):
    exp, rows, seqs, stats, n_batches = twin_file(kslam, CN, world)
    assert n_batches == 3 and stats["n_events"] > 1000 and len(rows) > 3 and stats["n_intervals"] > 500
    loci = [bytes(e["locusTag"]) for e in world["case"]["entries"]]
    assert exp == R.fasta_bytes(rows, seqs, loci)
    got, st = stream_file(kslam, CN, world, str(tmp_path / "l1.fa"), 1)
    assert got == exp and st["batches_pseudo_on_host"] == 0
    assert stream_file(kslam, CN, world, str(tmp_path / "l3.fa"), 3)[0] == exp
    # pseudo-assembly left to the host for every batch: the keys come in through kslam_consensus_add on the host stage's thread
    left, st = stream_file(kslam, CN, world, str(tmp_path / "cap.fa"), 2, env={"KSLAM_PSEUDO_CAP": "3"})
    assert st["batches_pseudo_on_host"] == 3 and left == exp
    assert [(p[0].encode(), p[2].encode()) for p in CN.parse(exp)] == [(loci[int(r["entry"])], s) for r, s in zip(rows, seqs)]
    # other parameters travel through kslam_stream_set_consensus
    params = (2, 750, R.FILL_REF, 40)
    strict = twin_file(kslam, CN, world, params=params)[0]
    assert strict != exp and stream_file(kslam, CN, world, str(tmp_path / "strict.fa"), 2, params=params)[0] == strict


def test_single_end_through_the_stream(kslam, CN, world, tmp_path):
    exp, rows, _, _, _ = twin_file(kslam, CN, world, single=True)
    assert len(rows) > 3
    assert stream_file(kslam, CN, world, str(tmp_path / "se.fa"), 2, single=True)[0] == exp


# ---- planted truth through the aligner ----

def test_planted_differences_are_found_through_the_aligner(kslam, CN, tmp_path):
    """Reads of a mutated copy as FASTQ against the UNMUTATED entry and two decoys.  Over the span every read of which lies inside
    the entry with a read length to spare, the reported sequence is the mutated copy: substitutions, the deletion and the
    insertion are called by majority (a read that holds a gap within a few bases of its end is clipped there and votes nothing)."""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    entry, copy, n_subs, reads = R.planted()
    rng = np.random.default_rng(98)
    ents = [entry, R.random_bases(rng, 3000), R.random_bases(rng, 3000)]
    loci = [b"planted.1", b"decoy.1", b"decoy.2"]
    goff = np.concatenate([[0], np.cumsum([len(e) for e in ents])]).astype(np.uint64)
    gbases = np.frombuffer(b"".join(ents) + bytes(64), dtype=np.uint8)
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    c = kslam.Context()
    h = _host_text(kslam, text)
    name = str(tmp_path / "planted.fa")
    fd = os.open(name, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    try:
        c.set_index_arrays(gbases, goff)
        S.classify_stream_native(c, T.IndexArrays(gbases[:int(goff[-1])], goff, loci, [1, 2, 3]), h.ptr, len(text), None, 0, len(reads),
                                 T.TailParams.default(paired=False), consensus_fd=fd, consensus_params=(3, 500, R.FILL_N, 1))
    finally:
        os.close(fd)
        c.close()
        h.close()
    got = CN.parse(open(name, "rb").read())
    assert [g[0] for g in got] == ["planted.1"]
    locus, fields, seq = got[0]
    assert fields["entry_length"] == len(entry) and fields["deletions"] == 3 and fields["insertions"] == 1 and fields["ambiguous"] == 0
    assert fields["substitutions"] == n_subs > 20
    assert len(seq) == len(copy) and seq[200:-200].encode() == copy[200:-200]
