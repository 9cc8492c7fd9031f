"""The SNV table on the GPU (csrc/variants.hip, include/kslam_variants.h): the device's rows and statistics against the host twin
(kslam_tail_variants) AND the plain-Python restatement (tests/variants_ref.py), exactly -- the walk, alphabet, entry, depth, run,
contributing-set, skip and grid seams, the filters, accumulation and the refusals, real batches through kslam_stream_classify
with one lane, three lanes, the host's SAM text and pseudo-assembly left to the host, and planted substitutions found again
through the aligner."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import variants_ref as R
from test_gpu_readsplit import _host_text, _indexed_context, world  # noqa: F401  (the fixture and its helpers)

pytestmark = pytest.mark.gpu
CASES = R.cases()
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = 1, 4, 5   # include/kslam.h: kslam_status


@pytest.fixture(scope="module")
def VR(kslam):
    return importlib.import_module("kslam_amd.variants")


class _Bench:
    """one context; the index is rebuilt when a case brings other entries (kslam_set_index drops the state)"""

    def __init__(self, kslam, VR):
        self.c, self.VR, self.entries = kslam.Context(), VR, None

    def on(self, case):
        key = (case["gbases"].tobytes(), case["goff"].tobytes())
        if key != self.entries:
            self.keep = np.concatenate([case["gbases"], np.zeros(64, dtype=np.uint8)])
            self.c.set_index_arrays(self.keep, case["goff"])
            assert not self.VR.get_variants(self.c)   # a new index frees the state
            self.entries = key
            self.c.set_pairing(stages=3)
            self.VR.set_variants(self.c, True)
        else:
            self.VR.reset(self.c)
        return self.c


@pytest.fixture(scope="module")
def bench(kslam, VR):
    b = _Bench(kslam, VR)
    yield b
    b.c.set_pairing(stages=0)
    b.c.close()


def twin(VR, c, min_alt=1, min_depth=0):
    return VR.tail_variants(c["gbases"], c["goff"], c["ov"], c["pool"], c["rbases"], c["roff"], c["rp"], c["pr"], min_alt, min_depth)


def _add(VR, ctx, c):
    VR.add(ctx, c["ov"], c["pool"], c["rbases"], c["roff"], c["rp"], c["pr"])


def _expect(VR, c, min_alt=1, min_depth=0):
    rows, stats = R.table(c, min_alt, min_depth)
    got, got_stats = twin(VR, c, min_alt, min_depth)
    assert R.fields(got) == R.fields(rows) and got_stats == stats
    return rows, stats


def _device_equals(VR, ctx, c, rows, stats, min_alt=1, min_depth=0):
    got, got_stats = VR.take(ctx, min_alt, min_depth)
    assert got_stats == stats, c["name"]
    assert R.fields(got) == R.fields(rows), c["name"]
    assert not got["pad"].any()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_rows_equal_twin_and_restatement(VR, bench, case):
    ctx = bench.on(case)
    rows, stats = _expect(VR, case)
    _add(VR, ctx, case)
    _device_equals(VR, ctx, case, rows, stats)


def test_filters(VR, bench):
    c = R.filter_case()
    ctx = bench.on(c)
    _add(VR, ctx, c)
    for min_alt in (1, 2, 3):
        for min_depth in (4, 5, 6):
            rows, stats = _expect(VR, c, min_alt, min_depth)
            _device_equals(VR, ctx, c, rows, stats, min_alt, min_depth)
    assert [r[1] for r in R.fields(VR.take(ctx, 2, 5)[0])] == [40, 50]


def test_accumulation_reset_growth_and_switch(VR, bench):
    a = R.random_case("a", 71, 900, 7, 300)
    ents = [a["gbases"][int(a["goff"][e]):int(a["goff"][e + 1])].tobytes() for e in range(7)]
    b = R.random_case("b", 72, 9000, 7, entries=ents)          # ten times a's events: the buffers grow and keep a's keys
    both, other = R.concat(a, b), R.concat(b, a)
    rows, stats = _expect(VR, both)
    assert _expect(VR, other)[1] == stats and stats["n_events"] > 10 * R.table(a)[1]["n_events"] > 0
    ctx = bench.on(a)
    _add(VR, ctx, a)
    first = R.table(a)
    _device_equals(VR, ctx, a, *first)
    _add(VR, ctx, b)                                           # an add after a take
    _device_equals(VR, ctx, both, rows, stats)
    _device_equals(VR, ctx, both, rows, stats)                 # take twice: the same rows
    _device_equals(VR, ctx, both, *R.table(both, 2, 3), 2, 3)  # and with other thresholds
    VR.reset(ctx)
    _add(VR, ctx, both)                                        # one add of the concatenation
    _device_equals(VR, ctx, both, rows, stats)
    VR.reset(ctx)
    _add(VR, ctx, b)                                           # the order of the batches does not matter
    _add(VR, ctx, a)
    _device_equals(VR, ctx, both, rows, stats)
    empty = dict.fromkeys(R.STAT_NAMES, 0)
    VR.reset(ctx)
    got, got_stats = VR.take(ctx, 1, 0)
    assert len(got) == 0 and got_stats == empty
    _add(VR, ctx, a)
    VR.set_variants(ctx, False)
    assert not VR.get_variants(ctx)
    VR.set_variants(ctx, True)                                 # off and on again starts from nothing
    got, got_stats = VR.take(ctx, 1, 0)
    assert len(got) == 0 and got_stats == empty
    _add(VR, ctx, a)
    _device_equals(VR, ctx, a, *first)
    assert VR.kernel_ms(ctx)[0] > 0 and VR.kernel_ms(ctx)[1] > 0
    # kslam_set_index frees the state too
    bench.entries = None
    ctx = bench.on(a)
    got, got_stats = VR.take(ctx, 1, 0)
    assert len(got) == 0 and got_stats == empty


def test_refusals(kslam, VR):
    L = VR.lib()
    bld = R.Builder("x", [b"ACGT" * 25])
    bld.group([(0, bld.aligned(0, 0, [(20, "M")], 0, mismatch_at=(3,)), bld.aligned(0, 30, [(20, "M")], 1, mismatch_at=(3,)))])
    bld.single(bld.aligned(0, 50, [(4, "M")], 0, mismatch_at=(0,)))
    case = bld.done()
    keep = np.concatenate([case["gbases"], np.zeros(64, dtype=np.uint8)])

    def args(**kw):
        a = {k: kw.get(k, case[k]) for k in ("ov", "pool", "rbases", "roff", "rp", "pr")}
        return (a["ov"].ctypes.data, len(a["ov"]), a["pool"].ctypes.data, len(a["pool"]), a["rbases"].ctypes.data, a["roff"].ctypes.data,
                len(a["roff"]) - 1, a["rp"].ctypes.data, len(a["rp"]), a["pr"].ctypes.data, len(a["pr"]))

    c = kslam.Context()
    try:
        c.set_pairing(stages=3)
        assert L.kslam_set_variants(c._h, 1) == ERR_STATE                 # no index
        assert b"kslam_set_index" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=0)
        c.set_index_arrays(keep, case["goff"])
        assert L.kslam_set_variants(c._h, 1) == ERR_STATE                 # the pairing is off
        assert b"kslam_set_pairing" in c._L.kslam_last_error(c._h)
        for call in (lambda: L.kslam_variants_reset(c._h), lambda: L.kslam_variants_add(c._h, *args())):
            assert call() == ERR_STATE and b"kslam_set_variants" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=3)
        VR.set_variants(c, True)
        for field, kw, message in (("pr", ("r1", 1, len(case["ov"])), b"refers to overlap record"), ("rp", ("count", 1, 2), b"outside the pairs array"),
                                   ("rp", ("first", 1, 0), b"ascend"), ("ov", ("cigar_off", 1, len(case["pool"])), b"outside the pool"),
                                   ("ov", ("read", 2, len(case["roff"]) - 1), b"refers to read")):
            bad = case[field].copy()
            bad[kw[0]][kw[1]] = kw[2]
            assert L.kslam_variants_add(c._h, *args(**{field: bad})) == ERR_ARG
            assert message in c._L.kslam_last_error(c._h)
        got, stats = VR.take(c, 1, 0)
        assert len(got) == 0 and stats == dict.fromkeys(R.STAT_NAMES, 0)   # nothing was added
        VR.add(c, case["ov"], case["pool"], case["rbases"], case["roff"], case["rp"], case["pr"])
        assert R.fields(VR.take(c, 1, 0)[0]) == R.fields(R.table(case)[0])
        VR.set_variants(c, False)
    finally:
        c.set_pairing(stages=0)
        c.close()
    c = kslam.Context(report_cigar=False)
    try:
        c.set_index_arrays(keep, case["goff"])
        c.set_pairing(stages=3)
        assert L.kslam_set_variants(c._h, 1) == ERR_STATE and b"report_cigar" in c._L.kslam_last_error(c._h)
    finally:
        c.set_pairing(stages=0)
        c.close()
    m = kslam.MultiContext([0])
    try:
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)   # (tests/test_gpu_readsplit.py: the first context)
        assert L.kslam_set_variants(h, 1) == ERR_UNSUPPORTED
        assert L.kslam_stream_set_variants(h, 1, 2, 1) == ERR_UNSUPPORTED
    finally:
        m.close()


# ---- real batches through the lanes: the world of tests/test_gpu_readsplit.py ----

def _fastq_bases(text):
    return [line.rstrip(b"\r") for line in text.split(b"\n")[1::4]]


def _stream_files(kslam, VR, world, tmp, tag, lanes, env=None, single=False, variants=True):
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
        names = {k: str(tmp / (tag + "." + k)) for k in ("vcf", "per_read", "sam")}
        fds = {k: os.open(p, os.O_RDWR | os.O_CREAT | os.O_TRUNC) for k, p in names.items()}
        P = T.TailParams.default(paired=not single)
        st = S.classify_stream_native(c, world["db"], h1.ptr, len(r1), None if single else h2.ptr, 0 if single else len(r2), 300, P, taxdb=tax,
                                      sam_fd=fds["sam"], per_read_fd=fds["per_read"], depth=3, variants_fd=fds["vcf"] if variants else None,
                                      variants_min_alt=1, variants_min_depth=1)
        assert not VR.get_variants(c)   # the call switched it off again
        for fd in fds.values():
            os.close(fd)
        c.close()
        h1.close()
        h2.close()
    finally:
        for k in env:
            del os.environ[k]
    return {k: open(p, "rb").read() for k, p in names.items()}, st


def _twin_file(kslam, VR, world, single=False):
    """the same batches through the Python loop, which leaves the SAM text to the host: the final arrays of every batch with its
    CIGAR pool and its reads, concatenated, through the host twin and the VCF writer"""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    r1, r2, n = world["case"]["r1"], world["case"]["r2"], world["n"]
    b1, b2 = _fastq_bases(r1), _fastq_bases(r2)
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
    whole = None
    for k, (ov, cg, rp, pr, bases_off) in enumerate(got):
        reads = b1[300 * k:300 * k + 300] + ([] if single else b2[300 * k:300 * k + 300])   # a batch is [R1 block | R2 block]
        roff = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
        assert roff.tolist() == (bases_off - bases_off[0]).tolist()
        part = {"name": "batch", "gbases": gbases, "goff": goff, "rbases": np.frombuffer(b"".join(reads), dtype=np.uint8), "roff": roff,
                "pool": cg.astype(np.uint32), "ov": ov.astype(R.OVERLAP_DT), "rp": rp.astype(R.READ_PAIR_DT), "pr": pr.astype(R.PAIRED_OVERLAP_DT)}
        whole = part if whole is None else R.concat(whole, part)
    rows, stats = twin(VR, whole, 1, 1)
    ref_rows, ref_stats = R.table(whole, 1, 1)
    assert R.fields(rows) == R.fields(ref_rows) and stats == ref_stats and stats["n_skipped"] == 0 and stats["n_events"] > 1000
    return VR.report_bytes(world["db"], rows, stats), rows


def test_three_batches_through_the_stream(kslam, VR, world, tmp_path):
    exp, rows = _twin_file(kslam, VR, world)
    plain, _ = _stream_files(kslam, VR, world, tmp_path, "plain", 1, variants=False)
    assert plain["vcf"] == b""
    files, st = _stream_files(kslam, VR, world, tmp_path, "l1", 1)
    assert files["vcf"] == exp and st["batches_pseudo_on_host"] == 0
    assert files["sam"] == plain["sam"] and files["per_read"] == plain["per_read"] and len(plain["sam"]) > 10000   # nothing else moves
    assert _stream_files(kslam, VR, world, tmp_path, "l3", 3)[0]["vcf"] == exp
    assert _stream_files(kslam, VR, world, tmp_path, "host", 2, env={"KSLAM_HOST_SAM_TEXT": "1"})[0]["vcf"] == exp
    # pseudo-assembly left to the host for every batch: the keys come in through kslam_variants_add on the host stage's thread
    left, st = _stream_files(kslam, VR, world, tmp_path, "cap", 2, env={"KSLAM_PSEUDO_CAP": "3"})
    assert st["batches_pseudo_on_host"] == 3 and left["vcf"] == exp
    entries = world["case"]["entries"]
    got = R.read_vcf(exp, [bytes(e["locusTag"]) for e in entries], [len(e["bases"]) for e in entries])
    assert got == R.fields(rows) and len(got) > 500


def test_single_end_through_the_stream(kslam, VR, world, tmp_path):
    exp, rows = _twin_file(kslam, VR, world, single=True)
    assert len(rows) > 200
    assert _stream_files(kslam, VR, world, tmp_path, "se", 2, single=True)[0]["vcf"] == exp


# ---- planted truth through the aligner ----

def test_planted_sites_are_found_through_the_aligner(kslam, VR, tmp_path):
    """The reads of tests/test_variants_host.py's planted case as FASTQ against the UNMUTATED entry and two decoys.  At min_alt = 2
    every row is a planted site with the planted alt and AO == DP (a clipped column is neither an event nor depth), and at least
    95 of the 100 sites are there: the non-GPU test checks that every site has at least 4 reads that hold it 3 or more bases
    from both ends, so losing a site takes the aligner dropping or clipping deep into several error-free reads."""
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    entry, sites, reads = R.planted()
    rng = np.random.default_rng(99)
    ents = [entry, R.random_bases(rng, 5000), R.random_bases(rng, 5000)]
    loci = [b"planted.1", b"decoy.1", b"decoy.2"]
    goff = np.concatenate([[0], np.cumsum([len(e) for e in ents])]).astype(np.uint64)
    gbases = np.frombuffer(b"".join(ents) + bytes(64), dtype=np.uint8)
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r[0], b"I" * len(r[0])) for i, r in enumerate(reads))
    c = kslam.Context()
    h = _host_text(kslam, text)
    name = str(tmp_path / "planted.vcf")
    fd = os.open(name, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    try:
        c.set_index_arrays(gbases, goff)
        S.classify_stream_native(c, T.IndexArrays(gbases[:int(goff[-1])], goff, loci, [1, 2, 3]), h.ptr, len(text), None, 0, len(reads),
                                 T.TailParams.default(paired=False), variants_fd=fd, variants_min_alt=2, variants_min_depth=1)
    finally:
        os.close(fd)
        c.close()
        h.close()
    got = R.read_vcf(open(name, "rb").read(), loci, [len(e) for e in ents])
    assert all(e == 0 and sites.get(pos) == alt and fwd + rev == depth for e, pos, ref, alt, fwd, rev, depth in got)
    assert len({pos for _, pos, *_ in got}) >= 95 and len(got) == len({pos for _, pos, *_ in got})
