"""The reads of chosen taxa on the GPU (csrc/taxreads.hip, include/kslam_taxreads.h): the device-built set S alone against the
plain-Python restatement (tests/taxreads_ref.py) at the wave and block seams of the tree; the flag pass and the copy against the
host twin (kslam_tail_taxon_reads) byte for byte at the seams of the batch, plain and BGZF; real batches through
kslam_stream_classify with one lane, three lanes and the host's route, next to the Kraken-style report and the reads split; and
the refusals."""
import ctypes as C
import gzip
import importlib
import os

import numpy as np
import pytest

import bgzf_check
import kreport_ref as K
import readsplit_ref as RS
import taxreads_ref as R
from test_gpu_readsplit import _host_text, _indexed_context, world  # noqa: F401  (the fixture and its helpers)

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = 1, 4, 5   # include/kslam.h: kslam_status


@pytest.fixture(scope="module")
def TR(kslam):
    return importlib.import_module("kslam_amd.taxreads")


class _Bench:
    """one context over a one-entry index with the pairing on; the annotations are set again when a case brings another tree"""

    def __init__(self, kslam, TR):
        self.TR, self.tax_text, self.tax = TR, None, None
        self.ST = importlib.import_module("kslam_amd.samtext")
        self.T = importlib.import_module("kslam_amd.tail")
        self.X = importlib.import_module("kslam_amd.taxonomy")
        self.c = kslam.Context()
        bases, off = np.frombuffer(b"ACGT" * 25, dtype=np.uint8), np.array([0, 100], dtype=np.uint64)
        self.c.set_index_arrays(bases, off)
        self.index = self.T.IndexArrays(bases, off, taxonomy_ids=[10])
        self.c.set_pairing(stages=3)

    def tree(self, tax_text):
        if tax_text != self.tax_text:
            self.tax = self.X.TaxDB(tax_text)
            self.ST.set_annotations(self.c, self.index, self.tax)
            assert len(self.TR.get_taxon_reads(self.c)[0]) == 0   # new annotations drop the selection
            self.tax_text = tax_text
        return self.c, self.tax


@pytest.fixture(scope="module")
def bench(kslam, TR):
    b = _Bench(kslam, TR)
    yield b
    b.c.close()


# ---- the mask pass alone ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1000])
def test_mask_equals_restatement(TR, bench, n):
    """every tree shape at n nodes (the chain of 1 000 exercises the depth cap), the chosen-id edge list, all eight modes"""
    for shape, recs in R.trees(n).items():
        tax = K.tax_text(recs)
        ctx, _ = bench.tree(tax)
        tree = K.Tree(tax)
        for name, ids in R.chosen_lists(recs).items():
            for mode in R.MODES:
                TR.set_taxon_reads(ctx, ids, mode)
                got_ids, got_mode = TR.get_taxon_reads(ctx)
                assert got_ids.tolist() == ids and got_mode == mode
                m, unknown, all_nonzero = TR.mask(ctx)
                em, eu, ea = R.mask(tax, ids, mode, tree)
                assert m.tolist() == em.tolist(), (shape, name, mode)
                assert unknown.tolist() == eu and all_nonzero == ea, (shape, name, mode)
    assert TR.kernel_ms(ctx)[0] > 0
    TR.set_taxon_reads(ctx, [], 0)
    assert len(TR.get_taxon_reads(ctx)[0]) == 0


def test_many_chosen_ids(TR, bench):
    """more chosen ids than a workgroup holds, most of them unknown and repeated: the unknown list is sorted and deduplicated"""
    recs = R.forest(300)
    tax = K.tax_text(recs)
    ctx, _ = bench.tree(tax)
    rng = np.random.default_rng(8)
    ids = rng.integers(1, 900, 700).tolist()
    for mode in (0, R.CHILDREN, R.PARENTS, 7):
        TR.set_taxon_reads(ctx, ids, mode)
        m, unknown, all_nonzero = TR.mask(ctx)
        em, eu, ea = R.mask(tax, ids, mode)
        assert m.tolist() == em.tolist() and unknown.tolist() == eu and all_nonzero == ea
        assert len(eu) > 256


# ---- the flag pass and the copy ----

TREE = R.with_root(R.forest(30))
TAX = K.tax_text(TREE)
CHOSEN = [102, 90001]           # 102: a node with children; 90001: an id the tree does not know
KNOWN_NOT_CHOSEN, UNKNOWN_NOT_CHOSEN = 114, 90002


def _mixes(n):
    inside = [i for i in K.Tree(TAX).order if i in R.chosen_set(K.Tree(TAX), CHOSEN, R.CHILDREN)[0]]
    assert len(inside) > 2 and KNOWN_NOT_CHOSEN not in inside
    ends = np.full(n, KNOWN_NOT_CHOSEN, dtype=np.uint32)
    if n:
        ends[0] = ends[-1] = inside[-1]
    return {"all_zero": np.zeros(n, dtype=np.uint32),
            "all_matched": np.array([inside[k % len(inside)] for k in range(n)], dtype=np.uint32),
            "none_matched": np.array([(KNOWN_NOT_CHOSEN, 0, UNKNOWN_NOT_CHOSEN)[k % 3] for k in range(n)], dtype=np.uint32),
            "one_at_each_end": ends,
            "unknown_ids": np.array([(90001, 90002, 0, 90001, 102)[k % 5] for k in range(n)], dtype=np.uint32)}


@pytest.mark.parametrize("single", [False, True], ids=["paired", "single"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_flag_pass_and_copy_equal_the_twin(TR, bench, n, single):
    ctx, tax = bench.tree(TAX)
    r1 = RS.text_of(n, [b"\n", b"\r\n"], n_bases=21)
    r2 = None if single else RS.text_of(n, b"\n", n_bases=17, mate=2)
    records = np.arange(n)
    rp = RS.read_pairs(records, n, paired=not single)
    for mode in (R.CHILDREN, R.CHILDREN | R.EXCLUDE, R.PARENTS):
        TR.set_taxon_reads(ctx, CHOSEN, mode)
        for name, pair_ids in _mixes(n).items():
            host = TR.tail_taxon_reads(tax, CHOSEN, mode, r1, r2, rp, pair_ids)
            dev = TR.taxon_reads_text(ctx, r1, r2, rp, pair_ids)
            assert dev["blocks"] == host["blocks"] and dev["n_records"] == host["n_records"] and dev["flags"] == 0, (name, mode)
            exp, n_exp = R.select(TAX, CHOSEN, mode, r1, r2, records, pair_ids)
            assert dev["blocks"] == exp and dev["n_records"] == n_exp, (name, mode)
    if n:
        _, flag_ms, copy_ms, moved = TR.kernel_ms(ctx)
        assert flag_ms > 0 and copy_ms > 0


def test_pairs_in_any_order_and_fewer_than_records(TR, bench):
    """read pairs name a subset of the records, out of order; the records without a pair go with EXCLUDE"""
    ctx, tax = bench.tree(TAX)
    n = 300
    r1, r2 = RS.text_of(n, n_bases=33), RS.text_of(n, b"\r", n_bases=30, mate=2)
    records = np.random.default_rng(2).permutation(n)[:170]
    rp = RS.read_pairs(records, n)
    pair_ids = R.pair_ids_for(TREE, len(rp), 5, extra=[90001, 90002])
    for mode in R.MODES:
        TR.set_taxon_reads(ctx, CHOSEN, mode)
        dev = TR.taxon_reads_text(ctx, r1, r2, rp, pair_ids)
        exp, n_exp = R.select(TAX, CHOSEN, mode, r1, r2, records, pair_ids)
        assert dev["blocks"] == exp and dev["n_records"] == n_exp
        assert TR.tail_taxon_reads(tax, CHOSEN, mode, r1, r2, rp, pair_ids)["blocks"] == exp


@pytest.mark.parametrize("deflate", [0, 1], ids=["fixed", "dynamic"])
def test_bgzf(kslam, TR, bench, deflate):
    """257 pairs of 150 bases: the selected stream is longer than one member's 65 280 input bytes; an empty stream has no member"""
    Z = importlib.import_module("kslam_amd.bgzf")
    RSm = importlib.import_module("kslam_amd.readsplit")
    ctx, tax = bench.tree(TAX)
    n = 257
    r1, r2 = RS.text_of(n, n_bases=150), RS.text_of(n, b"\r\n", n_bases=150, mate=2)
    rp = RS.read_pairs(np.arange(n), n)
    mixes = _mixes(n)
    Z.set_deflate(ctx, deflate)
    RSm.set_reads_out_bgzf(ctx, True)
    try:
        for mode in (R.CHILDREN, R.CHILDREN | R.EXCLUDE):
            TR.set_taxon_reads(ctx, CHOSEN, mode)
            for name in ("all_matched", "unknown_ids", "all_zero"):
                plain = TR.tail_taxon_reads(tax, CHOSEN, mode, r1, r2, rp, mixes[name])["blocks"]
                dev = TR.taxon_reads_text(ctx, r1, r2, rp, mixes[name])
                assert dev["flags"] == RSm.FLAG_BGZF
                for k in range(2):
                    z = dev["blocks"][k]
                    assert gzip.decompress(z + Z.EOF) == plain[k], (name, mode, k)
                    assert z == Z.compress(ctx, plain[k])   # the host route (kslam_bgzf_compress) writes the same file
                    if deflate == 0:
                        assert bgzf_check.check(z + Z.EOF) == plain[k]
                    if not plain[k]:
                        assert z == b""
        big = TR.tail_taxon_reads(tax, CHOSEN, R.CHILDREN, r1, r2, rp, mixes["all_matched"])["blocks"][0]
        assert len(big) > bgzf_check.MAX_INPUT
    finally:
        RSm.set_reads_out_bgzf(ctx, False)
        Z.set_deflate(ctx, 0)


# ---- real batches through the lanes: the world of tests/test_gpu_readsplit.py ----

def _stream(kslam, TR, world, tmp, tag, lanes, chosen=None, mode=0, env=None, kreport=False, reads_out=False, bgzf=False):
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    ST = importlib.import_module("kslam_amd.samtext")
    RSm = importlib.import_module("kslam_amd.readsplit")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    env = dict(env or {}, KSLAM_LANES=str(lanes))
    os.environ.update(env)
    names = {k: str(tmp / (tag + "." + k)) for k in ("x1", "x2", "kreport", "sam", "per_read", "c1", "c2", "u1", "u2")}
    try:
        c = _indexed_context(kslam, world)
        h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
        tax = X.TaxDB(world["case"]["taxdb"])
        fds = {k: os.open(p, os.O_RDWR | os.O_CREAT | os.O_TRUNC) for k, p in names.items()}
        if chosen is not None:
            ST.set_annotations(c, world["db"], tax)
            c.set_pairing(stages=7)
            TR.set_taxon_reads(c, chosen, mode)
        if bgzf:
            RSm.set_reads_out_bgzf(c, True)
        st = S.classify_stream_native(c, world["db"], h1.ptr, len(r1), h2.ptr, len(r2), 300, T.TailParams.default(paired=True), taxdb=tax,
                                      sam_fd=fds["sam"], per_read_fd=fds["per_read"], sam_header=b"@HD\tVN:1.0\n", depth=3,
                                      kreport_fd=fds["kreport"] if kreport else -1,
                                      reads_out_fds=[fds[k] for k in ("c1", "c2", "u1", "u2")] if reads_out else None,
                                      taxon_reads_fds=[fds["x1"], fds["x2"]] if chosen is not None else None)
        assert len(TR.get_taxon_reads(c)[0]) == 0   # the call switched the selection off again
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


def _per_read_ids(world, per_read):
    """the run's _PerRead lines -> (record numbers, taxonomy ids)"""
    number = {i: k for k, i in enumerate(world["case"]["ids"])}
    lines = [x for x in per_read.split(b"\n") if x]
    return [number[x.split(b"\t")[0]] for x in lines], [int(x.rsplit(b"\t", 1)[1]) for x in lines]


def test_three_batches_through_the_stream(kslam, TR, world, tmp_path):
    KR = importlib.import_module("kslam_amd.kreport")
    tax_text, r1, r2, n = world["case"]["taxdb"], world["case"]["r1"], world["case"]["r2"], world["n"]
    off, st_off = _stream(kslam, TR, world, tmp_path, "off", 1, kreport=True, reads_out=True)
    records, ids = _per_read_ids(world, off["per_read"])
    assert st_off["n_batches"] == 3 and st_off["batches_pseudo_on_host"] == 0 and len(ids) > 100 and off["x1"] == b"" == off["x2"]
    # a species that has reads of its own and below it: the node of the most frequent id's parent
    tree = K.Tree(tax_text)
    common = max(set(ids), key=ids.count)
    chosen = [tree.parent[common] if not tree.top(common) else common]
    exp, n_exp = R.select(tax_text, chosen, R.CHILDREN, r1, r2, records, ids)
    assert 0 < n_exp[0] < n and len(exp[0]) > 1000
    files, st = _stream(kslam, TR, world, tmp_path, "l1", 1, chosen, R.CHILDREN, kreport=True, reads_out=True)
    assert [files["x1"], files["x2"]] == exp
    # next to the report of the same call: the CHILDREN record count is the chosen id's clade count
    row = [x for x in KR.parse_report(files["kreport"]) if x["taxid"] == chosen[0]]
    assert len(row) == 1 and row[0]["clade"] == n_exp[0]
    # every other output is what it is with the switch off (the split and the report included)
    for k in ("kreport", "sam", "per_read", "c1", "c2", "u1", "u2"):
        assert files[k] == off[k] and len(files[k]) > 0, k
    assert st["abbreviated"] == st_off["abbreviated"] and st["tax_ids"].tolist() == st_off["tax_ids"].tolist()
    # alone, the selection gives the same bytes as next to the split and the report
    alone, _ = _stream(kslam, TR, world, tmp_path, "alone", 1, chosen, R.CHILDREN)
    assert [alone["x1"], alone["x2"]] == exp and alone["sam"] == off["sam"] and alone["per_read"] == off["per_read"]
    # three lanes, and every batch by the host's route
    l3, _ = _stream(kslam, TR, world, tmp_path, "l3", 3, chosen, R.CHILDREN)
    assert [l3["x1"], l3["x2"]] == exp
    host, st_host = _stream(kslam, TR, world, tmp_path, "host", 2, chosen, R.CHILDREN, env={"KSLAM_HOST_SAM_TEXT": "1"})
    assert [host["x1"], host["x2"]] == exp and host["per_read"] == off["per_read"]
    # pseudo-assembly left to the host for every batch: no lane made the ids
    left, st_left = _stream(kslam, TR, world, tmp_path, "cap", 2, chosen, R.CHILDREN, env={"KSLAM_PSEUDO_CAP": "3"})
    assert st_left["batches_pseudo_on_host"] == 3 and [left["x1"], left["x2"]] == exp
    # EXCLUDE: everything else, the reads without alignment included
    ex, _ = _stream(kslam, TR, world, tmp_path, "ex", 2, chosen, R.CHILDREN | R.EXCLUDE)
    exp_ex, n_ex = R.select(tax_text, chosen, R.CHILDREN | R.EXCLUDE, r1, r2, records, ids)
    assert [ex["x1"], ex["x2"]] == exp_ex and n_ex[0] == n - n_exp[0] > n // 2
    # BGZF: the batches' members and the EOF marker, the same file by both routes
    z, _ = _stream(kslam, TR, world, tmp_path, "z", 2, chosen, R.CHILDREN, bgzf=True)
    zh, _ = _stream(kslam, TR, world, tmp_path, "zh", 2, chosen, R.CHILDREN, env={"KSLAM_HOST_SAM_TEXT": "1"}, bgzf=True)
    for k in range(2):
        assert bgzf_check.check(z["x%d" % (k + 1)]) == exp[k] and z["x%d" % (k + 1)] == zh["x%d" % (k + 1)]


def test_a_batch_through_the_lanes(kslam, TR, world):
    """submit -> collect -> kslam_collect_taxon_reads: the blocks, once; a batch without the per-read stage is left to the host"""
    ST = importlib.import_module("kslam_amd.samtext")
    X = importlib.import_module("kslam_amd.taxonomy")
    RSm = importlib.import_module("kslam_amd.readsplit")
    L = TR.lib()
    r1, r2, n = world["case"]["r1"], world["case"]["r2"], world["n"]
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    tax = X.TaxDB(world["case"]["taxdb"])
    try:
        c.set_pairing(stages=7)
        ST.set_annotations(c, world["db"], tax)
        tk = c.submit_batch_fastq_text(h1.ptr, len(r1), h2.ptr, len(r2))
        c.collect_batch(tk)[4]()
        ro = RSm.ReadsOut()
        assert L.kslam_collect_taxon_reads(c._h, tk, C.byref(ro)) == ERR_STATE    # the switch was off for that batch
        TR.set_taxon_reads(c, [1], R.CHILDREN)
        tk = c.submit_batch_fastq_text(h1.ptr, len(r1), h2.ptr, len(r2))
        c.collect_batch(tk)[4]()
        got = TR.collect_taxon_reads(c, tk)
        assert got["flags"] == RSm.FLAG_LEFT_TO_HOST and got["blocks"] == [None, None]   # no per-read stage: the ids are the host's
        ST.set_sam_text(c, want_sam=False, want_per_read=True)
        tk = c.submit_batch_fastq_text(h1.ptr, len(r1), h2.ptr, len(r2))
        release = c.collect_batch(tk)[4]
        rp = c.last_pairs[0].copy()
        release()
        got = TR.collect_taxon_reads(c, tk)
        assert got["flags"] == 0 and 0 < got["n_records"][0] <= len(rp) and sum(got["n_records"]) == n
        assert got["blocks"][0].count(b"\n") == 4 * got["n_records"][0] == got["blocks"][1].count(b"\n")
        assert L.kslam_collect_taxon_reads(c._h, tk, C.byref(ro)) == ERR_STATE    # taken already
        # a batch submitted by columns: no text on the device
        case = world["case"]
        cat = np.frombuffer(b"".join(case["bases"]), dtype=np.uint8)
        qcat = np.frombuffer(b"".join(case["quals"]), dtype=np.uint8)
        off = np.zeros(2 * n + 1, dtype=np.uint64)
        np.cumsum([len(b) for b in case["bases"]], out=off[1:])
        ST.set_sam_text(c, want_sam=False, want_per_read=False)
        tk = c.submit_batch_columns(2 * n, cat.ctypes.data, qcat.ctypes.data, off.ctypes.data)
        c.collect_batch(tk)[4]()
        assert L.kslam_collect_taxon_reads(c._h, tk, C.byref(ro)) == ERR_UNSUPPORTED
        assert b"kslam_submit_batch_fastq_text" in c._L.kslam_last_error(c._h)
        # new annotations switch the selection off
        ST.set_annotations(c, world["db"], tax)
        assert len(TR.get_taxon_reads(c)[0]) == 0
    finally:
        c.set_pairing(stages=0)
        c.close()
        h1.close()
        h2.close()


def test_refusals(kslam, TR):
    L = TR.lib()
    ST = importlib.import_module("kslam_amd.samtext")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    RSm = importlib.import_module("kslam_amd.readsplit")
    c = kslam.Context()
    ids = np.array([10, 20], dtype=np.uint32)
    zero = np.array([10, 0], dtype=np.uint32)
    try:
        assert L.kslam_set_taxon_reads(c._h, ids.ctypes.data, 2, 0) == ERR_STATE            # no annotations at all
        assert b"kslam_set_sam_annotations" in c._L.kslam_last_error(c._h)
        bases, off = np.frombuffer(b"ACGT" * 25, dtype=np.uint8), np.array([0, 100], dtype=np.uint64)
        c.set_index_arrays(bases, off)
        index = T.IndexArrays(bases, off, taxonomy_ids=[10])
        ST.set_annotations(c, index, None)
        assert L.kslam_set_taxon_reads(c._h, ids.ctypes.data, 2, 0) == ERR_STATE            # annotations without a tree
        assert b"taxonomy tree" in c._L.kslam_last_error(c._h)
        ST.set_annotations(c, index, X.TaxDB(K.tax_text(K.FIVE)))
        assert L.kslam_set_taxon_reads(c._h, ids.ctypes.data, 2, 0) == ERR_STATE            # the pairing is off
        assert b"kslam_set_pairing" in c._L.kslam_last_error(c._h)
        c.set_pairing(stages=3)
        assert L.kslam_set_taxon_reads(c._h, zero.ctypes.data, 2, 0) == ERR_ARG             # id 0
        assert L.kslam_set_taxon_reads(c._h, ids.ctypes.data, 2, 8) == ERR_ARG              # mode bits above 7
        assert L.kslam_set_taxon_reads(c._h, None, 2, 0) == ERR_ARG
        assert len(TR.get_taxon_reads(c)[0]) == 0
        ro = RSm.ReadsOut()
        r1 = RS.text_of(3)
        rp = RS.read_pairs([0], 3, paired=False)
        assert L.kslam_taxon_reads_text(c._h, r1, len(r1), None, 0, 0, 1, rp.ctypes.data, ids.ctypes.data, 1, C.byref(ro)) == ERR_STATE   # nothing chosen
        m, n, u, nu, a = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64(), C.c_int()
        assert L.kslam_taxon_reads_mask(c._h, C.byref(m), C.byref(n), C.byref(u), C.byref(nu), C.byref(a)) == ERR_STATE
        assert L.kslam_set_taxon_reads(c._h, ids.ctypes.data, 2, 7) == 0
        assert TR.get_taxon_reads(c)[0].tolist() == [10, 20]
        assert L.kslam_set_taxon_reads(c._h, None, 0, 99) == 0                              # n == 0: off, whatever the mode says
        assert len(TR.get_taxon_reads(c)[0]) == 0
    finally:
        c.set_pairing(stages=0)
        c.close()
    m = kslam.MultiContext([0])
    try:
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)   # (tests/test_gpu_readsplit.py: the first context)
        assert L.kslam_set_taxon_reads(h, ids.ctypes.data, 2, 0) == ERR_UNSUPPORTED
        assert L.kslam_stream_set_taxon_reads(h, None) == ERR_UNSUPPORTED
    finally:
        m.close()


def test_the_stream_needs_a_tree_and_chosen_ids(kslam, TR, world, tmp_path):
    S = importlib.import_module("kslam_amd.stream")
    T = importlib.import_module("kslam_amd.tail")
    X = importlib.import_module("kslam_amd.taxonomy")
    r1, r2 = world["case"]["r1"], world["case"]["r2"]
    c = _indexed_context(kslam, world)
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    fd = os.open(str(tmp_path / "none.fq"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    try:
        for taxdb in (None, X.TaxDB(world["case"]["taxdb"])):   # no tree; a tree, but nothing chosen
            with pytest.raises(kslam.KslamError) as e:
                S.classify_stream_native(c, world["db"], h1.ptr, len(r1), h2.ptr, len(r2), 300, T.TailParams.default(paired=True), taxdb=taxdb,
                                         taxon_reads_fds=[fd, -1])
            assert e.value.status == ERR_STATE
        assert os.fstat(fd).st_size == 0
    finally:
        os.close(fd)
        c.close()
        h1.close()
        h2.close()
