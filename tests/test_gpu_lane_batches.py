"""The lane worker's bookkeeping (csrc/api_lanes.hip) on the smallest batches there are -- tests/ragged_world.py's ordinary batch of
64 pairs, its batch of one pair and its empty batch (64 pairs from nowhere): every page-locked block a batch takes goes back whichever way the batch
ends (kslam_debug_pinned_in_use counts the blocks marked in use on the context and its lanes), the four forms of a batch --
pointers, columns, FASTQ fields, FASTQ text -- give the same arrays, and a batch that fails leaves the batches before and after
it on the same context as they are alone.

kslam_wait_batch hands overlaps and CIGAR pool to the caller and everything else of the batch back.  Until it did so through
kslam_release_batch it left the SAM text, the per-read lines and the taxonomy ids of a batch marked in use:
test_no_block_stays_in_use[wait-*] counted 9 blocks after its three waited batches, on one lane and on two, and counts 0 now."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import ragged_world as W
from test_gpu_readsplit import _host_text, _indexed_context

pytestmark = pytest.mark.gpu
THR = W.SCORE_THRESHOLD
ERR_ARG, ERR_UNSUPPORTED = 1, 4                        # include/kslam.h: kslam_status
LONG_READ = [b"ACGT" * 2500]                           # tests/test_gpu_parity.py: 10 000 bases, beyond the supported 9 000
ARRAYS = ("ov", "cg", "det", "md", "rp", "pr", "stats")
EMPTY = "nowhere"                                      # the world's empty batch: 64 pairs, no overlap record, no read pair
KINDS = ("ordinary", "single", EMPTY)


@pytest.fixture(scope="module")
def rw(kslam, synth, tmp_path_factory):
    """the ragged world, its database loaded, the three batches"""
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    world = W.make(synth)
    tmp = tmp_path_factory.mktemp("lane_batches")
    RL.write_case(W.case_of(world, ["single"]), tmp, D)
    db = D.Database.load(os.path.join(str(tmp), "db", "database"))
    cases = {k: W.case_of(world, [k]) for k in KINDS}
    bad = dict(cases["ordinary"])                      # tests/test_gpu_ragged_stream.py's malformed record: one without its "+" line
    plus = bad["r1"].index(b"\n+\n", bad["r1"].index(b"@ordinary011/1"))
    bad["r1"] = bad["r1"][:plus] + bad["r1"][plus + 2:]
    cases["malformed"] = bad
    return {"world": world, "db": db, "cases": cases}


class Lanes:
    """a context on the world's index with the device pairing at stages = 7 and, with text=True, kslam_set_sam_text(sam, per_read)"""

    def __init__(self, kslam, rw, monkeypatch, lanes, text=True):
        monkeypatch.setenv("KSLAM_LANES", str(lanes))
        self.K, self.rw, self.keep = kslam, rw, []
        self.F, self.RS = importlib.import_module("kslam_amd.fastq"), importlib.import_module("kslam_amd.readsplit")
        self.c = _indexed_context(kslam, rw, score_threshold=THR)
        self.c.set_pairing(paired=True, score_threshold=THR, stages=7)
        self.tax = None
        if text:
            ST = importlib.import_module("kslam_amd.samtext")
            self.tax = importlib.import_module("kslam_amd.taxonomy").TaxDB(rw["world"]["taxdb"])
            ST.set_annotations(self.c, rw["db"], self.tax)
            ST.set_sam_text(self.c, True, True)

    def close(self):
        self.c.close()
        if self.tax is not None:
            self.tax.close()
        for k in self.keep:
            if hasattr(k, "close"):
                k.close()

    def in_use(self):
        return self.c.debug_pinned_in_use()

    def submit(self, case, form, quals=True):
        """one batch in one of the four forms -> ticket; what the library borrows lives until close()"""
        c, bases, n = self.c, case["bases"], len(case["bases"])
        if form == "pointers":
            return self.submit_reads(bases, case["quals"] if quals else None)
        if form == "columns":
            cat, qcat = (np.frombuffer(b"".join(x) + bytes(64), dtype=np.uint8) for x in (bases, case["quals"]))
            off = np.zeros(n + 1, dtype=np.uint64)
            np.cumsum([len(b) for b in bases], out=off[1:])
            self.keep += [cat, qcat, off]
            return c.submit_batch_columns(n, cat.ctypes.data, qcat.ctypes.data, off.ctypes.data)
        h1, h2 = _host_text(self.K, case["r1"]), _host_text(self.K, case["r2"])
        self.keep += [h1, h2]
        if form == "text":
            return c.submit_batch_fastq_text(h1.ptr, len(case["r1"]), h2.ptr, len(case["r2"]))
        assert form == "fields"
        ix, v1, v2 = self.F.index_pair(h1.ptr, len(case["r1"]), h2.ptr, len(case["r2"]))
        assert (v1, v2, ix.n_reads) == (len(case["r1"]), len(case["r2"]), n)
        self.keep.append(ix)
        return c.submit_batch_fastq(h1.ptr, len(case["r1"]), h2.ptr, len(case["r2"]), n, ix._cols.bases_off, ix.layout.bases_at, ix.layout.quality_at)

    def submit_reads(self, bases, quals=None):
        """kslam_submit_batch: the reads are copied before it returns"""
        def pointers(items):
            kept = [C.create_string_buffer(b, len(b) + 1) for b in items]
            return kept, C.cast((C.c_char_p * len(items))(*[C.cast(x, C.c_char_p) for x in kept]), C.c_void_p)
        lens = np.array([len(b) for b in bases], dtype=np.uint32)
        kb, bp = pointers(bases)
        kq, qp = pointers(quals) if quals is not None else (None, None)
        return self.c.submit_batch_full(len(bases), bp, qp, lens.ctypes.data)

    def collect(self, ticket):
        """kslam_collect_batch -> every field as bytes / numbers (copies), the batch released"""
        c, K = self.c, self.K
        r = K.BatchResult()
        c._chk(c._L.kslam_collect_batch(c._h, ticket, C.byref(r)))
        try:
            def raw(ptr, nbytes):
                return C.string_at(ptr, int(nbytes)) if ptr and nbytes else b""
            n = int(r.n_reads)
            got = {"ov": raw(r.overlaps, r.n_overlaps * K.OVERLAP_DT.itemsize), "cg": raw(r.cigar_pool, r.n_cigar * 4),
                   "det": raw(r.details, r.n_overlaps * K.ROW_DETAIL_DT.itemsize), "md": raw(r.md_pool, r.n_md),
                   "rp": raw(r.read_pairs, r.n_read_pairs * K.READ_PAIR_DT.itemsize), "pr": raw(r.pairs, r.n_pairs * K.PAIRED_OVERLAP_DT.itemsize),
                   "stats": r.pair_stats.as_dict(), "counts": (int(r.n_overlaps), int(r.n_cigar), int(r.n_md), int(r.n_read_pairs), int(r.n_pairs)),
                   "n_reads": n, "consumed": (int(r.consumed1), int(r.consumed2)), "flags": int(r.text_flags),
                   "sam": raw(r.sam_text, r.sam_text_len), "per_read": raw(r.per_read_text, r.per_read_len), "tax": raw(r.tax_ids, 4 * r.n_read_pairs),
                   "bases_off": np.frombuffer(raw(r.reads_bases_off, 8 * (n + 1)), dtype=np.uint64).tolist(),
                   "ids_off": np.frombuffer(raw(r.reads_ids_off, 8 * (n + 1)), dtype=np.uint64).tolist()}
            got["ids"] = raw(r.reads_ids, got["ids_off"][n] if got["ids_off"] else 0)
        finally:
            c._L.kslam_release_batch(c._h, C.byref(r))
        return got

    def wait(self, ticket):
        """kslam_wait_batch, the two arrays it returns handed back with kslam_free_batch -> (n_overlaps, n_cigar)"""
        c = self.c
        po, pc, no, nc = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        c._chk(c._L.kslam_wait_batch(c._h, ticket, C.byref(po), C.byref(no), C.byref(pc), C.byref(nc)))
        c._L.kslam_free_batch(c._h, po, pc)
        return int(no.value), int(nc.value)


@pytest.fixture
def lanes_of(kslam, rw, monkeypatch):
    made = []

    def make(lanes, text=True):
        made.append(Lanes(kslam, rw, monkeypatch, lanes, text))
        return made[-1]
    yield make
    for x in made:
        x.close()


# ---- 1. no block stays in use ----

def _collect_release(L, cases):
    for kind in KINDS:
        got = L.collect(L.submit(cases[kind], "text"))
        assert got["n_reads"] == 2 * cases[kind]["n_pairs"] and (len(got["sam"]) > 0) == (kind != EMPTY)


def _wait(L, cases):
    for kind in KINDS:
        L.collect(L.submit(cases[kind], "text"))
        n_out, _ = L.wait(L.submit(cases[kind], "text"))
        assert (n_out > 0) == (kind != EMPTY)


def _fails_in_load(L, cases):
    with pytest.raises(L.K.KslamError) as e:
        L.collect(L.submit(cases["malformed"], "text"))
    assert e.value.status == ERR_ARG


def _fails_between_good_batches(L, cases):
    """the 10 000-base read through the pointer form (refused where the batch's reads are measured, in front of the kernels)"""
    tickets = [L.submit(cases["ordinary"], "pointers"), L.submit_reads(LONG_READ), L.submit(cases["single"], "pointers")]
    assert len(L.collect(tickets[0])["ov"]) > 0
    with pytest.raises(L.K.KslamError, match="9000") as e:
        L.collect(tickets[1])
    assert e.value.status == ERR_UNSUPPORTED
    assert len(L.collect(tickets[2])["ov"]) > 0


def _pointers_with_and_without_qualities(L, cases):
    for kind in KINDS:
        with_q, without = L.collect(L.submit(cases[kind], "pointers")), L.collect(L.submit(cases[kind], "pointers", quals=False))
        assert (len(with_q["det"]) > 0) == (kind != EMPTY) and without["det"] == b"" and len(without["ov"]) == len(with_q["ov"])


def _reads_out_collected(L, cases):
    L.RS.set_reads_out(L.c, 3)
    tk = L.submit(cases["ordinary"], "text")
    L.collect(tk)
    ro = L.RS.collect_reads_out(L.c, tk)               # (copies the blocks and frees them)
    assert ro["flags"] == 0 and sum(len(b) for b in ro["blocks"]) > 0


WAYS = {"collect_release": _collect_release, "wait": _wait, "fails_in_load": _fails_in_load, "fails_between_good_batches": _fails_between_good_batches,
        "pointers_with_and_without_qualities": _pointers_with_and_without_qualities, "reads_out_collected": _reads_out_collected}


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("way", sorted(WAYS))
def test_no_block_stays_in_use(rw, lanes_of, way, lanes):
    """pairing on, kslam_set_sam_text(sam, per_read) on: whichever way a batch ends, no page-locked block of the context or of a lane
    stays marked in use.  (kslam_set_reads_out and kslam_set_taxon_reads stay off but for the one case that collects the split:
    their *_ready maps hold blocks by design.)  way = wait counted 9 blocks, 3 per waited batch, before kslam_wait_batch released the batch."""
    L = lanes_of(lanes)
    assert L.in_use() == 0
    WAYS[way](L, rw["cases"])
    n = L.in_use()
    print(way, lanes, "blocks in use:", n)
    assert n == 0


# ---- 2. the four forms agree ----

@pytest.mark.parametrize("kind", KINDS)
def test_the_four_forms_agree(rw, lanes_of, kind):
    """the same batch as pointers, columns, FASTQ fields and FASTQ text: overlaps, CIGAR pool, row details, MD pool, read pairs,
    alignment pairs and pair statistics are equal byte for byte; the text form's identifiers and offsets are the input's"""
    L, case = lanes_of(2, text=False), rw["cases"][kind]
    got = {form: L.collect(L.submit(case, form)) for form in ("pointers", "columns", "fields", "text")}
    for form in ("columns", "fields", "text"):
        for f in ARRAYS + ("counts",):
            assert got[form][f] == got["pointers"][f], (form, f)
    one = got["pointers"]
    if kind == EMPTY:
        assert one["counts"] == (0, 0, 0, 0, 0) and all(one[f] == b"" for f in ARRAYS[:-1])
    else:
        assert all(len(one[f]) > 0 for f in ARRAYS[:-1]) and one["stats"]["stages_done"] & 7 == 7
    text, ids = got["text"], case["ids"] * 2
    assert text["n_reads"] == len(case["bases"]) and text["consumed"] == (len(case["r1"]), len(case["r2"]))
    assert text["bases_off"] == np.cumsum([0] + [len(b) for b in case["bases"]]).tolist()
    assert text["ids_off"] == np.cumsum([0] + [len(i) for i in ids]).tolist() and text["ids"] == b"".join(ids)
    assert all(got[form]["n_reads"] == 0 and got[form]["ids"] == b"" for form in ("pointers", "columns", "fields"))
    assert L.in_use() == 0


# ---- 3. a failed batch leaves its neighbours whole ----

@pytest.fixture(scope="module")
def alone(kslam, rw):
    """the good batches, each the only batch of a context of its own: (kind, form) -> the collected batch"""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for kind, form in (("ordinary", "text"), ("single", "text"), ("ordinary", "pointers"), ("single", "pointers")):
            L = Lanes(kslam, rw, mp, 1)
            try:
                out[(kind, form)] = L.collect(L.submit(rw["cases"][kind], form))
            finally:
                L.close()
    finally:
        mp.undo()
    return out


FAILING = {"malformed": ("text", ERR_ARG, "quality line is not as long as its bases line"),
           "long_read": ("pointers", ERR_UNSUPPORTED, "reads longer than 9000 bases are not supported (read 0 of the batch has 10000)")}


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("what", sorted(FAILING))
def test_a_failed_batch_leaves_its_neighbours_whole(rw, lanes_of, alone, what, lanes):
    """good, failing, good on one context, all three in flight: the good batches are what they are alone (SAM text, per-read
    lines and taxonomy ids included), the failing ticket gives its status and message once and "no such ticket" after that"""
    form, status, message = FAILING[what]
    L, cases = lanes_of(lanes), rw["cases"]
    before = L.submit(cases["ordinary"], form)
    failing = L.submit(cases["malformed"], "text") if what == "malformed" else L.submit_reads(LONG_READ)
    after = L.submit(cases["single"], form)
    assert L.collect(after) == alone[("single", form)]
    with pytest.raises(L.K.KslamError) as e:
        L.collect(failing)
    print(what, e.value.status, str(e.value))
    assert e.value.status == status and message in str(e.value)
    with pytest.raises(L.K.KslamError, match="no such ticket") as e:
        L.collect(failing)
    assert e.value.status == ERR_ARG
    got = L.collect(before)
    assert got == alone[("ordinary", form)] and len(got["rp"]) > 0
    assert (len(got["sam"]) > 0 and len(got["per_read"]) > 0 and got["ov"] == b"") if form == "text" else (len(got["ov"]) > 0 and got["sam"] == b"")
    assert L.in_use() == 0
