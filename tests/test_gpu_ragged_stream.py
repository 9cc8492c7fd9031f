"""The batch loop (host/stream.cpp), the lane worker (csrc/api_lanes.hip) and every output at once on the ragged world of
tests/ragged_world.py: batches without an overlap record, without a surviving read pair, without a proper pair, with exactly one,
of one pair -- first each kind alone through a lane, then the three orders through kslam_stream_classify on every route and in
every form of the SAM file, then the calls that fail in the middle and what the next call on the same context writes.

Every expected byte is tests/ragged_expect.py's: the oracle chain batch by batch for SAM, per-read lines, taxonomy ids, the XML
report and the summary, tests/samseq_rules.py and tests/unmapped_rules.py for SEQ / QUAL and the rows of the reads without
alignment (both switches are on in every run), each report's plain-Python restatement for the ten opt-in outputs.  The arrays
the restatements read are the oracle's; test_the_python_loop_hands_back_the_oracles_arrays holds the arrays the lanes return to
them first, and the restatements give the same files on either.

Additive outputs (ragged_expect.ADDITIVE: coverage, genes, VCF, consensus, alignment QC, depth, the classified reads and the
reads of chosen taxa): an empty batch leaves them as the same call writes them with that batch's reads taken out of the FASTQ
text.  Not additive: the read QC report (it counts every read that comes in), the unclassified reads and the Kraken-style report
(both count the pairs read); and the SAM, per-read and XML outputs, which the reads without alignment or the batch's own
insert-size limit feed."""
import ctypes as C
import importlib
import os
import signal
import threading

import numpy as np
import pytest

import alignqc_ref
import bgzf_check
import consensus_ref
import depth_ref
import ragged_expect as E
import ragged_world as W
import readqc_ref
import unmapped_check as UC
import variants_ref
from test_gpu_readsplit import _host_text, _indexed_context
from test_gpu_stream_reports import OUTPUTS, _assert_put_away, _call, _modules
from test_samseq_host import cigar_star

pytestmark = pytest.mark.gpu
THR = W.SCORE_THRESHOLD
EOL2 = b"\r\n"                           # R2 with CRLF line ends: the splits write LF
ERR_ARG = 1                              # include/kslam.h: kslam_status
TEXT_FLAGS = 1 | 2 | 4 | 32 | 64         # KSLAM_TEXT_PAIRS_SORTED | _SAM | _PER_READ | _SAM_SEQ | _SAM_UNMAPPED
REPORT_FILES = ["coverage", "genes", "kreport", "vcf", "fasta", "read_qc", "align_qc", "bedgraph"]   # in the order they are finished
SPLIT_FILES = ["c1", "c2", "u1", "u2", "x1", "x2"]
OVERLAP_FIELDS = ("read", "entry", "rel", "revcomp", "score", "ref_begin", "ref_end", "query_begin", "query_end")


@pytest.fixture(scope="module")
def rw(kslam, oracle, synth, tmp_path_factory):
    """the world, its database loaded, the taxon chosen for the selected reads (the most frequent id of the first order)"""
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    world = W.make(synth)
    tmp = tmp_path_factory.mktemp("ragged")
    RL.write_case(W.case_of(world, ["single"]), tmp, D)
    db = D.Database.load(os.path.join(str(tmp), "db", "database"))
    ids = [t for k in W.ORDERS["plain"] for t in W.chain_batch(oracle, world, k)["tax"]]
    return {"world": world, "db": db, "case": {"taxdb": world["taxdb"]}, "chosen": [max(set(ids), key=ids.count)],
            "source": kslam.lib().kslam_version().split()[0], "memo": {}}


def _expected(oracle, rw, kinds, paired=True, without=()):
    key = (tuple(kinds), paired, tuple(without))
    if key not in rw["memo"]:
        rw["memo"][key] = E.files(oracle, rw["world"], kinds, paired, without, eol2=EOL2, chosen=rw["chosen"], source=rw["source"])
    return rw["memo"][key]


def _more_modules():
    return {k: importlib.import_module("kslam_amd." + k) for k in ("samseq", "samunmapped", "bgzf", "bam")}


def _texts(kslam, case, paired=True):
    h1 = _host_text(kslam, case["r1"])
    h2 = _host_text(kslam, case["r2"]) if paired else None
    return ((h1, len(case["r1"])), (h2, len(case["r2"]) if paired else 0))


def _close(texts):
    for h, _ in texts:
        if h is not None:
            h.close()


def _context(kslam, rw, X, seq=True, unmapped=True):
    """a context on the world's index whose aligner screens at the run's score threshold, SEQ / QUAL and the rows of the reads
    without alignment switched on"""
    c = _indexed_context(kslam, rw, score_threshold=THR)
    X["samseq"].set_sam_seq(c, seq)
    X["samunmapped"].set_sam_unmapped(c, unmapped)
    return c


def _params(M, paired=True):
    return M["tail"].TailParams.default(paired=paired, score_threshold=THR)


# ---- one lane batch at a time: the narrowest run, first in the file ----

@pytest.fixture(scope="module")
def lane(kslam, rw):
    """one context for the tests that arm everything by hand (_arm)"""
    M, X = _modules(), _more_modules()
    tax = M["taxonomy"].TaxDB(rw["world"]["taxdb"])
    c = _context(kslam, rw, X)
    yield M, c, tax
    c.close()
    tax.close()


def _arm(M, c, rw, tax):
    """the pairing at stages = 7, the SAM text, the per-read stage and every report switched on and empty (switching on what is on
    changes nothing; kslam_stream_classify leaves everything off)"""
    c.set_pairing(paired=True, score_threshold=THR, stages=7)
    M["coverage"].set_coverage(c, True)
    M["variants"].set_variants(c, True)
    M["consensus"].set_consensus(c, True)
    M["depth"].set_depth(c, True)
    M["readqc"].set_read_qc(c, True, E.PARAMS["read_qc_max_cycles"])
    M["alignqc"].set_align_qc(c, True, E.PARAMS["align_qc_max_cycles"])
    M["samtext"].set_annotations(c, rw["db"], tax)     # (they drop the gene table, the Kraken report and the chosen taxa: those go behind)
    M["samtext"].set_sam_text(c, True, True)
    M["genes"].set_genes(c, True)
    M["kreport"].set_kreport(c, True)
    M["taxreads"].set_taxon_reads(c, rw["chosen"], E.TAXON_MODE)
    M["readsplit"].set_reads_out(c, 3)
    for name in ("coverage", "variants", "consensus", "depth", "readqc", "alignqc", "genes", "kreport"):
        M[name].reset(c)


def _taken_reports(M, c, rw, tax, n_pairs):
    """every report's take, through its writer -> {file: bytes}"""
    db, P = rw["db"], E.PARAMS
    out = {}
    rows, skipped = M["coverage"].take(c)
    assert skipped == 0
    out["coverage"] = M["coverage"].report_bytes(db, rows)
    rows, st = M["genes"].take(c)
    assert st["n_skipped"] == 0
    out["genes"] = M["genes"].table_bytes(db, rows)
    rows, st = M["kreport"].take(c)
    out["kreport"] = M["kreport"].report_bytes(tax, rows, n_pairs)
    rows, st = M["variants"].take(c, P["variants_min_alt"], P["variants_min_depth"])
    assert st["n_skipped"] == 0
    out["vcf"] = M["variants"].report_bytes(db, rows, st)
    rows, seq, st = M["consensus"].take(c, *P["consensus_params"])
    out["fasta"] = M["consensus"].report_bytes(db, rows, seq)
    out["read_qc"] = M["readqc"].report_bytes(M["readqc"].take(c))
    out["align_qc"] = M["alignqc"].report_bytes(M["alignqc"].take(c))
    rows, st = M["depth"].take(c, P["depth_min"])
    out["bedgraph"] = M["depth"].report_bytes(db, rows)
    return out


@pytest.mark.parametrize("kind", W.KINDS)
def test_one_lane_batch_of_each_kind(kslam, oracle, rw, lane, kind):
    """kslam_submit_batch_fastq_text -> kslam_collect_batch with everything armed, one batch kind alone: its counts, text_flags, SAM
    and per-read bytes, taxonomy ids, both read splits, and every report's take are the kind's expectations"""
    M, c, tax = lane
    b = W.chain_batch(oracle, rw["world"], kind)
    exp, facts = _expected(oracle, rw, [kind])
    case = facts["case"]
    _arm(M, c, rw, tax)
    texts = _texts(kslam, case)
    r = kslam.BatchResult()
    try:
        tk = c.submit_batch_fastq_text(texts[0][0].ptr, texts[0][1], texts[1][0].ptr, texts[1][1])
        c._chk(c._L.kslam_collect_batch(c._h, tk, C.byref(r)))
        counts = (int(r.n_reads), int(r.n_overlaps), int(r.n_read_pairs), int(r.consumed1), int(r.consumed2))
        stats, flags = r.pair_stats.as_dict(), int(r.text_flags)
        sam = C.string_at(r.sam_text, r.sam_text_len) if r.sam_text_len else b""
        per_read = C.string_at(r.per_read_text, r.per_read_len) if r.per_read_len else b""
        ids = np.frombuffer(C.string_at(r.tax_ids, 4 * r.n_read_pairs), dtype=np.uint32).tolist() if r.n_read_pairs else []
        ro = M["readsplit"].collect_reads_out(c, tk)
        tr = M["taxreads"].collect_taxon_reads(c, tk)
    finally:
        c._L.kslam_release_batch(c._h, C.byref(r))
        _close(texts)
    print(kind, counts, stats, flags)
    assert counts == (2 * b["n"], len(b["ov"]), len(b["rp"]), len(case["r1"]), len(case["r2"]))
    assert stats["stages_done"] & 7 == 7 and stats["n_read_pairs"] == len(b["rp"])
    assert (stats["n_overlaps_screened"], stats["n_insert_sizes"], stats["max_insert_size"]) == \
        (b["st"]["n_overlaps_screened"], b["st"]["n_insert_sizes"], b["st"]["max_insert_size"])
    assert flags == TEXT_FLAGS
    assert sam == E.sam_of_batch(b) and per_read == b["per_read"] and ids == b["tax"]
    assert ro["flags"] == 0 and ro["blocks"] == [exp[f] for f in OUTPUTS["reads_out"]]
    assert tr["flags"] == 0 and tr["blocks"] == [exp[f] for f in OUTPUTS["taxon_reads"]]
    got = _taken_reports(M, c, rw, tax, b["n"])
    for f in REPORT_FILES:
        assert got[f] == exp[f], (kind, f)


# ---- the arrays the restatements read ----

def _compacted(rp, pr):
    """the device leaves the records where they are when the second screen shrinks a group; the oracle hands the survivors back
    packed (tests/test_gpu_tail.py)"""
    cnt = rp["count"].astype(np.int64)
    starts = np.cumsum(cnt) - cnt
    idx = np.repeat(rp["first"].astype(np.int64) - starts, cnt) + np.arange(int(cnt.sum()))
    out = rp.copy()
    out["first"] = starts
    return out, pr[idx]


def _pair_fields(pr):
    return [tuple(int(p[f]) for f in ("combined_score", "entry", "ref_start", "ref_end", "insert_size", "r1", "r2")) for p in pr]


def test_the_python_loop_hands_back_the_oracles_arrays(kslam, oracle, rw, tmp_path):
    """classify_stream (the same lanes, the host's SAM text): batch by batch the overlap records, their CIGARs, the final read
    pairs and alignment pairs and the insert-size limit are the oracle's for that batch -- as the lane returned them
    (before_batch) exactly, after the host stage (on_batch) up to the order writeSAMOutputPairs' sort leaves a read pair's records
    in -- and the restatements write the same files from the arrays of on_batch as from the oracle's"""
    M, X = _modules(), _more_modules()
    kinds = W.ORDERS["plain"]
    exp, facts = _expected(oracle, rw, kinds)
    texts = _texts(kslam, facts["case"])
    (h1, n1), (h2, n2) = texts
    tax = M["taxonomy"].TaxDB(rw["world"]["taxdb"])
    c = _context(kslam, rw, X, seq=False, unmapped=False)
    before, after = [], []
    names = [str(tmp_path / n) for n in ("py.sam", "py.per_read")]
    fds = [os.open(p, os.O_RDWR | os.O_CREAT | os.O_TRUNC) for p in names]
    header = W.sam_header(oracle, rw["world"])
    try:
        res = M["stream"].classify_stream(
            c, rw["db"], h1.ptr, n1, h2.ptr, n2, W.PAIRS_PER_BATCH, _params(M), taxdb=tax, sam_fd=fds[0], per_read_fd=fds[1], sam_header=header,
            before_batch=lambda k, ov, cg, det, md, rp, pr, pst, reads: before.append((k, np.array(ov), np.array(cg), np.array(rp), np.array(pr), dict(pst))),
            on_batch=lambda rec, ov, cg, rp, pr, reads: after.append((rec["batch"], np.array(ov), np.array(cg), np.array(rp), np.array(pr))))
    finally:
        for fd in fds:
            os.close(fd)
        c.close()
        tax.close()
        _close(texts)
    recs = sorted(res["batches"], key=lambda x: x["batch"])
    assert [x["pairs"] for x in recs] == facts["plan"] == W.plan(rw["world"], kinds)
    assert [x["max_insert_size"] for x in recs] == facts["limits"]
    assert res["tax_ids"].tolist() == facts["tax_ids"]
    batches = [W.chain_batch(oracle, rw["world"], k) for k in kinds]
    assert open(names[0], "rb").read() == header + b"".join(b["sam"] for b in batches)
    assert open(names[1], "rb").read() == exp["per_read"]
    before.sort(key=lambda x: x[0])
    after.sort(key=lambda x: x[0])
    assert len(before) == len(after) == len(batches)
    for b, (_, ov, cg, rp, pr, pst), (_, ov2, cg2, rp2, pr2) in zip(batches, before, after):
        assert len(ov) == len(b["ov"]) and pst["max_insert_size"] == b["st"]["max_insert_size"] and pst["stages_done"] & 7 == 7, b["kind"]
        for f in OVERLAP_FIELDS:
            assert ov[f].tolist() == b["ov"][f].tolist(), (b["kind"], f)
        # the lanes walk the CIGAR of the records the final pairs name and of no other (the pairing runs in front of the CIGAR
        # stage): those are the CIGARs every output reads
        named = {int(i) for f in ("r1", "r2") for i in b["pr"][f] if int(i) != 0xFFFFFFFF}
        for i, (o, e) in enumerate(zip(ov, b["ov"])):
            if i in named:
                assert int(o["cigar_len"]) == int(e["cigar_len"]), (b["kind"], i)
                assert cg[int(o["cigar_off"]):int(o["cigar_off"]) + int(o["cigar_len"])].tolist() == \
                    b["pool"][int(e["cigar_off"]):int(e["cigar_off"]) + int(e["cigar_len"])].tolist()
            else:
                assert int(o["cigar_len"]) in (0, int(e["cigar_len"])), (b["kind"], i)
        crp, cpr = _compacted(rp, pr)
        assert crp.tolist() == b["rp"].tolist() and _pair_fields(cpr) == _pair_fields(b["pr"]), b["kind"]
        assert ov2.tobytes() == ov.tobytes() and cg2.tobytes() == cg.tobytes()
        crp2, cpr2 = _compacted(rp2, pr2)
        assert crp2.tolist() == b["rp"].tolist()
        for g in crp2:
            lo, hi = int(g["first"]), int(g["first"]) + int(g["count"])
            assert sorted(_pair_fields(cpr2[lo:hi])) == sorted(_pair_fields(b["pr"][lo:hi])), b["kind"]
    again, _ = E.files(oracle, rw["world"], kinds, eol2=EOL2, chosen=rw["chosen"], source=rw["source"], arrays=[x[1:] for x in after])
    for f in ("coverage", "genes", "vcf", "fasta", "align_qc", "bedgraph"):
        assert again[f] == exp[f], f


# ---- the stream: one call, every output armed ----

ROUTES = {"l1": {"KSLAM_LANES": "1"}, "l3": {"KSLAM_LANES": "3"}, "host_text": {"KSLAM_LANES": "2", "KSLAM_HOST_SAM_TEXT": "1"},
          "host_pseudo": {"KSLAM_LANES": "2", "KSLAM_PSEUDO_CAP": "3"}}
# (the two host routes of tests/test_gpu_stream.py; at a cap of 3 alignment pairs per entry the device hands the ordinary and the
# one-mate batch back, the batches without a read pair never)
RUNS = [(order, route, "text", True) for order in sorted(W.ORDERS) for route in ("l1", "l3")] + \
       [("plain", "host_text", "text", True), ("plain", "host_pseudo", "text", True), ("plain", "l3", "bgzf", True), ("plain", "l3", "bam", True),
        ("plain", "l3", "text", False)]


def _run(kslam, oracle, rw, tmp, tag, kinds, form="text", paired=True, without=(), case=None, instead=None, ctx=None, report=None):
    """one kslam_stream_classify over `kinds` with every output armed -> (files, statistics, expected files, facts).  case: other
    texts than the kinds' (the failing calls); ctx: (context, taxonomy tree) of an earlier call to run on"""
    M, X = _modules(), _more_modules()
    exp, facts = _expected(oracle, rw, kinds, paired, without)
    texts = _texts(kslam, case or facts["case"], paired)
    c, tax = ctx if ctx is not None else (_context(kslam, rw, X), M["taxonomy"].TaxDB(rw["world"]["taxdb"]))
    X["bgzf"].set_sam_bgzf(c, form == "bgzf")
    X["bam"].set_sam_bam(c, form == "bam")
    header = W.sam_header(oracle, rw["world"], W.COMMAND_LINE if paired else b"SLAM --db db R1.fq")
    try:
        files, st = _call(M, c, rw, texts, tax, tmp, tag, list(OUTPUTS), rw["chosen"], per_batch=W.PAIRS_PER_BATCH, params=_params(M, paired),
                          header=header, report=report, instead=instead)
        _assert_put_away(M, c)
    finally:
        _close(texts)
        if ctx is None:
            c.close()
            tax.close()
    return files, st, exp, facts


def _assert_files(files, exp, form="text", names=None):
    for f in names if names is not None else files:
        if f == "sam" and form == "bgzf":
            assert bgzf_check.check(files[f]) == exp[f]
        elif f == "sam" and form == "bam":
            head = exp[f][:len(exp[f]) - len(_rows(exp[f]))]
            assert UC.check(files[f]) == head + cigar_star(_rows(exp[f]))
        else:
            assert files[f] == exp[f], f


def _rows(sam):
    return b"".join(line + b"\n" for line in sam.split(b"\n")[:-1] if not line.startswith(b"@"))


@pytest.mark.parametrize("order,route,form,paired", RUNS, ids=["%s-%s-%s-%s" % (o, r, f, "paired" if p else "single_end") for o, r, f, p in RUNS])
def test_every_output_of_one_call(kslam, oracle, rw, tmp_path, monkeypatch, order, route, form, paired):
    from test_taxonomy import _xml_restatement
    M = _modules()
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    report = M["taxonomy"].Report()
    files, st, exp, facts = _run(kslam, oracle, rw, tmp_path, "run", W.ORDERS[order], form, paired, report=report)
    tax = M["taxonomy"].TaxDB(rw["world"]["taxdb"])
    try:
        xml = tax.report_xml(report, rw["db"], rw["db"].gene_extras(), st["n_pairs"])
        ents = rw["world"]["entries"]
        genes = [[{"start": g["start"], "stop": g["stop"], "name": g["geneName"], "protein": g["proteinID"], "product": g["product"],
                   "locus": g["locusTag"], "reference": g["referenceSequence"], "id": g["geneID"]} for g in e["genes"]] for e in ents]
        exml, _ = _xml_restatement(tax, [e["taxonomyID"] for e in ents], genes, None, facts["batches"], facts["n_pairs"])
        assert xml == exml and xml.count(b"<read>") > 60
        assert tax.summary(st["tax_ids"], st["n_pairs"]) == exp["abbreviated"]
    finally:
        tax.close()
        report.close()
    batches = [W.chain_batch(oracle, rw["world"], k, paired) for k in facts["kinds"]]
    assert st["n_batches"] == len(facts["plan"]) == 6 and st["n_pairs"] == facts["n_pairs"] == sum(facts["plan"])
    assert st["n_overlaps"] == sum(len(b["ov"]) for b in batches) and st["n_read_pairs_aligned"] == sum(len(b["rp"]) for b in batches)
    assert st["n_alignment_pairs"] == sum(len(b["pr"]) for b in batches) and st["per_read_bytes"] == len(exp["per_read"])
    if paired:
        assert st["first_max_insert_size"] == facts["limits"][0]
    assert st["tax_ids"].tolist() == facts["tax_ids"]
    assert (st["batches_pseudo_on_host"] >= 2) if route == "host_pseudo" else (st["batches_pseudo_on_host"] == 0)
    if form == "text":
        assert st["sam_bytes"] == len(_rows(exp["sam"]))
    assert sorted(files) == sorted(f for f in exp if f != "abbreviated" and exp[f] is not None)
    _assert_files(files, exp, form)
    assert all(len(files[f]) > 0 for f in files)       # (every file of this world says something)


def test_an_empty_batch_adds_nothing_to_the_additive_outputs(kslam, oracle, rw, tmp_path, monkeypatch):
    """the first order with the reads of the nowhere batch, then of the screened-out batch, taken out of the FASTQ text: every
    file is that shorter call's expectation, and the additive outputs are byte for byte the full call's"""
    monkeypatch.setenv("KSLAM_LANES", "2")
    kinds = W.ORDERS["plain"]
    full, _, exp, _ = _run(kslam, oracle, rw, tmp_path, "full", kinds)
    _assert_files(full, exp)
    for gone in ("nowhere", "screened"):
        less, st, exp_less, facts = _run(kslam, oracle, rw, tmp_path, "less_" + gone, kinds, without=(gone,))
        assert st["n_batches"] == 5 and facts["plan"] == [W.PAIRS_PER_BATCH] * 4 + [1]
        _assert_files(less, exp_less)
        for f in E.ADDITIVE:
            assert less[f] == full[f], (gone, f)
        assert less["read_qc"] != full["read_qc"] and less["kreport"] != full["kreport"] and less["u1"] != full["u1"]


def test_a_call_starts_every_report_from_nothing(kslam, oracle, rw, lane, tmp_path):
    """the caller's own context, every report switched on by hand and fed an ordinary batch through a lane: the call empties what
    it finds (Report::started), writes the files of its own batches alone, and switches everything off"""
    M, c, tax = lane
    exp1, facts1 = _expected(oracle, rw, ["ordinary"])
    _arm(M, c, rw, tax)
    texts = _texts(kslam, facts1["case"])
    try:
        tk = c.submit_batch_fastq_text(texts[0][0].ptr, texts[0][1], texts[1][0].ptr, texts[1][1])
        c.collect_batch(tk)[4]()
    finally:
        _close(texts)
    fed = _taken_reports(M, c, rw, tax, facts1["n_pairs"])
    assert all(fed[f] == exp1[f] and len(fed[f]) > 0 for f in REPORT_FILES)      # the accumulators hold a batch
    files, st, exp, _ = _run(kslam, oracle, rw, tmp_path, "after_feeding", W.ORDERS["plain"], ctx=(c, tax))
    _assert_files(files, exp)


# ---- failed ends: every one is refused by host code ----

def _bad_case(rw, oracle, what):
    """the first order's texts with one fault -> (case, the batches in front of the failing one)"""
    kinds = W.ORDERS["plain"]
    case = dict(W.case_of(rw["world"], kinds, eol2=EOL2))
    if what == "malformed":          # a record of the fourth batch without its "+" line
        at = case["r1"].index(b"@screened011/1")
        plus = case["r1"].index(b"\n+\n", at)
        case["r1"] = case["r1"][:plus] + case["r1"][plus + 2:]
        return case, 3
    if what == "r2_short":           # R2 ends with the fifth batch; the last batch finds R1's record without a mate
        case["r2"] = case["r2"][:case["r2"].rstrip(b"\r\n").rfind(b"\n@") + 1]
        return case, 5
    if what == "long_id":            # a read id of 255 bytes in the third batch
        for k in ("r1", "r2"):
            assert case[k].count(b"@one_mate010/") == 1
            case[k] = case[k].replace(b"@one_mate010/", b"@" + b"L" * 255 + b"/")
        return case, 2
    return case, None


def _dead_pipe():
    rd, wr = os.pipe()
    os.close(rd)
    return wr


def _pipe_that_closes_after(n_bytes):
    """a pipe whose reader takes n_bytes and goes away: the writer fails with EPIPE in the middle of its file"""
    rd, wr = os.pipe()

    def reader():
        got = 0
        while got < n_bytes:
            chunk = os.read(rd, min(4096, n_bytes - got))
            if not chunk:
                break
            got += len(chunk)
        os.close(rd)
    t = threading.Thread(target=reader)
    t.start()
    return wr, t


FAILURES = {"malformed": "quality line is not as long as its bases line", "r2_short": "mismatch in R1 and R2", "long_id": "longer than 254 bytes",
            "sam_epipe": "SAM", "variants_epipe": "writing the VCF file failed", "depth_epipe": "writing the depth file failed"}


@pytest.mark.parametrize("what", sorted(FAILURES))
def test_a_failed_call_and_the_next_call_on_its_context(kslam, oracle, rw, tmp_path, monkeypatch, what):
    """the status and the message; every switch, descriptor and parameter put away; the files as include/kslam_stream.h promises
    them for a failed call; and the same call again on the same context with good inputs writes what a fresh context writes
    (test_every_output_of_one_call: the expectation): no batch of the failed call is left in any accumulator"""
    M, X = _modules(), _more_modules()
    monkeypatch.setenv("KSLAM_LANES", "2")
    kinds = W.ORDERS["plain"]
    form = "bam" if what == "long_id" else "text"
    case, n_good = _bad_case(rw, oracle, what)
    c, tax = _context(kslam, rw, X), M["taxonomy"].TaxDB(rw["world"]["taxdb"])
    batches = [W.chain_batch(oracle, rw["world"], k) for k in kinds]
    old = signal.signal(signal.SIGPIPE, signal.SIG_IGN)
    instead, reader = {}, None
    try:
        if what == "sam_epipe":
            instead["sam"], reader = _pipe_that_closes_after(30000)      # (the header and a part of the first batch's rows get through)
        elif what == "variants_epipe":
            instead["vcf"] = _dead_pipe()
        elif what == "depth_epipe":
            instead["bedgraph"] = _dead_pipe()
        with pytest.raises(kslam.KslamError) as e:
            _run(kslam, oracle, rw, tmp_path, "failed", kinds, form, case=case, instead=instead, ctx=(c, tax))
        assert e.value.status == ERR_ARG and FAILURES[what] in str(e.value), str(e.value)
        _assert_put_away(M, c)
        got = {f: open(str(tmp_path / ("failed." + f)), "rb").read() for o in OUTPUTS for f in OUTPUTS[o] if f not in instead}
        got["per_read"] = open(str(tmp_path / "failed.per_read"), "rb").read()
        exp, _ = _expected(oracle, rw, kinds)
        if n_good is not None:
            # refused in a batch: the batches in front of it are in the per-read and the split files, whole and in order; no
            # report file has a byte
            front, _ = _expected(oracle, rw, kinds[:n_good])
            assert got["per_read"] == front["per_read"] == b"".join(b["per_read"] for b in batches[:n_good])
            for f in SPLIT_FILES:
                assert got[f] == front[f], f
            for f in REPORT_FILES:
                assert got[f] == b"", f
            if form == "text":
                assert open(str(tmp_path / "failed.sam"), "rb").read() == front["sam"]
        elif what != "sam_epipe":
            # refused writing a report behind the last batch: the reports in front of it are whole, those behind it untouched
            failing = REPORT_FILES.index("vcf" if what == "variants_epipe" else "bedgraph")
            for k, f in enumerate(REPORT_FILES):
                if k != failing:
                    assert got[f] == (exp[f] if k < failing else b""), f
            for f in ["per_read"] + SPLIT_FILES:
                assert got[f] == exp[f], f
            assert open(str(tmp_path / "failed.sam"), "rb").read() == exp["sam"]
        else:
            assert exp["per_read"].startswith(got["per_read"]) and all(exp[f].startswith(got[f]) for f in SPLIT_FILES)
        # the same call with good inputs
        files, st, exp, _ = _run(kslam, oracle, rw, tmp_path, "again", kinds, form, ctx=(c, tax))
        assert st["n_batches"] == 6
        _assert_files(files, exp, form)
    finally:
        signal.signal(signal.SIGPIPE, old)
        for fd in instead.values():
            os.close(fd)
        if reader is not None:
            reader.join()
        c.close()
        tax.close()


# ---- the reports' own ABI around an empty add ----

def test_an_empty_add_changes_nothing_and_a_report_never_fed_is_empty(kslam, oracle, rw, lane):
    """kslam_*_add with zero records, zero groups and zero reads before and after a batch: the rows and the statistics stay; take on
    a report nobody fed gives no rows and zero statistics (tests/test_gpu_variants.py has the empty add alone: grid-0)"""
    M, c, tax = lane
    P = E.PARAMS
    b = W.chain_batch(oracle, rw["world"], "ordinary")
    part = E._part(rw["world"], b)
    none = E._part(rw["world"], dict(b, bases=[], quals=[], ov=b["ov"][:0], pool=b["pool"][:0], rp=b["rp"][:0], pr=b["pr"][:0]))

    def add(p):
        a = (p["ov"], p["pool"], p["rbases"], p["roff"], p["rp"], p["pr"])
        M["coverage"].add(c, p["ov"], p["rp"], p["pr"])
        M["genes"].add(c, p["rp"], p["pr"])
        M["kreport"].add(c, np.asarray(b["tax"] if len(p["rp"]) else [], dtype=np.uint32))
        M["variants"].add(c, *a)
        M["consensus"].add(c, *a)
        M["depth"].add(c, p["ov"], p["pool"], p["roff"], p["rp"], p["pr"])
        M["alignqc"].add(c, *a, p["rqual"], True)
        reads = [bytes(p["rbases"][int(p["roff"][i]):int(p["roff"][i + 1])]) for i in range(len(p["roff"]) - 1)]
        quals = [bytes(p["rqual"][int(p["roff"][i]):int(p["roff"][i + 1])]) for i in range(len(p["roff"]) - 1)]
        M["readqc"].add(c, reads, quals, True)

    def tables(mod):      # (`paired` says what kind of batches came, not what was counted)
        t = mod.take(c)
        t.pop("paired")
        return t

    def state():
        rows, seq, cst = M["consensus"].take(c, *P["consensus_params"])
        return {"coverage": [x.tolist() if hasattr(x, "tolist") else x for x in M["coverage"].take(c)],
                "genes": [M["genes"].take(c)[0].tolist(), M["genes"].take(c)[1]],
                "kreport": [M["kreport"].take(c)[0].tolist(), M["kreport"].take(c)[1]],
                "variants": [variants_ref.fields(M["variants"].take(c, P["variants_min_alt"], P["variants_min_depth"])[0]), M["variants"].take(c, 1, 1)[1]],
                "consensus": [consensus_ref.fields(rows), seq, cst],
                "depth": [depth_ref.fields(M["depth"].take(c, P["depth_min"])[0]), M["depth"].take(c, 1)[1]],
                "align_qc": tables(M["alignqc"]), "read_qc": tables(M["readqc"])}

    _arm(M, c, rw, tax)
    never = state()
    assert never["coverage"][1] == 0 and not any(v for row in never["coverage"][0] for v in row)
    for name in ("genes", "kreport", "variants", "depth"):
        assert never[name][0] == [] and not any(never[name][1].values()), name
    assert never["consensus"][0] == [] and never["consensus"][1] == b"" and not any(never["consensus"][2].values())
    without_paired = lambda t: {k: v for k, v in t.items() if k != "paired"}   # noqa: E731
    assert never["align_qc"] == without_paired(alignqc_ref.empty(P["align_qc_max_cycles"]))
    assert never["read_qc"] == without_paired(readqc_ref.tables([], [], False, P["read_qc_max_cycles"]))
    add(none)
    assert state() == never
    add(part)
    exp, _ = _expected(oracle, rw, ["ordinary"])
    fed = state()
    got = _taken_reports(M, c, rw, tax, b["n"])
    for f in REPORT_FILES:
        assert got[f] == exp[f], f
    add(none)
    assert state() == fed and fed != never
