"""include/kslam_samseq.h on the GPU: the device's SEQ / QUAL (csrc/samtext.hip: put_seq_text / put_seq_bam) byte for byte
against the host twins, as text and as BAM records, on tests/test_gpu_bam.py's shapes and on a made-up batch of every length
0 .. 33; the rules (tests/samseq_rules.py) on the device's output; SLAM --sam-seq plain, BGZF and BAM against the library
route, across host / 1 / 3 lanes, single end, --just-align and batch boundaries; and the switch going off again."""
import importlib

import numpy as np
import pytest

import bgzf_check
import samseq_check as S
import samseq_rules as R
from test_cli import _fixture_case, _run
from test_gpu_bgzf import _cl, _run_env
from test_gpu_samtext import _case
from test_samseq_host import cigar_star, made_up_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(kslam):
    return [importlib.import_module("kslam_amd." + m) for m in ("tail", "bam", "samtext", "samseq")]


def _device_and_host(kslam, mods, rb, gb, quals, ids, I, paired=True, num_alignments=10, sam_xa=False, score_threshold=0,
                     report_cigar=True, pseudo=True, with_qual=True, overlaps=None):
    """-> dict of device / host bytes: text and records with the switch on, the device's with it off before and after"""
    T, M, ST, Q = mods
    c = kslam.Context(score_threshold=score_threshold, report_cigar=report_cigar)
    c.set_index(gb)
    c.load_reads(rb)
    n_out, n_cig = c.align_resident()
    if with_qual:
        c.load_qualities(quals)
    c.pair_screen(paired=paired, score_threshold=score_threshold, stages=7 if pseudo else 3)
    det = md = None
    if report_cigar:
        c.row_details(of_pairs=True)
        det, md = c.take_row_details(n_out)
    ov, cg = c.fetch_results(n_out, n_cig)
    rp, pr = c.take_pairs()
    ST.set_annotations(c, I, None)
    ST.load_read_ids(c, ids)
    kw = dict(paired=paired, num_alignments=num_alignments, sam_xa=sam_xa)
    out = {}
    assert not Q.get_sam_seq(c)
    out["dev_off_text"] = ST.sam_text(c, **kw)[0]
    Q.set_sam_seq(c, True)
    assert Q.get_sam_seq(c)
    out["dev_text"] = ST.sam_text(c, **kw)[0]
    out["dev_bam"] = M.sam_bam(c, **kw)
    Q.set_sam_seq(c, False)                     # 9: off after on, same context
    out["dev_off_again_text"] = ST.sam_text(c, **kw)[0]
    out["dev_off_again_bam"] = M.sam_bam(c, **kw)
    c.close()
    P = T.TailParams.default(paired=paired, pseudo_assembly=False, num_sam_alignments=num_alignments, sam_xa=sam_xa,
                             score_threshold=score_threshold, report_cigar=report_cigar)
    Rd = T.Reads(rb, quals, ids)
    view = Rd if with_qual else Q.without_qualities(Rd)
    out["host_text"] = Q.tail_finish_rows_seq(P, view, I, ov, cg, det, md, rp.copy(), pr.copy())[0]
    out["host_bam"] = Q.tail_finish_rows_seq(P, view, I, ov, cg, det, md, rp.copy(), pr.copy(), bam=True)[0]
    out["host_off_bam"] = M.tail_finish_rows_bam(P, Rd, I, ov, cg, det, md, rp.copy(), pr.copy())[0]
    chunks = []
    T.tail_finish_rows(P, Rd, I, ov, cg, det, md, rp.copy(), pr.copy(), chunks.append)
    out["host_off_text"] = b"".join(chunks)
    return out


@pytest.mark.parametrize("kw", [{}, {"num_alignments": 1}, {"num_alignments": 3}, {"num_alignments": 3, "sam_xa": True}, {"paired": False},
                                {"score_threshold": 150}, {"report_cigar": False}, {"pseudo": False}, {"with_qual": False, "report_cigar": False}])
def test_device_bytes_equal_the_host_twins(kslam, synth, mods, kw):
    T, M, ST, Q = mods
    n_pairs = 2500
    rb, gb, quals, ids, I, _ = _case(synth, T, 31, n_pairs)
    ids = [b"u%d" % (i % n_pairs) for i in range(2 * n_pairs)]   # unique per read pair: the rules look reads up by QNAME
    paired = kw.get("paired", True)
    if not paired:
        rb, quals, ids = rb[:n_pairs], quals[:n_pairs], ids[:n_pairs]
    o = _device_and_host(kslam, mods, rb, gb, quals, ids, I, **kw)
    assert len(o["host_text"]) > 100000
    assert o["dev_text"] == o["host_text"]                                        # 6
    assert o["dev_bam"] == o["host_bam"]
    assert o["dev_off_text"] == o["host_off_text"] == o["dev_off_again_text"]     # 9
    assert o["dev_off_again_bam"] == o["host_off_bam"]
    # 7: the rules on the device's output
    assert S.strip_text(o["dev_text"]) == o["dev_off_text"]                       # 1
    assert S.strip_records(o["dev_bam"]) == o["host_off_bam"]
    n_primary, n_secondary = R.check_rows(o["dev_text"], R.name_reads(ids, paired), rb, quals if kw.get("with_qual", True) else None,
                                          paired)   # 2, 3
    assert n_primary > n_pairs // 2
    head = T.sam_header(I, b"x")
    assert S.decode(M.header(I, head) + o["dev_bam"])[1] == cigar_star(o["dev_text"])   # 5
    if kw.get("report_cigar", True):                                              # 4
        locus = {b"NC_%06d.%d" % (i, i % 3): i for i in range(len(gb))}
        checked, skipped, primary_mapped = R.check_against_genome(o["dev_text"], gb, locus)
        print("rows checked against the genome %d, skipped for want of a CIGAR %d, primary mapped rows %d" % (checked, skipped, primary_mapped))
        assert checked + skipped == primary_mapped and checked > n_pairs // 2
        if not kw.get("score_threshold"):
            assert skipped == 0


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("with_qual", [True, False])
def test_made_up_batch_on_the_device(kslam, synth, mods, paired, with_qual):
    """reads of every length 0 .. 33 (the 8- and 16-byte edges, odd lengths), N, lower case, IUPAC codes, every length on both
    strands: the reads are too short to align, so the rows come from overlap records handed to the device's pairing as they are"""
    import torch
    from test_samseq_host import BOTH_STRANDS_AT_EVERY_LENGTH
    T, M, ST, Q = mods
    gb = synth.to_bytes(synth.make_genomes(5, 1, 1, 8000))
    I = T.Index(gb, taxonomy_ids=[9])
    seen, seen_bam = set(), set()
    for flip in (0, 1):
        bases, quals, ids, ov = made_up_batch(kslam, paired, flip)
        c = kslam.Context(report_cigar=False)
        c.set_index(gb)
        c.load_reads(bases)
        if with_qual:
            c.load_qualities(quals)
        d_ov = torch.from_numpy(ov.view(np.uint8).copy()).cuda()
        d_cig = torch.zeros(4, dtype=torch.int32, device="cuda")
        c.adopt_results_device(d_ov.data_ptr(), len(ov), d_cig.data_ptr(), 0)
        c.pair_screen(paired=paired, score_threshold=0, stages=3)
        rp, pr = c.take_pairs()
        ST.set_annotations(c, I, None)
        ST.load_read_ids(c, ids)
        Q.set_sam_seq(c, True)
        text = ST.sam_text(c, paired=paired, num_alignments=10, sam_xa=False)[0]
        bam = M.sam_bam(c, paired=paired, num_alignments=10, sam_xa=False)
        c.close()
        P = T.TailParams.default(paired=paired, pseudo_assembly=False, report_cigar=False)
        Rd = T.Reads(bases, quals, ids)
        view = Rd if with_qual else Q.without_qualities(Rd)
        assert text == Q.tail_finish_rows_seq(P, view, I, ov, np.zeros(0, np.uint32), None, None, rp.copy(), pr.copy())[0]
        assert bam == Q.tail_finish_rows_seq(P, view, I, ov, np.zeros(0, np.uint32), None, None, rp.copy(), pr.copy(), bam=True)[0]
        read_of = R.name_reads(ids, paired)
        n_primary, _ = R.check_rows(text, read_of, bases, quals if with_qual else None, paired, seen=seen)
        assert n_primary == len(bases)
        body = S.decode(M.header(I, T.sam_header(I, b"x")) + bam)[1]
        R.check_rows(body, read_of, bases, quals if with_qual else None, paired, through_bam=True, seen=seen_bam)
    # the device wrote every length 1 .. 33 forward and reverse, as text and as BAM
    assert seen == BOTH_STRANDS_AT_EVERY_LENGTH and seen_bam == BOTH_STRANDS_AT_EVERY_LENGTH


@pytest.mark.parametrize("tag", ["a", "b"])
def test_binary_sam_seq(kslam, tmp_path, tag):
    """SLAM --sam-seq, plain / --sam-bgzf / --sam-bam, with --output-file and with --just-align, on the reference loop's inputs
    (several batches, a batch boundary inside the files).  Where the issue says "files equal the library route's" this holds
    each file to more than another route of the same library: stripped of the two columns it is the file of a run without
    the flag (which the existing tests pin to the reference's own loop), and the columns are the FASTQ records' by the rules
    restated in samseq_rules, down to the genome.  The three forms agree; host formatter, one lane and three lanes give the
    same file; the report files do not change"""
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case(tag)
    RL.write_case(case, tmp_path, D)
    tail = ["--num-reads-at-once", str(int(z[tag + "_per_batch"]))] + ([] if bool(z[tag + "_pseudo"]) else ["--no-pseudo-assembly"])
    plain = ["--db=db", "--sam-file", "p.sam", "--output-file=p"] + tail + ["R1.fq", "R2.fq"]
    _run(plain, tmp_path)
    off = (tmp_path / "p.sam").read_bytes()

    def body(text, args):
        lines = text.replace(_cl(args), b"CL").split(b"\n")
        head = [l for l in lines if l.startswith(b"@")]
        return b"\n".join(head) + b"\n", b"\n".join(l for l in lines if not l.startswith(b"@"))

    files = {}
    for kind, flags, name, read in (("plain", [], "o.sam", lambda b: b), ("bgzf", ["--sam-bgzf"], "o.sam.gz", bgzf_check.check),
                                    ("bam", ["--sam-bam"], "o.bam", S.check)):
        args = ["--db=db", "--sam-file", name, "--output-file=o", "--sam-seq"] + flags + tail + ["R1.fq", "R2.fq"]
        _run(args, tmp_path)
        blob = (tmp_path / name).read_bytes()
        files[kind] = body(read(blob), args)
        for suffix in ("", "_abbreviated", "_PerRead"):
            assert (tmp_path / ("o" + suffix)).read_bytes() == (tmp_path / ("p" + suffix)).read_bytes(), (kind, suffix)
        for env in ({"KSLAM_HOST_SAM_TEXT": "1"}, {"KSLAM_LANES": "1"}, {"KSLAM_LANES": "3"}):
            _run_env(args, tmp_path, env)
            assert (tmp_path / name).read_bytes() == blob, (kind, env)
    head_off, rows_off = body(off, plain)
    assert files["plain"][0] == head_off and files["bgzf"] == files["plain"]
    assert S.strip_text(files["plain"][1]) == rows_off
    assert files["bam"][1] == cigar_star(files["plain"][1])
    # the rules, from the FASTQ files themselves
    n = case["n_pairs"]
    ids = list(case["ids"])   # one per read pair, unique
    assert len(ids) == n and len(case["bases"]) == 2 * n
    n_primary, _ = R.check_rows(files["plain"][1], R.name_reads(ids + ids, True), case["bases"], case["quals"], True)
    assert n_primary
    locus = {e["locusTag"]: k for k, e in enumerate(case["entries"])}
    checked, skipped, primary_mapped = R.check_against_genome(files["plain"][1], [e["bases"] for e in case["entries"]], locus)
    print("rows checked against the genome %d, skipped for want of a CIGAR %d, primary mapped rows %d" % (checked, skipped, primary_mapped))
    assert skipped == 0 and checked == primary_mapped and checked > 0
    # --just-align, paired, all three forms: the same SAM file as with --output-file, and no report files
    for kind, flags, name, read in (("plain", [], "j.sam", lambda b: b), ("bgzf", ["--sam-bgzf"], "j.sam.gz", bgzf_check.check),
                                    ("bam", ["--sam-bam"], "j.bam", S.check)):
        args = ["--db=db", "--sam-file", name, "--just-align", "--sam-seq"] + flags + tail + ["R1.fq", "R2.fq"]
        _run(args, tmp_path)
        assert body(read((tmp_path / name).read_bytes()), args) == files[kind], kind


def test_binary_sam_seq_single_end_and_just_align(kslam, synth, tmp_path):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    single = RL.make_case(synth, n_pairs=400, seed=6202, paired=False)
    RL.write_case(single, tmp_path, D)
    for mode in (["--output-file", "o"], ["--just-align"]):
        plain = ["--db", "db", "--sam-file", "s.sam", "--num-reads-at-once", "150"] + mode + ["R1.fq"]
        _run(plain, tmp_path)
        off = (tmp_path / "s.sam").read_bytes()
        for flags, name, read in (([], "q.sam", lambda b: b), (["--sam-bam"], "q.bam", S.check), (["--sam-xa"], "x.sam", lambda b: b)):
            args = ["--db", "db", "--sam-file", name, "--sam-seq", "--num-reads-at-once", "150"] + flags + mode + ["R1.fq"]
            _run(args, tmp_path)
            blob = (tmp_path / name).read_bytes()
            text = read(blob)
            rows = b"".join(l + b"\n" for l in text.split(b"\n")[:-1] if not l.startswith(b"@"))
            if "--sam-xa" not in flags:
                want = b"".join(l + b"\n" for l in off.split(b"\n")[:-1] if not l.startswith(b"@"))
                assert S.strip_text(rows) == (cigar_star(want) if name.endswith(".bam") else want)
            assert any(f[9] != b"*" for f in S.sam_rows(rows))
            _run_env(args, tmp_path, {"KSLAM_HOST_SAM_TEXT": "1"})
            assert (tmp_path / name).read_bytes() == blob


def _stream_to(S, ctx, index, files, per_batch, P, header, path):
    import os
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
    try:
        return S.classify_stream_native(ctx, index, files.h[0].ptr, files.len, files.h[1].ptr, files.len, per_batch, P, sam_fd=fd,
                                        sam_header=header)
    finally:
        os.close(fd)


def _rows(text):
    return b"".join(l + b"\n" for l in text.split(b"\n")[:-1] if not l.startswith(b"@"))


def test_large_batch_spans_compressor_rounds_with_seq(kslam, tmp_path, monkeypatch):
    """a stream of two batches whose first, with SEQ and QUAL, is more than 1024 BGZF members (one compressor launch round) as
    text and as BAM records: the lanes' members inflate to the host twin's bytes (the same stream formatted on the CPUs), to
    the plain --sam-seq text, and, stripped, to the switch-off file; the columns are the FASTQ records' by the rules"""
    import torch
    from bench_legs import FastqFiles
    W = importlib.import_module("kslam_amd.workload")
    S_ = importlib.import_module("kslam_amd.stream")
    Z = importlib.import_module("kslam_amd.bgzf")
    T, M, ST, Q = [importlib.import_module("kslam_amd." + m) for m in ("tail", "bam", "samtext", "samseq")]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    db, offs = W.make_database(dev, gen, 40, 5, 400_000)
    gen.manual_seed(12)
    n_pairs, per_batch = 200_000, 150_000
    reads = W.make_reads(dev, gen, db, offs, n_pairs, read_len=150)
    ctx = kslam.Context(report_cigar=True)
    ctx.set_index_device(len(offs) - 1, db.data_ptr(), offs)
    _, entry_tax = W.taxonomy(40, 5)
    index = T.IndexArrays(np.zeros(1, dtype=np.uint8), offs, taxonomy_ids=entry_tax)
    files = FastqFiles(kslam, dev, [reads], 150)
    del reads
    header = T.sam_header(index, b"SLAM --db synthetic R1.fq R2.fq")
    P = T.TailParams.default()
    out = {}
    try:
        fastq = [bytes(files.h[k].a[:files.len]) for k in (0, 1)]
        out["off"] = _stream_to(S_, ctx, index, files, per_batch, P, header, str(tmp_path / "off.sam"))
        Q.set_sam_seq(ctx, True)
        for kind in ("plain", "bgzf", "bam"):
            Z.set_sam_bgzf(ctx, kind == "bgzf")
            M.set_sam_bam(ctx, kind == "bam")
            out[kind] = _stream_to(S_, ctx, index, files, per_batch, P, header, str(tmp_path / ("dev." + kind)))
            monkeypatch.setenv("KSLAM_HOST_SAM_TEXT", "1")
            out[kind + "_host"] = _stream_to(S_, ctx, index, files, per_batch, P, header, str(tmp_path / ("host." + kind)))
            monkeypatch.delenv("KSLAM_HOST_SAM_TEXT")
        Q.set_sam_seq(ctx, False)
        Z.set_sam_bgzf(ctx, False)
        M.set_sam_bam(ctx, False)
        out["off_again"] = _stream_to(S_, ctx, index, files, per_batch, P, header, str(tmp_path / "off2.sam"))
    finally:
        files.close()
        ctx.close()
    assert all(r["n_batches"] == 2 for r in out.values())
    off = (tmp_path / "off.sam").read_bytes()
    assert (tmp_path / "off2.sam").read_bytes() == off                         # 9, through the lanes
    plain = (tmp_path / "dev.plain").read_bytes()
    assert (tmp_path / "host.plain").read_bytes() == plain
    assert S.strip_text(_rows(plain)) == _rows(off) and plain[:len(header)] == header == off[:len(header)]
    for kind, head_len in (("bgzf", len(header)), ("bam", len(M.header(index, header)))):
        blob = (tmp_path / ("dev." + kind)).read_bytes()
        members = bgzf_check.members(blob)
        at, k = 0, 0
        while at < head_len:         # the header's members
            at += members[k][3]
            k += 1
        assert at == head_len
        first = 0
        while members[k][3] == bgzf_check.MAX_INPUT:   # the first batch: full members up to its last one
            first += members[k][3]
            k += 1
        first += members[k][3]
        assert first > 1024 * bgzf_check.MAX_INPUT, (kind, first)
        raw = bgzf_check.check(blob)
        assert raw == bgzf_check.check((tmp_path / ("host." + kind)).read_bytes()), kind   # device bytes == host twin's
        if kind == "bgzf":
            assert raw == plain
        else:
            text, body = S.decode(raw)
            assert text == header and body == cigar_star(_rows(plain))
    # the columns against the FASTQ texts themselves
    bases, quals, ids = [], [], []
    for mate in (0, 1):
        lines = fastq[mate].split(b"\n")
        ids += [l[1:].split(b" ")[0].split(b"/")[0] for l in lines[0:4 * n_pairs:4]]
        bases += lines[1:4 * n_pairs:4]
        quals += lines[3:4 * n_pairs:4]
    assert len(bases) == 2 * n_pairs
    n_primary, _ = R.check_rows(_rows(plain), R.name_reads(ids, True), bases, quals, True)
    assert n_primary > n_pairs
