"""include/kslam_bam.h on the GPU: the device's BAM records (csrc/samtext.hip: put_record) byte for byte against the host's
(host/tail.cpp: put_record) on tests/test_gpu_samtext.py's shapes, and the executable's --sam-bam decoded against the reference
loop's own SAM files and against plain runs of the same inputs (single end, --just-align, a batch of records larger than one
compressor round); a read id BAM cannot hold is refused through the lanes and the context goes on."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import bam_check as B
import bgzf_check
from test_cli import SLAM, _fixture_case, _run
from test_gpu_bgzf import _cl, _run_env
from test_gpu_samtext import _case

pytestmark = pytest.mark.gpu


def _cigar_star(sam):
    """a mapped row's empty CIGAR decodes as '*' (the one field BAM does not give back)"""
    out = []
    for line in sam.split(b"\n")[:-1]:
        f = line.split(b"\t")
        if not line.startswith(b"@") and f[5] == b"":
            f[5] = b"*"
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def _device_and_host_records(kslam, T, M, ST, rb, gb, quals, ids, I, paired=True, num_alignments=10, sam_xa=False, score_threshold=0,
                             report_cigar=True, pseudo=True):
    c = kslam.Context(score_threshold=score_threshold, report_cigar=report_cigar)
    c.set_index(gb)
    c.load_reads(rb)
    n_out, n_cig = c.align_resident()
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
    got = M.sam_bam(c, paired=paired, num_alignments=num_alignments, sam_xa=sam_xa)
    c.close()
    P = T.TailParams.default(paired=paired, pseudo_assembly=False, num_sam_alignments=num_alignments, sam_xa=sam_xa,
                             score_threshold=score_threshold, report_cigar=report_cigar)
    R = T.Reads(rb, quals, ids)
    exp, _ = M.tail_finish_rows_bam(P, R, I, ov, cg, det, md, rp.copy(), pr.copy())
    chunks = []
    T.tail_finish_rows(P, R, I, ov, cg, det, md, rp.copy(), pr.copy(), chunks.append)
    return got, exp, b"".join(chunks)


@pytest.fixture(scope="module")
def mods(kslam):
    return [importlib.import_module("kslam_amd." + m) for m in ("tail", "bam", "samtext")]


@pytest.mark.parametrize("kw", [{}, {"num_alignments": 1}, {"num_alignments": 3, "sam_xa": True}, {"paired": False},
                                {"score_threshold": 150}, {"report_cigar": False}, {"pseudo": False}])
def test_device_records_equal_the_host_records(kslam, synth, mods, kw):
    T, M, ST = mods
    rb, gb, quals, ids, I, _ = _case(synth, T, 31, 2500)
    if kw.get("paired") is False:
        rb, quals, ids = rb[:2500], quals[:2500], ids[:2500]
    got, exp, text = _device_and_host_records(kslam, T, M, ST, rb, gb, quals, ids, I, **kw)
    assert len(exp) > 100000
    assert got == exp
    head = T.sam_header(I, b"x")
    assert B.decode(M.header(I, head) + got)[1] == _cigar_star(text)


@pytest.mark.parametrize("shape", ["tied_groups", "long_reads"])
def test_device_records_on_large_groups_and_250bp_reads(kslam, synth, mods, shape):
    T, M, ST = mods
    if shape == "tied_groups":   # > 16 alignment pairs per read pair, tied scores, host-evaluated qualities
        rb, gb, quals, ids, I, _ = _case(synth, T, 57, 1200, many_strains=True)
        runs = [{"num_alignments": 10, "pseudo": False}, {"num_alignments": 40, "pseudo": False}]
    else:
        rb, gb, quals, ids, I, _ = _case(synth, T, 43, 1500, read_len=250)
        runs = [{}]
    for kw in runs:
        got, exp, text = _device_and_host_records(kslam, T, M, ST, rb, gb, quals, ids, I, **kw)
        assert got == exp and len(exp) > 50000
        assert B.decode(M.header(I, T.sam_header(I, b"x")) + got)[1] == _cigar_star(text)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_binary_sam_bam_equals_the_reference_loop(kslam, tmp_path, tag):
    import ref_loop_case as R
    D = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case(tag)
    R.write_case(case, tmp_path, D)
    tail = ["--num-reads-at-once", str(int(z[tag + "_per_batch"]))] + ([] if bool(z[tag + "_pseudo"]) else ["--no-pseudo-assembly"])
    args = ["--db=db", "--sam-file", "out.bam", "--output-file=out", "--sam-bam"] + tail + ["R1.fq", "R2.fq"]
    _run(args, tmp_path)
    blob = (tmp_path / "out.bam").read_bytes()
    exp = z[tag + "_sam"].tobytes().replace(b'CL:"SLAM --db db R1.fq R2.fq"', b'CL:"' + _cl(args) + b'"')
    assert B.check(blob) == _cigar_star(exp)
    plain = ["--db=db", "--sam-file", "p.sam", "--output-file=p"] + tail + ["R1.fq", "R2.fq"]
    _run(plain, tmp_path)
    for suffix in ("", "_abbreviated", "_PerRead"):
        assert (tmp_path / ("out" + suffix)).read_bytes() == (tmp_path / ("p" + suffix)).read_bytes(), suffix
    # the same file from the host formatter and from one or three lanes
    for env in ({"KSLAM_HOST_SAM_TEXT": "1"}, {"KSLAM_LANES": "1"}, {"KSLAM_LANES": "3"}):
        _run_env(args, tmp_path, env)
        assert (tmp_path / "out.bam").read_bytes() == blob, env
    # --sam-bgzf adds nothing to --sam-bam
    both = args[:5] + ["--sam-bgzf"] + args[5:]
    _run(both, tmp_path)
    assert B.check((tmp_path / "out.bam").read_bytes()) == B.check(blob).replace(_cl(args), _cl(both))


def test_binary_sam_bam_single_end_and_just_align(kslam, synth, tmp_path):
    import ref_loop_case as R
    D = importlib.import_module("kslam_amd.db")
    single = R.make_case(synth, n_pairs=400, seed=6202, paired=False)
    R.write_case(single, tmp_path, D)
    for mode in (["--output-file", "o"], ["--just-align"]):
        args = ["--db", "db", "--sam-file", "s.bam", "--sam-bam", "--num-reads-at-once", "150"] + mode + ["R1.fq"]
        plain = ["--db", "db", "--sam-file", "s.sam", "--num-reads-at-once", "150"] + mode + ["R1.fq"]
        _run(args, tmp_path)
        _run(plain, tmp_path)
        got = B.check((tmp_path / "s.bam").read_bytes())
        assert got == _cigar_star((tmp_path / "s.sam").read_bytes().replace(_cl(plain), _cl(args)))
        _run_env(args, tmp_path, {"KSLAM_HOST_SAM_TEXT": "1"})
        assert B.check((tmp_path / "s.bam").read_bytes()) == got


def _stream(kslam, S, ctx, index, h1, n1, h2, n2, per_batch, P, header, path, total=0):
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
    try:
        return S.classify_stream_native(ctx, index, h1, n1, h2, n2, per_batch, P, sam_fd=fd, sam_header=header, max_pairs_total=total)
    finally:
        os.close(fd)


def test_large_batch_spans_compressor_rounds(kslam, tmp_path):
    """a batch whose records exceed 1024 members (one compressor launch round, ~64 MiB) in a stream of two batches"""
    import torch
    from bench_legs import FastqFiles
    W = importlib.import_module("kslam_amd.workload")
    T = importlib.import_module("kslam_amd.tail")
    S = importlib.import_module("kslam_amd.stream")
    M = importlib.import_module("kslam_amd.bam")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    db, offs = W.make_database(dev, gen, 40, 5, 400_000)
    gen.manual_seed(12)
    n_pairs, per_batch = 600_000, 450_000
    reads = W.make_reads(dev, gen, db, offs, n_pairs, read_len=150)
    ctx = kslam.Context(report_cigar=True)
    ctx.set_index_device(len(offs) - 1, db.data_ptr(), offs)
    _, entry_tax = W.taxonomy(40, 5)
    index = T.IndexArrays(np.zeros(1, dtype=np.uint8), offs, taxonomy_ids=entry_tax)
    files = FastqFiles(kslam, dev, [reads], 150)
    del reads
    header = T.sam_header(index, b"SLAM --db synthetic R1.fq R2.fq")
    P = T.TailParams.default()
    try:
        plain = _stream(kslam, S, ctx, index, files.h[0].ptr, files.len, files.h[1].ptr, files.len, per_batch, P, header,
                        str(tmp_path / "p.sam"))
        M.set_sam_bam(ctx, True)
        assert M.get_sam_bam(ctx)
        res = _stream(kslam, S, ctx, index, files.h[0].ptr, files.len, files.h[1].ptr, files.len, per_batch, P, header,
                      str(tmp_path / "o.bam"))
        M.set_sam_bam(ctx, False)
    finally:
        files.close()
        ctx.close()
    assert plain["n_batches"] == res["n_batches"] == 2
    blob = (tmp_path / "o.bam").read_bytes()
    members = bgzf_check.members(blob)
    head_len = len(M.header(index, header))
    at, k = 0, 0
    while at < head_len:         # the header's members
        at += members[k][3]
        k += 1
    assert at == head_len
    head_members = sum(m[1] for m in members[:k])
    first = 0
    while members[k][3] == bgzf_check.MAX_INPUT:   # the first batch: full members up to its last one
        first += members[k][3]
        k += 1
    first += members[k][3]
    assert first > 1024 * bgzf_check.MAX_INPUT, first
    assert B.check(blob) == _cigar_star((tmp_path / "p.sam").read_bytes())
    assert res["sam_bytes"] == len(blob) - head_members - len(bgzf_check.EOF_MARKER)   # compressed batch bytes


def test_long_read_id_is_refused_through_the_lanes_and_the_context_goes_on(kslam, synth, tmp_path):
    from test_gpu_stream import _make_case
    from test_gpu_end_to_end import _fastq_text
    D = importlib.import_module("kslam_amd.db")
    T = importlib.import_module("kslam_amd.tail")
    S = importlib.import_module("kslam_amd.stream")
    M = importlib.import_module("kslam_amd.bam")
    dbdir, _, rb, quals, ids, r1, r2 = _make_case(synth, tmp_path, 600, b"\n", seed=91)
    bad_ids = list(ids)
    bad_ids[450] = b"L" * 255
    b1 = _fastq_text(rb[:600], quals[:600], bad_ids, 1, b"\n")
    b2 = _fastq_text(rb[600:], quals[600:], bad_ids, 2, b"\n")
    db = D.Database.load(dbdir / "database")
    ctx = kslam.Context()
    bases_pp, lens_p = db.entry_pointers()
    ctx._chk(ctx._L.kslam_set_index(ctx._h, db.n_entries, C.cast(bases_pp, C.c_void_p), C.cast(lens_p, C.c_void_p)))
    header = T.sam_header(db, b"SLAM --db db R1.fq R2.fq")
    P = T.TailParams.default()
    bufs = []
    for t in (r1, r2, b1, b2):
        h = kslam.HostBuffer(len(t) + 64)
        h.a[:len(t)] = np.frombuffer(t, dtype=np.uint8)
        bufs.append(h)
    try:
        _stream(kslam, S, ctx, db, bufs[0].ptr, len(r1), bufs[1].ptr, len(r2), 200, P, header, str(tmp_path / "p.sam"))
        M.set_sam_bam(ctx, True)
        with pytest.raises(kslam.KslamError, match="longer than 254 bytes"):
            _stream(kslam, S, ctx, db, bufs[2].ptr, len(b1), bufs[3].ptr, len(b2), 200, P, header, str(tmp_path / "bad.bam"))
        _stream(kslam, S, ctx, db, bufs[0].ptr, len(r1), bufs[1].ptr, len(r2), 200, P, header, str(tmp_path / "o.bam"))
        assert M.get_sam_bam(ctx)
    finally:
        ctx.close()
    assert B.check((tmp_path / "o.bam").read_bytes()) == _cigar_star((tmp_path / "p.sam").read_bytes())
