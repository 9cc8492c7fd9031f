"""include/kslam_bam.h on the host (no GPU): kslam_tail_sam_bam decodes to kslam_tail_sam's text on random overlaps and on
aligned reads, kslam_bam_header round-trips kslam_sam_header, and read ids are refused past 254 bytes."""
import importlib

import numpy as np
import pytest

import bam_check as B
from test_tail import _aligned_case, _fuzz_overlaps


@pytest.fixture(scope="module")
def T(kslam):
    return importlib.import_module("kslam_amd.tail")


@pytest.fixture(scope="module")
def M(kslam):
    return importlib.import_module("kslam_amd.bam")


def cigar_star(sam):
    """the one field BAM does not give back: a mapped row's empty CIGAR decodes as '*'"""
    out = []
    for line in sam.split(b"\n")[:-1]:
        f = line.split(b"\t")
        if f[5] == b"":
            f[5] = b"*"
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def decoded(M, T, I, records):
    head = T.sam_header(I, b"SLAM test")
    text, body = B.decode(M.header(I, head) + records)
    assert text == head
    return body


def _fuzz_index(T, n_entries, genes, tax):
    g = [[(0, 4000, b"g%d" % e, b"", b"left half"), (4000, 8000, b"", b"P%d" % e, b"right")] for e in range(n_entries)] if genes else None
    return T.Index([b"A" * 8000] * n_entries, taxonomy_ids=[tax + e if tax else 0 for e in range(n_entries)], genes=g)


@pytest.mark.parametrize("seed,paired,genes,tax,kw", [
    (1, True, True, 50, {}),
    (2, True, False, 0, {"num_sam_alignments": 1}),
    (3, False, True, 70000, {}),
    (4, False, False, 300, {"num_sam_alignments": 1, "sam_xa": True}),
    (5, True, True, 65535, {"sam_xa": True}),
    (6, True, False, 65536, {"score_threshold": 150, "score_fraction": 0.8}),
])
def test_records_decode_to_the_text_on_random_overlaps(kslam, T, M, seed, paired, genes, tax, kw):
    rng = np.random.default_rng(seed)
    ov, n_reads = _fuzz_overlaps(kslam, rng, 3000, 12, paired=paired)
    reads = T.Reads([b"A" * 100] * n_reads)
    I = _fuzz_index(T, 12, genes, tax)
    P = T.TailParams.default(paired=paired, report_cigar=False, threads=4, **kw)
    sam, st = T.tail_sam(P, reads, I, ov, np.zeros(0, np.uint32))
    bam, bst = M.tail_sam_bam(P, reads, I, ov, np.zeros(0, np.uint32))
    assert sam and decoded(M, T, I, bam) == sam
    assert bst.sam_bytes == len(bam) and bst.n_read_pairs == st.n_read_pairs
    P1 = T.TailParams.default(paired=paired, report_cigar=False, threads=1, **kw)
    assert M.tail_sam_bam(P1, reads, I, ov, np.zeros(0, np.uint32))[0] == bam


@pytest.mark.parametrize("kw", [{}, {"num_sam_alignments": 1}, {"sam_xa": True}, {"score_threshold": 185}])
def test_records_decode_to_the_text_on_aligned_reads(kslam, oracle, synth, T, M, kw):
    rb, gb, quals, R, I = _aligned_case(oracle, synth, T, 21, 600)
    al, cig, _ = oracle.align_to_database(rb, gb, oracle.Params.default())
    P = T.TailParams.default(threads=4, **kw)
    sam, _ = T.tail_sam(P, R, I, al, cig)
    bam, _ = M.tail_sam_bam(P, R, I, al, cig)
    assert b"\tMD:Z:" in sam and b"\tXP:Z:" in sam and b"\tXR:Z:\"" in sam
    assert decoded(M, T, I, bam) == cigar_star(sam)
    # the finish route (the stream's host-formatted batches) writes the same records
    rp, pr, _ = T.tail_pairs(T.TailParams.default(threads=4, stages=8, **kw), R, al)
    text = []
    T.tail_finish_rows(P, R, I, al, cig, None, None, rp.copy(), pr.copy(), sink=text.append)
    got, _ = M.tail_finish_rows_bam(P, R, I, al, cig, None, None, rp.copy(), pr.copy())
    assert decoded(M, T, I, got) == cigar_star(b"".join(text))


def test_header_round_trips_the_sam_header(kslam, T, M):
    I = T.Index([b"ACGT" * 10, b"A" * 7, b""], locus_tags=[b"NC_1", b"chr2", b"x" * 40], taxonomy_ids=[9, 0, 70000])
    head = T.sam_header(I, b'SLAM --db db "r1.fq" r2.fq')
    blob = M.header(I, head)
    text, refs, end = B.parse_header(blob)
    assert text == head and end == len(blob)
    assert refs == [(b"NC_1", 40), (b"chr2", 7), (b"x" * 40, 0)]
    assert blob[:8] == b"BAM\x01" + len(head).to_bytes(4, "little")
    empty = M.header(I, b"")   # no text: the reference list alone
    assert empty == b"BAM\x01" + bytes(4) + blob[8 + len(head):]


@pytest.mark.parametrize("n,ok", [(254, True), (255, False)])
def test_read_id_length_limit(kslam, T, M, n, ok):
    rng = np.random.default_rng(9)
    ov, n_reads = _fuzz_overlaps(kslam, rng, 50, 3, paired=True)
    ids = [b"r%d" % (i % 50) for i in range(n_reads)]
    long_read = int(ov["read"][len(ov) // 2])
    ids[long_read] = (b"L%d_" % long_read + b"x" * n)[:n]
    reads = T.Reads([b"A" * 100] * n_reads, ids=ids)
    I = _fuzz_index(T, 3, False, 5)
    P = T.TailParams.default(paired=True, report_cigar=False, threads=2)
    if ok:
        bam, _ = M.tail_sam_bam(P, reads, I, ov, np.zeros(0, np.uint32))
        assert ids[long_read] + b"\0" in bam
        assert decoded(M, T, I, bam) == T.tail_sam(P, reads, I, ov, np.zeros(0, np.uint32))[0]
    else:
        with pytest.raises(kslam.KslamError) as e:
            M.tail_sam_bam(P, reads, I, ov, np.zeros(0, np.uint32))
        assert "longer than 254 bytes" in str(e.value) and ids[long_read][:20].decode() in str(e.value)
