"""include/kslam_samseq.h on the host (no GPU): the twins with the switch on against the switch-off text, the FASTQ records,
the genome, and the BAM records against the text.  The rules are restated in tests/samseq_rules.py."""
import importlib

import numpy as np
import pytest

import samseq_check as S
import samseq_rules as R
from test_tail import _aligned_case, _fuzz_overlaps


@pytest.fixture(scope="module")
def T(kslam):
    return importlib.import_module("kslam_amd.tail")


@pytest.fixture(scope="module")
def Q(kslam):
    return importlib.import_module("kslam_amd.samseq")


@pytest.fixture(scope="module")
def M(kslam):
    return importlib.import_module("kslam_amd.bam")


NO_CIGAR = np.zeros(0, np.uint32)


def decoded(M, T, I, records):
    head = T.sam_header(I, b"SLAM test")
    text, body = S.decode(M.header(I, head) + records)
    assert text == head
    return body


def cigar_star(sam):
    return b"".join(b"\t".join(f[:5] + [f[5] or b"*"] + f[6:]) + b"\n" for f in (l.split(b"\t") for l in sam.split(b"\n")[:-1]))


def random_reads(rng, n_reads, length=100, alphabet=b"ACGTN"):
    bases = [bytes(rng.choice(list(alphabet), length).astype(np.uint8)) for _ in range(n_reads)]
    quals = [bytes(rng.integers(33, 127, length, dtype=np.uint8)) for _ in range(n_reads)]
    return bases, quals


@pytest.mark.parametrize("seed,paired,kw", [
    (1, True, {}),
    (2, True, {"num_sam_alignments": 3}),
    (3, False, {}),
    (4, False, {"num_sam_alignments": 1, "sam_xa": True}),
    (5, True, {"sam_xa": True}),
])
def test_random_overlaps(kslam, T, Q, M, seed, paired, kw):
    rng = np.random.default_rng(seed)
    ov, n_reads = _fuzz_overlaps(kslam, rng, 2000, 12, paired=paired)
    bases, quals = random_reads(rng, n_reads)
    n_names = n_reads // 2 if paired else n_reads
    ids = [b"q%d" % (i % n_names) for i in range(n_reads)]
    reads = T.Reads(bases, quals, ids)
    I = T.Index([b"A" * 8000] * 12, taxonomy_ids=[50 + e for e in range(12)])
    P = T.TailParams.default(paired=paired, report_cigar=False, threads=4, **kw)
    off, _ = T.tail_sam(P, reads, I, ov, NO_CIGAR)
    on, st = Q.tail_sam_seq(P, reads, I, ov, NO_CIGAR)
    assert off and S.strip_text(on) == off                                   # 1
    bam_off, _ = M.tail_sam_bam(P, reads, I, ov, NO_CIGAR)
    bam_on, bst = Q.tail_sam_seq(P, reads, I, ov, NO_CIGAR, bam=True)
    assert S.strip_records(bam_on) == bam_off and bst.sam_bytes == len(bam_on) and st.sam_bytes == len(on)
    n_primary, n_secondary = R.check_rows(on, R.name_reads(ids, paired), bases, quals, paired)   # 2, 3
    assert n_primary and (n_secondary or kw.get("sam_xa") or kw.get("num_sam_alignments") == 1)
    assert decoded(M, T, I, bam_on) == on                                    # 5: upper-case ACGTN decode to themselves
    P1 = T.TailParams.default(paired=paired, report_cigar=False, threads=1, **kw)
    assert Q.tail_sam_seq(P1, reads, I, ov, NO_CIGAR)[0] == on


@pytest.mark.parametrize("kw", [{}, {"num_sam_alignments": 3}, {"sam_xa": True}, {"score_threshold": 185}])
def test_aligned_reads(kslam, oracle, synth, T, Q, M, kw):
    n_pairs = 600
    rb, gb, quals, Rd, I = _aligned_case(oracle, synth, T, 21, n_pairs)
    ids = [b"frag%d" % (i % n_pairs) for i in range(2 * n_pairs)]
    al, cig, _ = oracle.align_to_database(rb, gb, oracle.Params.default())
    P = T.TailParams.default(threads=4, **kw)
    off, _ = T.tail_sam(P, Rd, I, al, cig)
    on, _ = Q.tail_sam_seq(P, Rd, I, al, cig)
    assert S.strip_text(on) == off                                           # 1
    bam_on, _ = Q.tail_sam_seq(P, Rd, I, al, cig, bam=True)
    assert S.strip_records(bam_on) == M.tail_sam_bam(P, Rd, I, al, cig)[0]
    read_of = R.name_reads(ids, True)
    n_primary, _ = R.check_rows(on, read_of, rb, quals, True)                # 2, 3
    assert n_primary
    locus = {b"NC_%06d" % i: i for i in range(len(gb))}
    checked, skipped, primary_mapped = R.check_against_genome(on, gb, locus)   # 4
    print("rows checked against the genome %d, skipped for want of a CIGAR %d, primary mapped rows %d" % (checked, skipped, primary_mapped))
    assert checked + skipped == primary_mapped and checked > 0.8 * n_pairs
    if "score_threshold" not in kw:   # default options: every primary mapped row has its CIGAR
        assert skipped == 0 and checked == primary_mapped
    # both strands were held to the genome
    assert any(int(f[1]) & 0x10 and f[5] not in (b"*", b"") for f in S.sam_rows(on) if not int(f[1]) & 0x100)
    assert decoded(M, T, I, bam_on) == cigar_star(on)                        # 5
    # the finish route (the stream's host-formatted batches) writes the same bytes
    rp, pr, _ = T.tail_pairs(T.TailParams.default(threads=4, stages=8, **kw), Rd, al)
    text = []
    T.tail_finish_rows(P, Rd, I, al, cig, None, None, rp.copy(), pr.copy(), sink=text.append)
    fin, _ = Q.tail_finish_rows_seq(P, Rd, I, al, cig, None, None, rp.copy(), pr.copy())
    assert S.strip_text(fin) == b"".join(text)
    R.check_rows(fin, read_of, rb, quals, True)
    fin_bam, _ = Q.tail_finish_rows_seq(P, Rd, I, al, cig, None, None, rp.copy(), pr.copy(), bam=True)
    assert decoded(M, T, I, fin_bam) == cigar_star(fin)


def made_up_batch(kslam, paired=True, flip=0):
    """reads of every length 0 .. 33 with N, lower case, IUPAC codes and bytes that are no letters; every read has one overlap.
    Read i and read 34 + i (its mate when paired) both have length i and lie on opposite strands, so the two carry every
    length on both strands when paired; single end is the first 34 reads, and flip = 1 turns every strand round, so the two
    values of flip together do the same there."""
    rng = np.random.default_rng(77)
    alphabet = b"ACGTNacgtnRYKMSWBDHVrykm.="
    n = 34
    lens = list(range(n)) + list(range(n))
    bases = [bytes(rng.choice(list(alphabet), k).astype(np.uint8)) for k in lens]
    quals = [bytes(rng.integers(33, 127, k, dtype=np.uint8)) for k in lens]
    ids = [b"m%d" % (i % n) for i in range(2 * n)]
    n_reads = 2 * n if paired else n
    at = np.arange(n_reads)
    ov = np.zeros(n_reads, dtype=kslam.OVERLAP_DT)
    ov["read"] = at
    ov["entry"] = 0
    ov["rel"] = 100 + 10 * (at % n)
    ov["revcomp"] = (at + (at >= n) + flip) % 2   # length L: R1 on strand (L + flip) % 2, R2 on the other
    ov["score"] = 150
    ov["ref_begin"] = ov["rel"]
    ov["ref_end"] = ov["ref_begin"] + 40
    ov["query_begin"], ov["query_end"] = 0, 0
    return bases[:n_reads], quals[:n_reads], ids[:n_reads], ov


BOTH_STRANDS_AT_EVERY_LENGTH = {(k, rev) for k in range(1, 34) for rev in (False, True)}


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("with_qual", [True, False])
def test_made_up_batch(kslam, T, Q, M, paired, with_qual):
    seen, seen_bam = set(), set()
    for flip in (0, 1):
        bases, quals, ids, ov = made_up_batch(kslam, paired, flip)
        reads = T.Reads(bases, quals, ids)
        view = reads if with_qual else Q.without_qualities(reads)
        I = T.Index([b"A" * 8000], taxonomy_ids=[9])
        P = T.TailParams.default(paired=paired, report_cigar=False, threads=2, pseudo_assembly=False)
        on, _ = Q.tail_sam_seq(P, view, I, ov, NO_CIGAR)
        bam_on, _ = Q.tail_sam_seq(P, view, I, ov, NO_CIGAR, bam=True)
        assert S.strip_text(on) == T.tail_sam(P, reads, I, ov, NO_CIGAR)[0]
        read_of = R.name_reads(ids, paired)
        n_primary, _ = R.check_rows(on, read_of, bases, quals if with_qual else None, paired, seen=seen)
        assert n_primary == len(bases)
        rows = S.sam_rows(on)
        got = S.sam_rows(decoded(M, T, I, bam_on))
        assert len(got) == len(rows)
        for f, g in zip(rows, got):   # the BAM holds what samtools view -b stores for this text
            assert g[:9] == f[:9] and g[11:] == f[11:]
            assert (g[9], g[10]) == R.bam_view(f[9], f[10])
        # ... and, from the rule itself, nibble by nibble
        R.check_rows(decoded(M, T, I, bam_on), read_of, bases, quals if with_qual else None, paired, through_bam=True, seen=seen_bam)
    # every length 1 .. 33 was written forward and reverse, in text and in BAM (paired: already within one batch)
    assert seen == BOTH_STRANDS_AT_EVERY_LENGTH and seen_bam == BOTH_STRANDS_AT_EVERY_LENGTH


@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_loop_inputs_hold_seq_to_the_genome(kslam, oracle, T, Q, tag):
    """check 4 on the reads and entries of tests/golden/slam_loop.npz (the reference loop's inputs), through the host twin"""
    import os
    from test_reference_loop import load_fixture_case
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slam_loop.npz"), allow_pickle=False)
    case = load_fixture_case(z, tag)
    n = case["n_pairs"]
    gb = [e["bases"] for e in case["entries"]]
    al, cig, _ = oracle.align_to_database(case["bases"], gb, oracle.Params.default())
    Rd = T.Reads(case["bases"], case["quals"], list(case["ids"]) * 2)
    I = T.Index(gb, locus_tags=[e["locusTag"] for e in case["entries"]], taxonomy_ids=[e["taxonomyID"] for e in case["entries"]])
    on, _ = Q.tail_sam_seq(T.TailParams.default(threads=4), Rd, I, al, cig)
    R.check_rows(on, R.name_reads(list(case["ids"]) * 2, True), case["bases"], case["quals"], True)
    checked, skipped, primary_mapped = R.check_against_genome(on, gb, {e["locusTag"]: k for k, e in enumerate(case["entries"])})
    print("rows checked against the genome %d, skipped for want of a CIGAR %d, primary mapped rows %d" % (checked, skipped, primary_mapped))
    assert skipped == 0 and checked == primary_mapped and checked > n
