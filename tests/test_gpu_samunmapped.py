"""include/kslam_samunmapped.h on the GPU (csrc/samunmapped.hip): the device's rows for the reads without alignment byte for byte
against the host twin (kslam_tail_sam_unmapped) and the rules (tests/unmapped_rules.py), as text and as BAM records, through
kslam_sam_text / kslam_sam_bam and through the lanes; the seams of the 256-thread block, the scan tile and the 8- / 16-byte
stores; the partition property on the device's output; the switch going off again; and SLAM --sam-unmapped."""
import ctypes as C
import importlib

import numpy as np
import pytest

import bgzf_check
import samseq_check as S
import unmapped_check as UC
import unmapped_rules as UR
from test_cli import _fixture_case, _run
from test_gpu_bgzf import _cl, _run_env
from test_gpu_samtext import _case
from test_samseq_host import cigar_star, made_up_batch

pytestmark = pytest.mark.gpu

ALPHABET = b"ACGTNacgtnRYKMSWBDHVrykm.="
STORE_EDGE_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 150, 151]   # the 8- and 16-byte store edges and the odd nibble


@pytest.fixture(scope="module")
def mods(kslam):
    return [importlib.import_module("kslam_amd." + m) for m in ("tail", "bam", "samtext", "samseq", "samunmapped")]


@pytest.fixture(scope="module")
def small_index(synth, mods):
    gb = synth.to_bytes(synth.make_genomes(5, 1, 1, 8000))
    return gb, mods[0].Index(gb, taxonomy_ids=[9])


def synthetic_batch(kslam, n_records, rowless, paired, lens=STORE_EDGE_LENGTHS):
    """reads of the lengths `lens` in turn (R2 three places on), ids unique per record; every record outside `rowless` has one
    overlap record per read, made up as in made_up_batch: the reads need not align, the device's pairing takes the records
    as they are"""
    rng = np.random.default_rng(1000 * n_records + len(rowless))
    n_reads = 2 * n_records if paired else n_records
    length = [lens[(i % n_records + (3 if i >= n_records else 0)) % len(lens)] for i in range(n_reads)]
    bases = [bytes(rng.choice(list(ALPHABET), k).astype(np.uint8)) for k in length]
    quals = [bytes(rng.integers(33, 127, k, dtype=np.uint8)) for k in length]
    ids = [b"s%d" % (i % n_records) for i in range(n_reads)]
    gone = set(rowless)
    at = np.array([i for i in range(n_reads) if i % n_records not in gone], dtype=np.int64)
    ov = np.zeros(len(at), dtype=kslam.OVERLAP_DT)
    ov["read"] = at
    ov["rel"] = 100 + 10 * ((at % n_records) % 700)
    ov["revcomp"] = at >= n_records
    ov["score"] = 150
    ov["ref_begin"] = ov["rel"]
    ov["ref_end"] = ov["ref_begin"] + 40
    return bases, quals, ids, ov


def device_outputs(kslam, mods, index, bases, quals, ids, ov, paired, with_qual=True):
    """the resident twins on made-up overlap records -> {(seq, form): bytes} for form in off / on / again (text) and
    off_bam / on_bam / again_bam, the read pairs, and kslam_sam_unmapped_kernel_ms after every switch-on call"""
    import torch
    T, M, ST, Q, U = mods
    gb, I = index
    c = kslam.Context(report_cigar=False)
    out, stats = {}, {}
    try:
        c.set_index(gb)
        c.load_reads(bases)
        if with_qual:
            c.load_qualities(quals)
        d_ov = torch.from_numpy(np.concatenate([ov, np.zeros(1, dtype=ov.dtype)]).view(np.uint8).copy()).cuda()
        d_cig = torch.zeros(4, dtype=torch.int32, device="cuda")
        c.adopt_results_device(d_ov.data_ptr(), len(ov), d_cig.data_ptr(), 0)
        c.pair_screen(paired=paired, score_threshold=0, stages=2)
        rp, _ = c.take_pairs()
        ST.set_annotations(c, I, None)
        ST.load_read_ids(c, ids)
        kw = dict(paired=paired, num_alignments=10, sam_xa=False)
        assert not U.get_sam_unmapped(c) and U.kernel_ms(c) == (0.0, 0, 0)
        for seq in (False, True):
            Q.set_sam_seq(c, seq)
            for form, on in (("off", False), ("on", True), ("again", False)):   # on, then off again on one context
                U.set_sam_unmapped(c, on)
                assert U.get_sam_unmapped(c) == on
                out[seq, form] = ST.sam_text(c, **kw)[0]
                if on:
                    stats[seq, "text"] = U.kernel_ms(c)
                out[seq, form + "_bam"] = M.sam_bam(c, **kw)
                if on:
                    stats[seq, "bam"] = U.kernel_ms(c)
    finally:
        c.close()
    return out, rp, stats


def check_against_twin_and_rules(mods, out, rp, stats, bases, quals, ids, n_records, paired, with_qual=True, rowless=None):
    """the device's bytes == its switch-off bytes + the host twin's rows == + the rules' rows, text and BAM, SEQ off and on"""
    T, M, ST, Q, U = mods
    Rd = T.Reads(bases, quals, ids)
    view = Rd if with_qual else Q.without_qualities(Rd)
    q = quals if with_qual else None
    P = T.TailParams.default(paired=paired, pseudo_assembly=False, report_cigar=False)
    gone = UR.rowless_of(rp, n_records)
    if rowless is not None:
        assert gone == sorted(rowless)
    per = 2 if paired else 1
    for seq in (False, True):
        twin = U.tail_sam_unmapped(P, view, rp, n_records, bam=False, seq=seq)
        twin_bam = U.tail_sam_unmapped(P, view, rp, n_records, bam=True, seq=seq)
        assert twin == UR.expected_text(ids, bases, q, gone, n_records, paired, seq)
        assert twin_bam == UR.expected_records(ids, bases, q, gone, n_records, paired, seq)
        assert out[seq, "on"] == out[seq, "off"] + twin, seq                     # device against host twin, byte for byte
        assert out[seq, "on_bam"] == out[seq, "off_bam"] + twin_bam, seq
        assert out[seq, "again"] == out[seq, "off"] and out[seq, "again_bam"] == out[seq, "off_bam"]   # switching
        assert UC.decode_records(out[seq, "on_bam"][len(out[seq, "off_bam"]):]) == UC.decode_records(twin_bam)
        for form, want in (("text", twin), ("bam", twin_bam)):
            ms, n_bytes, n_rows = stats[seq, form]
            assert (n_bytes, n_rows) == (len(want), per * len(gone)) and ms >= 0 and (ms > 0 or not gone)
        # the partition on the device's own text: every read once per mate, the new rows exactly the rowless reads, in input order
        assert UR.check_partition(out[seq, "off"], out[seq, "on"], ids, bases, q, n_records, paired, seq) == per * len(gone)
    return gone


# ---- device against host twin on aligned reads ----
@pytest.mark.parametrize("paired", [True, False])
def test_device_equals_the_host_twin_on_aligned_reads(kslam, synth, mods, paired):
    """_case(synth, T, 31, 2500) of tests/test_gpu_samtext.py through the whole device path (alignment, pairing, screens,
    pseudo-assembly, per-row walk): the rows of the switch-on text behind the switch-off text are the host twin's"""
    T, M, ST, Q, U = mods
    n = 2500
    rb, gb, quals, ids, I, _ = _case(synth, T, 31, n)
    ids = [b"u%d" % (i % n) for i in range(2 * n)]   # unique per read pair: the partition check looks reads up by QNAME
    if not paired:
        rb, quals, ids = rb[:n], quals[:n], ids[:n]
    c = kslam.Context(report_cigar=True)
    out, stats = {}, {}
    try:
        c.set_index(gb)
        c.load_reads(rb)
        c.align_resident()
        c.load_qualities(quals)
        c.pair_screen(paired=paired, score_threshold=0, stages=7)
        c.row_details(of_pairs=True)
        rp, _ = c.take_pairs()
        ST.set_annotations(c, I, None)
        ST.load_read_ids(c, ids)
        kw = dict(paired=paired, num_alignments=10, sam_xa=False)
        for seq in (False, True):
            Q.set_sam_seq(c, seq)
            for form, on in (("off", False), ("on", True), ("again", False)):
                U.set_sam_unmapped(c, on)
                out[seq, form] = ST.sam_text(c, **kw)[0]
                if on:
                    stats[seq, "text"] = U.kernel_ms(c)
                out[seq, form + "_bam"] = M.sam_bam(c, **kw)
                if on:
                    stats[seq, "bam"] = U.kernel_ms(c)
    finally:
        c.close()
    gone = check_against_twin_and_rules(mods, out, rp, stats, rb, quals, ids, n, paired)
    print("records without a row: %d of %d" % (len(gone), n))
    assert 0 < len(gone) < n and len(out[True, "off"]) > 100000
    head = T.sam_header(I, b"x")
    assert UC.decode(M.header(I, head) + out[True, "on_bam"])[1] == cigar_star(out[True, "on"])   # the whole BAM is the whole text


# ---- the made-up batch: read lengths 0 .. 33 ----
@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("with_qual", [True, False])
def test_made_up_batch_on_the_device(kslam, mods, small_index, paired, with_qual):
    bases, quals, ids, ov = made_up_batch(kslam, paired)
    n = 34
    for rowless in ([p for p in range(n) if p % 3 == 1], list(range(n))):
        keep = ov[~np.isin(ov["read"] % n, rowless)]
        out, rp, stats = device_outputs(kslam, mods, small_index, bases, quals, ids, keep, paired, with_qual)
        check_against_twin_and_rules(mods, out, rp, stats, bases, quals, ids, n, paired, with_qual, rowless)


# ---- seams ----
def placements(n_records, n_rowless):
    """unaligned records first, last, and alternating with aligned ones in input order"""
    if n_rowless == 0:
        return {"none": []}
    alt = list(range(0, 2 * n_rowless, 2))
    return {"first": list(range(n_rowless)), "last": list(range(n_records - n_rowless, n_records)), "alternating": alt}


@pytest.mark.parametrize("n_rowless", [0, 1, 255, 256, 257, 513])
def test_block_seams(kslam, mods, small_index, n_rowless):
    """1, 255, 256, 257 and 513 unaligned pairs among as many aligned ones (and exactly 0: the output equals the switch-off
    output), at read lengths 0, 1, 7, 8, 9, 15, 16, 17, 150 and 151"""
    n = max(2 * n_rowless, 40)
    for name, rowless in placements(n, n_rowless).items():
        bases, quals, ids, ov = synthetic_batch(kslam, n, rowless, True)
        out, rp, stats = device_outputs(kslam, mods, small_index, bases, quals, ids, ov, True)
        check_against_twin_and_rules(mods, out, rp, stats, bases, quals, ids, n, True, rowless=rowless)
        if not rowless:
            assert out[True, "on"] == out[True, "off"] and out[False, "on_bam"] == out[False, "off_bam"] and stats[True, "text"][1:] == (0, 0)


@pytest.mark.parametrize("paired", [True, False])
def test_scan_tile_seam_and_no_groups_at_all(kslam, mods, small_index, paired):
    """4097 records, one past the scan's tile of 4096 lengths, alternating and ALL unaligned (n_groups == 0: no overlap record
    at all, the plan is never made)"""
    n = 4097
    for rowless in ([p for p in range(n) if p % 2 == 0 or p >= 4094], list(range(n))):
        bases, quals, ids, ov = synthetic_batch(kslam, n, rowless, paired, lens=[17, 0, 9, 33])
        out, rp, stats = device_outputs(kslam, mods, small_index, bases, quals, ids, ov, paired)
        assert (len(rp) == 0) == (len(rowless) == n)
        check_against_twin_and_rules(mods, out, rp, stats, bases, quals, ids, n, paired, rowless=rowless)


def test_all_pairs_unaligned_after_a_real_alignment(kslam, synth, mods):
    """reads drawn from a genome that is not in the index: the aligner finds nothing, n_groups == 0, every pair gets its rows.
    (A group that is present in read_pairs while its plan reports no row cannot be constructed through the device: the
    screens of pairs.hip compact the read pairs, so a group that reaches kslam_sam_text has count >= 1 and n_rows =
    min(count, max(num_alignments, 1)) >= 1; the host twin takes such a group in tests/test_samunmapped_host.py.)"""
    T, M, ST, Q, U = mods
    n = 300
    index_genomes = synth.make_genomes(41, 2, 1, 9000)
    other = synth.make_genomes(977, 1, 1, 9000)
    reads, _ = synth.make_paired_reads(42, other, n, read_len=100, frag_mean=300, frag_sd=30)
    rb, gb = synth.to_bytes(reads), synth.to_bytes(index_genomes)
    quals = [b"F" * len(b) for b in rb]
    ids = [b"x%d" % (i % n) for i in range(2 * n)]
    I = T.Index(gb, taxonomy_ids=[5, 6])
    c = kslam.Context(report_cigar=True)
    try:
        c.set_index(gb)
        c.load_reads(rb)
        n_out, _ = c.align_resident()
        assert n_out == 0
        c.load_qualities(quals)
        st = c.pair_screen(paired=True, score_threshold=0, stages=7)
        assert st["n_read_pairs"] == 0
        ST.set_annotations(c, I, None)
        ST.load_read_ids(c, ids)
        Q.set_sam_seq(c, True)
        assert ST.sam_text(c, paired=True)[0] == b""
        U.set_sam_unmapped(c, True)
        text = ST.sam_text(c, paired=True)[0]
        bam = M.sam_bam(c, paired=True)
    finally:
        c.close()
    assert text == UR.expected_text(ids, rb, quals, list(range(n)), n, True, True)
    assert bam == UR.expected_records(ids, rb, quals, list(range(n)), n, True, True)
    assert [(f[0], f[9], f[10]) for f in S.sam_rows(text)] == [(ids[p + m * n], rb[p + m * n], quals[p + m * n]) for p in range(n) for m in (0, 1)]


def test_a_long_id_fails_the_batch_and_names_the_lowest_read(kslam, mods, small_index):
    """the minimum is taken across both writers: an id of more than 254 bytes on a read WITH rows (the mapped writer refuses it)
    and on one without (the new writer does); the text is written all the same"""
    T, M, ST, Q, U = mods
    import torch
    gb, I = small_index
    n = 300
    rowless = [p for p in range(n) if p % 2 == 0]
    for long_with_rows, long_rowless, named in ((291, 280, b"L280_"), (271, 280, b"V271_"), (None, 298, b"L298_")):
        bases, quals, ids, ov = synthetic_batch(kslam, n, rowless, True)
        if long_with_rows is not None:
            ids[long_with_rows] = b"V%d_" % long_with_rows + b"v" * 260
        ids[long_rowless] = b"L%d_" % long_rowless + b"l" * 260
        ids[n + 299] = b"Z" * 255                        # R2 of the last record (with rows): the highest read of all, never named
        c = kslam.Context(report_cigar=False)
        try:
            c.set_index(gb)
            c.load_reads(bases)
            c.load_qualities(quals)
            d_ov = torch.from_numpy(ov.view(np.uint8).copy()).cuda()
            d_cig = torch.zeros(4, dtype=torch.int32, device="cuda")
            c.adopt_results_device(d_ov.data_ptr(), len(ov), d_cig.data_ptr(), 0)
            c.pair_screen(paired=True, score_threshold=0, stages=2)
            rp, _ = c.take_pairs()
            ST.set_annotations(c, I, None)
            ST.load_read_ids(c, ids)
            off = ST.sam_text(c, paired=True)[0]
            U.set_sam_unmapped(c, True)
            text = ST.sam_text(c, paired=True)[0]            # the text is written
            assert text == off + UR.expected_text(ids, bases, quals, UR.rowless_of(rp, n), n, True, False)
            with pytest.raises(kslam.KslamError, match="longer than 254 bytes") as e:
                M.sam_bam(c, paired=True)
            assert named.decode() in str(e.value)
            Rd = T.Reads(bases, quals, ids)
            if long_with_rows is None:   # the host twin names the same read
                with pytest.raises(Exception, match=named.decode()):
                    U.tail_sam_unmapped(T.TailParams.default(paired=True), Rd, rp, n, bam=True)
        finally:
            c.close()


# ---- through the lanes ----
def _host_text(kslam, text):
    h = kslam.HostBuffer(len(text) + 64)
    h.a[:len(text)] = np.frombuffer(text, dtype=np.uint8)
    return h


def _lane_batch(kslam, c, r1, r2):
    """kslam_submit_batch_fastq_text -> kslam_collect_batch -> (SAM bytes, text_flags, read pairs)"""
    h1, h2 = _host_text(kslam, r1), _host_text(kslam, r2)
    try:
        tk = c.submit_batch_fastq_text(h1.ptr, len(r1), h2.ptr, len(r2))
        r = kslam.BatchResult()
        c._chk(c._L.kslam_collect_batch(c._h, tk, C.byref(r)))
        text = C.string_at(r.sam_text, r.sam_text_len) if r.sam_text_len else b""
        rp = np.frombuffer(C.string_at(r.read_pairs, 24 * r.n_read_pairs), dtype=kslam.READ_PAIR_DT).copy() if r.n_read_pairs else \
            np.zeros(0, dtype=kslam.READ_PAIR_DT)
        flags, n_reads = int(r.text_flags), int(r.n_reads)
        c._L.kslam_release_batch(c._h, C.byref(r))
        return text, flags, rp, n_reads
    finally:
        h1.close()
        h2.close()


def test_batches_through_the_lanes(kslam, synth, mods):
    """a batch of which some pairs are from nowhere, the same batch without them (exactly 0 unaligned pairs: the bytes of the
    switch-off run, and text_flags still carries the bit), and a batch of nothing else (n_groups == 0), as text, BGZF and BAM"""
    import ref_loop_case as RL
    T, M, ST, Q, U = mods
    Z = importlib.import_module("kslam_amd.bgzf")
    n = 700
    case = RL.make_case(synth, n_pairs=n, seed=7311)
    rng = np.random.default_rng(8)
    bases = list(case["bases"])
    for i in range(n):
        if i % 3 == 1:   # a pair from nowhere
            for j in (i, n + i):
                bases[j] = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), len(bases[j])))
    quals, ids = case["quals"], list(case["ids"]) * 2

    def texts(sel):
        return (RL.fastq_text([bases[p] for p in sel], [quals[p] for p in sel], [ids[p] for p in sel], 1),
                RL.fastq_text([bases[n + p] for p in sel], [quals[n + p] for p in sel], [ids[p] for p in sel], 2, eol=b"\r\n"))

    gb = [e["bases"] for e in case["entries"]]
    I = T.Index(gb, locus_tags=[e["locusTag"] for e in case["entries"]], taxonomy_ids=[e["taxonomyID"] for e in case["entries"]])
    P = T.TailParams.default(paired=True, pseudo_assembly=False)
    c = kslam.Context(report_cigar=True)
    try:
        c.set_index(gb)
        ST.set_annotations(c, I, None)
        ST.set_sam_text(c, True, False)
        c.set_pairing(stages=2)   # the score screen alone: what a pair keeps does not depend on the rest of its batch
        everything = list(range(n))
        off, flags, rp, n_reads = _lane_batch(kslam, c, *texts(everything))
        assert n_reads == 2 * n and not flags & U.TEXT_SAM_UNMAPPED
        with_rows = sorted(int(g["r1_read"]) for g in rp if g["count"])
        assert 0 < len(with_rows) <= n - n // 3
        nowhere = [p for p in everything if p not in with_rows]
        for sel in (everything, with_rows, nowhere):
            b = [bases[p] for p in sel] + [bases[n + p] for p in sel]
            q = [quals[p] for p in sel] + [quals[n + p] for p in sel]
            i = [ids[p] for p in sel] * 2
            Rd = T.Reads(b, q, i)
            for seq in (False, True):
                Q.set_sam_seq(c, seq)
                U.set_sam_unmapped(c, False)
                off, flags, rp, _ = _lane_batch(kslam, c, *texts(sel))
                assert not flags & U.TEXT_SAM_UNMAPPED
                U.set_sam_unmapped(c, True)
                on, flags, rp_on, _ = _lane_batch(kslam, c, *texts(sel))
                assert flags & U.TEXT_SAM_UNMAPPED and rp_on.tobytes() == rp.tobytes()
                gone = UR.rowless_of(rp, len(sel))
                assert gone == [k for k, p in enumerate(sel) if p in nowhere]
                assert on == off + U.tail_sam_unmapped(P, Rd, rp, len(sel), seq=seq) == off + UR.expected_text(i, b, q, gone, len(sel), True, seq)
                assert U.kernel_ms(c)[1:] == (len(on) - len(off), 2 * len(gone))
                if sel is with_rows:
                    assert on == off and off
                if sel is nowhere:
                    assert off == b"" and len(rp) == 0
                UR.check_partition(off, on, i, b, q, len(sel), True, seq)
                # BGZF and BAM: the members hold the same rows
                Z.set_sam_bgzf(c, True)
                z, flags, _, _ = _lane_batch(kslam, c, *texts(sel))
                Z.set_sam_bgzf(c, False)
                assert flags & U.TEXT_SAM_UNMAPPED and bgzf_check.check(z + Z.EOF) == on
                M.set_sam_bam(c, True)
                z, flags, _, _ = _lane_batch(kslam, c, *texts(sel))
                M.set_sam_bam(c, False)
                records = bgzf_check.check(z + Z.EOF)
                assert flags & U.TEXT_SAM_UNMAPPED
                assert UC.decode(M.header(I, T.sam_header(I, b"x")) + records)[1] == cigar_star(on)
        U.set_sam_unmapped(c, False)
        Q.set_sam_seq(c, False)
    finally:
        c.set_pairing(stages=0)
        c.close()


def test_multi_contexts_refuse_the_switch(kslam, mods):
    U = mods[4]
    m = kslam.MultiContext([0])
    try:
        # the ABI hands out no handle to a kslam_multi's contexts: kslam_multi begins with their std::vector, whose first word
        # points at the first of them
        h = C.c_void_p.from_address(C.c_void_p.from_address(m._h.value).value)
        assert U.lib().kslam_set_sam_unmapped(h, 1) == 4   # KSLAM_ERR_UNSUPPORTED
        on = C.c_int(7)
        assert U.lib().kslam_get_sam_unmapped(h, C.byref(on)) == 0 and on.value == 0
    finally:
        m.close()


# ---- SLAM --sam-unmapped ----
def _rows(text):
    return b"".join(l + b"\n" for l in text.split(b"\n")[:-1] if not l.startswith(b"@"))


def _head(text, args):
    return [l for l in text.replace(_cl(args), b"CL").split(b"\n") if l.startswith(b"@")]


def _fastq_ids(text):
    return [l[1:].split(b" ")[0].split(b"/")[0] for l in text.split(b"\n")[0::4] if l]


def test_binary_sam_unmapped(kslam, tmp_path):
    """SLAM --sam-unmapped on the reference loop's inputs "a" (several batches; 0 < classified < n_pairs): plain, --sam-bgzf and
    --sam-bam --sam-seq; host formatter, one lane and three lanes write the same file; each batch's mapped rows, then its new
    rows; the report files do not move; the new rows' QNAMEs are the ids of --unclassified-out from the same run, in order"""
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    z, case = _fixture_case("a")
    RL.write_case(case, tmp_path, D)
    n, per_batch = case["n_pairs"], int(z["a_per_batch"])
    assert per_batch < n
    batches = [(first, min(per_batch, n - first)) for first in range(0, n, per_batch)]
    ids = list(case["ids"]) * 2
    tail = ["--num-reads-at-once", str(per_batch)] + ([] if bool(z["a_pseudo"]) else ["--no-pseudo-assembly"])
    runs = {}
    for seq in ([], ["--sam-seq"]):
        plain = ["--db=db", "--sam-file", "p.sam", "--output-file=p"] + seq + tail + ["R1.fq", "R2.fq"]
        _run(plain, tmp_path)
        off = _rows((tmp_path / "p.sam").read_bytes())
        forms = ((["--sam-bam"], "o.bam", UC.check),) if seq else (([], "o.sam", lambda b: b), (["--sam-bgzf"], "o.sam.gz", bgzf_check.check))
        for flags, name, read in forms:
            args = ["--db=db", "--sam-file", name, "--output-file=o", "--sam-unmapped", "--unclassified-out", "u#.fq"] + seq + flags + tail + \
                ["R1.fq", "R2.fq"]
            _run(args, tmp_path)
            blob = (tmp_path / name).read_bytes()
            text = read(blob)
            assert _head(text, args) == _head((tmp_path / "p.sam").read_bytes(), plain)   # the header is unchanged
            on = _rows(text)
            for suffix in ("", "_abbreviated", "_PerRead"):
                assert (tmp_path / ("o" + suffix)).read_bytes() == (tmp_path / ("p" + suffix)).read_bytes(), (name, suffix)
            want_off = cigar_star(off) if name.endswith(".bam") else off
            if name.endswith(".bam"):   # BAM says upper case / N; the fixture's reads are upper-case ACGTN, so the text comes back
                assert all(set(b) <= set(b"ACGTN") for b in case["bases"])
            n_new = UR.check_partition(want_off, on, ids, case["bases"], case["quals"], n, True, bool(seq), batches=batches)
            assert 0 < n_new < 2 * n
            new_ids = [f[0] for f in S.sam_rows(on) if UR.is_new_row(f)]
            assert new_ids[0::2] == new_ids[1::2] == _fastq_ids((tmp_path / "u1.fq").read_bytes()) == _fastq_ids((tmp_path / "u2.fq").read_bytes())
            for env in ({"KSLAM_HOST_SAM_TEXT": "1"}, {"KSLAM_LANES": "1"}, {"KSLAM_LANES": "3"}):
                _run_env(args, tmp_path, env)
                assert (tmp_path / name).read_bytes() == blob, (name, env)
            runs[name] = on
    assert runs["o.sam"] == runs["o.sam.gz"] and S.strip_text(runs["o.bam"]) == cigar_star(runs["o.sam"])
    r = _run(["--db=db", "--sam-unmapped", "--output-file=o", "R1.fq", "R2.fq"], tmp_path, check=False)
    assert r.returncode == 1 and b"--sam-unmapped" in r.stderr and b"--sam-file" in r.stderr
    assert b"--sam-unmapped" in _run(["--help"], tmp_path, check=False).stdout


def test_binary_sam_unmapped_single_end_and_just_align(kslam, synth, tmp_path):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    n = 400
    single = RL.make_case(synth, n_pairs=n, seed=6202, paired=False)
    RL.write_case(single, tmp_path, D)
    batches = [(first, min(150, n - first)) for first in range(0, n, 150)]
    for mode in (["--output-file", "o"], ["--just-align"]):
        plain = ["--db", "db", "--sam-file", "s.sam", "--sam-seq", "--num-reads-at-once", "150"] + mode + ["R1.fq"]
        _run(plain, tmp_path)
        off = _rows((tmp_path / "s.sam").read_bytes())
        for flags, name, read in (([], "q.sam", lambda b: b), (["--sam-bam", "--sam-deflate", "dynamic"], "q.bam", None)):
            args = ["--db", "db", "--sam-file", name, "--sam-seq", "--sam-unmapped", "--unclassified-out", "rest.fq", "--num-reads-at-once", "150"] + \
                flags + mode + ["R1.fq"]
            _run(args, tmp_path)
            blob = (tmp_path / name).read_bytes()
            if read is None:   # (dynamic Huffman members: gzip reads them, the strict BGZF reader knows stored and fixed ones)
                import gzip
                text, body = UC.decode(gzip.decompress(blob))
                on, want_off = body, cigar_star(off)
            else:
                on, want_off = _rows(read(blob)), off
            n_new = UR.check_partition(want_off, on, single["ids"], single["bases"], single["quals"], n, False, True, batches=batches)
            assert 0 < n_new < n
            new = [f for f in S.sam_rows(on) if UR.is_new_row(f)]
            assert all(f[1] == b"4" for f in new) and [f[0] for f in new] == _fastq_ids((tmp_path / "rest.fq").read_bytes())
            _run_env(args, tmp_path, {"KSLAM_HOST_SAM_TEXT": "1"})
            assert (tmp_path / name).read_bytes() == blob
