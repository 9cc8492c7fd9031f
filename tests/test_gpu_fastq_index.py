"""kslam_submit_batch_fastq_text (csrc/fastq_index.hip: k_fq_count, k_fq_events, k_fq_fields, k_fq_ids; csrc/details.hip:
k_gather_fields) against a plain line reader, at every seam of the kernels' tiling.

The reference is tests/fastq_seams.py: records(), a byte loop (tests/test_fastq_seams.py pins it to the restatement of the
reference's reader and to the host parser on these very texts).  For every case the device's record count, consumed bytes,
offsets and identifiers are the plain reader's; the alignment of the batch is the alignment of the plain reader's columns; and
with SEQ / QUAL switched on in the device's SAM text every primary row carries the FASTQ record's own lines
(tests/samseq_rules.py), clipped ends and unaligned qualities included, with a row for every planted read.

The texts come from the builder in tests/fastq_seams.py; the seam-matrix case asserts the census of the texts it submits."""
import ctypes as C
import importlib
import time

import numpy as np
import pytest

import fastq_seams as S
import samseq_check
import samseq_rules as R

pytestmark = pytest.mark.gpu


class Rig:
    """one context per genome set, reused by the cases: index, annotations for the SAM text"""

    def __init__(self, kslam, synth, which):
        self.K = kslam
        self.T, self.ST, self.Q, self.F = [importlib.import_module("kslam_amd." + m) for m in ("tail", "samtext", "samseq", "fastq")]
        self.genomes = S.genomes(synth, which)
        self.ctx = kslam.Context()
        self.ctx.set_index(self.genomes)
        self.index = self.T.Index(self.genomes, taxonomy_ids=list(range(1, len(self.genomes) + 1)))
        self.ST.set_annotations(self.ctx, self.index, None)

    def close(self):
        self.ctx.close()

    def collect(self, ticket):
        """kslam_collect_batch, the SAM text of the lane included -> dict (copies), or raises KslamError"""
        c = self.ctx
        r = self.K.BatchResult()
        c._chk(c._L.kslam_collect_batch(c._h, ticket, C.byref(r)))

        def view(ptr, n, dt):
            return np.frombuffer((C.c_char * (int(n) * dt.itemsize)).from_address(ptr), dtype=dt).copy() if n and ptr else np.zeros(0, dtype=dt)
        n = int(r.n_reads)
        out = {"ov": view(r.overlaps, r.n_overlaps, self.K.OVERLAP_DT), "cg": view(r.cigar_pool, r.n_cigar, np.dtype(np.uint32)),
               "det": view(r.details, r.n_overlaps if r.details else 0, self.K.ROW_DETAIL_DT), "md": view(r.md_pool, r.n_md, np.dtype(np.uint8)),
               "n_reads": n, "consumed": (int(r.consumed1), int(r.consumed2)), "has_reads": bool(r.reads_bases_off),
               "sam": C.string_at(r.sam_text, r.sam_text_len) if r.sam_text else None}
        if r.reads_bases_off:
            out["bases_off"] = view(r.reads_bases_off, n + 1, np.dtype(np.uint64))
            out["ids_off"] = view(r.reads_ids_off, n + 1, np.dtype(np.uint64))
            out["ids"] = view(r.reads_ids, int(out["ids_off"][n]) if n else 0, np.dtype(np.uint8)).tobytes()
        c._L.kslam_release_batch(c._h, C.byref(r))
        return out

    def lanes_plain(self):
        self.ctx.set_pairing(stages=0)
        self.ST.set_sam_text(self.ctx, False, False)
        self.Q.set_sam_seq(self.ctx, False)

    def lanes_with_sam_seq(self, paired):
        self.ctx.set_pairing(paired=paired, stages=3)
        self.ST.set_sam_text(self.ctx, True, False, num_alignments=10, sam_xa=False)
        self.Q.set_sam_seq(self.ctx, True)


@pytest.fixture(scope="module")
def rig(kslam, synth):
    r = Rig(kslam, synth, "small")
    yield r
    r.close()


def _host_text(kslam, t):
    h = kslam.HostBuffer(len(t) + 64)
    h.a[:len(t)] = np.frombuffer(t, dtype=np.uint8)
    h.a[len(t):] = 0
    return h


def _offsets(items):
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    if items:
        np.cumsum([len(x) for x in items], out=off[1:])
    return off


def check_case(rig, c):
    """-> (reads, planted reads, primary rows).  The whole comparison for one case that is expected to succeed."""
    kslam, ctx = rig.K, rig.ctx
    single = c["r2"] is None
    streams = [c["r1"]] if single else [c["r1"], c["r2"]]
    want = [S.records(t, c["max_pairs"], c["at_eof"]) for t in streams]
    ids = [x for w in want for x in w[0]]
    bases = [x for w in want for x in w[1]]
    quals = [x for w in want for x in w[2]]
    consumed = (want[0][3], 0 if single else want[1][3])
    assert single or len(want[0][0]) == len(want[1][0])
    assert all(len(b) == len(q) for b, q in zip(bases, quals))
    hs = [_host_text(kslam, t) for t in streams]
    args = (hs[0].ptr, len(streams[0]), None if single else hs[1].ptr, 0 if single else len(streams[1]))
    try:
        # ---- the index and the columns, lanes as plain as they come
        rig.lanes_plain()
        got = rig.collect(ctx.submit_batch_fastq_text(*args, max_pairs=c["max_pairs"], at_eof=c["at_eof"]))
        assert got["has_reads"]
        assert got["n_reads"] == len(bases), (c["name"], got["n_reads"], len(bases))
        assert got["consumed"] == consumed, (c["name"], got["consumed"], consumed)
        assert (got["bases_off"] == _offsets(bases)).all(), c["name"]
        assert (got["ids_off"] == _offsets(ids)).all(), c["name"]
        assert got["ids"] == b"".join(ids), c["name"]
        cat = np.frombuffer(b"".join(bases) + bytes(64), dtype=np.uint8)
        qcat = np.frombuffer(b"".join(quals) + bytes(64), dtype=np.uint8)
        off = _offsets(bases)
        ref = rig.collect(ctx.submit_batch_columns(len(bases), cat.ctypes.data, qcat.ctypes.data, off.ctypes.data))
        for f in ("ov", "cg", "det", "md"):
            assert got[f].tobytes() == ref[f].tobytes(), (c["name"], f)
        # ---- SEQ and QUAL of the device's SAM text: the gathered columns, byte for byte, whether aligned or not
        n_first = len(want[0][0])
        planted = [k for k in c["planted"] if k < n_first]
        rig.lanes_with_sam_seq(not single)
        sam = rig.collect(ctx.submit_batch_fastq_text(*args, max_pairs=c["max_pairs"], at_eof=c["at_eof"]))
        assert sam["ids"] == got["ids"] and sam["consumed"] == consumed
        assert sam["sam"] is not None, "the lane wrote no SAM text"
        for k in planted:
            assert ids[k] == b"p%d" % k
        read_of = {i: k for k, i in enumerate(ids[:n_first])}       # (fillers share identifiers; they have no rows)
        read_of.update({b"p%d" % k: k for k in planted})
        n_primary, _ = R.check_rows(sam["sam"], read_of, bases, quals, not single)
        seen = set()
        for f in samseq_check.sam_rows(sam["sam"]):
            flag = int(f[1])
            if not flag & 0x100:
                seen.add((f[0], bool(flag & 0x80)))
                assert f[0].startswith(b"p"), "a filler read has a row: %r" % f[0]
        mates = (False,) if single else (False, True)
        without = [(k, m) for k in planted for m in mates if (b"p%d" % k, m) not in seen]
        assert not without, (c["name"], "planted reads without a primary row", without[:10])
        assert n_primary == len(planted) * len(mates), (c["name"], n_primary, len(planted))
        assert not planted or len(got["ov"]) >= len(planted) * len(mates)
        return len(bases), len(planted) * len(mates), n_primary
    finally:
        rig.lanes_plain()
        for h in hs:
            h.close()


def _cases(synth, prefix):
    return [c for c in S.small_cases(synth) if c["name"].startswith(prefix)]


def test_seam_matrix(rig, synth):
    """every (terminator kind x seam x placement x line role) cell in R1 and in R2, R2 starting at 0, 1, 7, 8 and 15 mod 16 inside
    the device text, and single end; the census is asserted on the texts that are submitted"""
    cases = _cases(synth, "matrix")
    assert [len(c["r1"]) % 16 for c in cases if c["r2"] is not None] == list(S.R2_STARTS)
    assert sum(c["r2"] is None for c in cases) == 1
    for c in cases:
        for name, t in (("R1", c["r1"]), ("R2", c["r2"])):
            if t is not None:
                hits = S.census(t)
                assert [x for x in S.MATRIX if x not in hits] == [], (c["name"], name)
                print("%s %s: %d bytes, %d of %d cells hit, %d hits" % (c["name"], name, len(t), sum(x in hits for x in S.MATRIX),
                                                                      len(S.MATRIX), sum(hits.values())))
        n, planted, primary = check_case(rig, c)
        print("%s: %d reads, %d planted, %d primary rows" % (c["name"], n, planted, primary))
        assert planted > 1000


def test_lines_longer_than_a_tile(rig, synth):
    cases = _cases(synth, "long_lines")
    assert len(cases) == 2
    for c in cases:
        for t in (c["r1"], c["r2"]):
            if t is None:
                continue
            ls, _ = S.lines(t)
            span = max(e // 4096 - s // 4096 for s, e, _ in ls)
            assert span >= 2, "no line spans three tiles"
            lens = {ls[i][1] - ls[i][0] for i in range(1, len(ls), 4)}
            assert {255, 256, 257, 271, 272, 273} & lens and {4095, 4096, 4097} & lens and {0, 1, 15, 16, 17} & lens
            # the 4 097-base line starts on a tile's last byte and its terminator is the first byte of the tile after the next
            assert any(e - s == 4097 and s % 4096 == 4095 for s, e, _ in ls)
        n, planted, primary = check_case(rig, c)
        print("%s: %d reads, %d planted, %d primary rows" % (c["name"], n, planted, primary))
        assert planted >= 13
    both = {len(b) for c in cases for t in (c["r1"], c["r2"]) if t is not None for b in S.records(t)[1]}
    assert {0, 1, 15, 16, 17, 255, 256, 257, 271, 272, 273, 4095, 4096, 4097} <= both


def test_where_the_text_ends(rig, synth):
    cases = [c for c in S.small_cases(synth) if c["name"].split("_")[0] in ("ends", "prefix", "stream", "last", "max", "blank")]
    assert len(cases) == 20
    for c in cases:
        n, planted, primary = check_case(rig, c)
        print("%s: %d reads, %d planted, %d primary rows" % (c["name"], n, planted, primary))
    by = {c["name"]: c for c in cases}
    c = by["prefix_ends_in_cr_behind_a_tile_seam"]
    assert (len(c["r1"]) - 1) % 4096 == 0 and c["r1"][-1:] == b"\r"           # the scan is a whole tile shorter than the text
    a, b = S.records(c["r1"], 0, False), S.records(c["r1"], 0, True)
    assert len(a[0]) + 1 == len(b[0]) and a[3] < len(c["r1"]) == b[3]           # the record stays open in the prefix
    c = by["max_pairs_cuts_behind_CRLF_at_4095"]
    assert S.records(c["r1"], c["max_pairs"])[3] == 4097 and c["r1"][4095:4097] == b"\r\n"
    c = by["last_record_completed_by_the_empty_line"]
    assert len(S.records(c["r1"])[0]) == len(S.records(c["r1"], 0, False)[0]) + 1


def test_identifier_windows(rig, synth):
    cases = _cases(synth, "identifier_windows")
    assert len(cases) == 2
    for c in cases:
        n, _, _ = check_case(rig, c)
        assert n > 100
    ids = S.records(cases[0]["r1"])[0]
    assert {len(i) for i in ids} >= set(range(0, 34))
    assert ids[-1] == b"z" * 15 and cases[0]["r2"][:4] == b"@q/2"               # R1's last header is followed by R2's '/' and ' '


def test_errors_are_the_hosts_and_the_context_goes_on(rig, synth):
    kslam, ctx, F = rig.K, rig.ctx, rig.F
    cases = _cases(synth, "quality_line") + _cases(synth, "the_same") + _cases(synth, "r2_one") + _cases(synth, "r1_one")
    assert len(cases) == 4
    good = _cases(synth, "ends_at_a_tile_seam_eof_1")[0]
    for c in cases:
        hs = [_host_text(kslam, t) for t in (c["r1"], c["r2"])]
        try:
            # what the host says about the same texts: the column parser for the counts, the index-only entry for the lengths
            # (kslam_fastq_parse_pair keeps a ragged record and leaves it to the tail; kslam_fastq_index_pair refuses it)
            with pytest.raises(kslam.KslamError) as host:
                if c["error"] == "quality line":
                    F.index_pair(hs[0].ptr, len(c["r1"]), hs[1].ptr, len(c["r2"]))
                else:
                    F.parse_pair(c["r1"], c["r2"])
            assert c["error"] in str(host.value)
            rig.lanes_plain()
            tk = ctx.submit_batch_fastq_text(hs[0].ptr, len(c["r1"]), hs[1].ptr, len(c["r2"]))
            with pytest.raises(kslam.KslamError) as dev:
                rig.collect(tk)
            assert str(dev.value) == str(host.value) and dev.value.status == host.value.status, c["name"]
        finally:
            for h in hs:
                h.close()
        n, planted, primary = check_case(rig, good)                             # the context goes on
        assert planted and primary == planted
    # the ragged record is the one a tile seam cuts
    c = cases[0]
    ls, _ = S.lines(c["r1"])
    assert ls[-3][0] < 4096 <= ls[-1][1] and ls[-1][1] - ls[-1][0] == ls[-3][1] - ls[-3][0] + 1


def test_past_the_first_scan_tile(kslam, synth):
    """one pair of streams of more than 16 MiB each, all three terminators, irregular records, more than 4 096 records"""
    t0 = time.time()
    c = S.big_case(synth)
    rig = Rig(kslam, synth, "big")
    try:
        n, planted, primary = check_case(rig, c)
    finally:
        rig.close()
    print("%s: %d + %d bytes, %d reads, %d planted, %d primary rows, %.1f s" % (c["name"], len(c["r1"]), len(c["r2"]), n, planted, primary,
                                                                              time.time() - t0))
    assert min(len(c["r1"]), len(c["r2"])) > 4096 * 4096 and n > 2 * 4096 and planted > 4096
