"""The coordinate-sorted BAM through the lanes and the batch loop (kslam_stream_set_bam_sort, SLAM --sam-sorted; include/
kslam_bamsort.h).  The yardstick is existing behaviour: the records of the unsorted --sam-bam file of the same run, stably sorted
by the restatement (tests/bamsort_ref.py).  Three ragged batches, paired and single-end, with and without --sam-seq --sam-unmapped:
the file is bgzf(header) + bgzf(stream) + EOF, the index passes tests/bai_check.py and equals the restatement's, one lane, three
lanes, the host formatter and a pseudo-assembly left to the host give the same bytes, and every other output file is what it is
without --sam-sorted.  A call that fails in a batch leaves both descriptors empty and the switch off."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import bai_check
import bam_check
import bamsort_ref as R
import bgzf_check
import deflate_ref
from test_cli import SLAM, _run
from test_gpu_bgzf import _cl, _run_env

pytestmark = pytest.mark.gpu
TAIL = ["--num-reads-at-once", "190"]      # 500 records: batches of 190, 190 and 120


def _split_file(blob):
    """a BAM file -> (header text, [(name, length)], record stream)"""
    data = bgzf_check.check(blob)
    text, refs, pos = bam_check.parse_header(data)
    return text, refs, data[pos:]


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
@pytest.mark.parametrize("extra", [[], ["--sam-seq", "--sam-unmapped"]], ids=["plain", "seq_unmapped"])
def test_sorted_file_and_index_of_three_ragged_batches(kslam, synth, tmp_path, paired, extra):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    Z = importlib.import_module("kslam_amd.bgzf")
    BS = importlib.import_module("kslam_amd.bamsort")
    case = RL.make_case(synth, n_pairs=500, seed=7311, paired=paired)
    RL.write_case(case, tmp_path, D)
    files = ["R1.fq", "R2.fq"] if paired else ["R1.fq"]
    unsorted = ["--db=db", "--sam-file", "u.bam", "--output-file=u", "--sam-bam"] + extra + TAIL + files
    args = ["--db=db", "--sam-file", "s.bam", "--output-file=s", "--sam-sorted"] + extra + TAIL + files
    _run(unsorted, tmp_path)
    _run(args, tmp_path)
    bam, bai = (tmp_path / "s.bam").read_bytes(), (tmp_path / "s.bam.bai").read_bytes()
    u_text, u_refs, u_stream = _split_file((tmp_path / "u.bam").read_bytes())
    text, refs, stream = _split_file(bam)
    # the records: those of the unsorted file, stably sorted; the header: the unsorted file's with its sort order rewritten
    assert len(R.split(u_stream)) > 500
    assert stream == R.sort_batches([u_stream]) and stream != u_stream
    assert refs == u_refs and text == R.coordinate_header(u_text.replace(_cl(unsorted), _cl(args)))
    assert text.startswith(b"@HD\tVN:1.0\tSO:coordinate\n")
    # the file: bgzf(header) + bgzf(stream) + EOF
    header = R.bam_header(text, refs)
    ctx = kslam.Context()
    try:
        head, body = Z.compress(ctx, header), Z.compress(ctx, stream)
    finally:
        ctx.close()
    assert bam == head + body + bgzf_check.EOF_MARKER
    assert head == deflate_ref.compress(header)
    # the index: what an index must mean, and the restatement's bytes
    sizes = [m[1] for m in bgzf_check.members(body + bgzf_check.EOF_MARKER)][:-1]
    assert bai == R.bai(stream, len(refs), sizes, len(head))
    got = bai_check.check(bam, bai)
    assert got["n_records"] == len(R.split(stream))
    assert len(BS.parse_bai(bai)["refs"]) == len(refs)
    # every other output is what it is without --sam-sorted
    for suffix in ("", "_abbreviated", "_PerRead"):
        assert (tmp_path / ("s" + suffix)).read_bytes() == (tmp_path / ("u" + suffix)).read_bytes(), suffix
    # one lane, three lanes, the host formatter, a pseudo-assembly left to the host: the same bytes
    for env in ({"KSLAM_LANES": "1"}, {"KSLAM_LANES": "3"}, {"KSLAM_HOST_SAM_TEXT": "1"}, {"KSLAM_LANES": "2", "KSLAM_PSEUDO_CAP": "3"}):
        _run_env(args, tmp_path, env)
        assert (tmp_path / "s.bam").read_bytes() == bam and (tmp_path / "s.bam.bai").read_bytes() == bai, env


def test_sam_index_names_the_file_and_dynamic_deflate(kslam, synth, tmp_path):
    import ref_loop_case as RL
    D = importlib.import_module("kslam_amd.db")
    case = RL.make_case(synth, n_pairs=300, seed=7312)
    RL.write_case(case, tmp_path, D)
    args = ["--db=db", "--sam-file", "s.bam", "--just-align", "--sam-sorted", "--sam-index", "elsewhere.idx", "--sam-deflate", "dynamic"] + TAIL + \
        ["R1.fq", "R2.fq"]
    _run(args, tmp_path)
    assert not (tmp_path / "s.bam.bai").exists()
    bam, bai = (tmp_path / "s.bam").read_bytes(), (tmp_path / "elsewhere.idx").read_bytes()
    bai_check.check(bam, bai)
    fixed = [a for a in args if a not in ("--sam-deflate", "dynamic")]
    _run(fixed, tmp_path)
    assert len((tmp_path / "s.bam").read_bytes()) > len(bam)


def test_a_failed_batch_leaves_both_files_empty_and_the_switch_off(kslam, synth, tmp_path):
    from test_gpu_bam import _stream
    from test_gpu_end_to_end import _fastq_text
    from test_gpu_stream import _make_case
    D = importlib.import_module("kslam_amd.db")
    T = importlib.import_module("kslam_amd.tail")
    S = importlib.import_module("kslam_amd.stream")
    BS = importlib.import_module("kslam_amd.bamsort")
    dbdir, _, rb, quals, ids, r1, r2 = _make_case(synth, tmp_path, 600, b"\n", seed=93)
    short2 = _fastq_text(rb[600:1100], quals[600:1100], ids[:500], 2, b"\n")      # R2 one hundred records short: the third batch is refused
    db = D.Database.load(dbdir / "database")
    ctx = kslam.Context()
    bases_pp, lens_p = db.entry_pointers()
    ctx._chk(ctx._L.kslam_set_index(ctx._h, db.n_entries, C.cast(bases_pp, C.c_void_p), C.cast(lens_p, C.c_void_p)))
    header = T.sam_header(db, b"SLAM --db db R1.fq R2.fq")
    P = T.TailParams.default()
    bufs = []
    for t in (r1, r2, short2):
        h = kslam.HostBuffer(len(t) + 64)
        h.a[:len(t)] = np.frombuffer(t, dtype=np.uint8)
        bufs.append(h)

    def sorted_call(r2_buf, r2_len, name):
        sam = os.open(str(tmp_path / (name + ".bam")), os.O_RDWR | os.O_CREAT | os.O_TRUNC)
        idx = os.open(str(tmp_path / (name + ".bai")), os.O_RDWR | os.O_CREAT | os.O_TRUNC)
        try:
            return S.classify_stream_native(ctx, db, bufs[0].ptr, len(r1), r2_buf.ptr, r2_len, 200, P, sam_fd=sam, sam_header=header, sam_sorted=True,
                                            sam_index_fd=idx)
        finally:
            os.close(sam)
            os.close(idx)
    try:
        with pytest.raises(kslam.KslamError, match="sam_fd"):
            S.classify_stream_native(ctx, db, bufs[0].ptr, len(r1), bufs[1].ptr, len(r2), 200, P, sam_sorted=True)
        assert BS.stream_get_bam_sort(ctx) == (False, -1) and not BS.get_bam_sort(ctx)
        first = sorted_call(bufs[1], len(r2), "first")
        good = ((tmp_path / "first.bam").read_bytes(), (tmp_path / "first.bai").read_bytes())
        bai_check.check(*good)
        with pytest.raises(kslam.KslamError, match="mismatch in R1 and R2"):
            sorted_call(bufs[2], len(short2), "bad")
        assert (tmp_path / "bad.bam").read_bytes() == b"" and (tmp_path / "bad.bai").read_bytes() == b""
        assert not BS.get_bam_sort(ctx) and BS.stream_get_bam_sort(ctx) == (False, -1)
        again = sorted_call(bufs[1], len(r2), "again")      # the next call starts from nothing
        assert ((tmp_path / "again.bam").read_bytes(), (tmp_path / "again.bai").read_bytes()) == good
        # stats->sam_bytes: the record members' compressed bytes
        members = bgzf_check.members(good[0])
        head_len, at, k = len(BS.tail_bam_sort_header(header)), 0, 0
        while at < head_len:
            at += members[k][3]
            k += 1
        assert first["sam_bytes"] == again["sam_bytes"] == sum(m[1] for m in members[k:-1])
        # and a plain call afterwards writes what it always wrote
        _stream(kslam, S, ctx, db, bufs[0].ptr, len(r1), bufs[1].ptr, len(r2), 200, P, header, str(tmp_path / "p.sam"))
        assert (tmp_path / "p.sam").read_bytes().startswith(b"@HD\tVN:1.0\tSO:unsorted")
    finally:
        ctx.close()
