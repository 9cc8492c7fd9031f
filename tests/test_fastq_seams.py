"""The reference of tests/test_gpu_fastq_index.py pinned on the CPU, and the seams its texts hit.

tests/fastq_seams.py: records() is a plain byte loop; here it is held to the restatement of the reference's reader
(oracle.fastq_read), to the reference's own reader where it is compiled (oracle.have_ref_fastq()) and to the library's host
parser, on every text the GPU test submits and on tests/test_fastq.py's random streams.  The census of the built texts must
show every cell of the seam matrix in R1 and in R2: a condition, not a measurement.
Host-only: nothing here needs a GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest

import fastq_seams as S
from test_fastq import make_text


@pytest.fixture(scope="module")
def F(kslam):
    return importlib.import_module("kslam_amd.fastq")


def _pin(F, oracle, text, max_records, at_eof, tmp_path=None):
    """plain reader == host parser (any at_eof) == restatement (== reference) at the true end of the stream"""
    ids, bases, quals, consumed = S.records(text, max_records, at_eof)
    batch, used = F.parse(text, max_reads=max_records, at_eof=at_eof, threads=3)
    assert (batch.ids, batch.bases, batch.quality) == (ids, bases, quals)
    assert used == consumed
    batch.close()
    if at_eof:
        b, q, i, pos = oracle.fastq_read(text, max_reads=max_records or 0xFFFFFFFF)
        assert (i, b, q) == (ids, bases, quals)
        if max_records and len(ids) == max_records:
            assert pos == consumed
        if tmp_path is not None and oracle.have_ref_fastq() and not max_records:
            path = str(tmp_path / "x.fq")
            open(path, "wb").write(text)
            b, q, i, _ = oracle.ref_fastq_read(path)
            assert (i, b, q) == (ids, bases, quals), "the plain reader differs from the real reference"
    return ids, bases, quals, consumed


def _pin_case(F, oracle, kslam, c, tmp_path):
    streams = [t for t in (c["r1"], c["r2"]) if t is not None]
    got = [_pin(F, oracle, t, c["max_pairs"], c["at_eof"], tmp_path) for t in streams]
    if len(streams) == 2:
        # the two entry points the device test's errors are compared with
        b1, b2 = C.create_string_buffer(streams[0], len(streams[0]) + 64), C.create_string_buffer(streams[1], len(streams[1]) + 64)
        if c["error"]:
            with pytest.raises(kslam.KslamError, match=c["error"]):
                F.index_pair(C.addressof(b1), len(streams[0]), C.addressof(b2), len(streams[1]), max_pairs=c["max_pairs"], at_eof=c["at_eof"])
            return got
        ix, u1, u2 = F.index_pair(C.addressof(b1), len(streams[0]), C.addressof(b2), len(streams[1]), max_pairs=c["max_pairs"],
                                  at_eof=c["at_eof"])
        assert (u1, u2) == (got[0][3], got[1][3]) and ix.ids == got[0][0] + got[1][0]
        ix.close()
        # planted reads are whole and are mates: the same record of both streams, unique identifiers
        for k in c["planted"]:
            if k < len(got[0][0]):
                assert got[0][0][k] == got[1][0][k] == b"p%d" % k
    return got


def test_plain_reader_on_every_text_of_the_device_test(kslam, F, oracle, synth, tmp_path):
    n = 0
    for c in S.small_cases(synth):
        _pin_case(F, oracle, kslam, c, tmp_path)
        n += 1
    assert n > 30


def test_plain_reader_on_the_16_mib_text(kslam, F, oracle, synth, tmp_path):
    c = S.big_case(synth)
    got = _pin_case(F, oracle, kslam, c, None)
    assert all(len(g[0]) > 4096 for g in got)
    kinds = {k for t in (c["r1"], c["r2"]) for (k, _, _, _) in S.census(t)}
    assert {"LF", "CRLF", "CR"} <= kinds
    for t in (c["r1"], c["r2"]):
        ls, _ = S.lines(t)
        sizes = {ls[i + 3][2] - ls[i][0] for i in range(0, len(ls) - 3, 4)}
        assert len(sizes) > 500, "record lengths are meant to be irregular"


@pytest.mark.parametrize("seed", range(12))
def test_plain_reader_on_random_streams(F, oracle, tmp_path, seed):
    rng = np.random.default_rng(seed)
    text = make_text(rng, int(rng.integers(0, 400)), truncate=seed % 3 == 1, blank_tail=seed % 4)
    if seed == 7:
        text = text.rstrip(b"\r\n")
    if seed == 9:
        text = text.rstrip(b"\r\n") + b"\r"
    for at_eof in (True, False):
        for max_records in (0, 1, 7, 50):
            _pin(F, oracle, text, max_records, at_eof, tmp_path)


def test_planted_reads_occur_once_in_the_genomes(synth):
    g = S.genomes(synth, "small")
    cat = b"|".join(g)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    n = 0
    for c in S.small_cases(synth):
        if not c["planted"] or c["error"]:
            continue
        for t in (c["r1"], c["r2"]):
            if t is None:
                continue
            ids, bases, _, _ = S.records(t, c["max_pairs"], c["at_eof"])
            for k in c["planted"]:
                if k < len(bases) and n % 7 == 0:      # (one in seven: the count is a scan of the genomes)
                    assert len(bases[k]) >= 50
                    assert cat.count(bases[k]) + cat.count(bases[k].translate(comp)[::-1]) == 1
                n += 1
    assert n > 5000


def test_every_cell_of_the_seam_matrix_in_r1_and_in_r2(synth):
    """5 terminator kinds x 4 seams x 2 placements x 4 line roles = 160 cells, per stream"""
    assert len(S.MATRIX) == 160
    n = 0
    for c in S.matrix_cases(S.genomes(synth, "small")):
        for name, t in (("R1", c["r1"]), ("R2", c["r2"])):
            if t is not None:
                assert S.missing_cells(t) == [], (c["name"], name)
                n += 1
    assert n == 2 * len(S.R2_STARTS) + 1


def test_census_names_the_cell():
    """the census on texts small enough to read: one terminator at one seam each"""
    def one(text):
        return sorted(S.census(text))
    pad = b"@" + b"h" * 14          # 15 bytes
    assert one(pad + b"\nAC\n+\nII\n") == [("LF", 16, "last", 0)]
    assert one(pad + b"h\nAC\n+\nII\n") == [("LF", 16, "first", 0)]
    assert one(pad + b"\r\nAC\n+\nII\n") == [("CRLF", 16, "last", 0)]
    assert one(pad + b"\rAC\n+\nII\n") == [("CR", 16, "last", 0)]
    assert one(pad + b"\r\r\n+\n\n") == [("CRCRLF", 16, "last", 0)]
    # (the "\r" of "\n\r" is also a lone "\r" in its own right: the first byte behind the seam, ending the empty bases line)
    assert one(pad + b"\n\r+\n\n") == [("CR", 16, "first", 1), ("LFCR", 16, "last", 0)]
    assert one(b"@" + b"h" * 1019 + b"\nAC\r\n+\nII\n") == [("CRLF", 1024, "last", 1)]
    assert one(b"@" + b"h" * 4090 + b"\nAC\n+\r\nII\n") == [("CRLF", 4096, "first", 2)]
    assert one(b"@" + b"h" * 16374 + b"\nAC\n+\nII\r@x\n\n+\n\n")[0] == ("CR", 16384, "last", 3)
