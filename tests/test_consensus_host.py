"""The FASTA writer of the consensus caller (kslam_consensus_write, include/kslam_consensus.h) byte for byte against the
restatement's writer (tests/consensus_ref.py) -- lines of 59, 60 and 61 bases and an empty sequence -- the parser back from the
file, the refusals of the writer and of the host twin, and the exported symbols.  No GPU."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consensus_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def CN(kslam):
    return importlib.import_module("kslam_amd.consensus")


@pytest.fixture(scope="module")
def T(kslam):
    return importlib.import_module("kslam_amd.tail")


def _index(T, lengths, loci):
    goff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    return T.IndexArrays(np.frombuffer(b"A" * int(goff[-1]) + bytes(8), dtype=np.uint8)[:int(goff[-1])], goff, loci, np.arange(1, len(loci) + 1))


def _rows(CN, seqs, entries=None):
    rows = np.zeros(len(seqs), dtype=CN.ROW_DT)
    off = 0
    for i, s in enumerate(seqs):
        rows[i]["entry"], rows[i]["seq_off"], rows[i]["seq_len"] = (entries[i] if entries else i), off, len(s)
        rows[i]["entry_len"], rows[i]["covered"], rows[i]["substitutions"], rows[i]["deleted"] = 70 + i, 60 + i, i, 2 * i
        rows[i]["insertions"], rows[i]["inserted_bases"], rows[i]["ambiguous"] = 3 * i, 7 * i, 5 * i
        off += len(s)
    return rows


def test_library_exports_every_consensus_symbol(kslam, CN):
    h = open(os.path.join(ROOT, "include", "kslam_consensus.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 11 and declared == sorted(CN.EXPORTS) and all(hasattr(L, n) for n in declared)
    assert CN.ROW_DT.itemsize == 80 and ctypes.sizeof(CN.Stats) == 80 and ctypes.sizeof(CN.Params) == 16
    assert CN.STAT_NAMES == R.STAT_NAMES and (CN.FILL_N, CN.FILL_REF, CN.MAX_INS) == (R.FILL_N, R.FILL_REF, R.MAX_INS)
    assert kslam.lib().kslam_abi_version() == 10             # additive: the version stays


def test_the_file_byte_for_byte_and_back(CN, T):
    rng = np.random.default_rng(5)
    seqs = [R.random_bases(rng, n) for n in (59, 60, 61, 0, 1, 120, 121)]
    loci = [b"LOCUS_%d.%d" % (e, e % 3) for e in range(len(seqs))]
    rows = _rows(CN, seqs)
    text = CN.report_bytes(_index(T, [100] * len(seqs), loci), rows, b"".join(seqs))
    assert text == R.fasta_bytes(rows, seqs, loci)
    lines = text.split(b"\n")
    assert lines[0] == b">LOCUS_0.0 kslam_consensus entry_length=70 covered=60 substitutions=0 deletions=0 insertions=0 ambiguous=0"
    assert [len(x) for x in lines[1:9]] == [59, len(lines[2]), 60, len(lines[4]), 60, 1, len(lines[7]), len(lines[8])] and lines[2][:1] == lines[4][:1] == b">"
    assert lines[7].startswith(b">LOCUS_3.0 ") and lines[8].startswith(b">LOCUS_4.1 ")      # the empty sequence has no line
    parsed = CN.parse(text)
    assert [(p[0].encode(), p[2].encode()) for p in parsed] == list(zip(loci, seqs))
    assert [tuple(p[1][k] for k in CN.HEADER_FIELDS) for p in parsed] == \
        [tuple(int(r[k]) for k in ("entry_len", "covered", "substitutions", "deleted", "insertions", "ambiguous")) for r in rows]
    assert CN.report_bytes(_index(T, [100], [b"x"]), rows[:0], b"") == b"" and CN.parse(b"") == []
    # rows need not come in entry order for the writer, and two rows may share nothing but the array
    back = _rows(CN, seqs[:3], entries=[2, 0, 1])
    assert CN.report_bytes(_index(T, [100] * 3, loci[:3]), back, b"".join(seqs[:3])) == R.fasta_bytes(back, seqs[:3], loci)
    for bad in (b"ACGT\n", b">x kslam_consensus entry_length=1\nA\n", b">x other entry_length=1 covered=1 substitutions=0 deletions=0 insertions=0 ambiguous=0\n",
                b">x kslam_consensus entry_length=1 covered=1 substitutions=0 deletions=0 insertions=0 ambiguous=0\n" + b"A" * 61 + b"\n",
                b">x kslam_consensus entry_length=1 covered=1 substitutions=0 deletions=0 insertions=0 ambiguous=0\nAC\nAC\n"):
        with pytest.raises(ValueError):
            CN.parse(bad)


def test_refusals(CN, T):
    b = R.CB("x", [b"ACGT" * 25, b"TTTT"])
    b.group([(0, b.gapped(0, 0, [(20, "M")], 0, mismatch_at=(3,)), b.gapped(0, 30, [(20, "M")], 1, mismatch_at=(3,)))])
    b.single(b.gapped(1, 0, [(4, "M")], 0, mismatch_at=(0,)))
    c = b.done()
    args = lambda **kw: [kw.get(k, c[k]) for k in ("gbases", "goff", "ov", "pool", "rbases", "roff", "rp", "pr")]   # noqa: E731
    rows, seq, _ = CN.tail_consensus(*args())
    assert len(rows) == 2 and len(seq) == 104
    bad = c["pr"].copy()
    bad["r2"][0] = len(c["ov"])
    with pytest.raises(Exception, match="refers to overlap record"):
        CN.tail_consensus(*args(pr=bad))
    rp = c["rp"].copy()
    rp["count"][1] = 2
    with pytest.raises(Exception, match="outside the pairs array"):
        CN.tail_consensus(*args(rp=rp))
    rp = c["rp"].copy()
    rp["first"][1] = 0
    with pytest.raises(Exception, match="ascend"):
        CN.tail_consensus(*args(rp=rp))
    ov = c["ov"].copy()
    ov["cigar_off"][1] = len(c["pool"])
    with pytest.raises(Exception, match="CIGAR slice lies outside the pool"):
        CN.tail_consensus(*args(ov=ov))
    ov = c["ov"].copy()
    ov["read"][2] = len(c["roff"]) - 1
    with pytest.raises(Exception, match="refers to read"):
        CN.tail_consensus(*args(ov=ov))
    for params, message in (((0, 500, 0, 1), "min_depth"), ((1, 499, 0, 1), "call_permille"), ((1, 1000, 0, 1), "call_permille"), ((1, 500, 2, 1), "fill")):
        with pytest.raises(Exception, match=message):
            CN.tail_consensus(*args(), *params)
    # the writer: an entry with an empty locus is refused before anything is written; an entry outside the view too
    fd = os.memfd_create("fasta")
    try:
        with pytest.raises(Exception, match="empty locus"):
            CN.write(_index(T, [100, 4], [b"first", b""]), rows, seq, fd)
        wrong = rows.copy()
        wrong["entry"][-1] = 2
        with pytest.raises(Exception, match="not of this index"):
            CN.write(_index(T, [100, 4], [b"first", b"second"]), wrong, seq, fd)
        assert os.lseek(fd, 0, os.SEEK_END) == 0
    finally:
        os.close(fd)
