"""tests/samseq_check.py on hand-made inputs: what it accepts, and one bad input per rejection."""
import struct

import pytest

import samseq_check as S


def record(name=b"r1", flag=0, cigar=((4, "M"),), seq=b"ACGT", qual=b"IIII", l_seq=None, last_nibble=0, extra=0, tags=b""):
    """one BAM record on reference 0 at position 0; qual None = 0xFF; extra = bytes added to block_size's claim"""
    ops = b"".join(struct.pack("<I", n << 4 | "MIDNSHP=X".index(op)) for n, op in cigar)
    n = len(seq)
    packed = bytearray((n + 1) // 2)
    for i, c in enumerate(seq):
        packed[i >> 1] |= S.NT16.index(bytes([c])) << (0 if i & 1 else 4)
    if n & 1 and last_nibble:
        packed[-1] |= last_nibble
    q = b"\xff" * n if qual is None else bytes(c - 33 for c in qual)
    span = sum(k for k, op in cigar if op in "MD") if cigar else 0
    body = struct.pack("<iiBBHHHiiii", 0, 0, len(name) + 1, 50, S.B.reg2bin(0, max(1, span)), len(cigar), flag,
                       n if l_seq is None else l_seq, -1, -1, 0) + name + b"\0" + ops + bytes(packed) + q + tags
    return struct.pack("<i", len(body) + extra) + body


REFS = [(b"chr", 1000)]


def test_accepts_and_renders_records():
    data = record() + record(b"r2", 16, ((2, "S"), (3, "M")), b"NACGT", None) + record(b"r3", 256, (), b"", b"")
    lines = S.records(data, 0, REFS)
    assert lines[0] == b"r1\t0\tchr\t1\t50\t4M\t*\t0\t0\tACGT\tIIII"
    assert lines[1] == b"r2\t16\tchr\t1\t50\t2S3M\t*\t0\t0\tNACGT\t*"
    assert lines[2] == b"r3\t256\tchr\t1\t50\t*\t*\t0\t0\t*\t*"
    assert S.strip_records(data) == record(seq=b"", qual=b"") + record(b"r2", 16, ((2, "S"), (3, "M")), b"", b"") + record(b"r3", 256, (), b"", b"")


def test_rejects_l_seq_against_cigar():
    with pytest.raises(S.BamError, match="CIGAR"):
        S.records(record(cigar=((3, "M"),)), 0, REFS)
    with pytest.raises(S.BamError, match="CIGAR"):
        S.records(record(cigar=((2, "M"), (1, "D"), (1, "I")), seq=b"ACGT"), 0, REFS)


def test_rejects_nonzero_last_nibble():
    S.records(record(cigar=((3, "M"),), seq=b"ACG", qual=b"III"), 0, REFS)
    with pytest.raises(S.BamError, match="nibble"):
        S.records(record(cigar=((3, "M"),), seq=b"ACG", qual=b"III", last_nibble=1), 0, REFS)


def test_rejects_block_size_that_does_not_cover_seq_and_qual():
    good = record()
    short = struct.pack("<i", 32 + 3 + 4 + 2 + 3) + good[4:4 + 32 + 3 + 4 + 2 + 3]   # one qual byte short
    with pytest.raises(S.BamError, match="block_size"):
        S.records(short, 0, REFS)
    with pytest.raises(S.BamError, match="block_size"):
        S.records(record(extra=5), 0, REFS)   # claims bytes the data does not hold


def test_rejects_qual_above_93_but_takes_all_ff():
    S.records(record(qual=None), 0, REFS)
    with pytest.raises(S.BamError, match="93"):
        S.records(record(qual=bytes([33 + 94, 73, 73, 73])), 0, REFS)
    with pytest.raises(S.BamError, match="93"):
        S.records(record(qual=bytes([33 + 222, 33 + 222, 33 + 222, 73])), 0, REFS)   # 0xFF in part is no "no qualities"


def test_text_rows():
    ok = b"r1\t0\tchr\t1\t50\t4M\t*\t0\t0\tACGT\tIIII\tAS:i:8\nr1\t256\tchr\t9\t0\t4M\t*\t0\t0\t*\t*\nr2\t4\tchr\t1\t0\t*\t*\t0\t0\tAC\t*\n"
    rows = S.sam_rows(ok)
    assert [r[9] for r in rows] == [b"ACGT", b"*", b"AC"]
    assert S.strip_text(ok) == ok.replace(b"ACGT\tIIII", b"*\t*").replace(b"AC\t*", b"*\t*")
    with pytest.raises(S.SamError, match="QUAL"):
        S.sam_rows(b"r1\t0\tchr\t1\t50\t4M\t*\t0\t0\tACGT\tIII\n")        # SEQ / QUAL length mismatch
    with pytest.raises(S.SamError, match="CIGAR"):
        S.sam_rows(b"r1\t0\tchr\t1\t50\t1S4M\t*\t0\t0\tACGT\tIIII\n")     # SEQ against the CIGAR
    with pytest.raises(S.SamError, match="QUAL without SEQ"):
        S.sam_rows(b"r1\t0\tchr\t1\t50\t4M\t*\t0\t0\t*\tIIII\n")
    with pytest.raises(S.SamError, match="columns"):
        S.sam_rows(b"r1\t0\tchr\t1\t50\t4M\t*\t0\t0\tACGT\n")
