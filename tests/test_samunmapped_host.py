"""include/kslam_samunmapped.h on the host (no GPU): the twin kslam_tail_sam_unmapped against the rules restated in
tests/unmapped_rules.py, as text and as BAM records, with and without SEQ / QUAL, paired and single-end, with and without
qualities; ids of length 0, 1, 254 and 255; the rules and the strict reader (tests/unmapped_check.py) pinned on hand-written
rows."""
import ctypes
import importlib
import os
import re
import struct

import numpy as np
import pytest

import bam_check
import samseq_check as S
import samseq_rules as R
import unmapped_check as UC
import unmapped_rules as UR
from test_samseq_host import made_up_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T(kslam):
    return importlib.import_module("kslam_amd.tail")


@pytest.fixture(scope="module")
def Q(kslam):
    return importlib.import_module("kslam_amd.samseq")


@pytest.fixture(scope="module")
def U(kslam):
    return importlib.import_module("kslam_amd.samunmapped")


def read_pairs_of(T, with_rows, n_records, paired, empty=()):
    """the final read pairs of a batch in which the records `with_rows` have one alignment pair each; `empty`: records whose
    group is there without alignment pairs"""
    recs = sorted(set(with_rows) | set(empty))
    rp = np.zeros(len(recs), dtype=T.READ_PAIR_DT)
    at = 0
    for k, p in enumerate(recs):
        rp[k]["r1_read"] = p
        rp[k]["r2_read"] = p + n_records if paired else 0
        rp[k]["first"] = at
        rp[k]["count"] = 0 if p in empty else 1
        at += int(rp[k]["count"])
    return rp


# ---- the rules and the reader themselves, on rows written by hand ----
def test_the_rules_by_hand():
    ids, bases, quals = [b"a", b"b", b"a", b"b"], [b"ACG", b"", b"TTn", b"G"], [b"I#5", b"", b"!!~", b"J"]
    assert UR.expected_text(ids, bases, quals, [0, 1], 2, True, True) == (
        b"a\t77\t*\t0\t0\t*\t*\t0\t0\tACG\tI#5\n" b"a\t141\t*\t0\t0\t*\t*\t0\t0\tTTn\t!!~\n"
        b"b\t77\t*\t0\t0\t*\t*\t0\t0\t*\t*\n" b"b\t141\t*\t0\t0\t*\t*\t0\t0\tG\tJ\n")
    assert UR.expected_text(ids, bases, quals, [1], 2, True, False) == b"b\t77\t*\t0\t0\t*\t*\t0\t0\t*\t*\n" b"b\t141\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"
    assert UR.expected_text(ids, bases, None, [2], 4, False, True) == b"a\t4\t*\t0\t0\t*\t*\t0\t0\tTTn\t*\n"
    assert UR.expected_text(ids, bases, quals, [], 2, True, True) == b""
    # refID -1, pos -1, l_read_name 2, mapq 0, bin 4680 = 0x1248, n_cigar_op 0, flag 141 = 0x8D, l_seq 3, next -1 / -1, tlen 0,
    # "a\0", T T n -> 8 8 15 packed high nibble first with a zero last nibble, qualities - 33
    rec = UR.expected_records(ids, bases, quals, [0], 2, True, True)
    r2 = (b"\x27\x00\x00\x00" b"\xff\xff\xff\xff" b"\xff\xff\xff\xff" b"\x02\x00\x48\x12" b"\x00\x00\x8d\x00" b"\x03\x00\x00\x00"
          b"\xff\xff\xff\xff" b"\xff\xff\xff\xff" b"\x00\x00\x00\x00" b"a\x00" b"\x88\xf0" b"\x00\x00\x5d")
    assert rec.endswith(r2) and len(rec) == 2 * len(r2)
    assert UR.expected_records(ids, bases, None, [3], 4, False, True) == (
        b"\x24\x00\x00\x00" + b"\xff" * 8 + b"\x02\x00\x48\x12" b"\x00\x00\x04\x00" b"\x01\x00\x00\x00" + b"\xff" * 8 + b"\x00" * 4 + b"b\x00" b"\x40" b"\xff")
    assert bam_check.reg2bin(-1, 0) == 4680 == UC.UNPLACED_BIN
    assert UR.rowless_of(read_pairs_of(_DT, [0, 2], 4, True, empty=[3]), 4) == [1, 3]


class _DT:   # the record layout of kslam_read_pair, for the hand-written case above (the library's own is checked below)
    READ_PAIR_DT = np.dtype([("r1_read", "<u4"), ("r2_read", "<u4"), ("first", "<u8"), ("count", "<u8")])


def test_the_reader_by_hand(T):
    assert T.READ_PAIR_DT == _DT.READ_PAIR_DT
    ids, bases, quals = [b"a", b"a"], [b"ACGTN", b"acg"], [b"IIIII", b"#$%"]
    rec = UR.expected_records(ids, bases, quals, [0], 1, True, True)
    assert UC.decode_records(rec) == b"a\t77\t*\t0\t0\t*\t*\t0\t0\tACGTN\tIIIII\n" b"a\t141\t*\t0\t0\t*\t*\t0\t0\tACG\t#$%\n"
    assert UC.decode_records(UR.expected_records(ids, bases, None, [0], 1, True, True)).endswith(b"\tACG\t*\n")
    one = UR.expected_records(ids, bases, quals, [0], 2, False, False)
    assert UC.decode_records(one) == b"a\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"

    def patched(at, fmt, v, grow=b""):
        body = bytearray(one[4:] + grow)
        struct.pack_into(fmt, body, at, v)
        return struct.pack("<i", len(body)) + bytes(body)

    # refID -1 is accepted only with FLAG 0x4, pos -1, n_cigar_op 0, mapq 0, bin 4680 and no tags
    for what, blob in (("FLAG", patched(14, "<H", 0)), ("pos", patched(4, "<i", 0)), ("n_cigar_op", patched(12, "<H", 1)),
                       ("mapq", patched(9, "<B", 1)), ("bin", patched(10, "<H", 4681)), ("tags", patched(14, "<H", 4, b"NMC\x00")),
                       ("refID", patched(0, "<i", -2)), ("next_refID", patched(20, "<i", 0)), ("tlen", patched(28, "<i", 1))):
        with pytest.raises(UC.BamError):
            UC.decode_records(blob)
    # ... and the readers of switch-off output refuse it altogether
    for reader in (bam_check, S):
        with pytest.raises(bam_check.BamError):
            reader.records(one, 0, [(b"x", 10)])


def test_library_exports_every_samunmapped_symbol(kslam, U):
    h = open(os.path.join(ROOT, "include", "kslam_samunmapped.h")).read()
    assert "#define KSLAM_TEXT_SAM_UNMAPPED 64u" in h and U.TEXT_SAM_UNMAPPED == 64
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kslam_[a-z_0-9]+)\s*\(", h)))
    L = ctypes.CDLL(kslam.LIB_PATH)
    assert len(declared) == 4 and declared == sorted(U.EXPORTS) and all(hasattr(L, n) for n in declared)
    assert ctypes.sizeof(kslam.BatchResult) == 232   # kslam_batch_result keeps its size: callers allocate it


PATTERNS = {"none": lambda n: [], "all": lambda n: list(range(n)), "first": lambda n: list(range(1, n)), "last": lambda n: list(range(n - 1)),
            "alternating": lambda n: list(range(0, n, 2)), "one": lambda n: [n // 2]}


def _check(T, Q, U, ids, bases, quals, n_records, paired, with_rows, empty=()):
    """every (bam, seq, qualities) form of one batch against the rules -> the text with seq on"""
    reads = T.Reads(bases, quals, ids)
    P = T.TailParams.default(paired=paired, report_cigar=False, pseudo_assembly=False)
    rp = read_pairs_of(T, with_rows, n_records, paired, empty)
    rowless = UR.rowless_of(rp, n_records)
    assert rowless == [p for p in range(n_records) if p not in set(with_rows)]
    text_on = None
    for with_qual in (True, False):
        view = reads if with_qual else Q.without_qualities(reads)
        q = quals if with_qual else None
        for seq in (False, True):
            text = U.tail_sam_unmapped(P, view, rp, n_records, bam=False, seq=seq)
            assert text == UR.expected_text(ids, bases, q, rowless, n_records, paired, seq), (with_qual, seq)
            S.sam_rows(text)
            rec = U.tail_sam_unmapped(P, view, rp, n_records, bam=True, seq=seq)
            assert rec == UR.expected_records(ids, bases, q, rowless, n_records, paired, seq), (with_qual, seq)
            # the records decode to the text, as far as BAM can say it (upper case, N for what is no IUPAC letter)
            got = S.sam_rows(UC.decode_records(rec))
            want = S.sam_rows(text)
            assert len(got) == len(want) == len(rowless) * (2 if paired else 1)
            for f, g in zip(want, got):
                assert g[:9] == f[:9] and (g[9], g[10]) == R.bam_view(f[9], f[10])
            if with_qual and seq:
                text_on = text
    return text_on


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_made_up_batch(kslam, T, Q, U, paired, pattern):
    """read lengths 0 .. 33 with N, lower case, IUPAC codes and bytes that are no letters"""
    bases, quals, ids, _ = made_up_batch(kslam, paired)
    n = 34
    text = _check(T, Q, U, ids, bases, quals, n, paired, PATTERNS[pattern](n))
    if pattern == "none":   # all unaligned: every read's (id, bases, qualities) once, in input order
        rows = S.sam_rows(text)
        order = [(p, m) for p in range(n) for m in range(2 if paired else 1)]
        assert [(f[0], f[9], f[10]) for f in rows] == [(ids[p + m * n], bases[p + m * n] or b"*", quals[p + m * n] if bases[p + m * n] else b"*")
                                                       for p, m in order]


def test_a_group_without_alignment_pairs_counts_as_absent(kslam, T, Q, U):
    bases, quals, ids, _ = made_up_batch(kslam, True)
    _check(T, Q, U, ids, bases, quals, 34, True, [0, 5, 6, 33], empty=[1, 7, 32])


def test_fewer_records_consumed_than_loaded(kslam, T, U):
    bases, quals, ids, _ = made_up_batch(kslam, True)
    reads = T.Reads(bases, quals, ids)
    P = T.TailParams.default(paired=True)
    rp = read_pairs_of(T, [2, 30], 34, True)
    assert U.tail_sam_unmapped(P, reads, rp, 10, seq=True) == UR.expected_text(ids, bases, quals, [p for p in range(10) if p != 2], 34, True, True)
    assert U.tail_sam_unmapped(P, reads, rp, 0) == b""
    with pytest.raises(Exception, match="more consumed records"):
        U.tail_sam_unmapped(P, reads, rp, 35)
    bad = read_pairs_of(T, [2], 34, True)
    bad["r2_read"] = 40
    with pytest.raises(Exception, match="outside the batch"):
        U.tail_sam_unmapped(P, reads, bad, 34)


@pytest.mark.parametrize("paired", [True, False])
def test_id_lengths(kslam, T, Q, U, paired):
    """ids of length 0, 1 and 254 are written; one of 255 is written as text, and refused as BAM with the read named"""
    names = [b"", b"x", b"n" * 254, b"ok"]
    n = len(names)
    ids = names * (2 if paired else 1)
    rng = np.random.default_rng(5)
    bases = [bytes(rng.choice(list(b"ACGT"), 9 + i).astype(np.uint8)) for i in range(len(ids))]
    quals = [b"F" * len(b) for b in bases]
    _check(T, Q, U, ids, bases, quals, n, paired, [3])
    long_, longer = b"L" * 255, b"M" * 300
    ids = [b"a", long_, b"b", b"c"] + ([b"a", long_, longer, b"c"] if paired else [])
    reads = T.Reads(bases, quals, ids)
    P = T.TailParams.default(paired=paired)
    for with_rows in ([], [0], [1]):
        rp = read_pairs_of(T, with_rows, n, paired)
        rowless = UR.rowless_of(rp, n)
        for seq in (False, True):
            assert U.tail_sam_unmapped(P, reads, rp, n, seq=seq) == UR.expected_text(ids, bases, quals, rowless, n, paired, seq)
            if 1 in with_rows and not paired:   # the long id belongs to a record with rows: nothing to refuse here
                assert U.tail_sam_unmapped(P, reads, rp, n, bam=True, seq=seq) == UR.expected_records(ids, bases, quals, rowless, n, paired, seq)
                continue
            # the lowest such read: R1 of record 1 where it is rowless, else (paired) R2 of record 2, which carries the longer id
            name = long_ if 1 not in with_rows else longer
            with pytest.raises(Exception, match=name.decode() + '" is longer than 254 bytes'):
                U.tail_sam_unmapped(P, reads, rp, n, bam=True, seq=seq)
