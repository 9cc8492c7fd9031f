"""The yardsticks of the coordinate-sorted BAM (include/kslam_bamsort.h) against each other, without the library: the restatement
(tests/bamsort_ref.py) and the checker of what an index means (tests/bai_check.py) on the seam cases (tests/bamsort_cases.py), a
BAI index worked by hand for three records, the header's sort order, and the checker refusing indexes that are wrong.  No GPU."""
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bai_check  # noqa: E402
import bamsort_cases as BC  # noqa: E402
import bamsort_ref as R  # noqa: E402

CASES = BC.cases()


def _file(batches):
    stream = R.sort_batches(batches)
    head = BC.zlib_members(R.bam_header(R.coordinate_header(BC.SAM_HEADER), BC.REFS))
    body = BC.zlib_members(stream)
    hlen = sum(len(m) for m in head)
    return stream, b"".join(head) + b"".join(body) + BC.EOF, [len(m) for m in body], hlen


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_and_checker_agree(name):
    stream, bam, sizes, hlen = _file(CASES[name])
    bai = R.bai(stream, len(BC.REFS), sizes, hlen)
    got = bai_check.check(bam, bai)
    recs = R.split(stream)
    assert got["n_records"] == len(recs) == sum(len(R.split(b)) for b in CASES[name])
    assert got["n_no_coor"] == sum(R.fields(r)["ref"] < 0 for r in recs)
    assert sorted(recs) == sorted(r for b in CASES[name] for r in R.split(b))      # a permutation of the input


def test_ties_keep_submission_order():
    names = [r[36:r.index(b"\0", 36)] for r in R.split(R.sort_batches(CASES["all_keys_equal"]))]
    assert names == [b"b%d_%d" % (b, i) for b in range(3) for i in range(5)]
    order = [r[36:r.index(b"\0", 36)] for r in R.split(R.sort_batches(CASES["pos_minus_one_on_a_reference"]))]
    assert order == [b"m", b"first", b"a", b"n", b"z"]     # pos -1 in front of its reference's others
    order = [r[36:r.index(b"\0", 36)] for r in R.split(R.sort_batches(CASES["empty_batch_between"]))]
    assert order == [b"c", b"b", b"a", b"d"]               # refID -1 last


def test_a_bai_worked_by_hand():
    """Three records: chrA:100 50M, chrA:16380 10M (over the 16 kb window edge: bin 585), one without coordinate.  Their lengths
    are 42, 42 and 38 bytes; the header's members take H bytes, the one record member Z."""
    recs = [BC.rec(0, 100, b"a"), BC.rec(0, 16380, b"b", length=10), BC.rec(-1, -1, b"c", flag=4)]
    assert [len(r) for r in recs] == [42, 42, 38]
    H, Z = 777, 99
    s0, s1, s2, eof = H << 16, H << 16 | 42, H << 16 | 84, (H + Z) << 16
    want = b"BAI\x01" + struct.pack("<i", 3)
    want += struct.pack("<i", 3)                                        # chrA: two bins and the pseudo-bin
    want += struct.pack("<IiQQ", 585, 1, s1, s2)
    want += struct.pack("<IiQQ", 4681, 1, s0, s1)
    want += struct.pack("<IiQQQQ", 37450, 2, s0, s2, 2, 0)
    want += struct.pack("<iQQ", 2, s0, s1)                              # windows 0 and 1
    want += struct.pack("<ii", 0, 0) * 2                                # chrB, chrC: nothing
    want += struct.pack("<Q", 1)
    assert R.bai(b"".join(recs), 3, [Z], H) == want
    assert eof == R.voff_of([Z], H, 122)(122)


def test_a_position_at_a_members_end_is_the_next_members_start():
    stream, bam, sizes, hlen = _file(CASES["ends_at_member_edge"])
    assert len(stream) == BC.M and len(sizes) == 1
    v = R.voff_of(sizes, hlen, len(stream))
    assert v(BC.M) == (hlen + sizes[0]) << 16 and v(BC.M - 1) == hlen << 16 | (BC.M - 1)
    stream, bam, sizes, hlen = _file(CASES["ends_at_member_edge_plus_one"])
    v = R.voff_of(sizes, hlen, len(stream))
    assert len(sizes) == 2 and v(BC.M) == (hlen + sizes[0]) << 16 and v(BC.M + 1) == (hlen + sizes[0] + sizes[1]) << 16


def test_two_chunks_in_one_bin():
    stream, bam, sizes, hlen = _file(CASES["window_and_level_edges"])
    bai = R.bai(stream, 3, sizes, hlen)
    n_bin = struct.unpack_from("<i", bai, 8)[0]
    bins, pos = {}, 12
    for _ in range(n_bin):
        b, n_chunk = struct.unpack_from("<Ii", bai, pos)
        bins[b] = n_chunk
        pos += 8 + 16 * n_chunk
    assert bins == {4681: 1, 585: 1, 4681 + 7: 2, 73: 1, 4681 + 8: 2, 586: 1, 37450: 2}   # 585: over the window edge, 73: over the level boundary


def test_header_sort_order():
    assert R.coordinate_header(b"@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:x\tLN:5\n") == b"@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:x\tLN:5\n"
    assert R.coordinate_header(b"@HD\tVN:1.6\n@PG\tID:a\n") == b"@HD\tVN:1.6\tSO:coordinate\n@PG\tID:a\n"
    assert R.coordinate_header(b"@HD\tSO:queryname\tGO:none\n") == b"@HD\tSO:coordinate\tGO:none\n"
    assert R.coordinate_header(b"@SQ\tSN:x\tLN:5\n") == b"@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:x\tLN:5\n"
    assert R.coordinate_header(b"") == b"@HD\tVN:1.0\tSO:coordinate\n"


def test_the_checker_refuses_what_is_wrong():
    stream, bam, sizes, hlen = _file(CASES["window_and_level_edges"])
    bai = bytearray(R.bai(stream, 3, sizes, hlen))
    bai_check.check(bam, bytes(bai))
    for at, what in ((16, "first chunk's start"), (len(bai) - 8, "n_no_coor")):
        bad = bytearray(bai)
        bad[at] ^= 1
        with pytest.raises(ValueError):
            bai_check.check(bam, bytes(bad))
    unsorted_stream = b"".join(R.split(stream)[::-1])
    body = BC.zlib_members(unsorted_stream)
    head = bam[:hlen]
    with pytest.raises(bai_check.BaiError, match="not sorted"):
        bai_check.check(head + b"".join(body) + BC.EOF, bytes(bai))
    with pytest.raises(bai_check.BaiError, match="EOF"):
        bai_check.check(bam[:-28], bytes(bai))
