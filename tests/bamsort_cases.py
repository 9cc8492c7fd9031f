"""Hand-built record batches for the coordinate-sorted BAM (include/kslam_bamsort.h) at its seams, shared by the host and the GPU
tests: each case is a list of batches (bytes, in seq order) over the references REFS.  Also the file around a record stream, with
zlib as the compressor, for checks that need no library."""
import struct
import zlib

import bamsort_ref as R

REFS = [(b"chrA", 200000), (b"chrB", 3000), (b"chrC", 40000)]
SAM_HEADER = b"@HD\tVN:1.0\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + b"@PG\tID:test\n"
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
M = R.MEMBER_IN


def rec(ref, pos, name=b"r", length=50, flag=0, seq_len=0, cigar=None):
    if cigar is None:
        cigar = [] if flag & 4 or ref < 0 else [(length, 0)]
    return R.record(ref, pos, name=name, flag=flag, cigar=cigar, seq_len=seq_len)


def padded(ref, pos, size, name=b"p"):
    """a mapped record of exactly `size` bytes (size >= 60): the padding is SEQ, 3 bytes per 2 bases, and the name"""
    base = len(rec(ref, pos, name=name))
    extra = size - base
    seq_len = (extra // 3) * 2
    r = rec(ref, pos, name=name + b"x" * (extra - 3 * (seq_len // 2)), seq_len=seq_len)
    assert len(r) == size, (len(r), size)
    return r


def stream_of_size(total, ref=0, first_pos=10):
    """records of ascending position whose bytes come to exactly `total`"""
    out, pos, left = [], first_pos, total
    while left:
        size = 300 if left >= 600 else left if left < 360 else left - 100
        out.append(padded(ref, pos, size))
        pos += 7
        left -= size
    return out


def cases():
    c = {}
    c["empty"] = []
    c["one_empty_batch"] = [b""]
    c["one_record"] = [rec(0, 100)]
    c["empty_batch_between"] = [rec(2, 500, b"a") + rec(0, 7, b"b"), b"", rec(0, 6, b"c") + rec(-1, -1, b"d", flag=4)]
    c["all_keys_equal"] = [b"".join(rec(0, 1000, b"b%d_%d" % (b, i)) for i in range(5)) for b in range(3)]
    c["only_unplaced"] = [rec(-1, -1, b"u1", flag=4, seq_len=30) + rec(-1, -1, b"u2", flag=4), rec(-1, -1, b"u3", flag=4)]
    c["pos_minus_one_on_a_reference"] = [rec(0, 50, b"a") + rec(0, -1, b"m", flag=4) + rec(2, -1, b"n", flag=4) + rec(2, 0, b"z"), rec(0, 0, b"first")]
    c["ends_at_member_edge"] = [b"".join(stream_of_size(M)[::-1])]
    c["ends_at_member_edge_plus_one"] = [b"".join(stream_of_size(M + 1)[::-1])]
    straddle = stream_of_size(M - 100) + [padded(0, 70000, 300, b"straddler")] + stream_of_size(1000, ref=2)
    c["straddles_member_edge"] = [b"".join(straddle[1::2]), b"".join(straddle[0::2])]
    c["record_longer_than_a_member"] = [rec(2, 5, b"after") + padded(0, 20, M + 5000, b"long") + rec(0, 19, b"before"), rec(0, 21, b"behind")]
    c["empty_reference_between"] = [rec(2, 100, b"c1") + rec(0, 100, b"a1"), rec(2, 50, b"c2") + rec(0, 150, b"a2")]
    # a 16 kb window edge (16384) and a level boundary of the binning scheme (131072 = 2^17): bins 4688 and 4689 get two chunks each
    c["window_and_level_edges"] = [rec(0, 16380, b"w", length=10) + rec(0, 16000, b"v") + rec(0, 131000, b"b1") + rec(0, 131060, b"lvl", length=50)
                                   + rec(0, 131065, b"b2", length=5) + rec(0, 131072, b"n1") + rec(0, 131080, b"n0", length=300000 - 131080 - 150000)
                                   + rec(0, 140000, b"n2")]
    import random
    rng = random.Random(11)
    mixed = []
    for b in range(4):
        rs = []
        for i in range(400):
            ref = rng.choice([0, 0, 0, 2, 2, -1])
            if ref < 0:
                rs.append(rec(-1, -1, b"q%d_%d" % (b, i), flag=4, seq_len=rng.randrange(0, 200)))
            else:
                length = rng.randrange(1, 300)
                pos = rng.randrange(0, REFS[ref][1] - length)
                flag = 4 if rng.random() < 0.1 else 0
                rs.append(rec(ref, pos, b"q%d_%d" % (b, i), length=length, flag=flag, seq_len=rng.randrange(0, 400),
                              cigar=None if flag else [(3, 4), (length - length // 2, 0), (2, 1), (length // 2, 2 if length > 1 else 1)]))
        mixed.append(b"".join(rs))
    c["mixed"] = mixed
    return c


def zlib_members(data):
    """[(member bytes)] of 65 280 input bytes each, deflated by zlib: valid BGZF, not the library's bytes"""
    out = []
    for a in range(0, len(data), M):
        d = data[a:a + M]
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = z.compress(d) + z.flush()
        size = 18 + len(body) + 8
        out.append(bytes.fromhex("1f8b08040000000000ff0600424302") + b"\x00" + struct.pack("<H", size - 1) + body
                   + struct.pack("<II", zlib.crc32(d), len(d)))
    return out


def member_sizes(blob, skip_bytes):
    """the compressed sizes of the members of a BGZF file behind its first skip_bytes, without the EOF marker"""
    sizes, at = [], skip_bytes
    while at < len(blob) - len(EOF):
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        sizes.append(size)
        at += size
    assert at == len(blob) - len(EOF)
    return sizes
