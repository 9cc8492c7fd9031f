"""Plain gzip test files for include/kslam_gunzip.h: what zlib and gzip write at several levels, files cut into many
members, hand-written dynamic blocks for what zlib never emits, and corrupt twins.  Everything is generated from seeds.
A valid case is (blob, text, chunk size to test it with); a refusal is (blob, chunk size, member, kind)."""
import gzip
import random
import struct
import zlib

import numpy as np

import gunzip_ref as G
import inflate_cases as Cs
import inflate_ref as R

KIB = 1024


def fastq_like(n_bytes, seed):
    """FASTQ-like text by numpy: the generator of tests/test_gpu_inflate.py (_fastq_like), byte for byte"""
    rnd = np.random.default_rng(seed)
    L = 150
    rows = n_bytes // (14 + 2 * L) + 1
    rec = np.empty((rows, 10 + L + 3 + L + 1), dtype=np.uint8)
    rec[:, 0] = ord("@")
    idx = np.arange(rows)
    for d in range(8):
        rec[:, 8 - d] = ord("0") + (idx // 10 ** d) % 10
    rec[:, 9] = ord("\n")
    rec[:, 10:10 + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rnd.integers(0, 4, (rows, L))]
    rec[:, 10 + L:13 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 13 + L:13 + 2 * L] = np.frombuffer(b"FFFFFFF:,#", dtype=np.uint8)[rnd.integers(0, 10, (rows, L))]
    rec[:, 13 + 2 * L] = ord("\n")
    return rec.tobytes()[:n_bytes]


def gz(text, level=6, flags=0, extra=b"", name=b"", comment=b""):
    """one member around zlib's raw deflate data, with the optional header fields the flags ask for"""
    head = bytes([0x1F, 0x8B, 8, flags, 0, 0, 0, 0, 0, 0xFF])
    if flags & 4:
        head += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        head += name + b"\0"
    if flags & 16:
        head += comment + b"\0"
    if flags & 2:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + Cs.deflate_raw(text, level=level) + trailer(text)


def trailer(text):
    return struct.pack("<II", zlib.crc32(text), len(text) & 0xFFFFFFFF)


PLAIN_HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])


# ---- hand-written bit streams ----
class Bits:
    """inflate_cases.BitWriter's interface, without a big integer that grows with the stream"""
    def __init__(self):
        self.out, self.v, self.n = bytearray(), 0, 0

    def put(self, value, n):
        self.v |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.v & 0xFF)
            self.v >>= 8
            self.n -= 8

    def code(self, code, n):
        self.put(int(format(code, "0%db" % n)[::-1], 2), n)     # a Huffman code goes most significant bit first

    def bytes(self):
        return bytes(self.out) + (bytes([self.v]) if self.n else b"")


# one flat pair of codes for every hand-written dynamic block: 226 literal/length symbols of 8 bits and 60 of 9, two distance
# symbols of 4 bits and 28 of 5 (both complete); their lengths are sent one by one with a code-length code of four 2-bit codes
_LL_LENS, _D_LENS = [8] * 226 + [9] * 60, [4] * 2 + [5] * 28
_LL, _DC = Cs.canonical(_LL_LENS), Cs.canonical(_D_LENS)


def dynamic_block(w, tokens, final=False):
    cl = [0] * 19
    cl[4] = cl[5] = cl[8] = cl[9] = 2
    cc = Cs.canonical(cl)
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(len(_LL_LENS) - 257, 5)
    w.put(len(_D_LENS) - 1, 5)
    w.put(12 - 4, 4)
    for s in R.CL_ORDER[:12]:
        w.put(cl[s], 3)
    for l in _LL_LENS + _D_LENS:
        w.code(*cc[l])
    Cs.put_tokens(w, tokens, _LL, _DC)


def hand_member(blocks):
    """blocks: token lists, the last one final -> (member, text)"""
    w = Bits()
    for k, tokens in enumerate(blocks):
        dynamic_block(w, tokens, final=k == len(blocks) - 1)
    text = Cs.expand([t for b in blocks for t in b])
    return PLAIN_HEADER + w.bytes() + trailer(text), text


def edge_member(before, seed):
    """`before` random literals in one block, then a block whose FIRST token is a match of length 258 at distance 32 768"""
    rnd = random.Random(seed)
    lits = [rnd.randrange(256) for _ in range(before)]
    w = Bits()
    dynamic_block(w, lits)
    dynamic_block(w, [(258, 32768), 1, 2, 3])
    dynamic_block(w, [4, 5, 6], final=True)
    return PLAIN_HEADER + w.bytes(), lits


def stored_member(payload):
    out = bytearray(PLAIN_HEADER)
    pieces = [payload[i:i + 65535] for i in range(0, len(payload), 65535)] or [b""]
    for k, p in enumerate(pieces):
        out += bytes([1 if k == len(pieces) - 1 else 0]) + struct.pack("<HH", len(p), len(p) ^ 0xFFFF) + p
    return bytes(out) + trailer(payload)


def false_start_case():
    """An inner deflate stream of several dynamic blocks, stored verbatim inside level-0 blocks, its first byte 7 bytes
    behind the seam at 16 KiB: the finder takes it for a start, and the chain proves it false"""
    inner = Cs.deflate_raw(fastq_like(300000, seed=21))
    payload = bytes(16 * KIB + 7 - len(PLAIN_HEADER) - 5) + inner
    return stored_member(payload), payload


def far_case():
    """Fresh FASTQ-like text in pieces of uneven length, each ended with a sync flush (so that blocks -- and with 4 KiB
    chunks, live stretches -- begin often), and planted in it: 120 rare bytes X, the same X 32 100 bytes later (a far
    match into the stretches before), X once more 600 bytes on (a match that copies markers), and after the far copy a
    run of its last byte (a run-length match over a marker)"""
    rnd = random.Random(31)
    text = bytearray(fastq_like(260000, seed=32))
    for at in range(40000, len(text) - 2000, 9000):
        x = bytes(rnd.randrange(128, 256) for _ in range(120))
        text[at - 32100:at - 32100 + 120] = x
        text[at:at + 120] = x
        text[at + 120:at + 170] = x[-1:] * 50
        text[at + 600:at + 720] = x
    text = bytes(text)
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    parts, at = [], 0
    sizes = [47000, 9000, 8000, 9500, 47000, 15000, 14000, 9000, 8500, 9000, 38000, 9000]
    k = 0
    while at < len(text):
        n = sizes[k % len(sizes)]
        parts.append(c.compress(text[at:at + n]))
        at += n
        k += 1
        if at < len(text):
            parts.append(c.flush(zlib.Z_SYNC_FLUSH))
    parts.append(c.flush())
    return PLAIN_HEADER + b"".join(parts) + trailer(text), text


def bgzf_case():
    text = Cs.fastq_text(150000, seed=41)
    return Cs.bgzf(text) + Cs.EOF_MARKER, text


def straddle_cases():
    """two members, the first one's FNAME sized so that the seam at 4 KiB falls on each of the 8 trailer bytes and the 10 bytes
    of the second header in turn"""
    t1, t2 = Cs.fastq_text(9000, seed=51), Cs.fastq_text(5000, seed=52)
    base = len(gz(t1, flags=8, name=b""))
    k = (base + 4 * KIB - 1) // (4 * KIB) + 1          # the seam the first member's end is moved to
    out = {}
    for j in range(18):
        pad = k * 4 * KIB - (base - 8) - j               # the trailer begins j bytes before the seam
        m1 = gz(t1, flags=8, name=b"n" * pad)
        assert len(m1) - 8 + j == k * 4 * KIB
        out["straddle_%02d" % j] = (m1 + gz(t2), t1 + t2, 4 * KIB)
    return out


LEVELS_TEXT_BYTES = 1500000


def levels_text():
    return fastq_like(LEVELS_TEXT_BYTES, seed=8)


def valid_cases():
    """name -> (blob, text, chunk)"""
    out = {}
    text = levels_text()
    for level in (1, 6, 9):
        out["level%d" % level] = (gz(text, level=level), text, 32 * KIB)
    out["level6_chunk4k"] = (out["level6"][0], text, 4 * KIB)
    out["level6_chunk1k"] = (out["level6"][0], text, 1 * KIB)
    short = Cs.fastq_text(20000, seed=11)
    out["shorter_than_a_chunk"] = (gz(short), short, 32 * KIB)
    out["false_start"] = false_start_case() + (16 * KIB,)
    out["far_sources"] = far_case() + (4 * KIB,)
    head, lits = edge_member(32768, seed=61)
    text = Cs.expand(lits + [(258, 32768), 1, 2, 3, 4, 5, 6])
    out["edge_32768"] = (head + trailer(text), text, 16 * KIB)
    first = Cs.fastq_text(7000, seed=62)
    out["edge_32768_second_member"] = (gz(first) + head + trailer(text), first + text, 16 * KIB)
    parts = [Cs.fastq_text(6000 + 1500 * k, seed=70 + k) for k in range(5)]
    out["two_members"] = (gz(parts[0]) + gz(parts[1], level=9), parts[0] + parts[1], 1 * KIB)
    out["five_members"] = (b"".join(gz(p, level=1 + 2 * k) for k, p in enumerate(parts)), b"".join(parts), 2 * KIB)
    out["empty_member_between"] = (gz(parts[0]) + gz(b"") + gz(parts[1]) + gz(b""), parts[0] + parts[1], 1 * KIB)
    fields = gz(parts[2], flags=4 | 8 | 16 | 2, extra=b"\x01\x02" + bytes(range(40)), name=b"reads_R1.fastq", comment=b"lane 3")
    out["header_fields"] = (fields + gz(parts[3], flags=8 | 2, name=b"x"), parts[2] + parts[3], 1 * KIB)
    out["zero_padding"] = (gz(parts[0]) + gz(parts[4]) + bytes(700), parts[0] + parts[4], 1 * KIB)
    out["bgzf"] = bgzf_case() + (32 * KIB,)
    out.update(straddle_cases())
    return out


def refusals():
    """name -> (blob, chunk, member, kind): two good members, the second one damaged (or the file cut)"""
    t0, t1 = Cs.fastq_text(5000, seed=81), Cs.fastq_text(40000, seed=82)
    m0, m1 = gz(t0), gz(t1, flags=8, name=b"second")
    d_at = len(m0) + G.header(m1)              # where the second member's deflate data begins
    out = {}
    out["cut_in_header"] = (m0 + m1[:14], 1 * KIB, 1, G.HEADER)
    out["cut_in_data"] = (m0 + m1[:len(m1) // 2], 1 * KIB, 1, R.DATA_LENGTH)
    out["cut_in_trailer"] = (m0 + m1[:-3], 1 * KIB, 1, R.DATA_LENGTH)

    def flipped(at, bit=1):
        b = bytearray(m0 + m1)
        b[at] ^= bit
        return bytes(b)

    out["crc_byte"] = (flipped(len(m0) + len(m1) - 7), 1 * KIB, 1, R.CRC)
    out["isize_byte"] = (flipped(len(m0) + len(m1) - 4), 1 * KIB, 1, R.OUTPUT_UNDERRUN)     # ISIZE 40 000 -> 40 001: the text is one byte short of it
    out["garbage_behind_a_member"] = (m0 + m1 + b"garbage", 1 * KIB, 2, G.NOT_MEMBER)
    out["reserved_flag"] = (m0 + m1[:3] + bytes([m1[3] | 0x20]) + m1[4:], 1 * KIB, 1, G.HEADER)
    out["method_7"] = (m0 + m1[:2] + b"\x07" + m1[3:], 1 * KIB, 1, G.HEADER)
    out["no_magic_at_all"] = (b"@read0\nACGT\n+\nFFFF\n", 1 * KIB, 0, G.NOT_MEMBER)
    # a flipped data bit: which kind it gives depends on the bit; the restatement names it (tests/test_gunzip_ref.py)
    out["data_bit"] = (flipped(d_at + 1500, 0x10), 1 * KIB, 1, None)
    # the edge: 32 767 bytes before the match of distance 32 768, behind a first member whose bytes lie in the window
    head, lits = edge_member(32767, seed=61)
    text = bytes(lits) + bytes(265)          # (the text the trailer would describe; the member never gets that far)
    out["edge_32767_second_member"] = (gz(Cs.fastq_text(7000, seed=62)) + head + trailer(text), 16 * KIB, 1, R.DISTANCE)
    return out
