"""BGZF test files for include/kslam_inflate.h: what Python's zlib writes under every setting that changes the shape of the
stream, hand-written bit streams for what zlib never emits, and corrupt twins that differ from a valid member in one field.
Everything is generated from seeds; a case is (name, blob, text) or, corrupt, (name, blob, member index, error kind)."""
import random
import struct
import zlib

import inflate_ref as R

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CHUNK = 65280


def member(deflate, text=None, crc=None, isize=None):
    """the BGZF framing around deflate data; crc / isize default to the text's"""
    size = 18 + len(deflate) + 8
    assert size <= 65536, size
    head = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, ord("B"), ord("C"), 2, 0]) + struct.pack("<H", size - 1)
    return head + deflate + struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize)


def deflate_raw(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(data) + c.flush()


def bgzf(data, **kw):
    """members of at most CHUNK input bytes; a chunk is halved whenever its member would exceed 65 536 bytes"""
    out, at = [], 0
    while at < len(data):
        n = min(CHUNK, len(data) - at)
        while 18 + len(deflate_raw(data[at:at + n], **kw)) + 8 > 65536:
            n //= 2
        out.append(member(deflate_raw(data[at:at + n], **kw), data[at:at + n]))
        at += n
    return b"".join(out)


def fastq_text(n, seed=1):
    rnd = random.Random(seed)
    out, i = [], 0
    while sum(map(len, out)) < n:
        L = rnd.randrange(90, 151)
        out.append(b"@read%d/1\n%s\n+\n%s\n" % (i, bytes(rnd.choice(b"ACGT") for _ in range(L)),
                                             bytes(rnd.choice(b"FFFFFFF:,#") for _ in range(L))))
        i += 1
    return b"".join(out)[:n]


def inputs(n=2 * CHUNK + 777):
    return {"fastq": fastq_text(n), "random": random.Random(2).randbytes(n), "zeros": bytes(n)}


SETTINGS = {"level0": dict(level=0), "level1": dict(level=1), "level6": dict(level=6), "level9": dict(level=9),
            "mem1": dict(level=6, mem=1), "fixed": dict(level=6, strategy=zlib.Z_FIXED),
            "huffman_only": dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY), "rle": dict(level=6, strategy=zlib.Z_RLE)}


def flush_member(text):
    """one member whose deflate data holds sync and full flushes: empty stored blocks between the others"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    parts, step = [], len(text) // 11 + 1
    for k, at in enumerate(range(0, len(text), step)):
        parts.append(c.compress(text[at:at + step]))
        if at + step < len(text):
            parts.append(c.flush(zlib.Z_FULL_FLUSH if k % 2 else zlib.Z_SYNC_FLUSH))
    parts.append(c.flush())
    return member(b"".join(parts), text)


# ---- hand-written bit streams ----
class BitWriter:
    def __init__(self):
        self.v = self.n = 0

    def put(self, value, n):          # n bits, LSB first (headers, extra bits)
        self.v |= value << self.n
        self.n += n

    def code(self, code, n):          # a Huffman code: most significant bit first
        for k in range(n - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canonical(lens):
    """symbol -> (code, length) of the canonical Huffman code (RFC 1951 3.2.2)"""
    code, out = 0, {}
    for l in range(1, 16):
        for s, x in enumerate(lens):
            if x == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def length_symbol(length):
    for sym in range(285, 256, -1):
        k = sym - 257
        base, eb = (258, 0) if k == 28 else (3 + k, 0) if k < 8 else (3 + ((4 + (k & 3)) << ((k >> 2) - 1)), (k >> 2) - 1)
        if base <= length < base + (1 << eb) and not (sym == 284 and length == 258):
            return sym, eb, length - base
    raise ValueError(length)


def distance_symbol(dist):
    for d in range(29, -1, -1):
        base, eb = (1 + d, 0) if d < 4 else (1 + ((2 + (d & 1)) << ((d >> 1) - 1)), (d >> 1) - 1)
        if base <= dist:
            return d, eb, dist - base
    raise ValueError(dist)


def put_tokens(w, tokens, ll, dc):
    """tokens: int = literal, (length, distance) = match, ("ll", symbol) / ("match_dsym", length, dsym) = raw symbols"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*ll[t])
        elif t[0] == "ll":
            w.code(*ll[t[1]])
        else:
            raw = t[0] == "match_dsym"
            sym, eb, ev = length_symbol(t[1] if raw else t[0])
            w.code(*ll[sym])
            w.put(ev, eb)
            if raw:
                w.code(*dc[t[2]])
            else:
                d, eb, ev = distance_symbol(t[1])
                w.code(*dc[d])
                w.put(ev, eb)
    w.code(*ll[256])


def fixed_block(tokens):
    w = BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    put_tokens(w, tokens, canonical(R._FIXED[0]), canonical(R._FIXED[1]))
    return w.bytes()


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def crossing_dynamic_block(cl_len_of_18=2):
    """A dynamic block whose code-length repeat 16 runs from the literal/length lengths (256, 257) into the four distance
    lengths -- zlib writes the two sets apart and never does this.  Literal 'a' has 1 bit, 256 and 257 two; text 'aaaaaa'."""
    cl = [0] * 19
    cl[1] = cl[2] = cl[16] = 2
    cl[18] = cl_len_of_18          # 2: complete; 1: over-subscribed
    cc = canonical([2 if x else 0 for x in cl])   # the codes of the valid twin
    w = BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(258 - 257, 5)
    w.put(4 - 1, 5)
    w.put(18 - 4, 4)
    for s in R.CL_ORDER[:18]:
        w.put(cl[s], 3)
    for sym, eb, ev in ((18, 7, 97 - 11), (1, 0, 0), (18, 7, 138 - 11), (18, 7, 20 - 11), (2, 0, 0), (16, 2, 5 - 3)):
        w.code(*cc[sym])
        w.put(ev, eb)
    ll_lens = [0] * 258
    ll_lens[97], ll_lens[256], ll_lens[257] = 1, 2, 2
    put_tokens(w, [97, 97, 97, (3, 1)], canonical(ll_lens), canonical([2, 2, 2, 2]))
    return w.bytes(), b"aaaaaa"


def hand_cases():
    rnd = random.Random(3)
    far = [65] + [rnd.randrange(256) for _ in range(32767)] + [(3, 32768)]
    rle = [7, (258, 1)]
    edge = [97, 98, 99, 100, 101, (5, 5)]
    cases = {"far_32768": far, "rle_258": rle, "match_to_the_end": edge, "one_literal": [120]}
    out = {k: (member(fixed_block(t), expand(t)), expand(t)) for k, t in cases.items()}
    d, text = crossing_dynamic_block()
    out["repeat_crossing"] = (member(d, text), text)
    return out


def valid_cases():
    """name -> (blob, text)"""
    out = {}
    for iname, data in inputs().items():
        for sname, kw in SETTINGS.items():
            out["%s_%s" % (iname, sname)] = (bgzf(data, **kw), data)
    text = fastq_text(60000, seed=4)
    out["flushes"] = (flush_member(text), text)
    out.update(hand_cases())
    return out


def corrupt_cases():
    """name -> (blob, member index, error kind): two good members around the bad one"""
    good_text = fastq_text(3000, seed=5)
    good = member(deflate_raw(good_text), good_text)
    d = deflate_raw(good_text)
    stored = deflate_raw(good_text, level=0)
    edge = [97, 98, 99, 100, 101, (5, 5)]
    edge_text = expand(edge)
    bad = {}
    bad["crc"] = (member(d, good_text, crc=zlib.crc32(good_text) ^ 1), R.CRC)
    bad["isize_plus_1"] = (member(d, good_text, isize=len(good_text) + 1), R.OUTPUT_UNDERRUN)
    bad["isize_minus_1"] = (member(d, good_text, isize=len(good_text) - 1), R.OUTPUT_OVERRUN)
    bad["btype3"] = (member(bytes([d[0] | 6]) + d[1:], good_text), R.BAD_BLOCK_TYPE)
    assert stored[0] == 1 and stored[1:3] == struct.pack("<H", len(good_text))
    bad["stored_nlen"] = (member(stored[:3] + bytes([stored[3] ^ 1]) + stored[4:], good_text), R.STORED_LENGTH)
    bad["distance_before_start"] = (member(fixed_block(edge[:5] + [(5, 6)]), edge_text), R.DISTANCE)
    bad["match_overruns_isize"] = (member(fixed_block(edge[:5] + [(6, 5)]), edge_text), R.OUTPUT_OVERRUN)
    bad["data_cut_short"] = (member(d[:-4], good_text), R.DATA_LENGTH)
    bad["ll_symbol_286"] = (member(fixed_block(edge[:5] + [("ll", 286)]), edge_text), R.INVALID_SYMBOL)
    bad["distance_symbol_30"] = (member(fixed_block(edge[:5] + [("match_dsym", 5, 30)]), edge_text), R.INVALID_SYMBOL)
    bad["oversubscribed"] = (member(crossing_dynamic_block(cl_len_of_18=1)[0], b"aaaaaa"), R.OVERSUBSCRIBED)
    return {k: (good + m + good, 1, kind) for k, (m, kind) in bad.items()}
