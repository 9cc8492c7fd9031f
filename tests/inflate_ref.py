"""A pure-Python inflater (RFC 1951) for BGZF members: the yardstick of include/kslam_inflate.h's tests.  Besides the bytes
it reports, per member, what the stream contains (block types, longest code, largest distance, whether a code-length repeat
ran from the literal/length lengths into the distance lengths), so that a test case can prove it holds the seam it is named
for; on bad input it names the kind of error as the library does (k-slam_amd/inflate.py: ERROR_KINDS)."""
import struct

KINDS = ("bad block type", "stored length check", "code lengths over-subscribed", "code lengths incomplete", "invalid symbol",
         "distance too far back", "output overrun", "output underrun", "CRC mismatch", "deflate data length")
(BAD_BLOCK_TYPE, STORED_LENGTH, OVERSUBSCRIBED, INCOMPLETE, INVALID_SYMBOL, DISTANCE, OUTPUT_OVERRUN, OUTPUT_UNDERRUN, CRC,
 DATA_LENGTH) = KINDS
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_CRC_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0xEDB88320 if _c & 1 else _c >> 1
    _CRC_TABLE.append(_c)


class InflateError(Exception):
    def __init__(self, kind, member=None):
        super().__init__(kind if member is None else "member %d: %s" % (member, kind))
        self.kind, self.member = kind, member


class Report:
    def __init__(self):
        self.blocks = []            # (BTYPE, bytes the block produced)
        self.max_ll_len = 0         # longest literal/length code, longest distance code (9 and 5 in a fixed block)
        self.max_d_len = 0
        self.max_distance = 0
        self.max_length = 0
        self.first_byte_match = False   # a match whose source starts at the member's first byte
        self.repeat_crossed = False     # a code-length repeat (16, 17, 18) covered literal/length AND distance lengths

    @property
    def types(self):
        return [b[0] for b in self.blocks]


def crc32(data):
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC_TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


class _Bits:
    """LSB-first bits; behind the data come zeros, and check() refuses having used any of them"""
    def __init__(self, data):
        self.d, self.pos, self.end = data, 0, 8 * len(data)

    def peek(self):   # at least 25 bits from pos on
        p = self.pos >> 3
        return int.from_bytes(self.d[p:p + 4], "little") >> (self.pos & 7)

    def bits(self, n):
        x = self.peek() & ((1 << n) - 1)
        self.pos += n
        return x

    def check(self):
        if self.pos > self.end:
            raise InflateError(DATA_LENGTH)


def _build(lens, is_cl):
    count = [0] * 16
    for l in lens:
        count[l] += 1
    left, total, longest = 1, 0, 0
    for k in range(1, 16):
        left = (left << 1) - count[k]
        if left < 0:
            raise InflateError(OVERSUBSCRIBED)
        total += count[k]
        if count[k]:
            longest = k
    if left > 0 and total > 0 and (is_cl or longest != 1):
        raise InflateError(INCOMPLETE)
    return count, sorted((s for s, l in enumerate(lens) if l), key=lambda s: (lens[s], s))


def _decode(br, code):
    count, symbols = code
    c = first = index = 0
    w = br.peek()
    for k in range(1, 16):
        c |= (w >> (k - 1)) & 1
        if c - first < count[k]:
            br.pos += k
            return symbols[index + c - first]
        index += count[k]
        first = (first + count[k]) << 1
        c <<= 1
    return None


def _dynamic(br, rep):
    hlit, hdist, hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
    if hlit > 286 or hdist > 30:
        raise InflateError(INVALID_SYMBOL)
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = br.bits(3)
    br.check()
    code = _build(cl, True)
    lens, prev = [], 0
    while len(lens) < hlit + hdist:
        sym = _decode(br, code)
        if sym is None:
            raise InflateError(INVALID_SYMBOL)
        v, n = sym, 1
        if sym == 16:
            if not lens:
                raise InflateError(INVALID_SYMBOL)
            v, n = prev, 3 + br.bits(2)
        elif sym == 17:
            v, n = 0, 3 + br.bits(3)
        elif sym == 18:
            v, n = 0, 11 + br.bits(7)
        br.check()
        if len(lens) + n > hlit + hdist:
            raise InflateError(INVALID_SYMBOL)
        if sym >= 16 and len(lens) < hlit < len(lens) + n:
            rep.repeat_crossed = True
        lens += [v] * n
        prev = v
    if lens[256] == 0:
        raise InflateError(INCOMPLETE)
    return lens[:hlit], lens[hlit:]


_FIXED = ([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32)


def inflate_member(deflate, isize, crc):
    """deflate data of one member -> (bytes, Report); InflateError(kind) in the order csrc/inflate.hip checks"""
    br, out, rep = _Bits(deflate), bytearray(), Report()
    last = False
    while not last:
        last, btype = br.bits(1) != 0, br.bits(2)
        br.check()
        at = len(out)
        if btype == 3:
            raise InflateError(BAD_BLOCK_TYPE)
        if btype == 0:
            br.pos = (br.pos + 7) & ~7
            n, nn = br.bits(16), br.bits(16)
            br.check()
            if n ^ nn != 0xFFFF:
                raise InflateError(STORED_LENGTH)
            src = br.pos >> 3
            if src + n > len(deflate):
                raise InflateError(DATA_LENGTH)
            if len(out) + n > isize:
                raise InflateError(OUTPUT_OVERRUN)
            out += deflate[src:src + n]
            br.pos += 8 * n
            rep.blocks.append((0, n))
            continue
        ll_lens, d_lens = _FIXED if btype == 1 else _dynamic(br, rep)
        ll, dc = _build(ll_lens, False), _build(d_lens, False)
        rep.max_ll_len, rep.max_d_len = max(rep.max_ll_len, max(ll_lens)), max(rep.max_d_len, max(d_lens))
        while True:
            sym = _decode(br, ll)
            if sym is not None and sym < 256:
                br.check()
                if len(out) >= isize:
                    raise InflateError(OUTPUT_OVERRUN)
                out.append(sym)
                continue
            if sym == 256:
                br.check()
                break
            if sym is None or sym > 285:
                raise InflateError(INVALID_SYMBOL)
            k, length = sym - 257, 258
            if k < 8:
                length = 3 + k
            elif k < 28:
                eb = (k >> 2) - 1
                length = 3 + ((4 + (k & 3)) << eb) + br.bits(eb)
            d = _decode(br, dc)
            if d is None or d > 29:
                raise InflateError(INVALID_SYMBOL)
            dist = 1 + d
            if d >= 4:
                eb = (d >> 1) - 1
                dist = 1 + ((2 + (d & 1)) << eb) + br.bits(eb)
            br.check()
            if dist > len(out):
                raise InflateError(DISTANCE)
            if len(out) + length > isize:
                raise InflateError(OUTPUT_OVERRUN)
            rep.max_distance, rep.max_length = max(rep.max_distance, dist), max(rep.max_length, length)
            rep.first_byte_match |= dist == len(out)
            s = len(out) - dist
            for i in range(length):
                out.append(out[s + i])
        rep.blocks.append((btype, len(out) - at))
    if len(out) != isize:
        raise InflateError(OUTPUT_UNDERRUN)
    if (br.pos + 7) >> 3 != len(deflate):
        raise InflateError(DATA_LENGTH)
    if crc32(out) != crc:
        raise InflateError(CRC)
    return bytes(out), rep


def members(blob):
    """[(offset, size)] by htslib's rule; ValueError on anything kslam_bgzf_scan refuses"""
    at, ms = 0, []
    while at < len(blob):
        h = blob[at:at + 18]
        if len(h) < 18 or h[:4] != b"\x1f\x8b\x08\x04" or h[10:16] != b"\x06\x00BC\x02\x00":
            raise ValueError("member %d at %d: not a BGZF header" % (len(ms), at))
        size = struct.unpack_from("<H", h, 16)[0] + 1
        if size < 26 or at + size > len(blob):
            raise ValueError("member %d at %d: BSIZE" % (len(ms), at))
        ms.append((at, size))
        at += size
    return ms


def inflate(blob):
    """a BGZF file -> (text, [Report per member]); InflateError carries the member's index"""
    text, reps = bytearray(), []
    for k, (at, size) in enumerate(members(blob)):
        crc, isize = struct.unpack_from("<II", blob, at + size - 8)
        try:
            data, rep = inflate_member(blob[at + 18:at + size - 8], isize, crc)
        except InflateError as e:
            raise InflateError(e.kind, k) from None
        text += data
        reps.append(rep)
    return bytes(text), reps
