"""include/kslam_gunzip.h restated in Python on top of tests/inflate_ref.py: the RFC 1952 header walk, the walk over a whole
file that notes where every block and member begins, the finder's rule for the start of a chunk, the chain of live starts
with the figures kslam_gunzip_last_stats reports, and the 16-bit symbols of a live stretch -- so that a test case can prove it
holds the seam it is named for.  Errors carry the member and the kind the library names."""
import struct
import zlib

import numpy as np

import inflate_ref as R

HEADER, NOT_MEMBER = "gzip header", "not a gzip member"
WINDOW = 32768


class GunzipError(Exception):
    def __init__(self, kind, member=0, at=0):
        super().__init__("gzip member %d (byte offset %d): %s" % (member, at, kind))
        self.kind, self.member, self.at = kind, member, at


def header(blob, at=0):
    """the member header at blob[at:] -> the offset of its deflate data; GunzipError(NOT_MEMBER / HEADER)"""
    end = len(blob)
    if end - at < 2 or blob[at] != 0x1F or blob[at + 1] != 0x8B:
        raise GunzipError(NOT_MEMBER)
    if end - at < 10 or blob[at + 2] != 8:
        raise GunzipError(HEADER)
    flg = blob[at + 3]
    if flg & 0xE0:
        raise GunzipError(HEADER)
    p = at + 10
    if flg & 4:
        if end - p < 2:
            raise GunzipError(HEADER)
        p += 2 + struct.unpack_from("<H", blob, p)[0]
        if p > end:
            raise GunzipError(HEADER)
    for bit in (8, 16):
        if flg & bit:
            z = blob.find(b"\0", p)
            if z < 0:
                raise GunzipError(HEADER)
            p = z + 1
    if flg & 2:
        if end - p < 2:
            raise GunzipError(HEADER)
        p += 2
    return p


class Walk:
    """what one serial pass over the file sees"""
    def __init__(self):
        self.text = bytearray()
        self.blocks = []       # (bit offset of the block header, text offset, member, BTYPE)
        self.members = []      # (header offset, text offset of its first byte, text offset behind its last, trailer offset)
        self.matches = []      # (text offset, distance, length)


def walk(blob):
    """the whole file, serially -> Walk; GunzipError(kind, member, header offset) for what kslam_gunzip_inflate refuses"""
    blob = bytes(blob)
    w, at, member = Walk(), 0, 0
    out = w.text
    while at < len(blob):
        m_at, m_out = at, len(out)
        try:
            br = R._Bits(blob)
            br.pos = 8 * header(blob, at)
            rep = R.Report()
            last = False
            while not last:
                start = br.pos
                last, btype = br.bits(1) != 0, br.bits(2)
                br.check()
                w.blocks.append((start, len(out), member, btype))
                if btype == 3:
                    raise R.InflateError(R.BAD_BLOCK_TYPE)
                if btype == 0:
                    br.pos = (br.pos + 7) & ~7
                    n, nn = br.bits(16), br.bits(16)
                    br.check()
                    if n ^ nn != 0xFFFF:
                        raise R.InflateError(R.STORED_LENGTH)
                    src = br.pos >> 3
                    if src + n > len(blob):
                        raise R.InflateError(R.DATA_LENGTH)
                    out += blob[src:src + n]
                    br.pos += 8 * n
                    continue
                ll_lens, d_lens = R._FIXED if btype == 1 else R._dynamic(br, rep)
                ll, dc = R._build(ll_lens, False), R._build(d_lens, False)
                while True:
                    sym = R._decode(br, ll)
                    if sym is not None and sym < 256:
                        br.check()
                        out.append(sym)
                        continue
                    if sym == 256:
                        br.check()
                        break
                    if sym is None or sym > 285:
                        raise R.InflateError(R.INVALID_SYMBOL)
                    k, length = sym - 257, 258
                    if k < 8:
                        length = 3 + k
                    elif k < 28:
                        eb = (k >> 2) - 1
                        length = 3 + ((4 + (k & 3)) << eb) + br.bits(eb)
                    d = R._decode(br, dc)
                    if d is None or d > 29:
                        raise R.InflateError(R.INVALID_SYMBOL)
                    dist = 1 + d
                    if d >= 4:
                        eb = (d >> 1) - 1
                        dist = 1 + ((2 + (d & 1)) << eb) + br.bits(eb)
                    br.check()
                    if dist > len(out) - m_out:
                        raise R.InflateError(R.DISTANCE)
                    w.matches.append((len(out), dist, length))
                    s = len(out) - dist
                    if dist >= length:
                        out += out[s:s + length]
                    else:
                        for i in range(length):
                            out.append(out[s + i])
            trailer = (br.pos + 7) >> 3
            if trailer + 8 > len(blob):
                raise R.InflateError(R.DATA_LENGTH)
            crc, isize = struct.unpack_from("<II", blob, trailer)
            if zlib.crc32(bytes(out[m_out:])) != crc:
                raise R.InflateError(R.CRC)
            produced = (len(out) - m_out) & 0xFFFFFFFF
            if produced != isize:
                raise R.InflateError(R.OUTPUT_UNDERRUN if produced < isize else R.OUTPUT_OVERRUN)
        except (R.InflateError, GunzipError) as e:
            raise GunzipError(e.kind, member, m_at) from None
        w.members.append((m_at, m_out, len(out), trailer))
        member += 1
        at = trailer + 8
        while at < len(blob) and blob[at] == 0:      # zero bytes behind a member are skipped
            at += 1
    return w


# ---- the finder's rule ----
def _field(bits, p, off, n):
    v = np.zeros(len(p), dtype=np.int64)
    for i in range(n):
        v |= bits[p + off + i].astype(np.int64) << i
    return v


def candidates(blob):
    """the bit offsets of the whole file that pass everything a numpy pass can decide: the 17 header bits (BFINAL 0, BTYPE 2,
    HLIT <= 29, HDIST <= 29), the code-length code's bits lying inside the file, and its Kraft sum being complete -- which is
    what _build(cl, True) asks, except that it lets a code of no symbols through, and that one fails at its first length"""
    bits = np.unpackbits(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8), bitorder="little")
    end = 8 * len(blob)
    p = np.flatnonzero((bits[:end] == 0) & (bits[1:end + 1] == 0) & (bits[2:end + 2] == 1))
    p = p[(_field(bits, p, 3, 5) <= 29) & (_field(bits, p, 8, 5) <= 29)]
    hclen = _field(bits, p, 13, 4) + 4
    keep = p + 17 + 3 * hclen <= end
    p, hclen = p[keep], hclen[keep]
    kraft = np.zeros(len(p), dtype=np.int64)
    for i in range(19):
        l = _field(bits, p, 17 + 3 * i, 3)
        kraft += np.where((i < hclen) & (l > 0), 128 >> l, 0)
    return p[kraft == 128]


def is_start(blob, p):
    """THE RULE at bit offset p, in inflate_ref's terms: bits(3) == 4, then _dynamic, then two _build"""
    br = R._Bits(blob)
    br.pos = p
    if br.bits(3) != 4:
        return False
    try:
        ll, dc = R._dynamic(br, R.Report())
        R._build(ll, False)
        R._build(dc, False)
    except R.InflateError:
        return False
    return True


class Finder:
    """the candidates of one file, checked in full once each, for any chunk size"""
    def __init__(self, blob):
        self.blob, self.cand, self.known = bytes(blob), candidates(blob), {}

    def starts(self, chunk):
        """{chunk number: the LOWEST bit offset inside it at which the rule holds}, for every chunk but the first"""
        out = {}
        n_chunks = (len(self.blob) + chunk - 1) // chunk
        for p in self.cand:
            p = int(p)
            k = p // (8 * chunk)
            if k == 0 or k in out or k >= n_chunks:
                continue
            if p not in self.known:
                self.known[p] = is_start(self.blob, p)
            if self.known[p]:
                out[k] = p
        return out


class Plan:
    """the chain for one chunk size: the figures of kslam_gunzip_last_stats, and the live stretches"""
    def __init__(self, blob, w, found, chunk):
        true_starts = {b[0]: b[1] for b in w.blocks}          # bit offset -> text offset
        self.found = dict(found)
        live = sorted(p for p in found.values() if p in true_starts)
        first = w.blocks[0][0]
        chain = sorted(set(live) | {first})
        self.spans = [(p, true_starts[p]) for p in chain]      # (bit offset, text offset) of every live stretch, in order
        self.stats = {"members": len(w.members), "chunks": (len(blob) + chunk - 1) // chunk, "starts_found": len(found),
                      "starts_live": len(live), "starts_dropped": len(found) - len(live), "text_len": len(w.text)}

    def span_lengths(self, text_len):
        offs = [s[1] for s in self.spans] + [text_len]
        return [b - a for a, b in zip(offs, offs[1:])]


def plan(blob, chunk, w=None, finder=None):
    blob = bytes(blob)
    if not blob:
        p = Plan.__new__(Plan)
        p.found, p.spans = {}, []
        p.stats = {"members": 0, "chunks": 0, "starts_found": 0, "starts_live": 0, "starts_dropped": 0, "text_len": 0}
        return p
    w = w or walk(blob)
    finder = finder or Finder(blob)
    return Plan(blob, w, finder.starts(chunk), chunk)


class SymbolReport:
    def __init__(self):
        self.far_spans_back = set()     # matches of distance >= 32 000 that reach before their stretch: how many stretches back the source begins
        self.marker_copied = False      # a match inside a stretch copied a marker
        self.rle_over_markers = False   # ... with distance < length
        self.first_tokens = {}          # stretch number -> (distance, length) of a match that is its very first token


def symbols(w, pl):
    """the decode pass on every live stretch: which symbols are markers, and what the matches did with them"""
    rep = SymbolReport()
    offs = [s[1] for s in pl.spans] + [len(w.text)]
    mi = 0
    for j, (a, b) in enumerate(zip(offs, offs[1:])):
        marker = np.zeros(b - a, dtype=bool)
        while mi < len(w.matches) and w.matches[mi][0] < b:
            pos, dist, length = w.matches[mi]
            mi += 1
            if pos < a:
                continue
            if pos == a:
                rep.first_tokens[j] = (dist, length)
            src = pos - dist
            if src < a and dist >= 32000:
                back = 0
                while offs[j - back] > src:
                    back += 1
                rep.far_spans_back.add(back)
            for i in range(length):
                s = src + (i % dist if dist < length else i)
                m = s < a or marker[s - a]
                marker[pos - a + i] = m
                if m and s >= a:
                    rep.marker_copied = True
                    if dist < length:
                        rep.rle_over_markers = True
    return rep
