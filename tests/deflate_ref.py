"""A pure-Python restatement of csrc/bgzf.hip, the BGZF member compressor of include/kslam_bgzf.h, in both of its modes: the
tile-by-tile match rule, the per-thread greedy parse, the length-limited code builder, the dynamic header, the choice between
stored, fixed and dynamic, and the framing.  compress() gives the bytes the device must give; code_lengths() is the code
builder alone (kslam_debug_bgzf_code_lengths); members() adds, per member, a report of what was chosen and why."""
import struct
import zlib

from inflate_ref import CL_ORDER

FIXED, DYNAMIC = 0, 1          # KSLAM_BGZF_DEFLATE_FIXED / _DYNAMIC
MEMBER_IN = 65280
THREADS, SEG = 256, 255        # one workgroup per member; thread t parses bytes [255 t, 255 t + 255)
HASH_BITS, WINDOW = 12, 32768


class MemberReport:
    def __init__(self):
        self.btype = 0
        self.stored_bytes = self.fixed_bytes = self.dynamic_bytes = 0   # dynamic_bytes = 0 in fixed mode
        self.n_matches = 0
        self.hlit = self.hdist = self.hclen = 0
        self.header_bits = 0
        self.cl_symbols = []           # the code-length symbols of the header, in order
        self.repeat_crossed = False    # a 16 / 17 / 18 covered literal/length AND distance lengths
        self.max_ll_len = self.max_d_len = 0


# ---- the code builder (csrc/bgzf.hip: build_code) ----
def code_lengths(counts, limit):
    """Length-limited prefix code over len(counts) >= 2 symbols: a list of lengths, 0 for unused symbols.
    1. fewer than two used symbols: the lowest-numbered symbols with count 0 get count 1 until two have one
    2. the used symbols sorted by (count, symbol)
    3. Huffman by two queues: on equal weight a leaf before an internal node, the older internal node before the younger
    4. deepest leaf above the limit: zlib's repair on the number of codes per length, lengths handed out shortest first in
       the order (count descending, symbol ascending).  `overflow` counts every NODE below the limit, leaves and internal
       nodes alike, as zlib's gen_bitlen does: a subtree of k leaves hanging below the limit holds 2 k - 2 such nodes and
       over-subscribes the clamped code by k - 1 codes of the limit's length, and each round of the repair frees one."""
    c = list(counts)
    n = len(c)
    assert n >= 2
    used, s = sum(1 for x in c if x), 0
    while used < 2:
        if c[s] == 0:
            c[s] = 1
            used += 1
        s += 1
    order = sorted((s for s in range(n) if c[s]), key=lambda s: (c[s], s))
    m = len(order)
    weight = [c[s] for s in order] + [0] * (m - 1)      # leaves 0 .. m - 1, internal nodes m .. 2 m - 2 in order of birth
    parent = [0] * (2 * m - 1)
    i, j = 0, m
    for k in range(m - 1):
        node = m + k
        for _ in range(2):
            if i < m and (j >= node or weight[i] <= weight[j]):
                pick, i = i, i + 1
            else:
                pick, j = j, j + 1
            parent[pick] = node
            weight[node] += weight[pick]
    depth = [0] * (2 * m - 1)
    for x in range(2 * m - 3, -1, -1):                  # a parent is born after its children
        depth[x] = depth[parent[x]] + 1
    lens = [0] * n
    if max(depth[:m]) <= limit:
        for r, s in enumerate(order):
            lens[s] = depth[r]
        return lens
    count = [0] * (limit + 1)
    for r in range(m):
        count[min(depth[r], limit)] += 1
    overflow = sum(1 for d in depth if d > limit)
    while True:
        b = limit - 1
        while count[b] == 0:
            b -= 1
        count[b] -= 1
        count[b + 1] += 2
        count[limit] -= 1
        overflow -= 2
        if overflow <= 0:
            break
    by_count = sorted((s for s in range(n) if c[s]), key=lambda s: (-c[s], s))
    at = 0
    for l in range(1, limit + 1):
        for _ in range(count[l]):
            lens[by_count[at]] = l
            at += 1
    return lens


def _rev(c, n):
    r = 0
    for _ in range(n):
        r, c = (r << 1) | (c & 1), c >> 1
    return r


def canonical_codes(lens):
    """RFC 1951 3.2.2, each code bit-reversed for the LSB-first stream"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = _rev(nxt[l], l)
            nxt[l] += 1
    return out


# ---- tokens ----
def length_symbol(length):
    """-> (symbol, extra bits, extra value)"""
    if length <= 10:
        return 254 + length, 0, 0
    if length == 258:
        return 285, 0, 0
    v = length - 3
    eb = v.bit_length() - 3
    return 257 + 4 * (eb + 1) + ((v >> eb) & 3), eb, v & ((1 << eb) - 1)


def distance_symbol(dist):
    v = dist - 1
    if v < 4:
        return v, 0, 0
    eb = v.bit_length() - 2
    return 2 * eb + 2 + ((v >> eb) & 1), eb, v & ((1 << eb) - 1)


_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_LL_CODE = canonical_codes(_FIXED_LL)
_FIXED_D = [5] * 30
_FIXED_D_CODE = canonical_codes(_FIXED_D + [5, 5])[:30]


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        self.total += n
        if self.n >= 64:
            self.out += (self.acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            self.acc >>= 64
            self.n -= 64

    def done(self):
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) // 8, "little")


# ---- match and parse ----
def candidates(d):
    """cand[p]: distance from p to the latest position of an EARLIER tile of 256 with the same hash of 4 bytes, 0 = none"""
    n = len(d)
    cand, table = [0] * n, {}
    shift = 32 - HASH_BITS
    for t0 in range(0, n, THREADS):
        hs = []
        for p in range(t0, min(t0 + THREADS, n - 3)):
            h = ((int.from_bytes(d[p:p + 4], "little") * 2654435761) & 0xFFFFFFFF) >> shift
            q = table.get(h)
            if q is not None and p - q <= WINDOW:
                cand[p] = p - q
            hs.append(h)
        for k, h in enumerate(hs):
            table[h] = t0 + k          # ascending p: the latest of the tile stays
    return cand


def _common(d, p, q, cap):
    if d[p:p + cap] == d[q:q + cap]:
        return cap
    L = 0
    while d[p + L] == d[q + L]:
        L += 1
    return L


def parse(d):
    """the tokens of a member: (byte,) or (length, distance), thread range by thread range"""
    cand, n, toks = candidates(d), len(d), []
    for s0 in range(0, n, SEG):
        e, p = min(s0 + SEG, n), s0
        while p < e:
            dist, L = cand[p], 0
            if dist:
                L = _common(d, p, p - dist, min(258, e - p))
            if L >= 3:
                toks.append((L, dist))
                p += L
            else:
                toks.append((d[p],))
                p += 1
    return toks


# ---- the dynamic header ----
def _run_length(seq):
    """the hlit + hdist lengths as ONE sequence -> [(symbol, extra bits, extra value, first index, covered)]"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        if v:
            out.append((v, 0, 0, i, 1))
            i, r = i + 1, r - 1
        while r >= 3:
            if v:
                k = min(r, 6)
                out.append((16, 2, k - 3, i, k))
            elif r >= 11:
                k = min(r, 138)
                out.append((18, 7, k - 11, i, k))
            else:
                k = r
                out.append((17, 3, k - 3, i, k))
            i, r = i + k, r - k
        for _ in range(r):
            out.append((v, 0, 0, i, 1))
            i += 1
    return out


def dynamic_header(ll_lens, d_lens, bits, rep):
    hlit = max(257, max(s for s in range(286) if ll_lens[s]) + 1)
    hdist = max(1, max(s for s in range(30) if d_lens[s]) + 1)
    toks = _run_length(ll_lens[:hlit] + d_lens[:hdist])
    hist = [0] * 19
    for t in toks:
        hist[t[0]] += 1
    cl_lens = code_lengths(hist, 7)
    cl_codes = canonical_codes(cl_lens)
    hclen = 19
    while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    at = bits.total
    bits.put(hlit - 257, 5)
    bits.put(hdist - 1, 5)
    bits.put(hclen - 4, 4)
    for k in range(hclen):
        bits.put(cl_lens[CL_ORDER[k]], 3)
    for sym, eb, ev, first, covered in toks:
        bits.put(cl_codes[sym], cl_lens[sym])
        if eb:
            bits.put(ev, eb)
        if sym >= 16 and first < hlit < first + covered:
            rep.repeat_crossed = True
    rep.hlit, rep.hdist, rep.hclen = hlit, hdist, hclen
    rep.cl_symbols = [t[0] for t in toks]
    rep.header_bits = bits.total - at


def _put_tokens(bits, toks, ll_lens, ll_codes, d_lens, d_codes):
    for t in toks:
        if len(t) == 1:
            bits.put(ll_codes[t[0]], ll_lens[t[0]])
            continue
        sym, eb, ev = length_symbol(t[0])
        bits.put(ll_codes[sym], ll_lens[sym])
        if eb:
            bits.put(ev, eb)
        sym, eb, ev = distance_symbol(t[1])
        bits.put(d_codes[sym], d_lens[sym])
        if eb:
            bits.put(ev, eb)
    bits.put(ll_codes[256], ll_lens[256])


def deflate_member(d, mode):
    """one member's deflate data (ONE block, BFINAL = 1) and its report"""
    rep, toks = MemberReport(), parse(d)
    rep.n_matches = sum(1 for t in toks if len(t) == 2)
    fixed = _Bits()
    fixed.put(3, 3)                                     # BFINAL = 1, BTYPE = 01
    _put_tokens(fixed, toks, _FIXED_LL, _FIXED_LL_CODE, _FIXED_D, _FIXED_D_CODE)
    rep.stored_bytes, rep.fixed_bytes = len(d) + 5, (fixed.total + 7) // 8
    best, rep.btype = fixed, 1
    if mode == DYNAMIC:
        ll_hist, d_hist = [0] * 286, [0] * 30
        for t in toks:
            if len(t) == 1:
                ll_hist[t[0]] += 1
            else:
                ll_hist[length_symbol(t[0])[0]] += 1
                d_hist[distance_symbol(t[1])[0]] += 1
        ll_hist[256] = 1
        ll_lens, d_lens = code_lengths(ll_hist, 15), code_lengths(d_hist, 15)
        dyn = _Bits()
        dyn.put(5, 3)                                   # BFINAL = 1, BTYPE = 10
        dynamic_header(ll_lens, d_lens, dyn, rep)
        _put_tokens(dyn, toks, ll_lens, canonical_codes(ll_lens), d_lens, canonical_codes(d_lens))
        rep.dynamic_bytes = (dyn.total + 7) // 8
        rep.max_ll_len, rep.max_d_len = max(ll_lens), max(d_lens)
        if rep.dynamic_bytes < rep.fixed_bytes:         # dynamic only when strictly smaller than fixed
            best, rep.btype = dyn, 2
    body = best.done()
    if len(body) > rep.stored_bytes:                    # stored only when strictly smaller than the winner
        rep.btype = 0
        body = b"\x01" + struct.pack("<HH", len(d), len(d) ^ 0xFFFF) + bytes(d)
    return body, rep


def members(data, mode=FIXED):
    """[(member bytes, MemberReport)] for members of MEMBER_IN input bytes; no EOF marker"""
    assert mode in (FIXED, DYNAMIC)
    data, out = bytes(data), []
    for at in range(0, len(data), MEMBER_IN):
        d = data[at:at + MEMBER_IN]
        body, rep = deflate_member(d, mode)
        size = 18 + len(body) + 8
        head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", size - 1)
        out.append((head + body + struct.pack("<II", zlib.crc32(d), len(d)), rep))
    return out


def compress(data, mode=FIXED):
    return b"".join(m for m, _ in members(data, mode))
