// bgzf.hip -- BGZF (blocked gzip: the framing of bgzip / htslib) compression of a byte string that lies in device memory:
// the SAM text a lane formats (samtext.hip) is compressed where it is, before the copy to the host.
//
// Output: one gzip member per BGZF_MEMBER_IN input bytes (the last one shorter), each
//   1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | 'B' 'C' SLEN 2 BSIZE (member size - 1) | deflate | CRC32 | ISIZE
// and each member's deflate data ONE block with BFINAL = 1: fixed Huffman (BTYPE 01), or stored (BTYPE 00) when that is
// smaller.  Members are independent (matches never reach into an earlier member), so a reader may start at any of them.
// With KSLAM_BGZF_DEFLATE_DYNAMIC (k_bgzf_member<true>, below the four phases) the block may also carry codes of its own
// (BTYPE 10); the smallest of the three forms is written.
//
// One workgroup of 256 threads (4 waves) per member.  LDS holds the member's bytes (65 280 B) and a 4 096-entry hash table of
// earlier positions (16 KiB): 80 KiB, so two workgroups share a CU's 160 KiB.  Four phases, each bounded whatever the data:
//   match   tile by tile (256 positions, one per thread): the hash of the 4 bytes at p looks up the latest position of an
//           EARLIER tile with that hash; the distance goes to a u16 per position in global scratch; after the tile the
//           table takes the tile's positions with atomicMax, so whichever thread runs first the table is the same
//   parse   thread t owns bytes [255 t, 255 t + 255) and walks them greedily (a match is taken when it is at least 3 bytes
//           long; it is cut at the end of the thread's range): at most 255 steps per thread, counting bits only
//   place   a workgroup exclusive scan of the bit counts gives every thread its first bit; the block is stored instead
//           when the fixed-Huffman bits would take more bytes than the stored form
//   emit    the same walk again writes its bits: words a thread covers completely are plain stores, the (zeroed) words
//           it shares with a neighbour take atomicOr -- OR commutes, so the bytes do not depend on the order
// The CRC32 (crc32.h, shared with inflate.hip): each thread's range by a byte table, shifted to its place by a multiplication
// with x^(8 * bytes after it) mod P (GF(2)), XOR-reduced.  Members are written into BGZF_SLOT-byte slots; scan.hip's exclusive scan of their sizes and
// a gather kernel pack them.  BGZF_ROUND members per launch: the scratch does not grow with the input.
//
// k_bgzf_member<true>: the 16 KiB of the hash table are free once the match phase ends; the CRC table takes 1 KiB of them,
// the histograms, the codes, the builder's scratch and the header bits the rest (BG_DYN_* below).  Between match and emit:
//   count   the same greedy walk adds each token's symbols to two LDS histograms (286 literal/length, 30 distance; symbol
//           256 once) and still counts the fixed bits, because the fixed size takes part in the choice
//   build   build_code (below) makes two prefix codes of at most 15 bits, wave 0 the literal/length code and wave 1 the
//           distance code, at the same time
//   header  one lane trims HLIT / HDIST, run-length codes the hlit + hdist lengths as ONE sequence (a run may cross from
//           the literal/length lengths into the distance lengths), wave 0 builds the code-length code (19 symbols, at most
//           7 bits), and one lane writes the header bits to LDS
//   place   a third walk counts each thread's bits with the real code lengths; both bit counts are scanned
//   choice  dynamic when strictly smaller than fixed, stored when strictly smaller than the winner of the two
// Every walk measures its matches again from the candidates: a match is (length 9 bits, distance 16 bits) and the u16 per
// position of the candidate scratch cannot hold it; the measuring is LDS reads only, the scratch would be global memory.
#include "bgzf.h"

#include "crc32.h"

namespace kslam {
namespace {

constexpr uint32_t BG_THREADS = 256;
constexpr uint32_t BG_SEG = BGZF_MEMBER_IN / BG_THREADS;   // 255 bytes per thread
constexpr uint32_t BG_WORDS = BGZF_MEMBER_IN / 4;          // 16 320
constexpr uint32_t BG_MISC = 64;                            // small shared values; also absorbs the one word read past the data
constexpr uint32_t BG_HASH_BITS = 12, BG_HASH = 1u << BG_HASH_BITS;
constexpr uint32_t BG_WINDOW = 32768;
constexpr uint32_t BG_HEADER = 18, BG_TRAILER = 8;
static_assert(BG_SEG * BG_THREADS == BGZF_MEMBER_IN, "one range per thread");
static_assert((BG_WORDS + BG_MISC + BG_HASH) * 4 <= 80 * 1024, "two workgroups per CU");

__device__ __forceinline__ uint32_t byte_at(const uint32_t *d, uint32_t p) { return (d[p >> 2] >> ((p & 3u) * 8u)) & 0xffu; }
__device__ __forceinline__ uint32_t word_at(const uint32_t *d, uint32_t p) {   // bytes p .. p + 3, little-endian
  const uint32_t i = p >> 2;
  return __builtin_amdgcn_alignbyte(d[i + 1], d[i], p & 3u);
}

__device__ inline uint32_t match_len(const uint32_t *d, uint32_t p, uint32_t q, uint32_t cap) {
  uint32_t L = 0;
  while (L < cap) {
    const uint32_t x = word_at(d, p + L) ^ word_at(d, q + L);
    if (x) {
      L += (uint32_t)__builtin_ctz(x) >> 3;
      break;
    }
    L += 4;
  }
  return L < cap ? L : cap;
}

struct Code {   // bits in stream order (LSB first), n <= 32
  uint32_t v, n;
};

__device__ __forceinline__ uint32_t rev(uint32_t c, uint32_t n) { return __builtin_bitreverse32(c) >> (32 - n); }

__device__ inline Code literal_code(uint32_t b) {   // RFC 1951 3.2.6: 0..143 -> 8 bits from 0x30, 144..255 -> 9 bits from 0x190
  return b < 144 ? Code{rev(0x30u + b, 8), 8} : Code{rev(0x190u + b - 144u, 9), 9};
}

struct Sym {   // a length or distance symbol with its extra bits
  uint32_t sym, eb, ev;
};

__device__ __forceinline__ Sym length_symbol(uint32_t len) {
  if (len <= 10) return Sym{254 + len, 0, 0};
  if (len == 258) return Sym{285, 0, 0};
  const uint32_t v = len - 3, eb = 31 - __builtin_clz(v) - 2;
  return Sym{257 + 4 * (eb + 1) + ((v >> eb) & 3u), eb, v & ((1u << eb) - 1)};
}

__device__ __forceinline__ Sym distance_symbol(uint32_t dist) {
  const uint32_t v = dist - 1;
  if (v < 4) return Sym{v, 0, 0};
  const uint32_t eb = 31 - __builtin_clz(v) - 1;
  return Sym{2 * eb + 2 + ((v >> eb) & 1u), eb, v & ((1u << eb) - 1)};
}

__device__ inline Code match_code(uint32_t len, uint32_t dist) {
  const Sym l = length_symbol(len), d = distance_symbol(dist);
  Code c = l.sym < 280 ? Code{rev(l.sym - 256, 7), 7} : Code{rev(l.sym - 280 + 0xC0u, 8), 8};
  c.v |= l.ev << c.n;   // extra bits: LSB first, not reversed
  c.n += l.eb;
  c.v |= rev(d.sym, 5) << c.n;
  c.n += 5;
  c.v |= d.ev << c.n;
  c.n += d.eb;
  return c;
}

// the greedy parse of [s0, e): sink.literal(byte) or sink.match(length, distance) per token
template <typename Sink>
__device__ inline void walk(const uint32_t *d, const uint16_t *cand, uint32_t s0, uint32_t e, Sink &sink) {
  uint32_t p = s0;
  while (p < e) {
    const uint32_t dist = cand[p];
    uint32_t L = 0;
    if (dist) L = match_len(d, p, p - dist, min(258u, e - p));
    if (L >= 3) {
      sink.match(L, dist);
      p += L;
    } else {
      sink.literal(byte_at(d, p));
      p++;
    }
  }
}

struct BitCount {
  uint32_t bits = 0;
  __device__ void operator()(Code c) { bits += c.n; }
};

template <typename Out>
struct FixedCoder {   // tokens -> the codes of RFC 1951 3.2.6
  Out &out;
  __device__ void literal(uint32_t b) { out(literal_code(b)); }
  __device__ void match(uint32_t len, uint32_t dist) { out(match_code(len, dist)); }
};

// A code of k_bgzf_member<true> is a table of one word per symbol: the code in stream order | its length << 16.
__device__ __forceinline__ Code packed_code(uint32_t pk) { return Code{pk & 0xffffu, pk >> 16}; }

template <typename Out>
struct DynamicCoder {   // tokens -> the member's own codes; a match is two pieces, it can be 48 bits long
  Out &out;
  const uint32_t *ll, *dc;
  __device__ void literal(uint32_t b) { out(packed_code(ll[b])); }
  __device__ void match(uint32_t len, uint32_t dist) {
    const Sym l = length_symbol(len), d = distance_symbol(dist);
    Code c = packed_code(ll[l.sym]);
    c.v |= l.ev << c.n;
    c.n += l.eb;
    out(c);
    c = packed_code(dc[d.sym]);
    c.v |= d.ev << c.n;
    c.n += d.eb;
    out(c);
  }
};

struct Histogram {   // count: the symbols into LDS, and the fixed bits
  uint32_t *ll, *dc;
  uint32_t fixed_bits = 0;
  __device__ void literal(uint32_t b) {
    atomicAdd(&ll[b], 1u);
    fixed_bits += b < 144 ? 8 : 9;
  }
  __device__ void match(uint32_t len, uint32_t dist) {
    const Sym l = length_symbol(len), d = distance_symbol(dist);
    atomicAdd(&ll[l.sym], 1u);
    atomicAdd(&dc[d.sym], 1u);
    fixed_bits += (l.sym < 280 ? 7 : 8) + l.eb + 5 + d.eb;
  }
};

struct BitWriter {
  uint32_t *words;
  uint64_t acc = 0;
  uint32_t nacc, w, w_first;
  bool first_shared;
  __device__ BitWriter(uint32_t *wd, uint32_t bit0) : words(wd), nacc(bit0 & 31u), w(bit0 >> 5), w_first(bit0 >> 5), first_shared((bit0 & 31u) != 0) {}
  __device__ void operator()(Code c) {
    acc |= (uint64_t)c.v << nacc;
    nacc += c.n;
    if (nacc >= 32) {
      const uint32_t x = (uint32_t)acc;
      if (w == w_first && first_shared) atomicOr(&words[w], x);
      else words[w] = x;
      w++;
      acc >>= 32;
      nacc -= 32;
    }
  }
  __device__ void finish() {
    if (nacc) atomicOr(&words[w], (uint32_t)acc);
  }
};

// ---- k_bgzf_member<true>: what lies where the hash table was (words) ----
constexpr uint32_t BG_LL = 286, BG_DC = 30, BG_CL = 19, BG_LL_PAD = 288, BG_DC_PAD = 32, BG_CL_PAD = 32;
constexpr uint32_t BG_CL_TOKENS = 320;      // at most 286 + 30 code-length symbols
constexpr uint32_t BG_HDR_WORDS = 160;      // 14 + 19 * 3 + 316 * (7 + 7) bits at the most
__host__ __device__ constexpr uint32_t build_scratch(uint32_t n) { return 7 * n + 48; }   // build_code's scratch for n symbols
constexpr uint32_t BG_DYN_LL_HIST = 256, BG_DYN_DC_HIST = BG_DYN_LL_HIST + BG_LL_PAD, BG_DYN_LL_CODE = BG_DYN_DC_HIST + BG_DC_PAD,
                   BG_DYN_DC_CODE = BG_DYN_LL_CODE + BG_LL_PAD, BG_DYN_HDR = BG_DYN_DC_CODE + BG_DC_PAD,
                   BG_DYN_LL_SCR = BG_DYN_HDR + BG_HDR_WORDS, BG_DYN_DC_SCR = BG_DYN_LL_SCR + build_scratch(BG_LL),
                   BG_DYN_END = BG_DYN_DC_SCR + build_scratch(BG_DC);
// the code-length code lives in the literal/length builder's scratch, which is free by then
constexpr uint32_t BG_DYN_CL_TOK = BG_DYN_LL_SCR, BG_DYN_CL_HIST = BG_DYN_CL_TOK + BG_CL_TOKENS, BG_DYN_CL_CODE = BG_DYN_CL_HIST + BG_CL_PAD,
                   BG_DYN_CL_SCR = BG_DYN_CL_CODE + BG_CL_PAD;
static_assert(BG_DYN_END <= BG_HASH, "the dynamic phases fit where the hash table was");
static_assert(BG_DYN_CL_SCR + build_scratch(BG_CL) <= BG_DYN_DC_SCR, "the code-length code fits the literal/length scratch");
constexpr uint32_t CL_ORDER[BG_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// A length-limited prefix code for the n <= 286 symbols with counts cnt[] (LDS; rule 1 may change two of them), built by
// ONE wave: code[s] = the canonical code of s in stream order | its length << 16, 0 for an unused symbol.  Every thread of
// the workgroup calls it (the barriers are the workgroup's), a wave that has nothing to build with n = 0.  scr: build_scratch(n) words.
//   1. fewer than two used symbols: the lowest-numbered symbols with count 0 get count 1 until two have one, so that every
//      code is complete
//   2. the used symbols sorted by (count, symbol), by counting: each lane counts the symbols below its own
//   3. Huffman by two queues over the sorted leaves, one lane: on equal weight a leaf goes before an internal node and the
//      older internal node before the younger; then each lane walks its nodes' parent chains for their depths
//   4. deepest leaf above the limit: zlib's repair on the number of codes per length -- clamp; overflow = the NODES, leaves
//      and internal, that were deeper than the limit (a subtree of k leaves hanging below the limit holds 2 k - 2 of them
//      and over-subscribes the clamped code by k - 1 codes of the limit's length; each round of the loop frees one) -- and
//      the lengths handed out shortest first to the symbols in the order (count descending, symbol ascending)
//   5. canonical codes (RFC 1951 3.2.2), bit-reversed
__device__ void build_code(uint32_t *cnt, uint32_t n, uint32_t limit, uint32_t *code, uint32_t *scr, uint32_t lane) {
  uint32_t *order = scr, *rdesc = scr + n, *weight = scr + 2 * n, *parent = scr + 4 * n, *len = scr + 6 * n, *per_len = scr + 7 * n,
           *upto = per_len + 16;   // per_len[l]: codes of length l; upto[l]: codes of length <= l / the first code of length l
  // 1
  uint32_t used = 0;
  for (uint32_t s = lane; s < n; s += 64) used += cnt[s] != 0;
  for (int o = 32; o >= 1; o >>= 1) used += __shfl_xor(used, o, 64);
  if (lane == 0)
    for (uint32_t s = 0, u = used; u < 2 && s < n; s++)
      if (cnt[s] == 0) {
        cnt[s] = 1;
        u++;
      }
  if (lane < 16 && n) per_len[lane] = 0;
  const uint32_t m = n ? max(used, 2u) : 0u, root = m ? 2 * m - 2 : 0u;
  __syncthreads();
  // 2
  for (uint32_t s = lane; s < n; s += 64) {
    const uint32_t c = cnt[s];
    len[s] = 0;
    if (!c) continue;
    uint32_t lt = 0, gt = 0, eq_before = 0;
    for (uint32_t s2 = 0; s2 < n; s2++) {
      const uint32_t c2 = cnt[s2];
      if (!c2) continue;
      lt += c2 < c;
      gt += c2 > c;
      eq_before += c2 == c && s2 < s;
    }
    order[lt + eq_before] = s;
    weight[lt + eq_before] = c;
    rdesc[s] = gt + eq_before;
  }
  __syncthreads();
  // 3: leaves 0 .. m - 1 in sorted order, internal nodes m .. 2 m - 2 in order of birth
  if (lane == 0 && m) {
    uint32_t i = 0, j = m;
    for (uint32_t node = m; node <= root; node++) {
      uint32_t w = 0;
      for (int k = 0; k < 2; k++) {
        const uint32_t pick = i < m && (j >= node || weight[i] <= weight[j]) ? i++ : j++;
        parent[pick] = node;
        w += weight[pick];
      }
      weight[node] = w;
    }
  }
  __syncthreads();
  uint32_t deepest = 0, overflow = 0;
  for (uint32_t x = lane; x < root; x += 64) {
    uint32_t d = 0;
    for (uint32_t y = x; y != root; y = parent[y]) d++;
    if (x < m) {
      len[order[x]] = min(d, limit);
      deepest = max(deepest, d);
    }
    overflow += d > limit;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    deepest = max(deepest, (uint32_t)__shfl_xor(deepest, o, 64));
    overflow += __shfl_xor(overflow, o, 64);
  }
  __syncthreads();
  // 4
  const bool repair = deepest > limit;
  if (repair)
    for (uint32_t s = lane; s < n; s += 64)
      if (len[s]) atomicAdd(&per_len[len[s]], 1u);
  __syncthreads();
  if (repair && lane == 0) {
    int left = (int)overflow;
    do {
      uint32_t b = limit - 1;
      while (per_len[b] == 0) b--;
      per_len[b]--;
      per_len[b + 1] += 2;
      per_len[limit]--;
      left -= 2;
    } while (left > 0);
    uint32_t sum = 0;
    for (uint32_t l = 1; l <= limit; l++) upto[l] = sum += per_len[l];
  }
  __syncthreads();
  if (repair)
    for (uint32_t s = lane; s < n; s += 64)
      if (cnt[s]) {
        uint32_t l = 1;
        while (upto[l] <= rdesc[s]) l++;
        len[s] = l;
      }
  if (lane < 16 && n) per_len[lane] = 0;
  __syncthreads();
  // 5
  for (uint32_t s = lane; s < n; s += 64)
    if (len[s]) atomicAdd(&per_len[len[s]], 1u);
  __syncthreads();
  if (lane == 0 && n) {
    uint32_t first = 0;
    for (uint32_t l = 1; l < 16; l++) upto[l] = first = (first + (l > 1 ? per_len[l - 1] : 0u)) << 1;
  }
  __syncthreads();
  for (uint32_t s = lane; s < n; s += 64) {
    const uint32_t l = len[s];
    uint32_t before = 0;
    for (uint32_t s2 = 0; s2 < s; s2++) before += len[s2] == l;
    code[s] = l ? rev(upto[l] + before, l) | l << 16 : 0u;
  }
  __syncthreads();
}

struct LdsBits {   // the header bits, written by one lane
  uint32_t *words;
  uint64_t acc = 0;
  uint32_t nacc = 0, w = 0;
  __device__ void operator()(uint32_t v, uint32_t n) {
    acc |= (uint64_t)v << nacc;
    nacc += n;
    if (nacc >= 32) {
      words[w++] = (uint32_t)acc;
      acc >>= 32;
      nacc -= 32;
    }
  }
  __device__ uint32_t finish() {
    words[w] = (uint32_t)acc;
    return 32 * w + nacc;
  }
};

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x, uint32_t lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += y;
  }
  return x;
}

template <bool DYNAMIC>
__global__ __launch_bounds__(BG_THREADS) void k_bgzf_member(const uint8_t *__restrict__ in, uint64_t n, uint64_t m0,
                                                            uint16_t *__restrict__ cand_all, uint8_t *__restrict__ slots,
                                                            uint32_t *__restrict__ sizes) {
  __shared__ uint32_t lds[BG_WORDS + BG_MISC + BG_HASH];
  uint32_t *data = lds, *misc = lds + BG_WORDS, *table = lds + BG_WORDS + BG_MISC;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint64_t start = (m0 + blockIdx.x) * (uint64_t)BGZF_MEMBER_IN;
  const uint32_t len = (uint32_t)min<uint64_t>(BGZF_MEMBER_IN, n - start);
  uint16_t *cand = cand_all + (uint64_t)blockIdx.x * BGZF_MEMBER_IN;
  uint8_t *slot = slots + (uint64_t)blockIdx.x * BGZF_SLOT;
  uint32_t *slot32 = reinterpret_cast<uint32_t *>(slot);

  // ---- the member into LDS, the table empty (0 = no position; entries are position + 1) ----
  const uint8_t *src = in + start;
  const bool aligned = ((uintptr_t)src & 3u) == 0;
  for (uint32_t i = t; i < BG_WORDS; i += BG_THREADS) {
    uint32_t x = 0;
    if (aligned && 4 * i + 4 <= len) {
      x = reinterpret_cast<const uint32_t *>(src)[i];
    } else {
      for (uint32_t b = 0; b < 4; b++)
        if (4 * i + b < len) x |= (uint32_t)src[4 * i + b] << (8 * b);
    }
    data[i] = x;
  }
  for (uint32_t i = t; i < BG_HASH; i += BG_THREADS) table[i] = 0;
  if (t < BG_MISC) misc[t] = 0;
  __syncthreads();

  // ---- match: candidates from earlier tiles only ----
  for (uint32_t t0 = 0; t0 < len; t0 += BG_THREADS) {
    const uint32_t p = t0 + t;
    uint32_t h = BG_HASH;
    if (p + 4 <= len) {
      h = (word_at(data, p) * 2654435761u) >> (32 - BG_HASH_BITS);
      const uint32_t q = table[h];
      const uint32_t dist = q ? p - (q - 1) : 0;
      cand[p] = (uint16_t)(dist <= BG_WINDOW ? dist : 0);
    } else if (p < len) {
      cand[p] = 0;
    }
    __syncthreads();
    if (h < BG_HASH) atomicMax(&table[h], p + 1);
    __syncthreads();
  }

  // ---- the CRC table where the hash table was ----
  uint32_t *crc_tab = table;
  crc_tab[t] = crc_table_entry(t);
  uint32_t *ll_hist = table + BG_DYN_LL_HIST, *dc_hist = table + BG_DYN_DC_HIST, *ll_code = table + BG_DYN_LL_CODE,
           *dc_code = table + BG_DYN_DC_CODE, *hdr = table + BG_DYN_HDR;
  if constexpr (DYNAMIC)
    for (uint32_t i = t; i < BG_LL_PAD + BG_DC_PAD; i += BG_THREADS) ll_hist[i] = 0;   // both histograms: they are adjacent
  __syncthreads();

  // ---- parse (bit count) + CRC of this thread's range ----
  const uint32_t s0 = min(t * BG_SEG, len), e = min(s0 + BG_SEG, len);
  const uint32_t last_t = (len - 1) / BG_SEG;
  uint32_t fixed_bits;
  if constexpr (DYNAMIC) {   // count
    Histogram hist{ll_hist, dc_hist};
    walk(data, cand, s0, e, hist);
    if (t == 0) atomicAdd(&ll_hist[256], 1u);
    fixed_bits = hist.fixed_bits;
  } else {
    BitCount counter;
    FixedCoder<BitCount> coder{counter};
    walk(data, cand, s0, e, coder);
    fixed_bits = counter.bits;
  }
  const uint32_t my_bits = fixed_bits + (t == 0 ? 3u : 0u) + (t == last_t ? 7u : 0u);
  uint32_t crc = 0xffffffffu;
  for (uint32_t p = s0; p < e; p++) crc = crc_tab[(crc ^ byte_at(data, p)) & 0xffu] ^ (crc >> 8);
  crc = e > s0 ? multmodp(x8nmodp(len - e), ~crc) : 0u;

  uint32_t my_dyn_bits = 0;
  if constexpr (DYNAMIC) {
    __syncthreads();
    // ---- build: wave 0 the literal/length code, wave 1 the distance code ----
    build_code(wave == 0 ? ll_hist : dc_hist, wave == 0 ? BG_LL : wave == 1 ? BG_DC : 0u, 15, wave == 0 ? ll_code : dc_code,
               table + (wave == 0 ? BG_DYN_LL_SCR : BG_DYN_DC_SCR), lane);
    // ---- header: the lengths as one run-length coded sequence, its code, its bits ----
    uint32_t *cl_tok = table + BG_DYN_CL_TOK, *cl_hist = table + BG_DYN_CL_HIST, *cl_code = table + BG_DYN_CL_CODE;
    if (t < BG_CL_PAD) cl_hist[t] = 0;
    __syncthreads();
    if (t == 0) {
      uint32_t hlit = BG_LL, hdist = BG_DC, n_tok = 0;
      while (hlit > 257 && ll_code[hlit - 1] == 0) hlit--;
      while (hdist > 1 && dc_code[hdist - 1] == 0) hdist--;
      auto length_at = [&](uint32_t i) { return (i < hlit ? ll_code[i] : dc_code[i - hlit]) >> 16; };
      auto token = [&](uint32_t sym, uint32_t extra) {
        cl_tok[n_tok++] = sym | extra << 8;
        cl_hist[sym]++;
      };
      const uint32_t total = hlit + hdist;
      for (uint32_t i = 0; i < total;) {
        const uint32_t v = length_at(i);
        uint32_t r = 1;
        while (i + r < total && length_at(i + r) == v) r++;
        if (v) {   // a repeat (16) copies the length before it
          token(v, 0);
          i++;
          r--;
        }
        while (r >= 3) {
          const uint32_t k = v ? min(r, 6u) : min(r, 138u);
          if (v) token(16, k - 3);
          else if (k >= 11) token(18, k - 11);
          else token(17, k - 3);
          i += k;
          r -= k;
        }
        for (; r; r--, i++) token(v, 0);
      }
      misc[13] = n_tok;
      misc[14] = hlit;
      misc[15] = hdist;
    }
    __syncthreads();
    build_code(cl_hist, wave == 0 ? BG_CL : 0u, 7, cl_code, table + BG_DYN_CL_SCR, lane);
    if (t == 0) {
      const uint32_t n_tok = misc[13];
      uint32_t hclen = BG_CL;
      while (hclen > 4 && cl_code[CL_ORDER[hclen - 1]] == 0) hclen--;
      LdsBits bits{hdr};
      bits(misc[14] - 257, 5);
      bits(misc[15] - 1, 5);
      bits(hclen - 4, 4);
      for (uint32_t k = 0; k < hclen; k++) bits(cl_code[CL_ORDER[k]] >> 16, 3);
      for (uint32_t k = 0; k < n_tok; k++) {
        const uint32_t sym = cl_tok[k] & 0xffu, c = cl_code[sym];
        bits(c & 0xffffu, c >> 16);
        if (sym >= 16) bits(cl_tok[k] >> 8, sym == 16 ? 2 : sym == 17 ? 3 : 7);
      }
      misc[12] = bits.finish();
    }
    __syncthreads();
    // ---- place, with the real code lengths ----
    BitCount counter;
    DynamicCoder<BitCount> coder{counter, ll_code, dc_code};
    walk(data, cand, s0, e, coder);
    my_dyn_bits = counter.bits + (t == 0 ? 3u + misc[12] : 0u) + (t == last_t ? ll_code[256] >> 16 : 0u);
  }

  // ---- place: exclusive scan of the bit counts, XOR of the CRC parts ----
  uint32_t x = wave_inclusive_scan(my_bits, lane);
  for (int o = 32; o >= 1; o >>= 1) crc ^= __shfl_xor(crc, o, 64);
  if (lane == 63) misc[wave] = x;
  if (lane == 0) misc[4 + wave] = crc;
  uint32_t xd = 0;
  if constexpr (DYNAMIC) {
    xd = wave_inclusive_scan(my_dyn_bits, lane);
    if (lane == 63) misc[8 + wave] = xd;
  }
  __syncthreads();
  uint32_t bit0 = x - my_bits, total_bits = 0, member_crc = 0;
  for (uint32_t k = 0; k < 4; k++) {
    if (k < wave) bit0 += misc[k];
    total_bits += misc[k];
    member_crc ^= misc[4 + k];
  }
  const uint32_t fixed_bytes = (total_bits + 7) / 8, stored_bytes = len + 5;
  // ---- choice: dynamic when strictly smaller than fixed, stored when strictly smaller than the winner ----
  bool dynamic = false;
  uint32_t coded_bytes = fixed_bytes, out_bits = my_bits;
  if constexpr (DYNAMIC) {
    uint32_t dyn_bit0 = xd - my_dyn_bits, dyn_total = 0;
    for (uint32_t k = 0; k < 4; k++) {
      if (k < wave) dyn_bit0 += misc[8 + k];
      dyn_total += misc[8 + k];
    }
    const uint32_t dynamic_bytes = (dyn_total + 7) / 8;
    dynamic = dynamic_bytes < fixed_bytes;
    if (dynamic) {
      coded_bytes = dynamic_bytes;
      out_bits = my_dyn_bits;
      bit0 = dyn_bit0;
    }
  }
  const bool stored = coded_bytes > stored_bytes;
  const uint32_t deflate_bytes = stored ? stored_bytes : coded_bytes;

  // ---- emit ----
  if (!stored) {
    const uint32_t first = BG_HEADER * 8 + bit0, end = first + out_bits;
    if (out_bits) {   // the words this thread shares with a neighbour start at zero
      if (first & 31u) slot32[first >> 5] = 0;
      if (end & 31u) slot32[end >> 5] = 0;
    }
    __syncthreads();
    if (out_bits) {
      BitWriter out(slot32, first);
      if (DYNAMIC && dynamic) {
        if (t == 0) {   // BFINAL = 1, BTYPE = 10, the header
          out(Code{5u, 3});
          const uint32_t hdr_bits = misc[12];
          for (uint32_t k = 0; k < hdr_bits / 32; k++) out(Code{hdr[k], 32});
          if (hdr_bits & 31u) out(Code{hdr[hdr_bits / 32], hdr_bits & 31u});
        }
        DynamicCoder<BitWriter> coder{out, ll_code, dc_code};
        walk(data, cand, s0, e, coder);
        if (t == last_t) out(packed_code(ll_code[256]));   // end of block
      } else {
        if (t == 0) out(Code{3u, 3});   // BFINAL = 1, BTYPE = 01
        FixedCoder<BitWriter> coder{out};
        walk(data, cand, s0, e, coder);
        if (t == last_t) out(Code{0u, 7});   // end of block: symbol 256, seven 0 bits
      }
      out.finish();
    }
  } else {
    for (uint32_t i = t; i < len; i += BG_THREADS) slot[BG_HEADER + 5 + i] = (uint8_t)byte_at(data, i);
    if (t == 0) {
      slot[BG_HEADER] = 1;   // BFINAL = 1, BTYPE = 00, then to the byte boundary
      slot[BG_HEADER + 1] = (uint8_t)len;
      slot[BG_HEADER + 2] = (uint8_t)(len >> 8);
      slot[BG_HEADER + 3] = (uint8_t)~len;
      slot[BG_HEADER + 4] = (uint8_t)(~len >> 8);
    }
  }
  __syncthreads();

  // ---- header and trailer ----
  if (t == 0) {
    const uint32_t size = BG_HEADER + deflate_bytes + BG_TRAILER, bsize = size - 1;
    const uint8_t head[BG_HEADER] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0,
                                     (uint8_t)bsize, (uint8_t)(bsize >> 8)};
    for (uint32_t i = 0; i < BG_HEADER; i++) slot[i] = head[i];
    uint8_t *tail = slot + BG_HEADER + deflate_bytes;
    for (uint32_t i = 0; i < 4; i++) {
      tail[i] = (uint8_t)(member_crc >> (8 * i));
      tail[4 + i] = (uint8_t)(len >> (8 * i));
    }
    sizes[blockIdx.x] = size;
  }
}

// kslam_debug_bgzf_code_lengths: build_code alone, in one workgroup
__global__ __launch_bounds__(BG_THREADS) void k_bgzf_code_lengths(const uint32_t *__restrict__ counts, uint32_t n, uint32_t limit,
                                                                  uint8_t *__restrict__ lengths) {
  __shared__ uint32_t cnt[BG_LL_PAD], code[BG_LL_PAD], scr[build_scratch(BG_LL)];
  const uint32_t t = threadIdx.x;
  for (uint32_t s = t; s < n; s += BG_THREADS) cnt[s] = counts[s];
  __syncthreads();
  build_code(cnt, t < 64 ? n : 0u, limit, code, scr, t & 63u);
  for (uint32_t s = t; s < n; s += BG_THREADS) lengths[s] = (uint8_t)(code[s] >> 16);
}

// the members of a round, packed at out + done + their exclusive offsets
__global__ __launch_bounds__(256) void k_bgzf_gather(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes,
                                                     const uint64_t *__restrict__ offs, const uint64_t *__restrict__ done,
                                                     uint8_t *__restrict__ out) {
  const uint8_t *src = slots + (uint64_t)blockIdx.x * BGZF_SLOT;
  const uint32_t *src32 = reinterpret_cast<const uint32_t *>(src);
  const uint32_t size = sizes[blockIdx.x];
  const uint64_t d0 = done[0] + offs[blockIdx.x], d1 = d0 + size;
  const uint64_t a0 = min((d0 + 3) & ~3ull, d1), a1 = max(d1 & ~3ull, a0);
  // the bytes before the first and after the last whole destination word
  if (threadIdx.x < a0 - d0) out[d0 + threadIdx.x] = src[threadIdx.x];
  if (threadIdx.x < d1 - a1) out[a1 + threadIdx.x] = src[a1 - d0 + threadIdx.x];
  uint32_t *out32 = reinterpret_cast<uint32_t *>(out + a0);
  const uint32_t so0 = (uint32_t)(a0 - d0), n_words = (uint32_t)((a1 - a0) / 4);
  for (uint32_t j = threadIdx.x; j < n_words; j += blockDim.x) {
    const uint32_t so = so0 + 4 * j;   // a source word may reach into the padding behind the slot
    out32[j] = __builtin_amdgcn_alignbyte(src32[(so >> 2) + 1], src32[so >> 2], so & 3u);
  }
}

__global__ void k_bgzf_advance(uint64_t *totals) {
  if (threadIdx.x == 0) totals[1] += totals[0];
}

}  // namespace

void bgzf_compress_device(const char *d_in, uint64_t n, int deflate, BgzfWork &W, DevBuf &out, uint64_t *out_len, hipStream_t s) {
  const uint64_t members = (n + BGZF_MEMBER_IN - 1) / BGZF_MEMBER_IN;
  out.ensure(n + members * (BG_HEADER + 5 + BG_TRAILER) + 64);   // every member stored: the largest the output can be
  *out_len = 0;
  if (!members) return;
  const uint64_t round = std::min<uint64_t>(members, BGZF_ROUND);
  W.cand.ensure(round * BGZF_MEMBER_IN * sizeof(uint16_t));
  W.slots.ensure(round * BGZF_SLOT + 64);
  W.sizes.ensure(round * sizeof(uint32_t));
  W.offs.ensure(round * sizeof(uint64_t));
  W.scan_tmp.ensure(scan_tmp_bytes(round));
  W.totals.ensure(2 * sizeof(uint64_t));
  uint64_t *totals = W.totals.as<uint64_t>();
  HIPCHK(hipMemsetAsync(totals, 0, 2 * sizeof(uint64_t), s));
  for (uint64_t m0 = 0; m0 < members; m0 += BGZF_ROUND) {
    const uint32_t g = (uint32_t)std::min<uint64_t>(BGZF_ROUND, members - m0);
    hipLaunchKernelGGL(deflate == KSLAM_BGZF_DEFLATE_DYNAMIC ? k_bgzf_member<true> : k_bgzf_member<false>, dim3(g), dim3(BG_THREADS), 0, s, (const uint8_t *)d_in, n, m0, W.cand.as<uint16_t>(),
                       W.slots.as<uint8_t>(), W.sizes.as<uint32_t>());
    exclusive_scan_u32_to_u64(W.sizes.as<uint32_t>(), W.offs.as<uint64_t>(), g, totals, W.scan_tmp.p, s);
    hipLaunchKernelGGL(k_bgzf_gather, dim3(g), dim3(256), 0, s, W.slots.as<const uint8_t>(), W.sizes.as<const uint32_t>(),
                       W.offs.as<const uint64_t>(), totals + 1, out.as<uint8_t>());
    hipLaunchKernelGGL(k_bgzf_advance, dim3(1), dim3(64), 0, s, totals);
    HIPCHK(hipGetLastError());
  }
  read_back(out_len, totals + 1, sizeof(uint64_t), s);
}

void bgzf_code_lengths_device(const uint32_t *d_counts, uint32_t n, uint32_t limit, uint8_t *d_lengths, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf_code_lengths, dim3(1), dim3(BG_THREADS), 0, s, d_counts, n, limit, d_lengths);
  HIPCHK(hipGetLastError());
}

}  // namespace kslam
