// inflate_core.h -- what the two inflaters share: inflate.hip (BGZF, one wave per member) and gunzip.hip (plain gzip, one
// wave per block start).  A wave-uniform bit reader over a window of 64 words held one per lane, the per-wave code tables
// in LDS built lane-parallel from the code lengths, the symbol decoder, and the reader of a dynamic block's code lengths.
// Everything here is per translation unit (anonymous namespace), as in crc32.h.  How the pieces work, the fence and why
// they are safe on any input is told at the head of inflate.hip.
#pragma once
#include "inflate.h"

namespace kslam {
namespace {

constexpr uint32_t LL_ROOT = 9, D_ROOT = 6, CL_ROOT = 7;
constexpr uint32_t MAX_LL = 288, MAX_D = 32, N_CL = 19;
constexpr uint32_t NO_SYMBOL = 0xffffu;

struct WaveLds {
  uint32_t cnt_ll[16], cnt_d[16];                  // codes per length
  uint16_t sorted_ll[MAX_LL], sorted_d[MAX_D];     // symbols in canonical order (by length, then by symbol)
  uint16_t fast_ll[1u << LL_ROOT], fast_d[1u << D_ROOT];   // symbol | length << 12 of the code the index starts with; 0: none that short
  uint8_t lens[MAX_LL + MAX_D], cl_lens[N_CL + 13];         // the code lengths being read; those of the code-length code
};
static_assert(sizeof(WaveLds) == 2272, "the LDS budget DESIGN.md states");
static_assert((1u << CL_ROOT) <= (1u << LL_ROOT) && N_CL <= MAX_LL, "the code-length code borrows the literal/length tables");

__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LSB-first bits of in[first .. end), every value the same in all lanes.  Positions are bits from the start of `in`.
struct BitReader {
  const uint32_t *words;
  uint32_t lane;
  uint32_t win = 0;        // per lane: word wbase + lane
  uint32_t wbase = 0, next = 0;
  uint32_t end = 0;        // the byte behind the deflate data
  uint64_t buf = 0;
  uint32_t n = 0;          // valid bits in buf

  __device__ void load_window() {
    wbase = next;
    const uint32_t w = wbase + lane, wend = (end + 3) >> 2;
    uint32_t x = w < wend ? words[w] : 0u;
    if (w == (end >> 2) && (end & 3u)) x &= (1u << (8u * (end & 3u))) - 1u;   // the trailer's bytes in the last word
    win = x;
  }
  __device__ uint32_t take() {
    if (next - wbase >= 64u) load_window();
    const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)win, (int)uni(next - wbase));
    next++;
    return w;
  }
  __device__ void start(uint32_t byte_pos) {   // the bytes of the first word before byte_pos are shifted out unseen
    next = byte_pos >> 2;
    load_window();
    const uint32_t sh = (byte_pos & 3u) * 8u;
    buf = take() >> sh;
    n = 32u - sh;
  }
  __device__ void refill() {   // afterwards n >= 33
    while (n <= 32u) {
      buf |= (uint64_t)take() << n;
      n += 32u;
    }
  }
  __device__ uint32_t peek(uint32_t k) const { return (uint32_t)buf & ((1u << k) - 1u); }
  __device__ void drop(uint32_t k) { buf >>= k; n -= k; }
  __device__ uint32_t bits(uint32_t k) {
    const uint32_t v = peek(k);
    drop(k);
    return v;
  }
  __device__ uint32_t bit_pos() const { return next * 32u - n; }   // of the next bit nobody consumed
};

// lens[0 .. n) -> cnt, sorted, fast[0 .. 1 << root).  0, or why RFC 1951 forbids these lengths: zlib's rule -- never
// over-subscribed; incomplete only as no code at all, or (not for the code-length code) a single code of one bit.
__device__ uint32_t build_code(const uint8_t *lens, uint32_t n, uint32_t *cnt, uint16_t *sorted, uint16_t *fast, uint32_t root, bool is_cl,
                               uint32_t lane) {
  uint32_t c[16];
#pragma unroll
  for (uint32_t k = 0; k < 16; k++) c[k] = 0;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t s = base + lane, l = s < n ? lens[s] : 0u;
#pragma unroll
    for (uint32_t k = 1; k < 16; k++) c[k] += (uint32_t)__popcll(__ballot(l == k));
  }
  int32_t left = 1;
  uint32_t total = 0, longest = 0;
#pragma unroll
  for (uint32_t k = 1; k < 16; k++) {
    left = (left << 1) - (int32_t)c[k];
    if (left < 0) return INF_OVERSUBSCRIBED;
    total += c[k];
    if (c[k]) longest = k;
  }
  if (left > 0 && total > 0 && (is_cl || longest != 1)) return INF_INCOMPLETE;
  uint32_t at[16];
  at[1] = 0;
#pragma unroll
  for (uint32_t k = 2; k < 16; k++) at[k] = at[k - 1] + c[k - 1];
  if (lane == 0) {
#pragma unroll
    for (uint32_t k = 1; k < 16; k++) cnt[k] = c[k];
  }
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t s = base + lane, l = s < n ? lens[s] : 0u;
#pragma unroll
    for (uint32_t k = 1; k < 16; k++) {
      const uint64_t m = __ballot(l == k);
      if (l == k) sorted[at[k] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)s;
      at[k] += (uint32_t)__popcll(m);
    }
  }
  wave_sync();
  for (uint32_t i = lane; i < (1u << root); i += 64) {   // entry i: the code that i's low bits start with, if it has <= root bits
    uint32_t e = 0, code = 0, first = 0, index = 0;
#pragma unroll
    for (uint32_t len = 1; len <= LL_ROOT; len++) {
      if (len <= root && e == 0) {
        code |= (i >> (len - 1)) & 1u;
        if (code - first < c[len]) e = sorted[index + code - first] | (len << 12);
        index += c[len];
        first = (first + c[len]) << 1;
        code <<= 1;
      }
    }
    fast[i] = (uint16_t)e;
  }
  wave_sync();
  return INF_OK;
}

// the next symbol of a code (the reader holds >= 15 bits); NO_SYMBOL: these bits start no code
__device__ uint32_t decode(BitReader &br, const uint16_t *fast, uint32_t root, const uint32_t *cnt, const uint16_t *sorted) {
  const uint32_t e = uni(fast[br.peek(root)]);
  if (e) {
    br.drop(e >> 12);
    return e & 0xfffu;
  }
  uint32_t code = 0, first = 0, index = 0, b = (uint32_t)br.buf;
  for (uint32_t len = 1; len <= 15; len++) {
    code |= b & 1u;
    b >>= 1;
    const uint32_t count = uni(cnt[len]);
    if (code - first < count) {
      br.drop(len);
      return uni(sorted[index + code - first]);
    }
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return NO_SYMBOL;
}

__constant__ uint8_t CL_ORDER[N_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// HLIT, HDIST, HCLEN, the code-length code and the two codes' lengths (RFC 1951 3.2.7) -> L.lens[0 .. *n_ll + *n_d)
__device__ uint32_t read_dynamic_lengths(BitReader &br, WaveLds &L, uint32_t end_bit, uint32_t lane, uint32_t *n_ll, uint32_t *n_d) {
  br.refill();
  const uint32_t hlit = br.bits(5) + 257u, hdist = br.bits(5) + 1u, hclen = br.bits(4) + 4u;
  if (hlit > 286u || hdist > 30u) return INF_INVALID_SYMBOL;
  if (lane < N_CL) L.cl_lens[lane] = 0;
  wave_sync();
  for (uint32_t i = 0; i < hclen; i++) {
    br.refill();
    const uint32_t v = br.bits(3);
    if (lane == 0) L.cl_lens[CL_ORDER[i]] = (uint8_t)v;
  }
  if (br.bit_pos() > end_bit) return INF_DATA_LENGTH;
  wave_sync();
  uint32_t err = build_code(L.cl_lens, N_CL, L.cnt_ll, L.sorted_ll, L.fast_ll, CL_ROOT, true, lane);
  if (err) return err;
  const uint32_t total = hlit + hdist;
  uint32_t i = 0, prev = 0;
  while (i < total) {
    br.refill();
    const uint32_t sym = decode(br, L.fast_ll, CL_ROOT, L.cnt_ll, L.sorted_ll);
    if (sym > 18u) return INF_INVALID_SYMBOL;
    uint32_t v = sym, rep = 1;
    if (sym == 16u) {
      if (i == 0) return INF_INVALID_SYMBOL;   // nothing to repeat
      v = prev;
      rep = 3u + br.bits(2);
    } else if (sym == 17u) {
      v = 0;
      rep = 3u + br.bits(3);
    } else if (sym == 18u) {
      v = 0;
      rep = 11u + br.bits(7);
    }
    if (br.bit_pos() > end_bit) return INF_DATA_LENGTH;
    if (i + rep > total) return INF_INVALID_SYMBOL;   // a repeat beyond the last length
    for (uint32_t j = lane; j < rep; j += 64) L.lens[i + j] = (uint8_t)v;
    prev = v;
    i += rep;
  }
  wave_sync();
  if (uni(L.lens[256]) == 0) return INF_INCOMPLETE;   // no end-of-block code: the block could never end
  *n_ll = hlit;
  *n_d = hdist;
  return INF_OK;
}

// the codes of a fixed block (RFC 1951 3.2.6) into the wave's tables
__device__ __forceinline__ void build_fixed_codes(WaveLds &L, uint32_t lane) {
  for (uint32_t s = lane; s < MAX_LL; s += 64) L.lens[s] = s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8;
  if (lane < MAX_D) L.lens[MAX_LL + lane] = 5;
  wave_sync();
  (void)build_code(L.lens, MAX_LL, L.cnt_ll, L.sorted_ll, L.fast_ll, LL_ROOT, false, lane);
  (void)build_code(L.lens + MAX_LL, MAX_D, L.cnt_d, L.sorted_d, L.fast_d, D_ROOT, false, lane);
}

}  // namespace
}  // namespace kslam
