// inflate.hip -- the members of a BGZF file (include/kslam_inflate.h) inflated on the device: RFC 1951 in full (stored, fixed
// and dynamic Huffman blocks, any number of blocks per member, distances up to 32 768), from the compressed bytes straight to
// each member's place in the text.  bgzf.hip is the writer; this is the reader, also of what other tools wrote.
//
// One WAVE per member, INFLATE_WAVES waves per workgroup.  Members are independent, and inside a member the symbols are
// a serial chain (the next code starts where this one ends), so the unit of parallelism is the member: the wave decodes with
// values that are the same in every lane (they live in scalar registers), and uses its 64 lanes for what is wide:
//   input    the next 256 bytes of deflate data sit one word per lane in a register; the bit reader takes word k with a
//            readlane, so a refill costs no memory access, and a window is loaded with one coalesced read
//   tables   per wave in LDS (WaveLds, 2 272 B): for each of the two codes the count per length, the symbols in canonical
//            order, and a direct table of the first 9 (literal/length) or 6 (distance) bits.  Built lane-parallel from the
//            code lengths: ranks by ballot, the direct table one ENTRY per lane (each entry walks the <= 9 lengths), so
//            the work is the same whatever the code looks like.  Codes longer than the direct table walk the counts (at
//            most 15 steps).  That is 928 entries of 16 bits, below the 1 444 (852 + 592) that zlib's two-level tables
//            need for the same roots: the canonical walk replaces the second level.
//   output   literals collect one per lane and leave as one coalesced store per 64; a match is copied by the whole wave,
//            byte i from src[i % distance] when it overlaps itself (distance < length)
//   CRC-32   each lane takes 1/64 of the member's text by the byte table, the parts are shifted and XOR-ed (crc32.h)
//
// The fence.  A match reads bytes that OTHER lanes of the same wave stored earlier (literals, earlier matches), through
// global memory.  Between those stores and the loads stands wave_sync(): a release fence, a wave barrier and an acquire
// fence, all of wavefront scope.  That suffices because both sides are the same wave: its vector memory instructions are
// issued in program order to the one L1 of its CU, which returns a load after an earlier store of the same wave to the
// same address with that store's data -- the AMDGPU memory model therefore needs no cache action and no wait for
// wavefront scope.  What the fence has to stop is the COMPILER moving a load above a store it cannot see a dependence
// on (another lane's address), and that is what it does.  No other wave ever reads a member's bytes before the kernel ends.
//
// Safe on any input.  Nothing here trusts the bytes: the window never loads a word beyond the member's deflate data and
// zeroes the bytes of its last word that lie behind them; every symbol is checked against the end of the data BEFORE it
// acts; a store happens only after outpos + length <= ISIZE, a match only after distance <= outpos; every loop step
// consumes at least one bit or ends.  The first violation ends the member with an InflateError.
#include "inflate.h"

#include "crc32.h"

namespace kslam {
namespace {

constexpr uint32_t INF_THREADS = INFLATE_WAVES * 64;
constexpr uint32_t LL_ROOT = 9, D_ROOT = 6, CL_ROOT = 7;
constexpr uint32_t MAX_LL = 288, MAX_D = 32, N_CL = 19;
constexpr uint32_t NO_SYMBOL = 0xffffu;
static_assert(INF_THREADS == 256, "the CRC byte table is filled one entry per thread");

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

// one member: in[M.in_off .. + M.in_len) -> o[0 .. M.isize)
__device__ uint32_t inflate_member(const uint8_t *__restrict__ in, const InflateMember &M, uint8_t *o, WaveLds &L, const uint32_t *crc_tab,
                                   uint32_t lane) {
  const uint32_t isize = M.isize, in_end = M.in_off + M.in_len, end_bit = in_end * 8u;
  BitReader br{reinterpret_cast<const uint32_t *>(in), lane};
  br.end = in_end;
  br.start(M.in_off);
  uint32_t outpos = 0;          // bytes produced, the waiting literals included
  uint32_t pend = 0, npend = 0; // literals waiting for their store: lane k holds byte outpos - npend + k
  bool fixed_ready = false;
  auto flush = [&] {
    if (lane < npend) o[outpos - npend + lane] = (uint8_t)pend;
    npend = 0;
  };
  for (bool last = false; !last;) {
    br.refill();
    last = br.bits(1) != 0;
    const uint32_t type = br.bits(2);
    if (br.bit_pos() > end_bit) return INF_DATA_LENGTH;
    if (type == 3u) return INF_BAD_BLOCK_TYPE;
    if (type == 0u) {   // stored: to the byte boundary, LEN, ~LEN, the bytes
      br.drop(br.n & 7u);
      br.refill();
      const uint32_t len = br.bits(16), nlen = br.bits(16);
      if (br.bit_pos() > end_bit) return INF_DATA_LENGTH;
      if ((len ^ nlen) != 0xffffu) return INF_STORED_LENGTH;
      const uint32_t src = br.bit_pos() >> 3;
      if (src + len > in_end) return INF_DATA_LENGTH;
      if (outpos + len > isize) return INF_OUTPUT_OVERRUN;
      flush();
      for (uint32_t i = lane; i < len; i += 64) o[outpos + i] = in[src + i];
      outpos += len;
      br.start(src + len);
      continue;
    }
    if (type == 1u) {
      if (!fixed_ready) {
        for (uint32_t s = lane; s < MAX_LL; s += 64) L.lens[s] = s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8;
        if (lane < MAX_D) L.lens[MAX_LL + lane] = 5;
        wave_sync();
        (void)build_code(L.lens, MAX_LL, L.cnt_ll, L.sorted_ll, L.fast_ll, LL_ROOT, false, lane);
        (void)build_code(L.lens + MAX_LL, MAX_D, L.cnt_d, L.sorted_d, L.fast_d, D_ROOT, false, lane);
        fixed_ready = true;
      }
    } else {
      fixed_ready = false;
      uint32_t n_ll = 0, n_d = 0;
      uint32_t err = read_dynamic_lengths(br, L, end_bit, lane, &n_ll, &n_d);
      if (!err) err = build_code(L.lens, n_ll, L.cnt_ll, L.sorted_ll, L.fast_ll, LL_ROOT, false, lane);
      if (!err) err = build_code(L.lens + n_ll, n_d, L.cnt_d, L.sorted_d, L.fast_d, D_ROOT, false, lane);
      if (err) return err;
    }
    for (;;) {   // every turn consumes at least one bit, or returns
      br.refill();
      const uint32_t sym = decode(br, L.fast_ll, LL_ROOT, L.cnt_ll, L.sorted_ll);
      if (sym < 256u) {
        if (br.bit_pos() > end_bit) return INF_DATA_LENGTH;
        if (outpos >= isize) return INF_OUTPUT_OVERRUN;
        if (lane == npend) pend = sym;
        npend++;
        outpos++;
        if (npend == 64u) flush();
        continue;
      }
      if (sym == 256u) {
        if (br.bit_pos() > end_bit) return INF_DATA_LENGTH;
        break;
      }
      if (sym > 285u) return INF_INVALID_SYMBOL;   // 286, 287 of the fixed code, and NO_SYMBOL
      const uint32_t k = sym - 257u;
      uint32_t len = 258;
      if (k < 8u) {
        len = 3u + k;
      } else if (k < 28u) {
        const uint32_t eb = (k >> 2) - 1u;
        len = 3u + ((4u + (k & 3u)) << eb) + br.bits(eb);
      }
      br.refill();
      const uint32_t d = decode(br, L.fast_d, D_ROOT, L.cnt_d, L.sorted_d);
      if (d > 29u) return INF_INVALID_SYMBOL;       // 30, 31 of the fixed code, and NO_SYMBOL
      uint32_t dist = 1u + d;
      if (d >= 4u) {
        const uint32_t eb = (d >> 1) - 1u;
        dist = 1u + ((2u + (d & 1u)) << eb) + br.bits(eb);
      }
      if (br.bit_pos() > end_bit) return INF_DATA_LENGTH;
      if (dist > outpos) return INF_DISTANCE;
      if (outpos + len > isize) return INF_OUTPUT_OVERRUN;
      flush();
      wave_sync();   // the sources are bytes other lanes stored: see the head of the file
      const uint8_t *src = o + (outpos - dist);
      for (uint32_t i = lane; i < len; i += 64) o[outpos + i] = src[dist < len ? i % dist : i];
      outpos += len;
    }
  }
  flush();
  if (outpos != isize) return INF_OUTPUT_UNDERRUN;
  if (((br.bit_pos() + 7u) >> 3) != in_end) return INF_DATA_LENGTH;   // the trailer does not follow the last block
  wave_sync();
  // ---- CRC-32 of the text: 1/64 per lane, shifted to its place, XOR-ed ----
  const uint32_t chunk = (isize + 63u) / 64u, s0 = min(lane * chunk, isize), e = min(s0 + chunk, isize);
  uint32_t crc = 0xffffffffu;
  for (uint32_t p = s0; p < e; p++) crc = crc_tab[(crc ^ o[p]) & 0xffu] ^ (crc >> 8);
  crc = e > s0 ? multmodp(x8nmodp(isize - e), ~crc) : 0u;
  for (int w = 32; w >= 1; w >>= 1) crc ^= __shfl_xor(crc, w, 64);
  return crc == M.crc ? INF_OK : INF_CRC;
}

__global__ __launch_bounds__(INF_THREADS) void k_inflate_members(const uint8_t *__restrict__ in, const InflateMember *__restrict__ members,
                                                                 uint32_t n, uint8_t *out, unsigned long long *first_bad) {
  __shared__ uint32_t crc_tab[256];
  __shared__ WaveLds lds[INFLATE_WAVES];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  crc_tab[t] = crc_table_entry(t);
  __syncthreads();
  const uint32_t m = blockIdx.x * INFLATE_WAVES + wave;
  if (m >= n) return;
  InflateMember M;
  M.in_off = uni(members[m].in_off);
  M.in_len = uni(members[m].in_len);
  M.out_off = uni(members[m].out_off);
  M.isize = uni(members[m].isize);
  M.crc = uni(members[m].crc);
  const uint32_t err = inflate_member(in, M, out + M.out_off, lds[wave], crc_tab, lane);
  if (err && lane == 0) atomicMin(first_bad, ((unsigned long long)m << 8) | err);
}

}  // namespace

const char *inflate_error_name(uint32_t kind) {
  static const char *const names[] = {"ok", "bad block type", "stored length check", "code lengths over-subscribed", "code lengths incomplete",
                                      "invalid symbol", "distance too far back", "output overrun", "output underrun", "CRC mismatch",
                                      "deflate data length"};
  return kind < sizeof names / sizeof names[0] ? names[kind] : "unknown error";
}

void inflate_members_device(const uint8_t *d_in, const InflateMember *d_members, uint32_t n, uint8_t *d_out, uint64_t *d_first_bad,
                            hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_inflate_members, dim3((n + INFLATE_WAVES - 1) / INFLATE_WAVES), dim3(INF_THREADS), 0, s, d_in, d_members, n, d_out,
                     reinterpret_cast<unsigned long long *>(d_first_bad));
  HIPCHK(hipGetLastError());
}

}  // namespace kslam
