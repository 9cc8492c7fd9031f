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
//
// The bit reader, the tables and the decoder live in inflate_core.h: gunzip.hip (plain gzip) uses the same ones.
#include "inflate.h"

#include "crc32.h"
#include "inflate_core.h"

namespace kslam {
namespace {

constexpr uint32_t INF_THREADS = INFLATE_WAVES * 64;
static_assert(INF_THREADS == 256, "the CRC byte table is filled one entry per thread");

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
        build_fixed_codes(L, lane);
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
