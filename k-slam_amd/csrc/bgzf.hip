// bgzf.hip -- BGZF (blocked gzip: the framing of bgzip / htslib) compression of a byte string that lies in device memory:
// the SAM text a lane formats (samtext.hip) is compressed where it is, before the copy to the host.
//
// Output: one gzip member per BGZF_MEMBER_IN input bytes (the last one shorter), each
//   1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | 'B' 'C' SLEN 2 BSIZE (member size - 1) | deflate | CRC32 | ISIZE
// and each member's deflate data ONE block with BFINAL = 1: fixed Huffman (BTYPE 01), or stored (BTYPE 00) when that is
// smaller.  Members are independent (matches never reach into an earlier member), so a reader may start at any of them.
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

struct Code {   // bits in stream order (LSB first), n <= 31
  uint32_t v, n;
};

__device__ __forceinline__ uint32_t rev(uint32_t c, uint32_t n) { return __builtin_bitreverse32(c) >> (32 - n); }

__device__ inline Code literal_code(uint32_t b) {   // RFC 1951 3.2.6: 0..143 -> 8 bits from 0x30, 144..255 -> 9 bits from 0x190
  return b < 144 ? Code{rev(0x30u + b, 8), 8} : Code{rev(0x190u + b - 144u, 9), 9};
}

__device__ inline Code match_code(uint32_t len, uint32_t dist) {
  uint32_t sym, eb = 0, ev = 0;
  if (len <= 10) {
    sym = 254 + len;
  } else if (len == 258) {
    sym = 285;
  } else {
    const uint32_t v = len - 3;
    eb = 31 - __builtin_clz(v) - 2;
    sym = 257 + 4 * (eb + 1) + ((v >> eb) & 3u);
    ev = v & ((1u << eb) - 1);
  }
  Code c = sym < 280 ? Code{rev(sym - 256, 7), 7} : Code{rev(sym - 280 + 0xC0u, 8), 8};
  c.v |= ev << c.n;   // extra bits: LSB first, not reversed
  c.n += eb;
  const uint32_t v = dist - 1;
  uint32_t dsym = v, deb = 0, dev = 0;
  if (v >= 4) {
    deb = 31 - __builtin_clz(v) - 1;
    dsym = 2 * deb + 2 + ((v >> deb) & 1u);
    dev = v & ((1u << deb) - 1);
  }
  c.v |= rev(dsym, 5) << c.n;
  c.n += 5;
  c.v |= dev << c.n;
  c.n += deb;
  return c;
}

// the greedy parse of [s0, e): sink(Code) per token
template <typename Sink>
__device__ inline void walk(const uint32_t *d, const uint16_t *cand, uint32_t s0, uint32_t e, Sink &sink) {
  uint32_t p = s0;
  while (p < e) {
    const uint32_t dist = cand[p];
    uint32_t L = 0;
    if (dist) L = match_len(d, p, p - dist, min(258u, e - p));
    if (L >= 3) {
      sink(match_code(L, dist));
      p += L;
    } else {
      sink(literal_code(byte_at(d, p)));
      p++;
    }
  }
}

struct BitCount {
  uint32_t bits = 0;
  __device__ void operator()(Code c) { bits += c.n; }
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
  __syncthreads();

  // ---- parse (bit count) + CRC of this thread's range ----
  const uint32_t s0 = min(t * BG_SEG, len), e = min(s0 + BG_SEG, len);
  const uint32_t last_t = (len - 1) / BG_SEG;
  BitCount counter;
  walk(data, cand, s0, e, counter);
  const uint32_t my_bits = counter.bits + (t == 0 ? 3u : 0u) + (t == last_t ? 7u : 0u);
  uint32_t crc = 0xffffffffu;
  for (uint32_t p = s0; p < e; p++) crc = crc_tab[(crc ^ byte_at(data, p)) & 0xffu] ^ (crc >> 8);
  crc = e > s0 ? multmodp(x8nmodp(len - e), ~crc) : 0u;

  // ---- place: exclusive scan of the bit counts, XOR of the CRC parts ----
  uint32_t x = my_bits;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += y;
  }
  for (int o = 32; o >= 1; o >>= 1) crc ^= __shfl_xor(crc, o, 64);
  if (lane == 63) misc[wave] = x;
  if (lane == 0) misc[4 + wave] = crc;
  __syncthreads();
  uint32_t bit0 = x - my_bits, total_bits = 0, member_crc = 0;
  for (uint32_t k = 0; k < 4; k++) {
    if (k < wave) bit0 += misc[k];
    total_bits += misc[k];
    member_crc ^= misc[4 + k];
  }
  const uint32_t fixed_bytes = (total_bits + 7) / 8, stored_bytes = len + 5;
  const bool stored = fixed_bytes > stored_bytes;
  const uint32_t deflate_bytes = stored ? stored_bytes : fixed_bytes;

  // ---- emit ----
  if (!stored) {
    const uint32_t first = BG_HEADER * 8 + bit0, end = first + my_bits;
    if (my_bits) {   // the words this thread shares with a neighbour start at zero
      if (first & 31u) slot32[first >> 5] = 0;
      if (end & 31u) slot32[end >> 5] = 0;
    }
    __syncthreads();
    if (my_bits) {
      BitWriter out(slot32, first);
      if (t == 0) out(Code{3u, 3});   // BFINAL = 1, BTYPE = 01
      walk(data, cand, s0, e, out);
      if (t == last_t) out(Code{0u, 7});   // end of block: symbol 256, seven 0 bits
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

void bgzf_compress_device(const char *d_in, uint64_t n, BgzfWork &W, DevBuf &out, uint64_t *out_len, hipStream_t s) {
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
    hipLaunchKernelGGL(k_bgzf_member, dim3(g), dim3(BG_THREADS), 0, s, (const uint8_t *)d_in, n, m0, W.cand.as<uint16_t>(),
                       W.slots.as<uint8_t>(), W.sizes.as<uint32_t>());
    exclusive_scan_u32_to_u64(W.sizes.as<uint32_t>(), W.offs.as<uint64_t>(), g, totals, W.scan_tmp.p, s);
    hipLaunchKernelGGL(k_bgzf_gather, dim3(g), dim3(256), 0, s, W.slots.as<const uint8_t>(), W.sizes.as<const uint32_t>(),
                       W.offs.as<const uint64_t>(), totals + 1, out.as<uint8_t>());
    hipLaunchKernelGGL(k_bgzf_advance, dim3(1), dim3(64), 0, s, totals);
    HIPCHK(hipGetLastError());
  }
  read_back(out_len, totals + 1, sizeof(uint64_t), s);
}

}  // namespace kslam
