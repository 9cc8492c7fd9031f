// gunzip.hip -- plain gzip (RFC 1952, any number of members) inflated on the device (include/kslam_gunzip.h).  inflate.hip
// reads BGZF, whose members the host finds from their headers; here nobody knows where a block begins, so the starts are
// guessed, proven and only then decoded -- the scheme pugz and rapidgzip use on CPU threads, with a wavefront where they have
// a thread.  The bit reader, the code tables and the decoder are inflate.hip's (inflate_core.h), with its fence and its rule
// that nothing trusts the bytes.
//
//   k_gunzip_find     one wave per chunk.  Lanes test 64 consecutive bit offsets at a time: first the 17 header bits (BFINAL 0,
//                     BTYPE 2, HLIT, HDIST <= 29: one offset in nine passes), then, still per lane, the Kraft sum of the code-length
//                     code (it must be complete: about one in a hundred of those).  What is left is taken in order by the WHOLE
//                     wave through read_dynamic_lengths and two build_code -- the finder's rule in full -- and the first offset
//                     that passes is the chunk's start.
//   k_gunzip_count    one wave per start: gz_walk<false> decodes lengths only, and at every block start looks whether it stands
//                     on a later start.  It crosses member ends (trailer, zero bytes, the next header) on its own.
//   k_gunzip_decode   one wave per live start: gz_walk<true>, the same walk, storing 16-bit symbols.  A symbol is a literal, or
//                     0x8000 | (k - 1) for the byte k before the wave's first output byte; matches copy symbols, markers included.
//   k_gunzip_window   ONE workgroup, the only serial part: for each live stretch in order, its last 32 768 symbols to text.
//                     A marker of stretch j points into the 32 KiB before it, which are tails of the stretches before (or the
//                     text of the round before), final by then.
//   k_gunzip_resolve  every symbol outside the tails to text, 16 per thread, one 16-byte store where a group is whole.
//   k_gunzip_crc      CRC-32 of every member's part in the round, in pieces of 64 KiB moved to their place (crc32.h).
//
// A wave on a false start decodes garbage.  That is harmless: the count pass stores nothing but its own link, every
// position is checked against the end of the file before it is used, and the host only follows links from the file's true
// first block (host/gunzip.cpp), which never lead to a false start's link.
#include "gunzip.h"

#include <algorithm>

#include "crc32.h"
#include "gzip_header.h"
#include "inflate_core.h"

namespace kslam {
namespace {

using kslam_host::GunzipLink;

constexpr uint32_t GZ_THREADS = GUNZIP_WAVES * 64;
constexpr uint32_t WINDOW_THREADS = 1024;

__device__ __forceinline__ uint64_t uni64(uint64_t x) { return (uint64_t)uni((uint32_t)x) | ((uint64_t)uni((uint32_t)(x >> 32)) << 32); }

// ---- stage 1 ----
__global__ __launch_bounds__(GZ_THREADS) void k_gunzip_find(const uint8_t *__restrict__ in, uint64_t len, uint64_t chunk, uint64_t n_chunks,
                                                            unsigned long long *found) {
  __shared__ WaveLds lds[GUNZIP_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t k = 1ull + (uint64_t)blockIdx.x * GUNZIP_WAVES + wave;
  if (k >= n_chunks) return;
  WaveLds &L = lds[wave];
  const uint64_t c0 = k * chunk;   // < len, a multiple of 4
  const uint32_t end = (uint32_t)min(len - c0, GUNZIP_SPAN_BYTES), end_bit = end * 8u, wend = (end + 3u) >> 2;
  const uint32_t n_bits = (uint32_t)min(chunk, len - c0) * 8u;   // chunk <= 2^28
  const uint32_t *words = reinterpret_cast<const uint32_t *>(in + c0);
  uint32_t hit = 0xffffffffu;
  for (uint32_t b = 0; b < n_bits && hit == 0xffffffffu; b += 64) {
    const uint32_t p = b + lane;
    bool cand = false;
    if (p < n_bits) {
      const uint32_t w = p >> 5, sh = p & 31u;
      const uint64_t lo = (uint64_t)(w < wend ? words[w] : 0u) | ((uint64_t)(w + 1 < wend ? words[w + 1] : 0u) << 32);
      const uint64_t hi = (uint64_t)(w + 2 < wend ? words[w + 2] : 0u) | ((uint64_t)(w + 3 < wend ? words[w + 3] : 0u) << 32);
      const uint64_t v = sh ? (lo >> sh) | (hi << (64u - sh)) : lo, vh = hi >> sh;
      const uint32_t h = (uint32_t)v & 0x1ffffu;
      const uint32_t hclen = ((h >> 13) & 15u) + 4u;
      if ((h & 7u) == 4u && ((h >> 3) & 31u) <= 29u && ((h >> 8) & 31u) <= 29u && p + 17u + 3u * hclen <= end_bit) {
        const uint64_t r = (v >> 17) | (vh << 47);   // the 3-bit lengths of the code-length code
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < N_CL; i++) {
          const uint32_t l = (uint32_t)(r >> (3u * i)) & 7u;
          if (i < hclen && l) sum += 128u >> l;
        }
        cand = sum == 128u;   // complete: what build_code(is_cl) asks (no code at all fails at the first length)
      }
    }
    for (uint64_t m = __ballot(cand); m; m &= m - 1) {   // the survivors in order, each by the whole wave
      const uint32_t pc = b + (uint32_t)__builtin_ctzll(m);
      BitReader br{words, lane};
      br.end = end;
      br.start(pc >> 3);
      br.drop(pc & 7u);
      br.refill();
      br.drop(3);
      uint32_t n_ll = 0, n_d = 0;
      uint32_t err = read_dynamic_lengths(br, L, end_bit, lane, &n_ll, &n_d);
      if (!err) err = build_code(L.lens, n_ll, L.cnt_ll, L.sorted_ll, L.fast_ll, LL_ROOT, false, lane);
      if (!err) err = build_code(L.lens + n_ll, n_d, L.cnt_d, L.sorted_d, L.fast_d, D_ROOT, false, lane);
      if (!err) {
        hit = pc;
        break;
      }
    }
  }
  if (lane == 0) found[k] = hit == 0xffffffffu ? GUNZIP_NO_START : c0 * 8ull + hit;
}

// ---- stages 2 and 3: the walk from a block start ----
struct Walk {
  uint32_t status = kslam_host::GZL_NONE, next = 0, need_back = 0;
  uint64_t out = 0, members = 0, member_at = 0, member_out = 0;
};
struct WalkIn {
  uint64_t start_bit;
  // count
  const uint64_t *starts;
  uint32_t n_starts, self;
  uint64_t budget_bits;
  // decode
  uint64_t stop_bit, cap, n_member_slots, out_abs;
  uint16_t *sym;
  GunzipMemberEnd *member_ends;
};

// From the block header at A.start_bit to a later start, the end of the file, or the first violation (returned: an
// InflateError or a GunzipKind; 0 with W.status set otherwise).  Positions are 32-bit, relative to `base`.
template <bool DECODE> __device__ __forceinline__ uint32_t gz_walk(const uint8_t *__restrict__ in, uint64_t len, const WalkIn &A, Walk &W, WaveLds &L, uint32_t lane) {
  const uint64_t base = (A.start_bit >> 3) & ~3ull;
  const uint8_t *bin = in + base;
  const uint32_t end = (uint32_t)min(len - base, GUNZIP_SPAN_BYTES), end_bit = end * 8u;
  const uint32_t rel_bit = (uint32_t)(A.start_bit - base * 8ull);
  BitReader br{reinterpret_cast<const uint32_t *>(bin), lane};
  br.end = end;
  br.start(rel_bit >> 3);
  br.drop(rel_bit & 7u);
  uint64_t outpos = 0;           // symbols produced, the waiting literals included
  uint32_t pend = 0, npend = 0;  // literals waiting for their store: lane k holds symbol outpos - npend + k
  bool fixed_ready = false, first_member = true;
  uint32_t j = A.self + 1;
  auto flush = [&] {
    if (DECODE && lane < npend) A.sym[outpos - npend + lane] = (uint16_t)pend;
    npend = 0;
  };
  for (;;) {
    // ---- a block start: is it a start someone else decodes from? ----
    const uint64_t cur = base * 8ull + br.bit_pos();
    if (DECODE) {
      if (cur == A.stop_bit) {
        W.status = kslam_host::GZL_HIT;
        break;
      }
      if (cur > A.stop_bit) return INF_DATA_LENGTH;   // (not what the count pass saw)
    } else {
      while (j < A.n_starts && uni64(A.starts[j]) < cur) j++;   // starts it has passed are skipped
      if (j < A.n_starts && uni64(A.starts[j]) == cur) {
        W.status = kslam_host::GZL_HIT;
        W.next = j;
        break;
      }
      if (A.budget_bits && (uint64_t)(br.bit_pos() - rel_bit) > A.budget_bits) {
        W.status = kslam_host::GZL_ABANDONED;
        break;
      }
    }
    br.refill();
    const bool last = br.bits(1) != 0;
    const uint32_t type = br.bits(2);
    if (br.bit_pos() > end_bit) return INF_DATA_LENGTH;
    if (type == 3u) return INF_BAD_BLOCK_TYPE;
    if (type == 0u) {   // stored: to the byte boundary, LEN, ~LEN, the bytes
      br.drop(br.n & 7u);
      br.refill();
      const uint32_t slen = br.bits(16), nlen = br.bits(16);
      if (br.bit_pos() > end_bit) return INF_DATA_LENGTH;
      if ((slen ^ nlen) != 0xffffu) return INF_STORED_LENGTH;
      const uint32_t src = br.bit_pos() >> 3;
      if (src + slen > end) return INF_DATA_LENGTH;
      if (DECODE) {
        if (outpos + slen > A.cap) return INF_OUTPUT_OVERRUN;
        flush();
        for (uint32_t i = lane; i < slen; i += 64) A.sym[outpos + i] = bin[src + i];
      }
      outpos += slen;
      br.start(src + slen);
    } else {
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
          if (DECODE) {
            if (outpos >= A.cap) return INF_OUTPUT_OVERRUN;
            if (lane == npend) pend = sym;
            npend++;
          }
          outpos++;
          if (DECODE && npend == 64u) flush();
          continue;
        }
        if (sym == 256u) {
          if (br.bit_pos() > end_bit) return INF_DATA_LENGTH;
          break;
        }
        if (sym > 285u) return INF_INVALID_SYMBOL;   // 286, 287 of the fixed code, and NO_SYMBOL
        const uint32_t k = sym - 257u;
        uint32_t mlen = 258;
        if (k < 8u) {
          mlen = 3u + k;
        } else if (k < 28u) {
          const uint32_t eb = (k >> 2) - 1u;
          mlen = 3u + ((4u + (k & 3u)) << eb) + br.bits(eb);
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
        // The source may lie before this wave's first byte, but never before its member's.  Where that member began
        // before the wave did, only the host knows where: it gets the furthest reach (need_back) to judge.
        if (first_member) {
          if (dist > outpos) W.need_back = max(W.need_back, dist - (uint32_t)outpos);
        } else if (dist > outpos - W.member_out) {
          return INF_DISTANCE;
        }
        if (DECODE) {
          if (outpos + mlen > A.cap) return INF_OUTPUT_OVERRUN;
          flush();
          wave_sync();   // the sources are symbols other lanes stored: see the head of inflate.hip
          for (uint32_t i = lane; i < mlen; i += 64) {
            const int64_t p = (int64_t)outpos - (int64_t)dist + (int64_t)(dist < mlen ? i % dist : i);
            A.sym[outpos + i] = p >= 0 ? A.sym[p] : (uint16_t)(0x8000u | (uint32_t)(-p - 1));   // -p - 1 <= 32 767
          }
        }
        outpos += mlen;
      }
    }
    if (!last) continue;
    // ---- a member's end: the trailer, then zero bytes, then the end of the file or the next member's header ----
    flush();
    const uint32_t tb = (br.bit_pos() + 7u) >> 3;
    if (tb + 8u > end) return INF_DATA_LENGTH;
    if (DECODE) {
      if (W.members >= A.n_member_slots) return INF_OUTPUT_OVERRUN;
      if (lane == 0) A.member_ends[W.members] = GunzipMemberEnd{base + tb, A.out_abs + outpos};
    }
    W.members++;
    uint32_t p = tb + 8u;
    for (;;) {   // p: the first byte that is not zero, or end
      const uint32_t q = p + lane;
      const uint64_t m = __ballot(q >= end || bin[q] != 0);
      if (m) {
        p += (uint32_t)__builtin_ctzll(m);
        break;
      }
      p += 64u;
    }
    if (p >= end) {
      W.status = kslam_host::GZL_EOF;
      break;
    }
    W.member_at = base + p;
    W.member_out = outpos;
    first_member = false;
    uint64_t deflate_at = 0;
    const uint32_t herr = gzip_header_walk(bin, p, end, &deflate_at);
    if (herr) return herr == GZH_NOT_MEMBER ? (uint32_t)kslam_host::GZK_NOT_MEMBER : (uint32_t)kslam_host::GZK_HEADER;
    br.start((uint32_t)uni64(deflate_at));
  }
  flush();   // the literals of the last block
  W.out = outpos;
  return 0;
}

// A wave that ran into the end of what it can address (not the end of the file) has seen nothing wrong with the file.
__device__ uint32_t span_limit(uint64_t len, uint64_t start_bit, const Walk &W, uint32_t err) {
  const uint64_t base = (start_bit >> 3) & ~3ull;
  if (len - base <= GUNZIP_SPAN_BYTES) return err;
  const bool at_end = err == INF_DATA_LENGTH || err == kslam_host::GZK_HEADER || err == kslam_host::GZK_NOT_MEMBER || (!err && W.status == kslam_host::GZL_EOF);
  return at_end ? (uint32_t)kslam_host::GZK_SPAN : err;
}

__global__ __launch_bounds__(GZ_THREADS) void k_gunzip_count(const uint8_t *__restrict__ in, uint64_t len, const uint64_t *__restrict__ starts,
                                                             uint32_t n_starts, uint32_t first, uint32_t n_run, uint64_t budget_bits,
                                                             GunzipLink *links) {
  __shared__ WaveLds lds[GUNZIP_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w = blockIdx.x * GUNZIP_WAVES + wave;
  if (w >= n_run) return;
  const uint32_t self = first + w;
  WalkIn A{};
  A.start_bit = uni64(starts[self]);
  A.starts = starts;
  A.n_starts = n_starts;
  A.self = self;
  A.budget_bits = budget_bits;
  Walk W;
  uint32_t err = A.start_bit < len * 8ull ? gz_walk<false>(in, len, A, W, lds[wave], lane) : (uint32_t)INF_DATA_LENGTH;
  err = span_limit(len, A.start_bit, W, err);
  if (lane == 0) {
    GunzipLink l{};
    l.status = err ? (uint32_t)kslam_host::GZL_ERROR : W.status;
    l.kind = err;
    l.next = W.next;
    l.need_back = W.need_back;
    l.out_bytes = W.out;
    l.members = W.members;
    l.member_at = W.member_at;
    l.member_out = W.member_out;
    links[self] = l;
  }
}

__global__ __launch_bounds__(GZ_THREADS) void k_gunzip_decode(const uint8_t *__restrict__ in, uint64_t len, const GunzipDecodeSpan *__restrict__ spans,
                                                              uint32_t n, uint16_t *sym, GunzipMemberEnd *member_ends,
                                                              unsigned long long *first_bad) {
  __shared__ WaveLds lds[GUNZIP_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w = blockIdx.x * GUNZIP_WAVES + wave;
  if (w >= n) return;
  WalkIn A{};
  A.start_bit = uni64(spans[w].bit);
  A.stop_bit = uni64(spans[w].stop_bit);
  A.cap = uni64(spans[w].n_out);
  A.n_member_slots = uni64(spans[w].n_members);
  A.out_abs = uni64(spans[w].out);
  A.sym = sym + uni64(spans[w].sym_off);
  A.member_ends = member_ends + uni64(spans[w].member_slot);
  A.n_starts = 0;
  Walk W;
  uint32_t err = A.start_bit < len * 8ull ? gz_walk<true>(in, len, A, W, lds[wave], lane) : (uint32_t)INF_DATA_LENGTH;
  if (!err && (W.out != A.cap || W.members != A.n_member_slots)) err = INF_OUTPUT_UNDERRUN;   // the count pass said otherwise
  if (!err && (W.status == kslam_host::GZL_EOF) != (A.stop_bit == GUNZIP_NO_START)) err = INF_DATA_LENGTH;
  if (err && lane == 0) atomicMin(first_bad, ((unsigned long long)w << 8) | err);
}

// ---- stage 4 ----
// One turn per stretch.  A thread takes up to 32 symbols of the tail: all their loads first, then the loads of the bytes the
// markers point at, then the stores -- three trips to memory per turn, not one per symbol.  That order is free because a
// marker never points into the tail being written: its byte lies before the stretch's first.
__global__ __launch_bounds__(WINDOW_THREADS) void k_gunzip_window(const GunzipDecodeSpan *__restrict__ spans, uint32_t n, const uint16_t *__restrict__ sym,
                                                                  uint8_t *text) {
  constexpr uint32_t PER = GUNZIP_WINDOW / WINDOW_THREADS;
  static_assert(PER * WINDOW_THREADS == GUNZIP_WINDOW, "a turn covers the whole tail");
  for (uint32_t j = 0; j < n; j++) {
    const uint64_t s = spans[j].sym_off, len = spans[j].n_out, e = s + len;
    const uint64_t t0 = e - min(len, (uint64_t)GUNZIP_WINDOW) + threadIdx.x;
    uint32_t v[PER];
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
      const uint64_t i = t0 + (uint64_t)k * WINDOW_THREADS;
      v[k] = i < e ? sym[i] : 0u;
    }
    uint8_t b[PER];
    // a marker's byte lies at most 32 768 before s: in the tails done in earlier turns, or in the text before the round
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) b[k] = (uint8_t)(v[k] < 0x8000u ? v[k] : text[(int64_t)s - 1 - (int64_t)(v[k] & 0x7fffu)]);
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
      const uint64_t i = t0 + (uint64_t)k * WINDOW_THREADS;
      if (i < e) text[i] = b[k];
    }
    __syncthreads();   // the next stretch reads what this one stored
  }
}

// ---- stage 5 ----
__global__ __launch_bounds__(256) void k_gunzip_resolve(const GunzipDecodeSpan *__restrict__ spans, uint32_t n, const uint16_t *__restrict__ sym,
                                                        uint8_t *text, uint64_t n_text) {
  const uint64_t p0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u;
  if (p0 >= n_text) return;
  uint32_t lo = 0, hi = n - 1;   // the last stretch that begins at or before p0
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (spans[mid].sym_off <= p0) lo = mid;
    else hi = mid - 1;
  }
  uint32_t j = lo;
  uint64_t s = spans[j].sym_off, e = s + spans[j].n_out, tail = e - min(spans[j].n_out, (uint64_t)GUNZIP_WINDOW);
  union { uint4 q[2]; uint16_t v[16]; } in;   // the scratch has 64 symbols to spare behind the round
  in.q[0] = reinterpret_cast<const uint4 *>(sym + p0)[0];
  in.q[1] = reinterpret_cast<const uint4 *>(sym + p0)[1];
  union { uint4 q; uint8_t b[16]; } out;
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t i = 0; i < 16; i++) {
    const uint64_t p = p0 + i;
    out.b[i] = 0;
    if (p >= n_text) continue;
    while (p >= e && j + 1 < n) {   // (stretches without text are stepped over)
      j++;
      s = spans[j].sym_off;
      e = s + spans[j].n_out;
      tail = e - min(spans[j].n_out, (uint64_t)GUNZIP_WINDOW);
    }
    if (p >= tail) continue;   // stage 4's
    const uint32_t v = in.v[i];
    out.b[i] = (uint8_t)(v < 0x8000u ? v : text[(int64_t)s - 1 - (int64_t)(v & 0x7fffu)]);
    mine |= 1u << i;
  }
  if (mine == 0xffffu) {
    *reinterpret_cast<uint4 *>(text + p0) = out.q;
  } else {
#pragma unroll
    for (uint32_t i = 0; i < 16; i++)
      if (mine & (1u << i)) text[p0 + i] = out.b[i];
  }
}

// ---- stage 6 ----
__device__ uint32_t x8nmodp64(uint64_t n) {   // x^(8 n) mod P; x^(2^k) has period 32 in k
  uint32_t p = 0x80000000u;
  for (uint32_t k = 3; n; n >>= 1, k++)
    if (n & 1u) p = multmodp(X2N[k & 31], p);
  return p;
}

__global__ __launch_bounds__(256) void k_gunzip_crc(const uint8_t *__restrict__ text, const GunzipCrcSeg *__restrict__ segs, uint32_t *crcs) {
  __shared__ uint32_t tab[256];
  const uint32_t t = threadIdx.x;
  tab[t] = crc_table_entry(t);
  __syncthreads();
  const GunzipCrcSeg S = segs[blockIdx.x];
  const uint64_t piece0 = (uint64_t)blockIdx.y * GUNZIP_CRC_PIECE;
  if (piece0 >= S.len && blockIdx.y != 0) return;
  const uint64_t n_here = piece0 < S.len ? min((uint64_t)GUNZIP_CRC_PIECE, S.len - piece0) : 0;
  constexpr uint32_t PER = GUNZIP_CRC_PIECE / 256;
  const uint64_t a = min((uint64_t)t * PER, n_here), e = min(a + PER, n_here);
  const uint8_t *src = text + S.off + piece0;
  uint32_t crc = 0xffffffffu;
  for (uint64_t p = a; p < e; p++) crc = tab[(crc ^ src[p]) & 0xffu] ^ (crc >> 8);
  uint32_t x = e > a ? multmodp(x8nmodp64(S.len - (piece0 + e)), ~crc) : 0u;
  if (blockIdx.y == 0 && t == 0 && S.prev_crc) x ^= multmodp(x8nmodp64(S.len), S.prev_crc);   // crc(A || B) = crc(A) x^(8 |B|) ^ crc(B)
  for (int w = 32; w >= 1; w >>= 1) x ^= __shfl_xor(x, w, 64);
  if ((t & 63u) == 0 && x) atomicXor(&crcs[blockIdx.x], x);
}

}  // namespace

void gunzip_find_device(const uint8_t *d_in, uint64_t len, uint64_t chunk, uint64_t n_chunks, uint64_t *d_found, hipStream_t s) {
  if (n_chunks < 2) return;
  const uint64_t blocks = (n_chunks - 1 + GUNZIP_WAVES - 1) / GUNZIP_WAVES;
  hipLaunchKernelGGL(k_gunzip_find, dim3((uint32_t)blocks), dim3(GZ_THREADS), 0, s, d_in, len, chunk, n_chunks,
                     reinterpret_cast<unsigned long long *>(d_found));
  HIPCHK(hipGetLastError());
}

void gunzip_count_device(const uint8_t *d_in, uint64_t len, const uint64_t *d_starts, uint32_t n_starts, uint32_t first, uint32_t n_run,
                         uint64_t budget_bits, kslam_host::GunzipLink *d_links, hipStream_t s) {
  if (!n_run) return;
  hipLaunchKernelGGL(k_gunzip_count, dim3((n_run + GUNZIP_WAVES - 1) / GUNZIP_WAVES), dim3(GZ_THREADS), 0, s, d_in, len, d_starts, n_starts, first,
                     n_run, budget_bits, d_links);
  HIPCHK(hipGetLastError());
}

void gunzip_decode_device(const uint8_t *d_in, uint64_t len, const GunzipDecodeSpan *d_spans, uint32_t n, uint16_t *d_sym,
                          GunzipMemberEnd *d_members, uint64_t *d_first_bad, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_gunzip_decode, dim3((n + GUNZIP_WAVES - 1) / GUNZIP_WAVES), dim3(GZ_THREADS), 0, s, d_in, len, d_spans, n, d_sym, d_members,
                     reinterpret_cast<unsigned long long *>(d_first_bad));
  HIPCHK(hipGetLastError());
}

void gunzip_window_device(const GunzipDecodeSpan *d_spans, uint32_t n, const uint16_t *d_sym, uint8_t *d_text, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_gunzip_window, dim3(1), dim3(WINDOW_THREADS), 0, s, d_spans, n, d_sym, d_text);
  HIPCHK(hipGetLastError());
}

void gunzip_resolve_device(const GunzipDecodeSpan *d_spans, uint32_t n, const uint16_t *d_sym, uint8_t *d_text, uint64_t n_text, hipStream_t s) {
  if (!n || !n_text) return;
  const uint64_t groups = (n_text + 15) / 16;
  hipLaunchKernelGGL(k_gunzip_resolve, dim3((uint32_t)((groups + 255) / 256)), dim3(256), 0, s, d_spans, n, d_sym, d_text, n_text);
  HIPCHK(hipGetLastError());
}

void gunzip_crc_device(const uint8_t *d_text, const GunzipCrcSeg *d_segs, uint32_t n, uint64_t longest, uint32_t *d_crc, hipStream_t s) {
  if (!n) return;
  HIPCHK(hipMemsetAsync(d_crc, 0, (size_t)n * sizeof(uint32_t), s));
  const uint64_t ny = std::max<uint64_t>(1, (longest + GUNZIP_CRC_PIECE - 1) / GUNZIP_CRC_PIECE);
  if (ny > 65535) throw StatusError{KSLAM_ERR_UNSUPPORTED, "a round of more than 4 GiB of text: lower kslam_gunzip_set_round"};
  hipLaunchKernelGGL(k_gunzip_crc, dim3(n, (uint32_t)ny), dim3(256), 0, s, d_text, d_segs, d_crc);
  HIPCHK(hipGetLastError());
}

}  // namespace kslam
