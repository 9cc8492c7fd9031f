// samsink.h -- what the writers of SAM rows share on the device (samtext.hip: the rows of the alignment pairs; samunmapped.hip:
// the rows of the reads without alignment): the two sinks that make a length pass and a write pass out of one piece of code,
// numbers, and the SEQ / QUAL columns of include/kslam_samseq.h as text and as BAM fields.
#pragma once
#include "common.h"
#include "seqcodes.h"

namespace kslam {
namespace {

struct CountSink {
  uint64_t n = 0;
  __device__ void ch(uint8_t) { n++; }
  __device__ void bytes(const uint8_t *, uint64_t k) { n += k; }
  __device__ void lit(const char *, uint32_t k) { n += k; }
  __device__ void skip(uint32_t k) { n += k; }
};
// Bytes collect in a 64-bit register and leave as ONE 8-byte store (unaligned stores are fine on gfx950): a line of ~200
// bytes is ~25 store instructions instead of ~200, and neighbouring threads' lines are neighbours in memory, so the stores
// of a wave fall into a few hundred consecutive cache lines that L2 merges.
struct ByteSink {
  uint8_t *w;
  uint64_t acc = 0;
  uint32_t k = 0;   // bytes waiting in acc
  __device__ explicit ByteSink(uint8_t *at) : w(at) {}
  __device__ void ch(uint8_t c) {
    acc |= (uint64_t)c << (8 * k);
    if (++k == 8) {
      __builtin_memcpy(w, &acc, 8);
      w += 8;
      acc = 0;
      k = 0;
    }
  }
  __device__ void bytes(const uint8_t *s, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) ch(s[i]);
  }
  __device__ void lit(const char *s, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) ch((uint8_t)s[i]);
  }
  // eight bytes at once (v's low byte first): one store whatever k is; the bytes that do not fit wait in acc
  __device__ void word(uint64_t v) {
    const uint64_t out = acc | (v << (8 * k));
    __builtin_memcpy(w, &out, 8);
    w += 8;
    acc = k ? v >> (64 - 8 * k) : 0;
  }
  __device__ void flush() {
    for (uint32_t i = 0; i < k; i++) w[i] = (uint8_t)(acc >> (8 * i));
    w += k;
    acc = 0;
    k = 0;
  }
};

__device__ inline uint32_t digits_u64(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) {
    v /= 10;
    d++;
  }
  return d;
}
template <class Sink>
__device__ inline void put_num(Sink &o, uint64_t v);
template <>
__device__ inline void put_num<CountSink>(CountSink &o, uint64_t v) { o.n += digits_u64(v); }
template <>
__device__ inline void put_num<ByteSink>(ByteSink &o, uint64_t v) {
  // the digits most significant first, from a register: up to 8 digits per 64-bit word (numbers here are < 2^32: 10 digits)
  uint32_t d = 0;
  uint64_t lo = 0, hi = 0;   // digit j of the reversed number in byte j
  do {
    const uint64_t q = v / 10;
    const uint64_t c = '0' + (v - q * 10);
    if (d < 8) lo |= c << (8 * d); else hi |= c << (8 * (d - 8));
    v = q;
    d++;
  } while (v);
  for (uint32_t j = d; j-- > 0;) o.ch((uint8_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xFF));
}
template <class Sink>
__device__ inline void put_snum(Sink &o, int64_t v) {
  if (v < 0) {
    o.ch('-');
    put_num(o, (uint64_t)(-v));
  } else {
    put_num(o, (uint64_t)v);
  }
}
#define LIT(o, s) (o).lit(s, (uint32_t)(sizeof(s) - 1))

// ---- SEQ / QUAL (include/kslam_samseq.h; host/tail.cpp: put_seq_text / put_seq_bam, same bytes) ------------------------
// The three byte tables of the switch-on kernels, in LDS: filled by the block's threads before anything else.
struct SeqLut {
  uint8_t comp[256];    // kslam_seq::complement
  uint8_t code[256];    // kslam_seq::nibble
  uint8_t rcode[256];   // nibble(complement(c)): a reverse row's code straight from the read's byte
};
__device__ inline void fill_lut(SeqLut &t) {
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) {   // (one trip with the 256-thread blocks of this file)
    const uint8_t c = kslam_seq::complement((uint8_t)i);
    t.comp[i] = c;
    t.code[i] = kslam_seq::nibble((uint8_t)i);
    t.rcode[i] = kslam_seq::nibble(c);
  }
}
// the block's tables, filled and behind a barrier; nothing, and no LDS, for the switch-off kernels
template <bool SEQ>
__device__ inline const SeqLut *block_lut() {
  if constexpr (SEQ) {
    __shared__ SeqLut t;
    fill_lut(t);
    __syncthreads();
    return &t;
  } else {
    return nullptr;
  }
}
struct SeqCols {   // where a row's two columns come from; lut is nullptr in the count pass
  const uint8_t *bases = nullptr, *qual = nullptr;   // the read's, qual nullptr: the batch has no qualities
  uint32_t len = 0;
  bool rev = false;     // FLAG 0x10
  const SeqLut *lut = nullptr;
};
__device__ inline uint64_t load8(const uint8_t *p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
__device__ inline uint64_t map8(uint64_t v, const uint8_t *t) {
  uint64_t r = 0;
#pragma unroll
  for (uint32_t b = 0; b < 8; b++) r |= (uint64_t)t[(v >> (8 * b)) & 0xFF] << (8 * b);
  return r;
}
// sixteen bases (a = the first eight in output order, low byte first) -> eight bytes, high nibble first
__device__ inline uint64_t pack16(uint64_t a, uint64_t b, const uint8_t *code) {
  uint64_t r = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    r |= (uint64_t)(code[(a >> (16 * j)) & 0xFF] << 4 | code[(a >> (16 * j + 8)) & 0xFF]) << (8 * j);
    r |= (uint64_t)(code[(b >> (16 * j)) & 0xFF] << 4 | code[(b >> (16 * j + 8)) & 0xFF]) << (8 * j + 32);
  }
  return r;
}
// s[0 .. n) forward, or from the end; t: a table every byte goes through (nullptr: none)
__device__ inline void copy_bytes(ByteSink &o, const uint8_t *s, uint32_t n, bool rev, const uint8_t *t) {
  const uint32_t nw = n >> 3, tail = n & 7;
  if (!rev) {
    for (uint32_t i = 0; i < nw; i++) o.word(load8(s + 8 * i));
    for (uint32_t j = 0; j < tail; j++) o.ch(s[8 * nw + j]);
  } else {
    for (uint32_t i = 0; i < nw; i++) {
      const uint64_t v = __builtin_bswap64(load8(s + n - 8 * (i + 1)));
      o.word(t ? map8(v, t) : v);
    }
    for (uint32_t j = tail; j-- > 0;) o.ch(t ? t[s[j]] : s[j]);
  }
}
// columns 10 and 11 of a line, without the tab in front
template <class Sink>
__device__ inline void put_seq_text(Sink &o, const SeqCols &c);
template <>
__device__ inline void put_seq_text<CountSink>(CountSink &o, const SeqCols &c) {
  o.n += c.len ? (c.qual ? 2ull * c.len + 1 : c.len + 2ull) : 3;
}
template <>
__device__ inline void put_seq_text<ByteSink>(ByteSink &o, const SeqCols &c) {
  if (!c.len) {   // a read without bases
    LIT(o, "*\t*");
    return;
  }
  copy_bytes(o, c.bases, c.len, c.rev, c.lut->comp);
  o.ch('\t');
  if (c.qual) copy_bytes(o, c.qual, c.len, c.rev, nullptr); else o.ch('*');
}
// seq and qual of a record
template <class Sink>
__device__ inline void put_seq_bam(Sink &o, const SeqCols &c);
template <>
__device__ inline void put_seq_bam<CountSink>(CountSink &o, const SeqCols &c) { o.n += (c.len + 1) / 2 + (uint64_t)c.len; }
template <>
__device__ inline void put_seq_bam<ByteSink>(ByteSink &o, const SeqCols &c) {
  const uint32_t n = c.len, n16 = n >> 4;
  const uint8_t *s = c.bases, *code = c.rev ? c.lut->rcode : c.lut->code;
  for (uint32_t i = 0; i < n16; i++) {
    uint64_t a, b;
    if (!c.rev) {
      a = load8(s + 16 * i);
      b = load8(s + 16 * i + 8);
    } else {
      a = __builtin_bswap64(load8(s + n - 16 * i - 8));
      b = __builtin_bswap64(load8(s + n - 16 * i - 16));
    }
    o.word(pack16(a, b, code));
  }
  for (uint32_t j = 16 * n16; j < n; j += 2) {   // the last nibble of an odd length is 0
    const uint32_t hi = code[c.rev ? s[n - 1 - j] : s[j]];
    const uint32_t lo = j + 1 < n ? code[c.rev ? s[n - 2 - j] : s[j + 1]] : 0u;
    o.ch((uint8_t)(hi << 4 | lo));
  }
  const uint32_t nw = n >> 3;
  if (!c.qual) {   // no qualities: 0xFF
    for (uint32_t i = 0; i < nw; i++) o.word(~0ull);
    for (uint32_t j = 8 * nw; j < n; j++) o.ch(0xFF);
    return;
  }
  // quality - 33 on eight bytes, borrows kept inside each byte
  const uint64_t H = 0x8080808080808080ull, Y = 0x2121212121212121ull;
  for (uint32_t i = 0; i < nw; i++) {
    const uint64_t x = c.rev ? __builtin_bswap64(load8(c.qual + n - 8 * (i + 1))) : load8(c.qual + 8 * i);
    o.word(((x | H) - Y) ^ ((x ^ ~Y) & H));
  }
  for (uint32_t j = 8 * nw; j < n; j++) o.ch((uint8_t)((c.rev ? c.qual[n - 1 - j] : c.qual[j]) - 33));
}

// little-endian integers of a BAM record
template <class Sink>
__device__ inline void put_le(Sink &o, uint32_t v, uint32_t k) {
  for (uint32_t i = 0; i < k; i++) o.ch((uint8_t)(v >> (8 * i)));
}

}  // namespace
}  // namespace kslam
