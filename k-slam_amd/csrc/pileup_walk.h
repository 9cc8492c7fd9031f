// pileup_walk.h -- the ONE walk of an overlap record for the pile-up reports (variants.hip, consensus.hip, depth.hip; alignqc.hip
// takes the record frame and the fit check and keeps its wave-cooperative column loop).
//
// A listed record is first checked whole (record_frame): entry / cigar_len / ref_begin, then its read and its slice of the CIGAR
// pool, then every M, I and D run of its CIGAR against the read's and the entry's length.  Only a record that held is walked
// (walk_record): ONE loop over 16-column chunks of its M runs, one unaligned 16-byte load per chunk and stream, the alphabet
// looked at only on the columns that differ; D runs and I runs are handed over on the way from one M run to the next.  What is
// emitted, and under which key, is the sink's business.
//
// Bounds -- stated here once, for every file that walks through this header:
//   * Nothing is handed to a sink before the whole CIGAR held: entry < n_entries, read < n_reads, the CIGAR slice inside the
//     pool, and every M run inside the read and the entry, every I run inside the read, every D run inside the entry.  So every
//     rp + j a sink sees lies inside the entry and every qp + j inside the read.
//   * A chunk's 16-byte load may run up to 15 bytes past the last base of the read or the entry -- at the arrays' end past the
//     arrays themselves, inside the slack every DevBuf has.  Those bytes are masked out (j < nn) before anything is compared.
//   * A reverse-strand chunk is the 16 bytes ENDING at a read index; for the batch's first read that load would begin before the
//     array (first < 0), so it is done bytewise from index 0 on.
//   * A sink without columns (Sink::COLUMNS == false) makes the walk touch neither in.rbases nor in.gbases: they may be null.
#pragma once
#include "common.h"

namespace kslam {

struct __attribute__((packed, aligned(1))) Bytes16 {
  uint32_t w[4];
};
__device__ inline uint32_t byte_of(const Bytes16 &v, uint32_t j) { return (v.w[j >> 2] >> (8 * (j & 3))) & 0xFFu; }

// complement of reverseComplement: A<->T, C<->G, upper case only
__device__ inline uint32_t complement(uint32_t c) {
  const uint32_t at = (c == 'A' || c == 'T') ? (uint32_t)('A' ^ 'T') : 0u;
  const uint32_t cg = (c == 'C' || c == 'G') ? (uint32_t)('C' ^ 'G') : 0u;
  return c ^ at ^ cg;
}
// A 0, C 1, G 2, T 3 (upper case), anything else 4
__device__ inline uint32_t acgt(uint32_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }

// the first i in [lo, hi) with a[i * STRIDE] >= v (hi when there is none)
template <int STRIDE = 1>
__device__ inline uint64_t lower_bound(const uint64_t *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t v) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a[mid * STRIDE] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct RecordFrame {              // where a record that held lies
  uint64_t rb, gb;                // its read's first byte in in.rbases, its entry's in in.gbases
  int64_t L, ref_len, q0;         // the read's and the entry's length; the first query position (query_begin, not below 0)
  const uint32_t *__restrict__ cig;   // its CIGAR words
};

// false: the record is skipped.  (The *_add entries refuse a read or a CIGAR slice outside the arrays before anything is
// launched, and a lane's records do not have them.)
__device__ inline bool record_frame(const kslam_overlap &o, const VariantInputs &in, RecordFrame &f) {
  if (o.entry >= in.n_entries || o.cigar_len == 0 || o.ref_begin < 0) return false;
  if (o.read >= in.n_reads || o.cigar_off > in.n_cig || o.cigar_len > in.n_cig - o.cigar_off) return false;
  f.rb = in.roff[o.read];
  f.L = (int64_t)(in.roff[o.read + 1] - f.rb);
  f.gb = in.goff[o.entry];
  f.ref_len = (int64_t)(in.goff[o.entry + 1] - f.gb);
  f.cig = in.pool + o.cigar_off;
  f.q0 = o.query_begin > 0 ? o.query_begin : 0;
  // the whole CIGAR against the read and the entry, before anything is emitted
  int64_t rp = o.ref_begin, qp = f.q0;
  for (uint32_t k = 0; k < o.cigar_len; k++) {
    const uint32_t c = f.cig[k], op = c & 15u;
    const int64_t len = c >> 4;
    if (op == 0) {
      if (rp + len > f.ref_len || qp + len > f.L) return false;
      rp += len;
      qp += len;
    } else if (op == 1) {
      if (qp + len > f.L) return false;
      qp += len;
    } else if (op == 2) {
      if (rp + len > f.ref_len) return false;
      rp += len;
    }
  }
  return true;
}

// the oriented bases of the I run at query positions qp .. qp + len - 1 (inside the read: the fit check covered them), bytewise,
// at 2 bits each, the first one highest; false: one of them is not ACGT.  len <= 32.  (consensus.hip, indels.hip)
__device__ inline bool insertion_bases(const kslam_overlap &o, const VariantInputs &in, const RecordFrame &f, int64_t qp, uint32_t len, uint64_t *bases) {
  uint64_t w = 0;
  bool ok = true;
  for (uint32_t j = 0; j < len; j++) {
    const int64_t q = qp + (int64_t)j;
    const uint32_t b = o.revcomp ? complement(in.rbases[f.rb + (uint64_t)(f.L - 1 - q)]) : (uint32_t)in.rbases[f.rb + (uint64_t)q];
    const uint32_t code = acgt(b);
    ok = ok && code < 4u;
    w = (w << 2) | (code & 3u);
  }
  *bases = w;
  return ok;
}

// Walks a record into `sink`; false: the record is skipped (nothing was handed to the sink).  rp and qp are positions in the
// entry and in the oriented query; the sink forms its keys from them and the frame.  Runs of length 0 are not handed over.
//   sink.m_run(o, f, rp, len), sink.d_run(o, f, rp, len)      an M run, a D run
//   Sink::INSERTIONS: sink.i_run(o, in, f, rp, qp, len)       an I run, at query positions qp .. qp + len - 1
//   Sink::COLUMNS:    sink.column(g, q, r, rc)                a column of an M run whose oriented query byte q differs from the
//                                                            entry's byte r; g = f.gb + its position in the entry
template <class Sink>
__device__ inline bool walk_record(const kslam_overlap &o, const VariantInputs &in, Sink &sink) {
  RecordFrame f;
  if (!record_frame(o, in, f)) return false;
  const bool rc = o.revcomp != 0;
  int64_t rp = o.ref_begin, qp = f.q0;
  uint32_t k = 0, m_len = 0, i0 = 0;
  for (;;) {
    if (i0 >= m_len) {   // the M run is used up: operations until the next one (I and D on the way)
      bool got = false;
      while (k < o.cigar_len) {
        const uint32_t c = f.cig[k], len = c >> 4, op = c & 15u;
        k++;
        if (op == 0) {
          if (len) {
            sink.m_run(o, f, rp, len);
            if constexpr (Sink::COLUMNS) {
              m_len = len;
              i0 = 0;
              got = true;
              break;
            }
          }
          if constexpr (!Sink::COLUMNS) {
            rp += len;
            qp += len;
          }
        } else if (op == 1) {
          if constexpr (Sink::INSERTIONS)
            if (len) sink.i_run(o, in, f, rp, qp, len);
          qp += len;
        } else if (op == 2) {
          if (len) sink.d_run(o, f, rp, len);
          rp += len;
        }
      }
      if (!got) break;
    }
    if constexpr (Sink::COLUMNS) {
      const uint8_t *__restrict__ ref = in.gbases + f.gb;
      const uint32_t nn = min(16u, m_len - i0);
      const Bytes16 R = *reinterpret_cast<const Bytes16 *>(ref + rp + i0);
      // forward: the bytes from query position qp + i0 on; reverse: the 16 bytes ENDING at read index L - 1 - qp - i0, back to front
      const int64_t first = rc ? (int64_t)f.rb + (f.L - 1 - qp) - (int64_t)i0 - 15 : (int64_t)f.rb + qp + (int64_t)i0;
      Bytes16 B;
      if (first >= 0) {
        B = *reinterpret_cast<const Bytes16 *>(in.rbases + first);
      } else {   // (reverse strand at the very start of the batch's first read: stay inside the array)
#pragma unroll
        for (int x = 0; x < 4; x++) B.w[x] = 0;
        for (int j = 0; j < 16; j++)
          if (first + j >= 0) B.w[j >> 2] |= (uint32_t)in.rbases[first + j] << (8 * (j & 3));
      }
      if (rc) {   // byte j of the chunk is byte 15 - j of what was loaded
        const uint32_t b0 = __builtin_bswap32(B.w[3]), b1 = __builtin_bswap32(B.w[2]), b2 = __builtin_bswap32(B.w[1]), b3 = __builtin_bswap32(B.w[0]);
        B.w[0] = b0; B.w[1] = b1; B.w[2] = b2; B.w[3] = b3;
      }
      // the columns that differ, without a branch; the alphabet is looked at once per difference
      uint32_t miss = 0;
#pragma unroll
      for (uint32_t j = 0; j < 16; j++) {
        const uint32_t b = byte_of(B, j), q = rc ? complement(b) : b;
        miss |= (j < nn && byte_of(R, j) != q ? 1u : 0u) << j;
      }
      while (miss) {
        const uint32_t j = (uint32_t)__builtin_ctz(miss);
        miss &= miss - 1;
        const uint32_t b = byte_of(B, j);
        sink.column(f.gb + (uint64_t)rp + i0 + j, rc ? complement(b) : b, byte_of(R, j), rc);
      }
      i0 += 16;
      if (i0 >= m_len) {   // the run is done
        rp += m_len;
        qp += m_len;
      }
    }
  }
  return true;
}

}  // namespace kslam
