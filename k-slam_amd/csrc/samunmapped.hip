// samunmapped.hip -- the rows of a batch's reads without alignment, written on the GPU (include/kslam_samunmapped.h).
//
// When the SAM stage of a batch has its plan (samtext.hip: k_sam_plan), everything these rows need lies in device memory: the
// gathered id, base and quality columns (fastq_index.hip), the final read pairs and the per-group plan.  So:
//   1. k_su_flags     one thread per read pair of the result: has_row[r1_read] = 1 when its plan reports a row
//                     (the shape of readsplit.hip's k_rs_flags, keyed on SamPlan.n_rows);
//   2. k_su_lengths   one thread per record of the batch: 0 for a record with rows, else the bytes of its one or two rows; for BAM
//                     the lowest read whose id a record cannot hold; the number of rows;
//   3. an exclusive scan (scan.hip): where every record's rows go; the total, the refusal and the row count in ONE read-back;
//   4. k_su_write     the same code through the storing sink, directly behind the batch's mapped rows.
// Lengths and write run ONE function (put_rows) through CountSink / ByteSink (samsink.h), so they cannot disagree.  A text
// row is a copy of the id, the bases and the qualities around 20 fixed bytes: all three spans go through ByteSink::word, eight
// bytes per store.  BAM rows pack their bases with samtext.hip's put_seq_bam.  (host/samunmapped.cpp: the same bytes.)
#include "common.h"
#include "samtext.h"
#include "samsink.h"

namespace kslam {

namespace {

// s[0 .. n) as it stands
template <class Sink>
__device__ inline void put_span(Sink &o, const uint8_t *s, uint64_t n);
template <>
__device__ inline void put_span<CountSink>(CountSink &o, const uint8_t *, uint64_t n) { o.n += n; }
template <>
__device__ inline void put_span<ByteSink>(ByteSink &o, const uint8_t *s, uint64_t n) { copy_bytes(o, s, (uint32_t)n, false, nullptr); }

// one read's row.  0x10 is never set: SEQ and QUAL as the FASTQ record has them (include/kslam_samseq.h)
template <bool BAM, bool SEQ, class Sink>
__device__ inline void put_row(Sink &o, const SamInputs &in, const SamSeq &sq, uint32_t read, uint32_t flag, const SeqLut *lut) {
  const uint8_t *id = in.ids + in.ids_off[read];
  const uint64_t id_len = in.ids_off[read + 1] - in.ids_off[read];
  SeqCols c;
  if (SEQ) {
    const uint64_t at = in.read_off[read];
    c.len = (uint32_t)(in.read_off[read + 1] - at);
    c.bases = sq.bases + at;
    c.qual = sq.qual ? sq.qual + at : nullptr;
    c.lut = lut;
  }
  if (BAM) {
    put_le(o, 32u + (uint32_t)id_len + 1u + (c.len + 1) / 2 + c.len, 4);   // block_size
    put_le(o, 0xFFFFFFFFu, 4);              // refID
    put_le(o, 0xFFFFFFFFu, 4);              // pos
    put_le(o, (uint32_t)id_len + 1, 1);     // l_read_name
    put_le(o, 0, 1);                        // mapq
    put_le(o, 4680, 2);                     // bin: htslib's reg2bin(-1, 0)
    put_le(o, 0, 2);                        // n_cigar_op
    put_le(o, flag, 2);
    put_le(o, c.len, 4);                    // l_seq
    put_le(o, 0xFFFFFFFFu, 4);              // next_refID
    put_le(o, 0xFFFFFFFFu, 4);              // next_pos
    put_le(o, 0, 4);                        // tlen
    put_span(o, id, id_len);
    o.ch(0);
    if (SEQ) put_seq_bam(o, c);
    return;
  }
  put_span(o, id, id_len);
  o.ch('\t');
  put_num(o, flag);
  LIT(o, "\t*\t0\t0\t*\t*\t0\t0\t");
  if (SEQ && c.len) {
    put_span(o, c.bases, c.len);
    o.ch('\t');
    if (c.qual) put_span(o, c.qual, c.len); else o.ch('*');
  } else {
    LIT(o, "*\t*");
  }
  o.ch('\n');
}

// record p's rows: R1 then R2 ([R1 block | R2 block]: the mate of p is p + n_pairs), or the one row of a single-end read
template <bool BAM, bool SEQ, class Sink>
__device__ inline void put_rows(Sink &o, const SamInputs &in, const SamSeq &sq, uint64_t p, uint64_t n_pairs, bool paired, const SeqLut *lut) {
  if (!paired) {
    put_row<BAM, SEQ>(o, in, sq, (uint32_t)p, 4u, lut);
    return;
  }
  put_row<BAM, SEQ>(o, in, sq, (uint32_t)p, 77u, lut);                // 0x1 | 0x4 | 0x8 | 0x40
  put_row<BAM, SEQ>(o, in, sq, (uint32_t)(p + n_pairs), 141u, lut);   // 0x1 | 0x4 | 0x8 | 0x80
}

__global__ __launch_bounds__(256) void k_su_flags(const kslam_read_pair *__restrict__ groups, const SamPlan *__restrict__ plan,
                                                  uint64_t n_groups, uint64_t n_pairs, uint8_t *__restrict__ has_row) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t r1 = groups[g].r1_read;
  if (plan[g].n_rows && r1 < n_pairs) has_row[r1] = 1;
}

// bad_read (initially 0xFFFFFFFF): as in k_sam_lengths; n_rows: the rows of the whole batch
template <bool BAM, bool SEQ>
__global__ __launch_bounds__(256) void k_su_lengths(const uint8_t *__restrict__ has_row, uint64_t n_pairs, int paired, SamInputs in, SamSeq sq,
                                                    uint32_t *__restrict__ len, uint32_t *__restrict__ bad_read,
                                                    unsigned long long *__restrict__ n_rows) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool rowless = p < n_pairs && !has_row[p];
  if (p < n_pairs) {
    CountSink o;
    if (rowless) {
      if (BAM) {
        if (in.ids_off[p + 1] - in.ids_off[p] > 254) atomicMin(bad_read, (uint32_t)p);
        if (paired && in.ids_off[p + n_pairs + 1] - in.ids_off[p + n_pairs] > 254) atomicMin(bad_read, (uint32_t)(p + n_pairs));
      }
      put_rows<BAM, SEQ>(o, in, sq, p, n_pairs, paired != 0, nullptr);
    }
    len[p] = (uint32_t)o.n;
  }
  const uint64_t m = __ballot(rowless);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_rows, (unsigned long long)__popcll(m) * (paired ? 2u : 1u));
}

template <bool BAM, bool SEQ>
__global__ __launch_bounds__(256) void k_su_write(const uint8_t *__restrict__ has_row, uint64_t n_pairs, int paired, SamInputs in, SamSeq sq,
                                                  const uint64_t *__restrict__ off, uint8_t *__restrict__ out) {
  const SeqLut *lut = block_lut<BAM && SEQ>();   // put_seq_bam's code table (before any thread leaves: it holds a barrier)
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs || has_row[p]) return;
  ByteSink o(out + off[p]);
  put_rows<BAM, SEQ>(o, in, sq, p, n_pairs, paired != 0, lut);
  o.flush();
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void sam_unmapped_plan(const kslam_read_pair *d_groups, const SamPlan *d_plan, uint64_t n_groups, uint64_t n_pairs, bool paired,
                       const SamInputs &in, bool bam, const SamSeq *seq, SamUnmappedWork &U, uint64_t *bytes, uint32_t *bad_read,
                       hipStream_t s) {
  *bytes = 0;
  *bad_read = 0xFFFFFFFFu;
  U.kernel_ms = 0;
  U.bytes = U.n_rows = 0;
  U.write_pending = false;
  if (n_pairs >= (1ull << 31)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^31 or more records in one batch"};
  if (!n_pairs) return;
  if (!U.ev[0])
    for (auto &e : U.ev) HIPCHK(hipEventCreate(&e));
  U.has_row.ensure(n_pairs + 16);
  U.len.ensure((n_pairs + 1) * sizeof(uint32_t));
  U.off.ensure((n_pairs + 1) * sizeof(uint64_t));
  U.scan_tmp.ensure(scan_tmp_bytes(n_pairs));
  U.totals.ensure(4 * sizeof(uint64_t));
  uint64_t *tot = U.totals.as<uint64_t>();   // [0] the bytes, [1] the rows, [2] low half: the BAM refusal
  uint32_t *d_bad = reinterpret_cast<uint32_t *>(tot + 2);
  const SamSeq sq = seq ? *seq : SamSeq{};
  HIPCHK(hipMemsetAsync(tot, 0, 4 * sizeof(uint64_t), s));
  HIPCHK(hipMemsetAsync(d_bad, 0xFF, 4, s));
  HIPCHK(hipMemsetAsync(U.has_row.p, 0, n_pairs + 16, s));
  HIPCHK(hipEventRecord(U.ev[0], s));
  if (n_groups)
    hipLaunchKernelGGL(k_su_flags, dim3(blocks_for(n_groups)), dim3(256), 0, s, d_groups, d_plan, n_groups, n_pairs, U.has_row.as<uint8_t>());
#define SU_LENGTHS(B, Q)                                                                                                              \
  hipLaunchKernelGGL((k_su_lengths<B, Q>), dim3(blocks_for(n_pairs)), dim3(256), 0, s, U.has_row.as<uint8_t>(), n_pairs, paired ? 1 : 0, in, \
                     sq, U.len.as<uint32_t>(), d_bad, reinterpret_cast<unsigned long long *>(tot + 1))
  if (bam) {
    if (seq) SU_LENGTHS(true, true); else SU_LENGTHS(true, false);
  } else {
    if (seq) SU_LENGTHS(false, true); else SU_LENGTHS(false, false);
  }
#undef SU_LENGTHS
  HIPCHK(hipGetLastError());
  exclusive_scan_u32_to_u64(U.len.as<uint32_t>(), U.off.as<uint64_t>(), n_pairs, tot, U.scan_tmp.p, s);
  HIPCHK(hipEventRecord(U.ev[1], s));
  uint64_t h[3];
  read_back(h, tot, sizeof h, s);
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, U.ev[0], U.ev[1]));
  U.kernel_ms = ms;
  if (bam && (uint32_t)h[2] != 0xFFFFFFFFu) {
    *bad_read = (uint32_t)h[2];
    return;   // nothing will be written
  }
  *bytes = U.bytes = h[0];
  U.n_rows = h[1];
}

void sam_unmapped_write(uint64_t n_pairs, bool paired, const SamInputs &in, bool bam, const SamSeq *seq, SamUnmappedWork &U, uint8_t *d_out,
                        hipStream_t s) {
  if (!n_pairs || !U.bytes) return;
  const SamSeq sq = seq ? *seq : SamSeq{};
  HIPCHK(hipEventRecord(U.ev[2], s));
#define SU_WRITE(B, Q)                                                                                                                      \
  hipLaunchKernelGGL((k_su_write<B, Q>), dim3(blocks_for(n_pairs)), dim3(256), 0, s, U.has_row.as<uint8_t>(), n_pairs, paired ? 1 : 0, in, sq, \
                     U.off.as<uint64_t>(), d_out)
  if (bam) {
    if (seq) SU_WRITE(true, true); else SU_WRITE(true, false);
  } else {
    if (seq) SU_WRITE(false, true); else SU_WRITE(false, false);
  }
#undef SU_WRITE
  HIPCHK(hipEventRecord(U.ev[3], s));
  HIPCHK(hipGetLastError());
  U.write_pending = true;
}

void sam_unmapped_timing(SamUnmappedWork &U) {
  if (!U.write_pending) return;
  U.write_pending = false;
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, U.ev[2], U.ev[3]));
  U.kernel_ms += ms;
}

}  // namespace kslam
