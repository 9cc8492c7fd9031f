// readqc.hip -- the read QC report's tables, tallied on the device (include/kslam_readqc.h).
//
// On the text route a lane holds the batch's bases and quality columns in device memory (gather_fields); this pass reads them
// once and adds into tables of fixed size.  Several lanes count into one state from their own streams, so every update of the
// global tables is a device-scope atomic; every accumulator is an integer add, so the result does not depend on who counted
// what in which order.
//
// The mapping is lane = cycle.  A wavefront counts one read at a time and walks it in chunks of 64 consecutive bytes of each
// column (the loads coalesce at any alignment; four chunks are requested together, and the next read's are in flight while
// this one is counted), so lane i always holds cycle 64 * chunk + i and two lanes of one wave instruction never share a
// per-cycle row below C.
//   tile         a workgroup owns RQ_TILE consecutive cycle rows (blockIdx.y) and a run of one stream's reads (blockIdx.x; a
//                launch holds reads of one stream); its LDS tile does not depend on C.  The grid has as many tiles as the longest
//                read of the call needs.
//   quality      s_q[row][95] in LDS, ds adds that return nothing.  The row stride of 95 words is odd: when every lane adds
//                to the same quality value -- the normal case on binned qualities -- lane i hits bank (q - i) mod 32, all
//                different inside a group of 32 lanes.  Only different waves can meet on an address.
//   base content s_b[row][7] likewise (six columns, stride 7: odd again).
//   row C        the pooled row is an ordinary row that MANY lanes of one instruction hit, so it is reduced inside the wave
//                first: six ballots for the base columns; the quality columns by combining equal values the way kreport.hip
//                combines equal nodes (one LDS add per distinct value per chunk).  Its counters are 64-bit LDS words: one
//                read may put any number of bytes there.  The last tile of the grid owns it.
//   per read     tile 0 walks the whole read, whatever its length: G+C and A+C+G+T are two ballots and a population count
//                per chunk, the number of quality bytes in 33..126 a third; only the quality sum is carried per lane (64-bit)
//                and reduced across the wave once per read.  mean_q and gc go to LDS bins.  The wave keeps the length it saw
//                last with a count (equal lengths are combined before the add; the usual run has one length) and min / max
//                in wave-uniform registers; at its end they go to 64-bit LDS words, the run's count into the workgroup's
//                slot when it has the workgroup's first length, else straight to the global histogram.
//   flush        once per workgroup: every non-zero LDS cell is added to its 64-bit global counter.
// Counter widths: a 32-bit LDS cell of s_q / s_b / s_mq / s_gc receives at most 1 per read the workgroup takes; a launch holds
// at most RQ_SLICE = 2^30 reads per stream, so no cell passes 2^30 < 2^32 before its flush.  Everything that one read can feed
// more than once (row C, n_bases, the length slot) is 64 bits wide.
// Bounds: a lane loads byte off[r] + cycle only for cycle < off[r + 1] - off[r]; a row index below C is < row_end <= C; the
// length entry is min(len, C + 1); the mean bin is a mean of values <= 93; the GC bin is (200 g + n) / 2n <= 100 for g <= n.
#include "common.h"
#include "../../include/kslam_readqc.h"

namespace kslam {

namespace {

constexpr int RQ_BLOCK = 1024;                 // 16 waves share one tile
constexpr int RQ_WAVES = RQ_BLOCK / 64;
constexpr uint32_t RQ_TILE = 128;              // cycle rows per workgroup: 128 * (95 + 7) * 4 = 52 KB of LDS, two workgroups per CU
constexpr uint32_t RQ_QS = KSLAM_READ_QC_QUAL_COLS;   // 95: the quality row's stride
constexpr uint32_t RQ_BS = 7;                  // the base row's stride (6 columns)
constexpr uint32_t RQ_MAX_BLOCKS = 512;        // workgroups per tile and stream: two per CU
constexpr uint64_t RQ_SLICE = 1ull << 30;      // reads per stream and launch
constexpr int RQ_UNROLL = 4;                   // chunks requested together
constexpr uint32_t RQ_NONE = 0xFFFFFFFFu;

// a stream's words (include/kslam_readqc.h)
__host__ __device__ inline uint64_t rq_len_hist(uint32_t) { return 4; }
__host__ __device__ inline uint64_t rq_base(uint32_t C) { return 4 + ((uint64_t)C + 2); }
__host__ __device__ inline uint64_t rq_qual(uint32_t C) { return rq_base(C) + ((uint64_t)C + 1) * KSLAM_READ_QC_BASE_COLS; }
__host__ __device__ inline uint64_t rq_mean(uint32_t C) { return rq_qual(C) + ((uint64_t)C + 1) * KSLAM_READ_QC_QUAL_COLS; }
__host__ __device__ inline uint64_t rq_gc(uint32_t C) { return rq_mean(C) + KSLAM_READ_QC_MEAN_BINS; }

__device__ inline uint32_t base_col(uint32_t b) {
  const uint32_t u = b & 0xDFu;   // 'a' -> 'A'; no other byte becomes a letter it was not
  return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : u == 'N' ? 4u : 5u;
}
__device__ inline uint32_t qual_col(uint32_t q) { return q - 33u <= 93u ? q - 33u : 94u; }

__device__ inline unsigned long long wave_sum(unsigned long long v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = ((unsigned long long)(uint32_t)__shfl_xor((int)hi, d) << 32) | (uint32_t)__shfl_xor((int)lo, d);
    v += o;
    lo = (uint32_t)v;
    hi = (uint32_t)(v >> 32);
  }
  return v;
}

// The n_here reads from r_lo on, all of stream `stream`; workgroup x takes the rpb reads from r_lo + x * rpb on.  tail_tile: the
// tile that owns row C (RQ_NONE: no read of the call is longer than C).
__global__ __launch_bounds__(RQ_BLOCK) void k_rq_count(const uint8_t *__restrict__ bases, const uint8_t *__restrict__ quality,
                                                       const uint64_t *__restrict__ off, uint64_t r_lo, uint64_t n_here, uint64_t rpb,
                                                       ReadQcTable T, uint32_t stream, uint32_t tail_tile) {
  __shared__ uint32_t s_q[RQ_TILE * RQ_QS];
  __shared__ uint32_t s_b[RQ_TILE * RQ_BS];
  __shared__ uint32_t s_mq[KSLAM_READ_QC_MEAN_BINS];
  __shared__ uint32_t s_gc[KSLAM_READ_QC_GC_BINS];
  __shared__ unsigned long long s_tail[KSLAM_READ_QC_BASE_COLS + KSLAM_READ_QC_QUAL_COLS];   // row C: base columns, then quality
  __shared__ unsigned long long s_stat[4];   // n_reads, n_bases, min_len, max_len
  __shared__ unsigned long long s_len_key, s_len_cnt;

  const uint32_t C = T.C;
  const uint32_t tile = blockIdx.y;
  unsigned long long *const W = T.words + (uint64_t)stream * T.n_words;
  const uint64_t row0 = (uint64_t)tile * RQ_TILE;
  const uint64_t row_end = row0 + RQ_TILE < C ? row0 + RQ_TILE : C;   // ordinary rows of this tile: [row0, row_end)
  const bool owns_tail = tile == tail_tile, owns_reads = tile == 0;
  uint64_t b_lo = r_lo + (uint64_t)blockIdx.x * rpb, b_hi = b_lo + rpb;
  const uint64_t s_hi = r_lo + n_here;
  if (b_lo > s_hi) b_lo = s_hi;
  if (b_hi > s_hi) b_hi = s_hi;

  for (uint32_t i = threadIdx.x; i < RQ_TILE * RQ_QS; i += RQ_BLOCK) s_q[i] = 0;
  for (uint32_t i = threadIdx.x; i < RQ_TILE * RQ_BS; i += RQ_BLOCK) s_b[i] = 0;
  if (threadIdx.x < KSLAM_READ_QC_MEAN_BINS) s_mq[threadIdx.x] = 0;
  if (threadIdx.x < KSLAM_READ_QC_GC_BINS) s_gc[threadIdx.x] = 0;
  if (threadIdx.x < KSLAM_READ_QC_BASE_COLS + KSLAM_READ_QC_QUAL_COLS) s_tail[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    s_stat[0] = s_stat[1] = s_stat[3] = 0;
    s_stat[2] = ~0ull;
    s_len_key = b_lo < b_hi ? off[b_lo + 1] - off[b_lo] : ~0ull;
    s_len_cnt = 0;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // wave-uniform, tile 0 only
  unsigned long long w_reads = 0, w_bases = 0, w_min = ~0ull, w_max = 0, run_len = ~0ull, run_cnt = 0;
  const unsigned long long len_key = s_len_key;

  auto flush_run = [&] {
    if (!run_cnt || lane) return;
    if (run_len == len_key) atomicAdd(&s_len_cnt, run_cnt);
    else atomicAdd(W + rq_len_hist(C) + (run_len <= C ? run_len : (unsigned long long)C + 1), run_cnt);
  };

  // the cycles this workgroup has to look at in a read of len bases: tile 0 all of them (the per-read sums), the tile of row C
  // everything from its first row on, any other tile its own rows
  auto range = [&](uint64_t len, uint64_t &c_lo, uint64_t &c_hi) {
    c_lo = owns_reads ? 0 : row0;
    c_hi = (owns_reads || owns_tail) ? len : (len < row_end ? len : row_end);
  };
  // RQ_UNROLL chunks of both columns from cycle c0 on; a lane past c_hi loads nothing
  auto load_group = [&](uint64_t at, uint64_t c0, uint64_t c_hi, uint32_t (&b)[RQ_UNROLL], uint32_t (&q)[RQ_UNROLL]) {
#pragma unroll
    for (int k = 0; k < RQ_UNROLL; k++) {
      const uint64_t cyc = c0 + 64 * k + lane;
      const bool ok = cyc < c_hi;
      b[k] = ok ? bases[at + cyc] : 0u;
      q[k] = ok ? quality[at + cyc] : 0u;
    }
  };
  // Two memory latencies stand between a read's number and its bytes (the offsets, then the columns), and a read of 150 bases
  // is three chunks of work: unpipelined, the pass is bound by those latencies.  So the wave runs three reads deep: while it
  // counts read r, the first group of read r + 16 is in flight (its offsets arrived an iteration ago) and the offsets of read
  // r + 32 are requested.
  const uint64_t r0 = b_lo + wave;
  uint64_t at0 = 0, len0 = 0, at1 = 0, len1 = 0;
  if (r0 < b_hi) {
    at0 = off[r0];
    len0 = off[r0 + 1] - at0;
  }
  if (r0 + RQ_WAVES < b_hi) {
    at1 = off[r0 + RQ_WAVES];
    len1 = off[r0 + RQ_WAVES + 1] - at1;
  }
  uint32_t cb[RQ_UNROLL], cq[RQ_UNROLL];
  {
    uint64_t c_lo, c_hi;
    range(len0, c_lo, c_hi);
    load_group(at0, c_lo, c_hi, cb, cq);
  }
  for (uint64_t r = r0; r < b_hi; r += RQ_WAVES) {
    uint64_t at2 = 0, len2 = 0;
    if (r + 2 * RQ_WAVES < b_hi) {
      at2 = off[r + 2 * RQ_WAVES];
      len2 = off[r + 2 * RQ_WAVES + 1] - at2;
    }
    uint32_t nb[RQ_UNROLL], nq[RQ_UNROLL];
    {
      uint64_t n_lo, n_hi;
      range(len1, n_lo, n_hi);   // (no next read: len1 = 0 and no lane loads)
      load_group(at1, n_lo, n_hi, nb, nq);
    }
    const uint64_t at = at0, len = len0;
    uint64_t c_lo, c_hi;
    range(len, c_lo, c_hi);
    unsigned long long q_sum = 0;                     // per lane
    unsigned long long n_gc = 0, n_acgt = 0, n_q = 0;   // wave-uniform
    for (uint64_t c0 = c_lo; c0 < c_hi; c0 += 64 * RQ_UNROLL) {
      if (c0 != c_lo) load_group(at, c0, c_hi, cb, cq);   // (a read longer than one group: its later groups are not prefetched)
#pragma unroll
      for (int k = 0; k < RQ_UNROLL; k++) {
        if (c0 + 64 * k >= c_hi) break;   // (uniform)
        const uint64_t cyc = c0 + 64 * k + lane;
        const bool ok = cyc < c_hi;
        const uint32_t bc = base_col(cb[k]), qc = qual_col(cq[k]);
        if (ok && cyc >= row0 && cyc < row_end) {
          const uint32_t row = (uint32_t)(cyc - row0);
          atomicAdd(&s_q[row * RQ_QS + qc], 1u);
          atomicAdd(&s_b[row * RQ_BS + bc], 1u);
        }
        if (owns_tail) {
          const bool in_tail = ok && cyc >= C;
          uint64_t pending = __ballot(in_tail);
          if (pending) {
#pragma unroll
            for (uint32_t col = 0; col < KSLAM_READ_QC_BASE_COLS; col++) {
              const uint64_t m = __ballot(in_tail && bc == col);
              if (m && lane == 0) atomicAdd(&s_tail[col], (unsigned long long)__popcll(m));
            }
            while (pending) {
              const int leader = __ffsll((long long)pending) - 1;
              const uint32_t q0 = __shfl(qc, leader);
              const uint64_t m = __ballot(in_tail && qc == q0);
              if (lane == leader) atomicAdd(&s_tail[KSLAM_READ_QC_BASE_COLS + q0], (unsigned long long)__popcll(m));
              pending &= ~m;
            }
          }
        }
        if (owns_reads) {
          n_gc += __popcll(__ballot(ok && (bc == 1u || bc == 2u)));
          n_acgt += __popcll(__ballot(ok && bc < 4u));
          n_q += __popcll(__ballot(ok && qc < 94u));
          if (ok && qc < 94u) q_sum += qc;
        }
      }
    }
    if (owns_reads) {
      const unsigned long long total = wave_sum(q_sum);
      if (lane == 0) {
        const bool small = len < (1u << 24);   // then every operand below fits 32 bits: 93 * len, 201 * len
        if (n_q) atomicAdd(&s_mq[small ? (uint32_t)total / (uint32_t)n_q : (uint32_t)(total / n_q)], 1u);
        if (n_acgt)
          atomicAdd(&s_gc[small ? (200u * (uint32_t)n_gc + (uint32_t)n_acgt) / (2u * (uint32_t)n_acgt) : (uint32_t)((200ull * n_gc + n_acgt) / (2ull * n_acgt))], 1u);
      }
      w_reads++;
      w_bases += len;
      w_min = len < w_min ? len : w_min;
      w_max = len > w_max ? len : w_max;
      if (len == run_len) run_cnt++;
      else {
        flush_run();
        run_len = len;
        run_cnt = 1;
      }
    }
    at0 = at1;
    len0 = len1;
    at1 = at2;
    len1 = len2;
#pragma unroll
    for (int k = 0; k < RQ_UNROLL; k++) {
      cb[k] = nb[k];
      cq[k] = nq[k];
    }
  }
  if (owns_reads && w_reads) {
    flush_run();
    if (lane == 0) {
      atomicAdd(&s_stat[0], w_reads);
      atomicAdd(&s_stat[1], w_bases);
      atomicMin(&s_stat[2], w_min);
      atomicMax(&s_stat[3], w_max);
    }
  }
  __syncthreads();

  // the flush: non-zero cells only
  unsigned long long *const g_base = W + rq_base(C), *const g_qual = W + rq_qual(C);
  for (uint32_t i = threadIdx.x; i < RQ_TILE * RQ_QS; i += RQ_BLOCK) {
    const uint32_t v = s_q[i];
    const uint64_t row = row0 + i / RQ_QS;
    if (v && row < row_end) atomicAdd(g_qual + row * KSLAM_READ_QC_QUAL_COLS + i % RQ_QS, (unsigned long long)v);
  }
  for (uint32_t i = threadIdx.x; i < RQ_TILE * RQ_BS; i += RQ_BLOCK) {
    const uint32_t v = s_b[i];
    const uint64_t row = row0 + i / RQ_BS;
    const uint32_t col = i % RQ_BS;
    if (v && row < row_end && col < KSLAM_READ_QC_BASE_COLS) atomicAdd(g_base + row * KSLAM_READ_QC_BASE_COLS + col, (unsigned long long)v);
  }
  if (owns_tail && threadIdx.x < KSLAM_READ_QC_BASE_COLS + KSLAM_READ_QC_QUAL_COLS) {
    const unsigned long long v = s_tail[threadIdx.x];
    if (v) {
      if (threadIdx.x < KSLAM_READ_QC_BASE_COLS) atomicAdd(g_base + (uint64_t)C * KSLAM_READ_QC_BASE_COLS + threadIdx.x, v);
      else atomicAdd(g_qual + (uint64_t)C * KSLAM_READ_QC_QUAL_COLS + (threadIdx.x - KSLAM_READ_QC_BASE_COLS), v);
    }
  }
  if (owns_reads) {
    if (threadIdx.x < KSLAM_READ_QC_MEAN_BINS && s_mq[threadIdx.x]) atomicAdd(W + rq_mean(C) + threadIdx.x, (unsigned long long)s_mq[threadIdx.x]);
    if (threadIdx.x < KSLAM_READ_QC_GC_BINS && s_gc[threadIdx.x]) atomicAdd(W + rq_gc(C) + threadIdx.x, (unsigned long long)s_gc[threadIdx.x]);
    if (threadIdx.x == 0 && s_stat[0]) {
      atomicAdd(W + 0, s_stat[0]);
      atomicAdd(W + 1, s_stat[1]);
      atomicMin(W + 2, s_stat[2]);
      atomicMax(W + 3, s_stat[3]);
      if (s_len_cnt) atomicAdd(W + rq_len_hist(C) + (s_len_key <= C ? s_len_key : (unsigned long long)C + 1), s_len_cnt);
    }
  }
}

__global__ void k_rq_min_init(unsigned long long *a, unsigned long long *b) {
  if (threadIdx.x == 0) *a = ~0ull;
  if (threadIdx.x == 1) *b = ~0ull;
}

}  // namespace

void readqc_zero_device(const ReadQcTable &T, hipStream_t s) {
  HIPCHK(hipMemsetAsync(T.words, 0, 2 * T.n_words * sizeof(uint64_t), s));
  hipLaunchKernelGGL(k_rq_min_init, dim3(1), dim3(64), 0, s, T.words + 2, T.words + T.n_words + 2);
  HIPCHK(hipGetLastError());
}

void readqc_count_device(const uint8_t *d_bases, const uint8_t *d_quality, const uint64_t *d_off, uint64_t n, bool paired, uint64_t max_len,
                         const ReadQcTable &T, ReadQcWork &W, bool timed, hipStream_t s) {
  if (timed) {
    W.ms = 0;
    if (!W.ev[0])
      for (auto &e : W.ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(W.ev[0], s));
  }
  const uint32_t C = T.C;
  // tiles: the ordinary rows the longest read reaches; with a read longer than C all of them, and the last one owns row C
  const uint64_t reach = max_len < C ? max_len : C;
  uint32_t n_tiles = (uint32_t)((reach + RQ_TILE - 1) / RQ_TILE);
  if (!n_tiles) n_tiles = 1;
  const uint32_t tail_tile = max_len > C ? n_tiles - 1 : RQ_NONE;
  const uint64_t per_stream = paired ? n / 2 : n;
  const uint32_t n_streams = paired ? 2 : 1;
  for (uint32_t z = 0; z < n_streams && per_stream; z++)
    for (uint64_t lo = 0; lo < per_stream; lo += RQ_SLICE) {
      const uint64_t m = per_stream - lo < RQ_SLICE ? per_stream - lo : RQ_SLICE;
      uint64_t rpb = (m + RQ_MAX_BLOCKS - 1) / RQ_MAX_BLOCKS;
      if (rpb < RQ_READS) rpb = RQ_READS;
      const unsigned gx = (unsigned)((m + rpb - 1) / rpb);
      hipLaunchKernelGGL(k_rq_count, dim3(gx, n_tiles, 1), dim3(RQ_BLOCK), 0, s, d_bases, d_quality, d_off, z * per_stream + lo, m, rpb, T, z, tail_tile);
    }
  HIPCHK(hipGetLastError());
  if (timed) {
    HIPCHK(hipEventRecord(W.ev[1], s));
    HIPCHK(stream_wait(s));
    HIPCHK(hipEventElapsedTime(&W.ms, W.ev[0], W.ev[1]));
  }
}

}  // namespace kslam
