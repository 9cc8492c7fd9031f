// coverage.hip -- the per-entry coverage table, accumulated on the device (include/kslam_coverage.h).
//
// When a lane has finished a batch, its final read pairs, their alignment-pair records and the overlap records those index lie
// in device memory; so does the index's entry-offset table.  The table is a bitmap with one bit per base of the index (every
// entry starts on a 64-bit word, so no word holds bits of two entries), four 64-bit counters per entry and a skip counter.
// Several lanes mark into it from their own streams, so every update is a device-scope atomic; every accumulator is an OR or an
// integer add, so the result does not depend on who marked what in which order.
//   1. k_cov_mark    one thread per alignment-pair RECORD (not per read pair: one read pair can hold thousands of records):
//                    it finds its group by binary search over the groups' ascending `first` and is live iff it lies below
//                    first + count.  A live record sets its mates' interval bits by mask per word -- a plain load first, the
//                    atomic only when bits are missing: bits only ever get set, so a stale load costs a redundant atomic, never
//                    a bit -- and flags its group when its entry differs from the group's first record's.  Intervals of more
//                    than COV_SHORT_WORDS words are not walked by their own lane: the wavefront takes them one after the
//                    other, one word per lane.  The counter adds of lanes that share an entry are summed in the wavefront first.
//   2. k_cov_unique  one thread per read pair: a group with live records and no flag adds one to its entry's unique_read_pairs.
//   3. k_cov_count   on request: the population count of the bitmap in equal tiles of COV_COUNT_TILE words with one entry
//                    lookup per tile end; a tile inside one entry (the rule for genomes) adds once per workgroup.
// Bounds: a mate is marked only after entry < n_entries, 0 <= ref_begin <= ref_end < the entry's length held, so every word
// index lies inside the entry's words; a counter row is touched only for an entry < n_entries.
#include "common.h"
#include "wave_add.h"
#include "../../include/kslam_coverage.h"

namespace kslam {

namespace {

constexpr uint32_t COV_SHORT_WORDS = 4;     // a 150-base interval touches at most 4 words
constexpr int COV_COUNT_BLOCK = 256;
constexpr int COV_COUNT_PER_THREAD = 8;
constexpr uint64_t COV_COUNT_TILE = (uint64_t)COV_COUNT_BLOCK * COV_COUNT_PER_THREAD;
enum { F_ALIGNMENTS = 0, F_UNIQUE = 1, F_ALIGNED = 2, F_COVERED = 3 };

__device__ inline uint64_t shfl64(uint64_t v, int lane) {
  const uint32_t lo = __shfl((uint32_t)v, lane), hi = __shfl((uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

// word w of an interval of nw words that begins at bit sb of its first word and ends at bit eb of its last
__device__ inline uint64_t word_mask(uint32_t w, uint32_t nw, uint32_t sb, uint32_t eb) {
  uint64_t m = ~0ull;
  if (w == 0) m &= ~0ull << sb;
  if (w == nw - 1) m &= ~0ull >> (63u - eb);
  return m;
}

__device__ inline void set_bits(unsigned long long *word, uint64_t m) {
  const uint64_t old = *word;
  if ((old & m) != m) atomicOr(word, (unsigned long long)m);
}

// the last e in [lo, hi) with off[e] <= w (off[lo] <= w is given)
__device__ inline uint64_t last_at_or_below(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t w) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= w) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(COV_MARK_BLOCK) void k_cov_mark(const kslam_overlap *__restrict__ ov, uint64_t n_ov,
                                                             const kslam_read_pair *__restrict__ groups, uint64_t n_groups,
                                                             const kslam_paired_overlap *__restrict__ pairs, uint64_t n_pairs,
                                                             CoverageTable T, uint32_t *__restrict__ gflag) {
  const uint64_t i = (uint64_t)blockIdx.x * COV_MARK_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // ---- which group, and live or dead ----
  bool live = false;
  uint64_t g = 0, first = 0;
  if (i < n_pairs && n_groups) {
    uint64_t lo = 0, hi = n_groups;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (groups[mid].first <= i) lo = mid;
      else hi = mid;
    }
    g = lo;
    first = groups[lo].first;
    live = first <= i && i - first < groups[lo].count;
  }
  uint32_t pe = 0, r[2] = {KSLAM_NO_OVERLAP, KSLAM_NO_OVERLAP};
  if (live) {
    pe = pairs[i].entry;
    r[0] = pairs[i].r1;
    r[1] = pairs[i].r2;
    if (i != first && pairs[first].entry != pe) atomicOr(gflag + g, 1u);
  }
  const bool pe_ok = live && pe < T.n_entries;
  uint64_t own_bases = 0;   // of the mates on the record's own entry: they go to memory with its `alignments`
  uint32_t n_skip = 0;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    // ---- the mate's interval ----
    bool valid = false;
    uint32_t e = 0, nw = 0, sb = 0, eb = 0;
    uint64_t w0 = 0, span = 0;
    if (r[k] != KSLAM_NO_OVERLAP) {
      if (r[k] < n_ov) {
        e = ov[r[k]].entry;
        const int32_t rb = ov[r[k]].ref_begin, re = ov[r[k]].ref_end;
        if (e < T.n_entries && rb >= 0 && re >= rb && (uint64_t)re < T.g_off[e + 1] - T.g_off[e]) {
          valid = true;
          w0 = T.word_off[e] + ((uint32_t)rb >> 6);
          nw = ((uint32_t)re >> 6) - ((uint32_t)rb >> 6) + 1;
          sb = (uint32_t)rb & 63u;
          eb = (uint32_t)re & 63u;
          span = (uint64_t)(re - rb) + 1;
        }
      }
      if (!valid) n_skip++;
    }
    // ---- its bits: short intervals by their own lane, long ones by the wavefront, one word per lane ----
    const bool is_long = valid && nw > COV_SHORT_WORDS;
    if (valid && !is_long)
      for (uint32_t w = 0; w < nw; w++) set_bits(T.bitmap + w0 + w, word_mask(w, nw, sb, eb));
    uint64_t longs = __ballot(is_long);
    while (longs) {
      const int leader = __ffsll((long long)longs) - 1;
      const uint64_t W0 = shfl64(w0, leader);
      const uint32_t NW = __shfl(nw, leader), SB = __shfl(sb, leader), EB = __shfl(eb, leader);
      for (uint32_t w = lane; w < NW; w += 64) set_bits(T.bitmap + W0 + w, word_mask(w, NW, SB, EB));
      longs &= longs - 1;
    }
    // ---- its bases ----
    const bool own = valid && pe_ok && e == pe;
    if (own) own_bases += span;
    wave_add(valid && !own, e, false, span, T.rows, F_ALIGNMENTS, F_ALIGNED);
  }
  wave_add(pe_ok, pe, true, own_bases, T.rows, F_ALIGNMENTS, F_ALIGNED);
  const uint64_t skips = wave_sum(n_skip);
  if (lane == 0 && skips) atomicAdd(T.skipped, (unsigned long long)skips);
}

__global__ __launch_bounds__(256) void k_cov_unique(const kslam_read_pair *__restrict__ groups, uint64_t n_groups,
                                                    const kslam_paired_overlap *__restrict__ pairs, uint64_t n_pairs, CoverageTable T,
                                                    const uint32_t *__restrict__ gflag) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool has = false;
  uint32_t e = 0;
  if (g < n_groups && groups[g].count > 0 && groups[g].first < n_pairs && gflag[g] == 0) {
    e = pairs[groups[g].first].entry;
    has = e < T.n_entries;
  }
  wave_add(has, e, true, 0, T.rows, F_UNIQUE, F_UNIQUE);
}

__global__ __launch_bounds__(256) void k_cov_clear_covered(unsigned long long *__restrict__ rows, uint64_t n_entries) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n_entries) rows[4 * e + F_COVERED] = 0;
}

__global__ __launch_bounds__(COV_COUNT_BLOCK) void k_cov_count(CoverageTable T) {
  __shared__ uint64_t s_e[2];
  __shared__ uint64_t s_part[COV_COUNT_BLOCK / 64];
  const uint64_t t0 = (uint64_t)blockIdx.x * COV_COUNT_TILE;
  const uint64_t t1 = t0 + COV_COUNT_TILE < T.n_words ? t0 + COV_COUNT_TILE : T.n_words;   // (the grid gives t0 < n_words)
  if (threadIdx.x < 2) s_e[threadIdx.x] = last_at_or_below(T.word_off, 0, T.n_entries, threadIdx.x ? t1 - 1 : t0);
  __syncthreads();
  const uint64_t e_lo = s_e[0], e_hi = s_e[1];
  if (e_lo == e_hi) {   // the tile lies inside one entry: one add
    uint64_t c = 0;
#pragma unroll
    for (int k = 0; k < COV_COUNT_PER_THREAD; k++) {
      const uint64_t w = t0 + (uint64_t)k * COV_COUNT_BLOCK + threadIdx.x;
      if (w < t1) c += __popcll(T.bitmap[w]);
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t total = 0;
      for (int k = 0; k < COV_COUNT_BLOCK / 64; k++) total += s_part[k];
      if (total) atomicAdd(T.rows + 4 * e_lo + F_COVERED, (unsigned long long)total);
    }
    return;
  }
  for (int k = 0; k < COV_COUNT_PER_THREAD; k++) {   // several entries: each word looks its own up between the tile's two
    const uint64_t w = t0 + (uint64_t)k * COV_COUNT_BLOCK + threadIdx.x;
    uint64_t c = 0;
    uint32_t e = 0;
    if (w < t1) {
      c = __popcll(T.bitmap[w]);
      if (c) e = (uint32_t)last_at_or_below(T.word_off, e_lo, e_hi + 1, w);
    }
    wave_add(c != 0, e, false, c, T.rows, F_COVERED, F_COVERED);
  }
}

}  // namespace

void coverage_mark_device(const kslam_overlap *d_ov, uint64_t n_ov, const kslam_read_pair *d_groups, uint64_t n_groups,
                          const kslam_paired_overlap *d_pairs, uint64_t n_pairs, const CoverageTable &T, CoverageMarkWork &W, hipStream_t s) {
  W.ms = 0;
  if (!n_groups || !n_pairs) return;
  if (n_pairs >= (1ull << 39) || n_groups >= (1ull << 39)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^39 or more alignment pairs in one batch"};
  if (!W.ev[0])
    for (auto &e : W.ev) HIPCHK(hipEventCreate(&e));
  W.gflag.ensure(n_groups * sizeof(uint32_t));
  HIPCHK(hipMemsetAsync(W.gflag.p, 0, n_groups * sizeof(uint32_t), s));
  HIPCHK(hipEventRecord(W.ev[0], s));
  hipLaunchKernelGGL(k_cov_mark, dim3((unsigned)((n_pairs + COV_MARK_BLOCK - 1) / COV_MARK_BLOCK)), dim3(COV_MARK_BLOCK), 0, s, d_ov, n_ov,
                     d_groups, n_groups, d_pairs, n_pairs, T, W.gflag.as<uint32_t>());
  hipLaunchKernelGGL(k_cov_unique, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, s, d_groups, n_groups, d_pairs, n_pairs, T,
                     W.gflag.as<uint32_t>());
  HIPCHK(hipEventRecord(W.ev[1], s));
  HIPCHK(hipGetLastError());
  HIPCHK(stream_wait(s));
  HIPCHK(hipEventElapsedTime(&W.ms, W.ev[0], W.ev[1]));
}

void coverage_count_device(const CoverageTable &T, hipEvent_t ev[2], hipStream_t s) {
  HIPCHK(hipEventRecord(ev[0], s));
  if (T.n_entries)
    hipLaunchKernelGGL(k_cov_clear_covered, dim3((unsigned)((T.n_entries + 255) / 256)), dim3(256), 0, s, T.rows, T.n_entries);
  if (T.n_words)
    hipLaunchKernelGGL(k_cov_count, dim3((unsigned)((T.n_words + COV_COUNT_TILE - 1) / COV_COUNT_TILE)), dim3(COV_COUNT_BLOCK), 0, s, T);
  HIPCHK(hipEventRecord(ev[1], s));
  HIPCHK(hipGetLastError());
}

}  // namespace kslam
