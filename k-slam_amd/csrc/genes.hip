// genes.hip -- the per-gene abundance table, counted on the device (include/kslam_genes.h).
//
// When a lane has finished a batch, its final read pairs and their alignment-pair records lie in device memory; so do the gene
// columns of the annotations (SamAnnot: gene_first, gene_start, gene_stop).  The table is four 64-bit counters per gene and
// four statistics counters.  Several lanes count into it from their own streams, so every update is a device-scope atomic;
// every accumulator is an integer add, so the result does not depend on who counted what in which order.
//   0. the lookup index, once per switch-on (genes_build_device): k_gene_records makes one 4-word record {entry, start biased
//      to unsigned, gene, stop} per gene, in gene-index order; the LSD radix sort (stable) orders them by (entry, start), ties
//      staying in gene-index order; k_gene_index unpacks them into order / sstart / sstop and scans the stops: a segmented
//      inclusive max-scan whose segments are the entries (a head wherever the record's entry differs from the one before it), in
//      three steps -- per workgroup, one wavefront over the workgroups' aggregates, and the carry into every position before
//      the workgroup's first head.
//   1. gene_of<LINEAR>, the device function of the count pass and of the test hook.  Indexed: hi = the end of the entry's prefix
//      with start < ref_end (binary search over sstart), lo = the first position whose running maximum exceeds ref_start
//      (binary search over runmax, which never falls inside an entry); the genes in [lo, hi) are scanned and the largest shared
//      kept, ties to the lowest gene index.  Exact for any columns: shared > 0 implies start < ref_end and stop > ref_start, and
//      a position whose stop exceeds ref_start has a running maximum that does.  LINEAR: the walk over all genes of the entry
//      (samtext.hip: best_gene, in 64 bits), kept as a cross-check and for measurement.
//   2. k_gene_count  one thread per alignment-pair RECORD (liveness and group as in coverage.hip: k_cov_mark): the record's gene
//                    into a scratch column, the counter adds of lanes that share a gene summed in the wavefront first.
//   3. k_gene_flag   one thread per record: flags its group when its gene differs from the gene of the group's first record or
//                    is none / skipped (the first record's gene is another thread's work, hence a pass of its own).
//   4. k_gene_unique one thread per read pair: a group with live records and no flag adds one to its gene's unique_read_pairs.
//   5. on request (genes_take_device): alignments > 0 is flagged, scanned (scan.hip) and the rows are compacted in gene order.
// Bounds: an entry is used only after entry < n_entries; its slice of the gene arrays is [gene_first[e], gene_first[e + 1])
// clamped to n_genes, and every position the searches and the scan touch lies inside it; a gene read from `order` or from the
// scratch column is used as an index only after gene < n_genes.
#include "common.h"
#include "wave_add.h"
#include "../../include/kslam_genes.h"

namespace kslam {

namespace {

constexpr uint32_t GENE_NONE = 0xFFFFFFFFu, GENE_SKIPPED = 0xFFFFFFFEu;
constexpr int32_t STOP_MIN = INT32_MIN;
enum { F_ALIGNMENTS = 1, F_UNIQUE = 2, F_OVERLAP = 3 };   // (slot 0 of a gene's four counters is not used)
enum { S_ALIGNMENTS = 0, S_IN_GENE = 1, S_NO_GENE = 2, S_SKIPPED = 3 };

struct GeneRow {   // kslam_gene_row
  unsigned long long gene, alignments, unique_read_pairs, overlap_bases;
};
static_assert(sizeof(GeneRow) == sizeof(kslam_gene_row), "the device row is the ABI's");

inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + GENES_BLOCK - 1) / GENES_BLOCK); }

// ---- the lookup index -------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(GENES_BLOCK) void k_gene_records(const uint64_t *__restrict__ gene_first, uint64_t n_entries,
                                                              const int32_t *__restrict__ gene_start, const int32_t *__restrict__ gene_stop,
                                                              uint64_t n_genes, uint4 *__restrict__ rec) {
  const uint64_t g = (uint64_t)blockIdx.x * GENES_BLOCK + threadIdx.x;
  if (g >= n_genes) return;
  uint64_t lo = 0, hi = n_entries;   // the last entry with gene_first[e] <= g (gene_first[0] == 0, n_entries > 0: checked by the caller)
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (gene_first[mid] <= g) lo = mid;
    else hi = mid;
  }
  rec[g] = make_uint4((uint32_t)lo, (uint32_t)gene_start[g] ^ 0x80000000u, (uint32_t)g, (uint32_t)gene_stop[g]);
}

// (f1, v1) then (f2, v2) of a segmented max-scan: a head forgets what came before it
__device__ inline void seg_join(bool f1, int32_t v1, bool &f2, int32_t &v2) {
  if (!f2) v2 = max(v1, v2);
  f2 = f2 || f1;
}

// inclusive, over the wavefront: f = a head at or before this lane, v = the maximum since the last head
__device__ inline void wave_seg_max(bool &f, int32_t &v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int pf = __shfl_up((int)f, o);
    const int32_t pv = __shfl_up(v, o);
    if (lane >= o) seg_join(pf != 0, pv, f, v);
  }
}

// the sorted records unpacked, and the scan inside each workgroup: runmax[i] = the largest stop since the last head in the
// workgroup; agg_f / agg_v [workgroup] = whether it holds a head, and the scan's value at its last position
__global__ __launch_bounds__(GENES_BLOCK) void k_gene_index(const uint4 *__restrict__ rec, uint64_t n, uint32_t *__restrict__ order,
                                                            int32_t *__restrict__ sstart, int32_t *__restrict__ sstop, int32_t *__restrict__ runmax,
                                                            uint32_t *__restrict__ agg_f, int32_t *__restrict__ agg_v) {
  __shared__ int s_f[GENES_BLOCK / 64];
  __shared__ int32_t s_v[GENES_BLOCK / 64];
  const uint64_t i = (uint64_t)blockIdx.x * GENES_BLOCK + threadIdx.x;
  const bool valid = i < n;
  const int w = threadIdx.x >> 6;
  bool f = false;
  int32_t v = STOP_MIN;   // (a position past the end joins as nothing)
  if (valid) {
    const uint4 r = rec[i];
    f = i == 0 || rec[i - 1].x != r.x;
    v = (int32_t)r.w;
    order[i] = r.z;
    sstart[i] = (int32_t)(r.y ^ 0x80000000u);
    sstop[i] = v;
  }
  wave_seg_max(f, v);
  if ((threadIdx.x & 63) == 63) {
    s_f[w] = f;
    s_v[w] = v;
  }
  __syncthreads();
  bool cf = false;
  int32_t cv = STOP_MIN;
  for (int k = 0; k < w; k++) {   // the wavefronts before this one
    bool kf = s_f[k] != 0;
    int32_t kv = s_v[k];
    seg_join(cf, cv, kf, kv);
    cf = kf;
    cv = kv;
  }
  seg_join(cf, cv, f, v);
  if (valid) runmax[i] = v;
  if (threadIdx.x == GENES_BLOCK - 1) {
    agg_f[blockIdx.x] = f;
    agg_v[blockIdx.x] = v;
  }
}

// one wavefront over the workgroups' aggregates, 64 at a time: agg_v[b] becomes the true running maximum at workgroup b's last position
__global__ __launch_bounds__(64) void k_gene_carry(const uint32_t *__restrict__ agg_f, int32_t *__restrict__ agg_v, uint64_t n_blocks) {
  bool cf = false;
  int32_t cv = STOP_MIN;
  for (uint64_t at = 0; at < n_blocks; at += 64) {
    const uint64_t b = at + threadIdx.x;
    bool f = false;
    int32_t v = STOP_MIN;
    if (b < n_blocks) {
      f = agg_f[b] != 0;
      v = agg_v[b];
    }
    wave_seg_max(f, v);
    seg_join(cf, cv, f, v);
    if (b < n_blocks) agg_v[b] = v;
    cf = __shfl((int)f, 63) != 0;
    cv = __shfl(v, 63);
  }
}

// the positions before a workgroup's first head continue the entry of the workgroup before: they take its running maximum in.
// The records ascend by entry, so "no head in [the workgroup's first position, i]" is "i's entry is that of the position before
// the workgroup".
__global__ __launch_bounds__(GENES_BLOCK) void k_gene_apply(const uint4 *__restrict__ rec, uint64_t n, const int32_t *__restrict__ agg_v,
                                                            int32_t *__restrict__ runmax) {
  const uint64_t i = (uint64_t)blockIdx.x * GENES_BLOCK + threadIdx.x;
  if (i >= n || blockIdx.x == 0) return;
  const uint64_t before = (uint64_t)blockIdx.x * GENES_BLOCK - 1;
  if (rec[i].x == rec[before].x) runmax[i] = max(runmax[i], agg_v[blockIdx.x - 1]);
}

// ---- the lookup -------------------------------------------------------------------------------------------------------------

__device__ inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

struct GeneHit {
  uint32_t gene;    // GENE_NONE, GENE_SKIPPED or a gene < n_genes
  int64_t shared;   // of that gene; 0 without one
};

template <bool LINEAR>
__device__ inline GeneHit gene_of(const GeneTable &T, uint32_t e, int32_t ref_start, int32_t ref_end) {
  GeneHit h{GENE_NONE, 0};
  if (e >= T.n_entries) {
    h.gene = GENE_SKIPPED;
    return h;
  }
  if (!T.n_genes) return h;
  uint64_t b = T.gene_first[e], t = T.gene_first[e + 1];
  if (t > T.n_genes) t = T.n_genes;
  if (b > t) b = t;
  const int64_t rs = ref_start, re = ref_end;
  if (LINEAR) {
    for (uint64_t g = b; g < t; g++) {
      const int64_t shared = min64(re, T.gene_stop[g]) - max64(rs, T.gene_start[g]);
      if (shared > h.shared) {
        h.gene = (uint32_t)g;
        h.shared = shared;
      }
    }
    return h;
  }
  uint64_t lo = b, hi = t;   // the first position with start >= ref_end: nothing from there on shares a base
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (T.sstart[mid] < ref_end) lo = mid + 1;
    else hi = mid;
  }
  const uint64_t end = lo;
  lo = b;                    // the first position whose running maximum of the stops exceeds ref_start: nothing before it does
  hi = end;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (T.runmax[mid] > ref_start) hi = mid;
    else lo = mid + 1;
  }
  for (uint64_t p = lo; p < end; p++) {
    const int64_t shared = min64(re, T.sstop[p]) - max64(rs, T.sstart[p]);
    if (shared <= 0 || shared < h.shared) continue;
    const uint32_t g = T.order[p];
    if (g >= T.n_genes) continue;
    if (shared > h.shared || g < h.gene) {
      h.gene = g;
      h.shared = shared;
    }
  }
  return h;
}

template <bool LINEAR>
__global__ __launch_bounds__(GENES_BLOCK) void k_gene_lookup(const uint32_t *__restrict__ entries, const int32_t *__restrict__ starts,
                                                             const int32_t *__restrict__ stops, uint64_t n, GeneTable T,
                                                             int64_t *__restrict__ gene_out, int64_t *__restrict__ shared_out) {
  const uint64_t i = (uint64_t)blockIdx.x * GENES_BLOCK + threadIdx.x;
  if (i >= n) return;
  const GeneHit h = gene_of<LINEAR>(T, entries[i], starts[i], stops[i]);
  gene_out[i] = h.gene == GENE_NONE ? -1 : h.gene == GENE_SKIPPED ? -2 : (int64_t)h.gene;
  shared_out[i] = h.shared;
}

// ---- the count passes -------------------------------------------------------------------------------------------------------

// the group of record i (the last one whose `first` is at or below i) and whether the record is live
__device__ inline bool live_record(const kslam_read_pair *__restrict__ groups, uint64_t n_groups, uint64_t i, uint64_t n_pairs, uint64_t &g,
                                   uint64_t &first) {
  g = first = 0;
  if (i >= n_pairs || !n_groups) return false;
  uint64_t lo = 0, hi = n_groups;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (groups[mid].first <= i) lo = mid;
    else hi = mid;
  }
  g = lo;
  first = groups[lo].first;
  return first <= i && i - first < groups[lo].count;
}

template <bool LINEAR>
__global__ __launch_bounds__(GENES_BLOCK) void k_gene_count(const kslam_read_pair *__restrict__ groups, uint64_t n_groups,
                                                            const kslam_paired_overlap *__restrict__ pairs, uint64_t n_pairs, GeneTable T,
                                                            uint32_t *__restrict__ gene) {
  const uint64_t i = (uint64_t)blockIdx.x * GENES_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint64_t g, first;
  const bool live = live_record(groups, n_groups, i, n_pairs, g, first);   // (no early return: every lane takes part in the ballots)
  GeneHit h{GENE_NONE, 0};
  if (live) {
    h = gene_of<LINEAR>(T, pairs[i].entry, pairs[i].ref_start, pairs[i].ref_end);
    gene[i] = h.gene;
  }
  const bool in_gene = live && h.gene < T.n_genes;
  wave_add(in_gene, h.gene, true, (uint64_t)h.shared, T.rows, F_ALIGNMENTS, F_OVERLAP);
  const uint64_t n_live = __popcll(__ballot(live)), n_in = __popcll(__ballot(in_gene));
  const uint64_t n_skip = __popcll(__ballot(live && h.gene == GENE_SKIPPED));
  if (lane == 0 && n_live) {
    atomicAdd(T.stats + S_ALIGNMENTS, (unsigned long long)n_live);
    if (n_in) atomicAdd(T.stats + S_IN_GENE, (unsigned long long)n_in);
    if (n_skip) atomicAdd(T.stats + S_SKIPPED, (unsigned long long)n_skip);
    if (n_live - n_in - n_skip) atomicAdd(T.stats + S_NO_GENE, (unsigned long long)(n_live - n_in - n_skip));
  }
}

__global__ __launch_bounds__(GENES_BLOCK) void k_gene_flag(const kslam_read_pair *__restrict__ groups, uint64_t n_groups, uint64_t n_pairs,
                                                           uint64_t n_genes, const uint32_t *__restrict__ gene, uint32_t *__restrict__ gflag) {
  const uint64_t i = (uint64_t)blockIdx.x * GENES_BLOCK + threadIdx.x;
  uint64_t g, first;
  if (!live_record(groups, n_groups, i, n_pairs, g, first)) return;
  const uint32_t mine = gene[i];
  if (mine >= n_genes || mine != gene[first]) atomicOr(gflag + g, 1u);   // (first <= i < n_pairs, and the first record is live)
}

__global__ __launch_bounds__(GENES_BLOCK) void k_gene_unique(const kslam_read_pair *__restrict__ groups, uint64_t n_groups, uint64_t n_pairs,
                                                             GeneTable T, const uint32_t *__restrict__ gene, const uint32_t *__restrict__ gflag) {
  const uint64_t g = (uint64_t)blockIdx.x * GENES_BLOCK + threadIdx.x;
  bool has = false;
  uint32_t k = 0;
  if (g < n_groups && groups[g].count > 0 && groups[g].first < n_pairs && gflag[g] == 0) {
    k = gene[groups[g].first];
    has = k < T.n_genes;
  }
  wave_add(has, k, true, 0, T.rows, F_UNIQUE, F_UNIQUE);
}

// ---- the take ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(GENES_BLOCK) void k_gene_flag_rows(const unsigned long long *__restrict__ rows, uint32_t *__restrict__ flag, uint64_t n_genes) {
  const uint64_t g = (uint64_t)blockIdx.x * GENES_BLOCK + threadIdx.x;
  if (g < n_genes) flag[g] = rows[4 * g + F_ALIGNMENTS] != 0;
}

// (the flags decide, not the counters read again: only a flagged gene has a place of its own among the rows)
__global__ __launch_bounds__(GENES_BLOCK) void k_gene_rows(const unsigned long long *__restrict__ rows, const uint32_t *__restrict__ flag,
                                                           const uint32_t *__restrict__ pos, GeneRow *__restrict__ out, uint64_t n_genes,
                                                           uint64_t n_rows) {
  const uint64_t g = (uint64_t)blockIdx.x * GENES_BLOCK + threadIdx.x;
  if (g >= n_genes || !flag[g]) return;
  const uint32_t at = pos[g];
  if (at < n_rows) out[at] = GeneRow{g, rows[4 * g + F_ALIGNMENTS], rows[4 * g + F_UNIQUE], rows[4 * g + F_OVERLAP]};
}

uint32_t bits_of(uint64_t max_value) {
  uint32_t b = 0;
  while (max_value >> b) b++;
  return b;
}

}  // namespace

void genes_build_device(uint64_t n_entries, uint64_t n_genes, const uint64_t *d_gene_first, const int32_t *d_gene_start, const int32_t *d_gene_stop,
                        uint32_t *d_order, int32_t *d_sstart, int32_t *d_sstop, int32_t *d_runmax, float *ms, hipStream_t s) {
  *ms = 0;
  if (!n_genes) return;
  if (!n_entries) throw StatusError{KSLAM_ERR_ARG, "genes without entries"};
  if (n_genes >= 0xFFFFFFFEull || n_entries >= (1ull << 32)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^32 - 2 or more genes"};
  const unsigned grid = blocks_of(n_genes);
  DevBuf rec_a, rec_b, agg_f, agg_v;   // the build's own buffers: they go when it returns
  SortWorkspace ws;
  rec_a.ensure(n_genes * sizeof(uint4));
  rec_b.ensure(n_genes * sizeof(uint4));
  agg_f.ensure((uint64_t)grid * sizeof(uint32_t));
  agg_v.ensure((uint64_t)grid * sizeof(int32_t));
  hipEvent_t ev[2] = {nullptr, nullptr};
  struct Events {
    hipEvent_t *e;
    ~Events() {
      for (int k = 0; k < 2; k++)
        if (e[k]) (void)hipEventDestroy(e[k]);
    }
  } events{ev};
  for (auto &e : ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(k_gene_records, dim3(grid), dim3(GENES_BLOCK), 0, s, d_gene_first, n_entries, d_gene_start, d_gene_stop, n_genes, rec_a.as<uint4>());
  HIPCHK(hipGetLastError());
  const uint4 *sorted = rec_a.as<uint4>();
  if (n_genes > 1) {
    SortPass passes[8];   // the start (word 1) below the entry (word 0); the gene index keeps equal keys in order (a stable sort)
    int n_passes = 0;
    for (int p = 0; p < 4; p++) passes[n_passes++] = SortPass{1u, (uint32_t)(8 * p), 0u};
    for (uint32_t bit = 0; bit < bits_of(n_entries - 1); bit += 8) passes[n_passes++] = SortPass{0u, bit, 0u};
    sorted = static_cast<const uint4 *>(radix_sort(rec_a.p, rec_b.p, n_genes, 4, passes, n_passes, ws, s, nullptr, nullptr, nullptr));
  }
  hipLaunchKernelGGL(k_gene_index, dim3(grid), dim3(GENES_BLOCK), 0, s, sorted, n_genes, d_order, d_sstart, d_sstop, d_runmax, agg_f.as<uint32_t>(),
                     agg_v.as<int32_t>());
  if (grid > 1) {
    hipLaunchKernelGGL(k_gene_carry, dim3(1), dim3(64), 0, s, agg_f.as<uint32_t>(), agg_v.as<int32_t>(), (uint64_t)grid);
    hipLaunchKernelGGL(k_gene_apply, dim3(grid), dim3(GENES_BLOCK), 0, s, sorted, n_genes, agg_v.as<int32_t>(), d_runmax);
  }
  HIPCHK(hipEventRecord(ev[1], s));
  HIPCHK(hipGetLastError());
  HIPCHK(stream_wait(s));   // (the build's buffers may go)
  HIPCHK(hipEventElapsedTime(ms, ev[0], ev[1]));
}

void genes_count_device(const kslam_read_pair *d_groups, uint64_t n_groups, const kslam_paired_overlap *d_pairs, uint64_t n_pairs,
                        const GeneTable &T, GenesCountWork &W, bool linear, hipStream_t s) {
  W.ms = 0;
  if (!n_groups || !n_pairs) return;
  if (n_pairs >= (1ull << 39) || n_groups >= (1ull << 39)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^39 or more alignment pairs in one batch"};
  if (!W.ev[0])
    for (auto &e : W.ev) HIPCHK(hipEventCreate(&e));
  W.gene.ensure(n_pairs * sizeof(uint32_t));
  W.gflag.ensure(n_groups * sizeof(uint32_t));
  HIPCHK(hipMemsetAsync(W.gflag.p, 0, n_groups * sizeof(uint32_t), s));
  HIPCHK(hipEventRecord(W.ev[0], s));
  if (linear) hipLaunchKernelGGL((k_gene_count<true>), dim3(blocks_of(n_pairs)), dim3(GENES_BLOCK), 0, s, d_groups, n_groups, d_pairs, n_pairs, T, W.gene.as<uint32_t>());
  else hipLaunchKernelGGL((k_gene_count<false>), dim3(blocks_of(n_pairs)), dim3(GENES_BLOCK), 0, s, d_groups, n_groups, d_pairs, n_pairs, T, W.gene.as<uint32_t>());
  hipLaunchKernelGGL(k_gene_flag, dim3(blocks_of(n_pairs)), dim3(GENES_BLOCK), 0, s, d_groups, n_groups, n_pairs, T.n_genes, W.gene.as<uint32_t>(),
                     W.gflag.as<uint32_t>());
  hipLaunchKernelGGL(k_gene_unique, dim3(blocks_of(n_groups)), dim3(GENES_BLOCK), 0, s, d_groups, n_groups, n_pairs, T, W.gene.as<uint32_t>(),
                     W.gflag.as<uint32_t>());
  HIPCHK(hipEventRecord(W.ev[1], s));
  HIPCHK(hipGetLastError());
  HIPCHK(stream_wait(s));
  HIPCHK(hipEventElapsedTime(&W.ms, W.ev[0], W.ev[1]));
}

void genes_take_device(const GeneTable &T, GenesTakeWork &W, uint64_t *n_rows, hipEvent_t ev[2], hipStream_t s) {
  *n_rows = 0;
  HIPCHK(hipEventRecord(ev[0], s));
  if (!T.n_genes) {
    HIPCHK(hipEventRecord(ev[1], s));
    W.rows.ensure(sizeof(GeneRow));
    return;
  }
  if (T.n_genes >= (1ull << 32)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^32 or more genes"};
  W.flag.ensure(T.n_genes * sizeof(uint32_t));
  W.pos.ensure(T.n_genes * sizeof(uint32_t));
  W.scan_tmp.ensure(scan_tmp_bytes(T.n_genes + 1));
  W.totals.ensure(sizeof(uint64_t));
  HIPCHK(hipMemsetAsync(W.totals.p, 0, sizeof(uint64_t), s));
  hipLaunchKernelGGL(k_gene_flag_rows, dim3(blocks_of(T.n_genes)), dim3(GENES_BLOCK), 0, s, T.rows, W.flag.as<uint32_t>(), T.n_genes);
  HIPCHK(hipGetLastError());
  exclusive_scan_u32(W.flag.as<uint32_t>(), W.pos.as<uint32_t>(), T.n_genes, W.totals.as<uint64_t>(), W.scan_tmp.p, s);
  uint64_t n = 0;
  read_back(&n, W.totals.p, sizeof n, s);
  W.rows.ensure((n + 1) * sizeof(GeneRow));
  if (n) hipLaunchKernelGGL(k_gene_rows, dim3(blocks_of(T.n_genes)), dim3(GENES_BLOCK), 0, s, T.rows, W.flag.as<uint32_t>(), W.pos.as<uint32_t>(),
                            W.rows.as<GeneRow>(), T.n_genes, n);
  HIPCHK(hipEventRecord(ev[1], s));
  HIPCHK(hipGetLastError());
  *n_rows = n;
}

void genes_lookup_device(const uint32_t *d_entries, const int32_t *d_starts, const int32_t *d_stops, uint64_t n, const GeneTable &T, bool linear,
                         int64_t *d_gene_out, int64_t *d_shared_out, hipStream_t s) {
  if (!n) return;
  if (linear) hipLaunchKernelGGL((k_gene_lookup<true>), dim3(blocks_of(n)), dim3(GENES_BLOCK), 0, s, d_entries, d_starts, d_stops, n, T, d_gene_out, d_shared_out);
  else hipLaunchKernelGGL((k_gene_lookup<false>), dim3(blocks_of(n)), dim3(GENES_BLOCK), 0, s, d_entries, d_starts, d_stops, n, T, d_gene_out, d_shared_out);
  HIPCHK(hipGetLastError());
}

}  // namespace kslam
