// depth.hip -- the per-base depth track, accumulated on the device (include/kslam_depth.h).
//
// What a lane holds after a batch is what variants.hip reads, less the bases: the final read pairs, their alignment-pair records,
// the overlap records those index, the CIGAR pool, the reads' and the entries' offsets.  A counter per base of the index would
// cost 20 GB for 5 Gb, so the track is kept as its DERIVATIVE: the boundaries where the depth changes, with the change.
// Key space: key = g_off[entry] + entry + pos -- one spare position per entry, so that the boundary after the last base of entry
// e (pos = its length) is not the first base of entry e + 1, and every entry's changes sum to 0 inside its own keys: no run can
// continue into the next entry.
// Per batch (depth_count_device, depth_write_device):
//   1-2. variants.hip's flag / scan / list passes (contributing_list_device): the overlap records a live pair names, once each
//   3. k_dep_count   one thread per listed record: walk_record (pileup_walk.h) checks the whole CIGAR against the read's and
//                    the entry's length and hands the M runs to a DepSink<CountEmit>, which counts them
//   4. one scan      lays out the slots
//   5. the caller makes room (api_depth.hip, under the state's lock)
//   6. k_dep_write   the same walk into a DepSink<WriteEmit>: per M run (begin << 1) and ((end + 1) << 1) | 1 into the pending keys
// Compaction (depth_compact_device), when the pending keys pass the threshold and at every take:
//   a. radix_sort of the pending keys, passes from the largest possible key
//   b. run heads ignoring the low bit (run_heads_device, run_starts_device: variants.hip's), a scan that numbers the runs, one thread per RUN: the begins sort before the ends, so a
//      binary search for the split gives both counts whatever the run's length (70 001 equal intervals cost ~17 steps); the run
//      becomes ONE record (key, begins - ends) with a 64-bit change
//   c. merge with the compacted list: both lists are sorted and distinct, so a record's place is its own index plus its rank in
//      the other list (one binary search per record, no atomics, the compacted list is never sorted again); a boundary that both
//      lists hold lands on two adjacent slots, the compacted one first
//   d. the first of equal keys takes the sum; sums of 0 are dropped; a scan of the keep flags and a scatter into the new list
// Take (depth_take_device): an inclusive 64-bit scan of the changes gives the depth from each boundary on (k_dep_tile_sums,
// k_dep_scan_tiles, k_dep_depth), k_dep_flag marks the boundaries that start a row and combines rows, covered bases and the
// largest depth per wavefront and then per block before one atomic each, a scan of the flags, and k_dep_rows resolves entry and
// start by binary search in the entry offsets and takes the end from the next boundary.
// Bounds: the walk's are stated in pileup_walk.h; with a sink that wants no columns it reads nothing but the record, its CIGAR
// words and four offsets.  Every other kernel indexes arrays by thread number below their length, by a scanned slot below the
// scan's total, or by a binary search's result inside [0, n).
#include "pileup_walk.h"
#include "wave_add.h"
#include "../../include/kslam_depth.h"

namespace kslam {

namespace {

constexpr int DEP_BLOCK = PILEUP_BLOCK;
constexpr int DEP_ITEMS = 4;
constexpr int DEP_TILE = DEP_BLOCK * DEP_ITEMS;   // of the 64-bit scan
constexpr int DEP_FLAG_ITEMS = 16;                // boundaries per thread of the flag pass

__device__ inline uint32_t wave_max32(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
  return v;
}
// inclusive scan over the 64 lanes of a wave
__device__ inline int64_t wave_scan64(int64_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t lo = __shfl_up((uint32_t)(uint64_t)v, o), hi = __shfl_up((uint32_t)((uint64_t)v >> 32), o);
    if (lane >= o) v += (int64_t)(((uint64_t)hi << 32) | lo);
  }
  return v;
}
// inclusive scan over the DEP_BLOCK threads of a block; *total: the block's sum.  lds: 4 values
__device__ inline int64_t block_scan64(int64_t v, int64_t *lds, int64_t *total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  v = wave_scan64(v);
  __syncthreads();   // (lds may still be read from the round before)
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  int64_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < DEP_BLOCK / 64; w++) {
    const int64_t x = lds[w];
    if (w < wave) before += x;
    all += x;
  }
  *total = all;
  return v + before;
}

struct CountEmit {
  uint32_t n = 0;
  __device__ void run(uint64_t, uint64_t) { n++; }
};
struct WriteEmit {
  uint64_t *out;
  __device__ void run(uint64_t begin, uint64_t end1) {
    *out++ = begin << 1;
    *out++ = (end1 << 1) | 1u;
  }
};
// the walk's sink (pileup_walk.h): the M runs alone, no columns -- the walk reads nothing but the record, its CIGAR words and four
// offsets.  A run's keys: the entry's first key is g_off[entry] + entry; the end is exclusive.
template <class Emit>
struct DepSink : Emit {
  static constexpr bool COLUMNS = false, INSERTIONS = false;
  __device__ void m_run(const kslam_overlap &o, const RecordFrame &f, int64_t rp, uint32_t len) {
    const uint64_t begin = f.gb + o.entry + (uint64_t)rp;
    Emit::run(begin, begin + len);
  }
  __device__ void d_run(const kslam_overlap &, const RecordFrame &, int64_t, uint32_t) {}
};

__global__ __launch_bounds__(DEP_BLOCK) void k_dep_count(VariantInputs in, const uint32_t *__restrict__ list, uint64_t n_list,
                                                         uint32_t *__restrict__ cnt, unsigned long long *__restrict__ tallies) {
  const uint64_t x = (uint64_t)blockIdx.x * DEP_BLOCK + threadIdx.x;
  uint64_t skip = 0;
  if (x < n_list) {
    const kslam_overlap o = in.ov[list[x]];
    DepSink<CountEmit> sink;
    if (!walk_record(o, in, sink)) skip = 1;
    cnt[x] = sink.n;
  }
  skip = wave_sum(skip);
  if ((threadIdx.x & 63) == 0 && skip) atomicAdd(tallies, (unsigned long long)skip);
}

__global__ __launch_bounds__(DEP_BLOCK) void k_dep_write(VariantInputs in, const uint32_t *__restrict__ list, uint64_t n_list,
                                                         const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off,
                                                         uint64_t *pending) {
  const uint64_t x = (uint64_t)blockIdx.x * DEP_BLOCK + threadIdx.x;
  if (x >= n_list || cnt[x] == 0) return;   // (a skipped record counted nothing)
  const kslam_overlap o = in.ov[list[x]];
  DepSink<WriteEmit> sink{{pending + 2 * off[x]}};
  (void)walk_record(o, in, sink);
}

// ---- compaction ----

__global__ __launch_bounds__(DEP_BLOCK) void k_dep_reduce(const uint64_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ starts,
                                                          uint64_t n_runs, uint64_t *__restrict__ pkey, int64_t *__restrict__ pnet) {
  const uint64_t r = (uint64_t)blockIdx.x * DEP_BLOCK + threadIdx.x;
  if (r >= n_runs) return;
  const uint64_t s = starts[r], e = r + 1 < n_runs ? (uint64_t)starts[r + 1] : n;
  const uint64_t g = key[s] >> 1;
  const uint64_t split = lower_bound(key, s, e, (g << 1) | 1u);   // the begins sort first
  pkey[r] = g;
  pnet[r] = (int64_t)(split - s) - (int64_t)(e - split);
}

// threads [0, n_c): the compacted records; [n_c, n_c + n_p): the reduced pending ones.  Of equal keys the compacted one comes first.
__global__ __launch_bounds__(DEP_BLOCK) void k_dep_merge(const uint64_t *__restrict__ ckey, const int64_t *__restrict__ cnet, uint64_t n_c,
                                                         const uint64_t *__restrict__ pkey, const int64_t *__restrict__ pnet, uint64_t n_p,
                                                         uint64_t *__restrict__ mkey, int64_t *__restrict__ mnet) {
  const uint64_t t = (uint64_t)blockIdx.x * DEP_BLOCK + threadIdx.x;
  if (t >= n_c + n_p) return;
  uint64_t k, at;
  int64_t v;
  if (t < n_c) {
    k = ckey[t];
    v = cnet[t];
    at = t + lower_bound(pkey, 0, n_p, k);
  } else {
    const uint64_t r = t - n_c;
    k = pkey[r];
    v = pnet[r];
    at = r + lower_bound(ckey, 0, n_c, k + 1);   // (keys stay far below 2^64 - 1)
  }
  mkey[at] = k;
  mnet[at] = v;
}

__device__ inline int64_t merged_net(const uint64_t *__restrict__ mkey, const int64_t *__restrict__ mnet, uint64_t n, uint64_t i) {
  return mnet[i] + (i + 1 < n && mkey[i + 1] == mkey[i] ? mnet[i + 1] : 0);
}

__global__ __launch_bounds__(DEP_BLOCK) void k_dep_keep(const uint64_t *__restrict__ mkey, const int64_t *__restrict__ mnet, uint64_t n,
                                                        uint32_t *__restrict__ keep) {
  const uint64_t i = (uint64_t)blockIdx.x * DEP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const bool head = i == 0 || mkey[i] != mkey[i - 1];
  keep[i] = head && merged_net(mkey, mnet, n, i) != 0 ? 1u : 0u;
}

__global__ __launch_bounds__(DEP_BLOCK) void k_dep_scatter(const uint64_t *__restrict__ mkey, const int64_t *__restrict__ mnet, uint64_t n,
                                                           const uint32_t *__restrict__ keep, const uint32_t *__restrict__ at,
                                                           uint64_t *__restrict__ nkey, int64_t *__restrict__ nnet) {
  const uint64_t i = (uint64_t)blockIdx.x * DEP_BLOCK + threadIdx.x;
  if (i >= n || !keep[i]) return;
  nkey[at[i]] = mkey[i];
  nnet[at[i]] = merged_net(mkey, mnet, n, i);
}

// ---- take ----

__global__ __launch_bounds__(DEP_BLOCK) void k_dep_tile_sums(const int64_t *__restrict__ net, uint64_t n, int64_t *__restrict__ tile_sum) {
  __shared__ int64_t lds[DEP_BLOCK / 64];
  const uint64_t first = (uint64_t)blockIdx.x * DEP_TILE + (uint64_t)threadIdx.x * DEP_ITEMS;
  int64_t v = 0;
#pragma unroll
  for (int j = 0; j < DEP_ITEMS; j++)
    if (first + j < n) v += net[first + j];
  int64_t total;
  (void)block_scan64(v, lds, &total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one block: the tiles' sums become the sums of the tiles before each
__global__ __launch_bounds__(DEP_BLOCK) void k_dep_scan_tiles(int64_t *__restrict__ tile_sum, uint64_t n_tiles) {
  __shared__ int64_t lds[DEP_BLOCK / 64];
  int64_t carry = 0;
  for (uint64_t base = 0; base < n_tiles; base += DEP_BLOCK) {
    const uint64_t i = base + threadIdx.x;
    const int64_t v = i < n_tiles ? tile_sum[i] : 0;
    int64_t total;
    const int64_t incl = block_scan64(v, lds, &total);
    if (i < n_tiles) tile_sum[i] = carry + incl - v;
    carry += total;
  }
}

// depth[i]: the depth from boundary i up to the next one.  (A depth outside [0, 2^32 - 1] is outside the envelope; it is clamped.)
__global__ __launch_bounds__(DEP_BLOCK) void k_dep_depth(const int64_t *__restrict__ net, uint64_t n, const int64_t *__restrict__ tile_off,
                                                         uint32_t *__restrict__ depth) {
  __shared__ int64_t lds[DEP_BLOCK / 64];
  const uint64_t first = (uint64_t)blockIdx.x * DEP_TILE + (uint64_t)threadIdx.x * DEP_ITEMS;
  int64_t x[DEP_ITEMS], v = 0;
#pragma unroll
  for (int j = 0; j < DEP_ITEMS; j++) {
    x[j] = first + j < n ? net[first + j] : 0;
    v += x[j];
  }
  int64_t total;
  int64_t d = tile_off[blockIdx.x] + block_scan64(v, lds, &total) - v;
#pragma unroll
  for (int j = 0; j < DEP_ITEMS; j++) {
    d += x[j];
    if (first + j < n) depth[first + j] = d < 0 ? 0u : d > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)d;
  }
}

// the last entry whose first key is at or below `key`
__device__ inline uint64_t entry_of(const uint64_t *__restrict__ goff, uint64_t n_entries, uint64_t key) {
  uint64_t lo = 0, hi = n_entries;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (goff[mid] + mid <= key) lo = mid;
    else hi = mid;
  }
  return lo;
}

// tot[0] rows, tot[1] covered bases, tot[2] the largest depth: before the filter.  A block takes DEP_FLAG_ITEMS rounds of DEP_BLOCK
// consecutive boundaries; its three sums are combined per wavefront, then over the block's wavefronts, before ONE atomic each (a
// wavefront's own atomics on three addresses were the whole cost of the take: 3.8 M of them per address for 242 M boundaries).
__global__ __launch_bounds__(DEP_BLOCK) void k_dep_flag(const uint64_t *__restrict__ key, const uint32_t *__restrict__ depth, uint64_t n,
                                                        const uint64_t *__restrict__ goff, uint64_t n_entries, uint32_t min_depth,
                                                        uint32_t *__restrict__ keep, unsigned long long *__restrict__ tot) {
  __shared__ uint64_t lds_rows[DEP_BLOCK / 64], lds_cov[DEP_BLOCK / 64];
  __shared__ uint32_t lds_max[DEP_BLOCK / 64];
  uint64_t row = 0, covered = 0;
  uint32_t deepest = 0;
  const uint64_t first = (uint64_t)blockIdx.x * (DEP_BLOCK * DEP_FLAG_ITEMS) + threadIdx.x;
#pragma unroll 4
  for (int j = 0; j < DEP_FLAG_ITEMS; j++) {
    const uint64_t i = first + (uint64_t)j * DEP_BLOCK;
    if (i >= n) break;
    const uint32_t d = depth[i];
    bool starts = d > 0 && i + 1 < n;   // (the last boundary closes the last run: the depth behind it is 0)
    // not a continuation of the same depth within the entry (the compaction keeps no boundary without a change: for the record)
    if (starts && i > 0 && depth[i - 1] == d && entry_of(goff, n_entries, key[i - 1]) == entry_of(goff, n_entries, key[i])) starts = false;
    if (starts) {
      row++;
      covered += key[i + 1] - key[i];
      deepest = max(deepest, d);
    }
    keep[i] = starts && d >= min_depth ? 1u : 0u;
  }
  row = wave_sum(row);
  covered = wave_sum(covered);
  deepest = wave_max32(deepest);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lds_rows[wave] = row;
    lds_cov[wave] = covered;
    lds_max[wave] = deepest;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < DEP_BLOCK / 64; w++) {
      row += lds_rows[w];
      covered += lds_cov[w];
      deepest = max(deepest, lds_max[w]);
    }
    if (row) {
      atomicAdd(tot, (unsigned long long)row);
      atomicAdd(tot + 1, (unsigned long long)covered);
      atomicMax(tot + 2, (unsigned long long)deepest);
    }
  }
}

__global__ __launch_bounds__(DEP_BLOCK) void k_dep_rows(const uint64_t *__restrict__ key, const uint32_t *__restrict__ depth, uint64_t n,
                                                        const uint32_t *__restrict__ keep, const uint32_t *__restrict__ at,
                                                        const uint64_t *__restrict__ goff, uint64_t n_entries, kslam_depth_row *__restrict__ rows) {
  const uint64_t i = (uint64_t)blockIdx.x * DEP_BLOCK + threadIdx.x;
  if (i + 1 >= n || !keep[i]) return;
  const uint64_t e = entry_of(goff, n_entries, key[i]), base = goff[e] + e;
  kslam_depth_row out;
  out.entry = (uint32_t)e;
  out.start = (uint32_t)(key[i] - base);
  out.end = (uint32_t)(key[i + 1] - base);
  out.depth = depth[i];
  rows[at[i]] = out;
}

}  // namespace

void depth_count_device(const VariantInputs &in, EmitWork &W, hipStream_t s) { emit_count_device(in, W, 1, k_dep_count, s); }

void depth_write_device(const VariantInputs &in, EmitWork &W, uint64_t *d_pending, hipStream_t s) { emit_write_device(in, W, k_dep_write, d_pending, s); }

void depth_compact_device(DepthWork &T, DevBuf &pending, uint64_t n_pend, DevBuf &ckey, DevBuf &cnet, uint64_t *n_keys, uint64_t max_key, hipStream_t s) {
  if (!n_pend) return;
  if (n_pend > 0xFFFFFFFFull) throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^32 - 1 pending depth keys in one sort"};
  const uint64_t n_c = *n_keys;
  T.alt.ensure(pending.cap);
  sort_keys(pending, T.alt, n_pend, (max_key << 1) | 1u, T.sortws, s);
  const uint64_t *key = pending.as<uint64_t>();
  T.head.ensure(n_pend * sizeof(uint32_t));
  T.run.ensure(n_pend * sizeof(uint32_t));
  T.scan_tmp.ensure(scan_tmp_bytes(std::max(n_pend, n_c + n_pend)));
  T.totals.ensure(4 * sizeof(uint64_t));
  uint64_t *d_tot = T.totals.as<uint64_t>();
  run_heads_device(key, n_pend, T.head.as<uint32_t>(), s);
  exclusive_scan_u32(T.head.as<uint32_t>(), T.run.as<uint32_t>(), n_pend, d_tot, T.scan_tmp.p, s);
  uint64_t n_p = 0;
  read_back(&n_p, d_tot, sizeof n_p, s);
  const uint64_t n_m = n_c + n_p;
  // (up to here only the ORDER of the pending keys has changed)
  if (n_m > 0xFFFFFFFFull) throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^32 - 1 depth boundaries in one merge"};
  T.starts.ensure(n_p * sizeof(uint32_t));
  T.pkey.ensure(n_p * sizeof(uint64_t));
  T.pnet.ensure(n_p * sizeof(int64_t));
  T.mkey.ensure(n_m * sizeof(uint64_t));
  T.mnet.ensure(n_m * sizeof(int64_t));
  T.keep.ensure(n_m * sizeof(uint32_t));
  T.at.ensure(n_m * sizeof(uint32_t));
  run_starts_device(T.head.as<uint32_t>(), T.run.as<uint32_t>(), n_pend, T.starts.as<uint32_t>(), s);
  hipLaunchKernelGGL(k_dep_reduce, dim3(pileup_blocks(n_p)), dim3(DEP_BLOCK), 0, s, key, n_pend, T.starts.as<uint32_t>(), n_p, T.pkey.as<uint64_t>(),
                     T.pnet.as<int64_t>());
  hipLaunchKernelGGL(k_dep_merge, dim3(pileup_blocks(n_m)), dim3(DEP_BLOCK), 0, s, ckey.as<uint64_t>(), cnet.as<int64_t>(), n_c, T.pkey.as<uint64_t>(),
                     T.pnet.as<int64_t>(), n_p, T.mkey.as<uint64_t>(), T.mnet.as<int64_t>());
  hipLaunchKernelGGL(k_dep_keep, dim3(pileup_blocks(n_m)), dim3(DEP_BLOCK), 0, s, T.mkey.as<uint64_t>(), T.mnet.as<int64_t>(), n_m, T.keep.as<uint32_t>());
  HIPCHK(hipGetLastError());
  exclusive_scan_u32(T.keep.as<uint32_t>(), T.at.as<uint32_t>(), n_m, d_tot + 1, T.scan_tmp.p, s);
  uint64_t n_new = 0;
  read_back(&n_new, d_tot + 1, sizeof n_new, s);
  T.nkey.ensure((n_new + 1) * sizeof(uint64_t));
  T.nnet.ensure((n_new + 1) * sizeof(int64_t));
  if (n_new)
    hipLaunchKernelGGL(k_dep_scatter, dim3(pileup_blocks(n_m)), dim3(DEP_BLOCK), 0, s, T.mkey.as<uint64_t>(), T.mnet.as<int64_t>(), n_m, T.keep.as<uint32_t>(),
                       T.at.as<uint32_t>(), T.nkey.as<uint64_t>(), T.nnet.as<int64_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(stream_wait(s));
  std::swap(ckey, T.nkey);
  std::swap(cnet, T.nnet);
  *n_keys = n_new;
}

void depth_take_device(DepthWork &T, const uint64_t *d_ckey, const int64_t *d_cnet, uint64_t n, const uint64_t *d_goff, uint64_t n_entries,
                       uint32_t min_depth, uint64_t out[4], hipStream_t s) {
  out[0] = out[1] = out[2] = out[3] = 0;
  if (n < 2) return;   // (one boundary alone cannot be: every begin has its end)
  const uint64_t n_tiles = (n + DEP_TILE - 1) / DEP_TILE;
  T.tile_sum.ensure(n_tiles * sizeof(int64_t));
  T.depth.ensure(n * sizeof(uint32_t));
  T.keep.ensure(n * sizeof(uint32_t));
  T.at.ensure(n * sizeof(uint32_t));
  T.scan_tmp.ensure(scan_tmp_bytes(n));
  T.totals.ensure(4 * sizeof(uint64_t));
  uint64_t *d_tot = T.totals.as<uint64_t>();
  HIPCHK(hipMemsetAsync(d_tot, 0, 4 * sizeof(uint64_t), s));
  hipLaunchKernelGGL(k_dep_tile_sums, dim3((unsigned)n_tiles), dim3(DEP_BLOCK), 0, s, d_cnet, n, T.tile_sum.as<int64_t>());
  hipLaunchKernelGGL(k_dep_scan_tiles, dim3(1), dim3(DEP_BLOCK), 0, s, T.tile_sum.as<int64_t>(), n_tiles);
  hipLaunchKernelGGL(k_dep_depth, dim3((unsigned)n_tiles), dim3(DEP_BLOCK), 0, s, d_cnet, n, T.tile_sum.as<int64_t>(), T.depth.as<uint32_t>());
  hipLaunchKernelGGL(k_dep_flag, dim3((unsigned)((n + DEP_BLOCK * DEP_FLAG_ITEMS - 1) / (DEP_BLOCK * DEP_FLAG_ITEMS))), dim3(DEP_BLOCK), 0, s, d_ckey, T.depth.as<uint32_t>(), n, d_goff, n_entries,
                     min_depth ? min_depth : 1u, T.keep.as<uint32_t>(), reinterpret_cast<unsigned long long *>(d_tot));
  HIPCHK(hipGetLastError());
  exclusive_scan_u32(T.keep.as<uint32_t>(), T.at.as<uint32_t>(), n, d_tot + 3, T.scan_tmp.p, s);
  read_back(out, d_tot, 4 * sizeof(uint64_t), s);
  if (!out[3]) return;
  T.rows.ensure(out[3] * sizeof(kslam_depth_row));
  hipLaunchKernelGGL(k_dep_rows, dim3(pileup_blocks(n)), dim3(DEP_BLOCK), 0, s, d_ckey, T.depth.as<uint32_t>(), n, T.keep.as<uint32_t>(), T.at.as<uint32_t>(),
                     d_goff, n_entries, T.rows.as<kslam_depth_row>());
  HIPCHK(hipGetLastError());
}

}  // namespace kslam
