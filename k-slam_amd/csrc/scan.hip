// scan.hip -- device-wide exclusive scan (plumbing for the join / dedupe /
// cigar-pool layout).  Three launches: tile sums, scan of the tile sums by one
// workgroup, tile-local scan + tile prefix.  Everything is HBM-streaming:
// 4 B read + 4/8 B written per element, plus a second 4 B read.
// Also the partition by bin and the sweep over growing bin lists that the SW
// tiers and the CIGAR bins share (common.h: BinLists).
#include "common.h"

namespace kslam {

namespace {
constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;

__device__ inline uint64_t wave_incl_scan_u64(uint64_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint64_t t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// block-wide exclusive scan of one u64 per thread; returns exclusive prefix,
// total in *total (all threads)
__device__ inline uint64_t block_excl_scan(uint64_t v, uint64_t *total, uint64_t *sm /*[5]*/) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t inc = wave_incl_scan_u64(v);
  if (lane == 63) sm[w] = inc;
  __syncthreads();
  uint64_t base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < SCAN_BLOCK / 64; i++) {
    uint64_t x = sm[i];
    if (i < w) base += x;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_tile_sums(const uint32_t *in, uint64_t n,
                                                          uint64_t *tile_sum) {
  __shared__ uint64_t sm[8];
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) {
    uint64_t idx = base + (uint64_t)i * SCAN_BLOCK + threadIdx.x;
    if (idx < n) acc += in[idx];
  }
  uint64_t tot;
  block_excl_scan(acc, &tot, sm);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_tile_sums(uint64_t *tile_sum, uint64_t n_tiles,
                                                               uint64_t *total_out) {
  __shared__ uint64_t sm[8];
  uint64_t carry = 0;
  for (uint64_t base = 0; base < n_tiles; base += SCAN_BLOCK) {
    uint64_t idx = base + threadIdx.x;
    uint64_t v = idx < n_tiles ? tile_sum[idx] : 0;
    uint64_t tot;
    uint64_t ex = block_excl_scan(v, &tot, sm);
    if (idx < n_tiles) tile_sum[idx] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0 && total_out) *total_out = carry;
}

// Tile-local scan + tile prefix.  A thread takes FOUR consecutive elements per round (one 16-byte load; a wave's loads and
// stores are then contiguous) over four rounds of 1 024 elements, instead of sixteen consecutive elements of its own
// (64-byte stride between lanes: every line fetched in four pieces, 1.45 TB/s); the block scan runs once per round with
// the carry of the rounds before it.
template <typename OutT>
__global__ __launch_bounds__(SCAN_BLOCK) void k_tile_scan(const uint32_t *in, OutT *out, uint64_t n,
                                                          const uint64_t *tile_prefix) {
  __shared__ uint64_t sm[8];
  constexpr int ROUNDS = SCAN_ITEMS / 4;
  const uint64_t tile = (uint64_t)blockIdx.x * SCAN_TILE;
  uint32_t v[ROUNDS][4];
  const bool in16 = (reinterpret_cast<uintptr_t>(in) & 15u) == 0, out16 = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
#pragma unroll
  for (int r = 0; r < ROUNDS; r++) {
    const uint64_t idx = tile + (uint64_t)r * (SCAN_BLOCK * 4) + (uint64_t)threadIdx.x * 4;
    if (idx + 4 <= n && in16) {
      const uint4 q = *reinterpret_cast<const uint4 *>(in + idx);   // (tile and thread offsets are multiples of 4 elements)
      v[r][0] = q.x; v[r][1] = q.y; v[r][2] = q.z; v[r][3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) v[r][j] = idx + j < n ? in[idx + j] : 0;
    }
  }
  uint64_t carry = tile_prefix[blockIdx.x];
#pragma unroll
  for (int r = 0; r < ROUNDS; r++) {
    const uint64_t mine = (uint64_t)v[r][0] + v[r][1] + v[r][2] + v[r][3];
    uint64_t tot;
    uint64_t ex = block_excl_scan(mine, &tot, sm) + carry;
    carry += tot;
    const uint64_t idx = tile + (uint64_t)r * (SCAN_BLOCK * 4) + (uint64_t)threadIdx.x * 4;
    OutT o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      o[j] = (OutT)ex;
      ex += v[r][j];
    }
    if (idx + 4 <= n && out16) {
      if (sizeof(OutT) == 4) {
        *reinterpret_cast<uint4 *>(out + idx) = make_uint4((uint32_t)o[0], (uint32_t)o[1], (uint32_t)o[2], (uint32_t)o[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) out[idx + j] = o[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (idx + j < n) out[idx + j] = o[j];
    }
  }
}

template <typename OutT>
void scan_impl(const uint32_t *d_in, OutT *d_out, uint64_t n, uint64_t *d_total, void *d_tmp,
               hipStream_t s) {
  uint64_t *tile_sum = reinterpret_cast<uint64_t *>(d_tmp);
  if (n == 0) {
    if (d_total) HIPCHK(hipMemsetAsync(d_total, 0, sizeof(uint64_t), s));
    return;
  }
  uint64_t n_tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
  hipLaunchKernelGGL(k_tile_sums, dim3((unsigned)n_tiles), dim3(SCAN_BLOCK), 0, s, d_in, n, tile_sum);
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(SCAN_BLOCK), 0, s, tile_sum, n_tiles, d_total);
  hipLaunchKernelGGL(k_tile_scan<OutT>, dim3((unsigned)n_tiles), dim3(SCAN_BLOCK), 0, s, d_in, d_out, n,
                     tile_sum);
  HIPCHK(hipGetLastError());
}

// partition_bins: the NT-way stable partition of the element numbers by bin: per-block counts, one small scan,
// then a scatter that ranks within the block by ballots.
constexpr int TIER_ITEMS = 4096;   // elements per block
constexpr int NT = 8;              // bins
__global__ __launch_bounds__(256) void k_tier_hist(const uint8_t *__restrict__ tier, uint64_t n,
                                                   uint32_t *__restrict__ block_hist, uint32_t n_blocks) {
  __shared__ uint32_t h[NT];
  if (threadIdx.x < NT) h[threadIdx.x] = 0;
  __syncthreads();
  uint32_t c[NT] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint64_t base = (uint64_t)blockIdx.x * TIER_ITEMS;
  for (uint32_t k = threadIdx.x; k < TIER_ITEMS; k += 256) {
    const uint64_t i = base + k;
    if (i < n && tier[i] < NT) c[tier[i]]++;
  }
#pragma unroll
  for (int k = 0; k < NT; k++) {
    uint32_t v = c[k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&h[k], v);
  }
  __syncthreads();
  if (threadIdx.x < NT) block_hist[threadIdx.x * n_blocks + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of block_hist per tier (each tier's list starts at 0); totals[k] = tier size
__global__ __launch_bounds__(1024) void k_tier_scan(uint32_t *__restrict__ block_hist, uint32_t n_blocks,
                                                    uint32_t *__restrict__ totals) {
  __shared__ uint32_t part[1024];
  const uint32_t k = blockIdx.x;   // tier
  uint32_t *a = block_hist + (size_t)k * n_blocks;
  const uint32_t per = (n_blocks + 1023) / 1024;
  const uint32_t lo = min(n_blocks, threadIdx.x * per), hi = min(n_blocks, lo + per);
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; i++) sum += a[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (uint32_t i = 0; i < 1024; i++) {
      const uint32_t v = part[i];
      part[i] = run;
      run += v;
    }
    totals[k] = run;
  }
  __syncthreads();
  uint32_t run = part[threadIdx.x];
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t v = a[i];
    a[i] = run;
    run += v;
  }
}

__global__ __launch_bounds__(256) void k_tier_scatter(const uint8_t *__restrict__ tier, uint64_t n,
                                                      const uint32_t *__restrict__ block_hist, uint32_t n_blocks,
                                                      BinLists out) {
  __shared__ uint32_t base[NT];      // running position of each tier inside this block
  __shared__ uint32_t wave_cnt[NT][4];
  if (threadIdx.x < NT) base[threadIdx.x] = block_hist[threadIdx.x * n_blocks + blockIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t b0 = (uint64_t)blockIdx.x * TIER_ITEMS;
  for (uint32_t r = 0; r < TIER_ITEMS / 256; r++) {
    const uint64_t i = b0 + (uint64_t)r * 256 + threadIdx.x;
    const int tk = (i < n && tier[i] < NT) ? (int)tier[i] : -1;   // bins >= NT: not listed
    uint32_t rank = 0;
#pragma unroll
    for (int k = 0; k < NT; k++) {
      const uint64_t m = __ballot(tk == k);
      if (tk == k) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wave_cnt[k][wv] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (tk >= 0) {
      uint32_t off = base[tk] + rank;
      for (uint32_t w = 0; w < wv; w++) off += wave_cnt[tk][w];
      out.list[tk][off] = (uint32_t)i;
    }
    __syncthreads();
    if (threadIdx.x < NT)
      base[threadIdx.x] += wave_cnt[threadIdx.x][0] + wave_cnt[threadIdx.x][1] + wave_cnt[threadIdx.x][2] +
                           wave_cnt[threadIdx.x][3];
    __syncthreads();
  }
}
}  // namespace

size_t scan_tmp_bytes(uint64_t n) { return ((n + SCAN_TILE - 1) / SCAN_TILE + 1) * sizeof(uint64_t); }

void exclusive_scan_u32(const uint32_t *d_in, uint32_t *d_out, uint64_t n, uint64_t *d_total,
                        void *d_tmp, hipStream_t s) {
  scan_impl<uint32_t>(d_in, d_out, n, d_total, d_tmp, s);
}
void exclusive_scan_u32_to_u64(const uint32_t *d_in, uint64_t *d_out, uint64_t n, uint64_t *d_total,
                               void *d_tmp, hipStream_t s) {
  scan_impl<uint64_t>(d_in, d_out, n, d_total, d_tmp, s);
}

void partition_bins(const uint8_t *d_bins, uint64_t n, const BinLists &B, DevBuf &pos, hipStream_t s) {
  if (n == 0) return;
  const uint32_t n_blocks = (uint32_t)((n + TIER_ITEMS - 1) / TIER_ITEMS);
  pos.ensure((size_t)NT * n_blocks * sizeof(uint32_t));
  hipLaunchKernelGGL(k_tier_hist, dim3(n_blocks), dim3(256), 0, s, d_bins, n, pos.as<uint32_t>(), n_blocks);
  hipLaunchKernelGGL(k_tier_scan, dim3(NT), dim3(1024), 0, s, pos.as<uint32_t>(), n_blocks, B.count);
  hipLaunchKernelGGL(k_tier_scatter, dim3(n_blocks), dim3(256), 0, s, d_bins, n, pos.as<uint32_t>(), n_blocks, B);
  HIPCHK(hipGetLastError());
}

void sweep_lists(uint32_t n_bins, const uint32_t *d_counts, uint32_t *h, size_t h_bytes, const uint64_t *first_cap, bool step,
                 const SweepLaunch &launch, const std::function<bool(int round)> &round_hook, hipStream_t s) {
  uint32_t done[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // entries of each list some launch covers (clamped to its length)
  if (!step)
    for (uint32_t b = 0; b < n_bins; b++) {
      if (!first_cap[b]) continue;
      launch(b, first_cap[b], 0, d_counts + b, h[b], -1);
      done[b] = (uint32_t)first_cap[b];
    }
  for (int round = 0;; round++) {
    if (round || !step) read_back(h, d_counts, h_bytes, s);
    for (uint32_t b = 0; b < n_bins; b++) done[b] = std::min(done[b], h[b]);
    bool progressed = round_hook && round_hook(round);
    for (uint32_t b = 0; b < n_bins; b++) {
      if (h[b] <= done[b]) continue;
      launch(b, h[b] - done[b], done[b], nullptr, 0, round);
      done[b] = h[b];
      progressed = true;
      if (step) read_back(h, d_counts, h_bytes, s);
    }
    if (!progressed) break;
  }
}

}  // namespace kslam
