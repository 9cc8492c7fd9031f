// bamsort.hip -- the coordinate-sorted BAM and its BAI index on the device (include/kslam_bamsort.h): what lies between the
// BAM records the lanes write (samtext.hip, samunmapped.hip) and the compressor (bgzf.hip).
//   1. k_bs_count / k_bs_write   the record index of a batch: one thread per segment (a read pair's rows, an unmapped row, or a
//                                stretch of kslam_bam_sort_add's records) walks its block_size chain, counts, and after a scan
//                                writes per record its offset, its length and what the sort and the index need of it
//   2. k_bs_keys / k_bs_order    one 4-word sort record per record for radix_sort.hip, and the sorted order's sources
//   3. k_bs_gather               the hot path: a permutation of the whole run's records.  Records are 100-600 bytes at any
//                                source and destination alignment: a group of 16 lanes (4 records per wavefront) or a wavefront
//                                moves one record as aligned 16-byte stores fed by 16-byte loads at whatever alignment the source
//                                has, with a byte head and tail (readsplit.hip's streaming copy).  The instantiation with one
//                                lane per record is the measured baseline.  2 bytes of traffic per byte, 16 bytes of index per record.
//   4. k_bs_index / k_bs_runs    over the sorted order: virtual offsets from the members' compressed sizes, the linear index by
//                                64-bit atomic min per window (order-independent), per-reference counters, and the heads of
//                                the runs of equal (ref, bin), compacted after a scan
#include "bamsort.h"

namespace kslam {

namespace {

struct __attribute__((packed, aligned(1))) BsBytes16 {
  uint32_t w[4];
};

__device__ inline uint32_t ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
__device__ inline uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

__device__ inline void segment_of(const uint64_t *__restrict__ seg_off, uint64_t n_seg, uint64_t base, uint64_t end, uint64_t i, uint64_t *p, uint64_t *e) {
  *p = base + seg_off[i];
  *e = i + 1 < n_seg ? base + seg_off[i + 1] : end;
}

__global__ __launch_bounds__(256) void k_bs_count(const uint8_t *__restrict__ data, const uint64_t *__restrict__ seg_off, uint64_t n_seg, uint64_t base,
                                                  uint64_t end, uint32_t *__restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_seg) return;
  uint64_t p, e;
  segment_of(seg_off, n_seg, base, end, i, &p, &e);
  uint32_t n = 0;
  while (p + 4 <= e) {
    const uint64_t len = 4 + (uint64_t)ld32(data + p);
    if (len > e - p) break;   // (a chain that leaves its segment: never from the library's writers, refused on the host for the others)
    p += len;
    n++;
  }
  cnt[i] = n;
}

__global__ __launch_bounds__(256) void k_bs_write(const uint8_t *__restrict__ data, const uint64_t *__restrict__ seg_off, uint64_t n_seg, uint64_t base,
                                                  uint64_t end, const uint32_t *__restrict__ first, uint32_t n_ref, BamSortCols cols) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_seg) return;
  uint64_t p, e;
  segment_of(seg_off, n_seg, base, end, i, &p, &e);
  uint64_t k = first[i];
  while (p + 4 <= e) {
    const uint64_t len = 4 + (uint64_t)ld32(data + p);
    if (len > e - p) break;
    uint32_t ref = n_ref, pos1 = 0, meta = 1;
    if (len >= 36) {
      const uint8_t *r = data + p + 4;
      const uint32_t id = ld32(r), l_name = r[8], n_cig = ld16(r + 12), flag = ld16(r + 14);
      ref = id < n_ref ? id : n_ref;
      pos1 = ld32(r + 4) + 1u;
      uint64_t reflen = 0;
      if (!(flag & 4u) && 36ull + l_name + 4ull * n_cig <= len)
        for (uint32_t c = 0; c < n_cig; c++) {
          const uint32_t w = ld32(r + 32 + l_name + 4 * c), op = w & 15u;
          if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += w >> 4;
        }
      if (reflen < 1) reflen = 1;
      if (reflen > (1ull << 29)) reflen = 1ull << 29;
      meta = (uint32_t)reflen | ((flag & 4u) ? BAMSORT_UNMAPPED : 0u);
    }
    cols.off[k] = p;
    cols.len[k] = (uint32_t)len;
    cols.ref[k] = ref;
    cols.pos1[k] = pos1;
    cols.meta[k] = meta;
    p += len;
    k++;
  }
}

__global__ __launch_bounds__(256) void k_bs_keys(BamSortCols cols, const uint8_t *bytes, uint64_t n, uint64_t at, uint4 *__restrict__ keys,
                                                 uint64_t *__restrict__ src, uint32_t *__restrict__ len, uint32_t *__restrict__ meta) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[at + i] = make_uint4(cols.pos1[i], cols.ref[i], (uint32_t)(at + i), 0u);
  src[at + i] = (uint64_t)reinterpret_cast<uintptr_t>(bytes + cols.off[i]);
  len[at + i] = cols.len[i];
  meta[at + i] = cols.meta[i];
}

__global__ __launch_bounds__(256) void k_bs_order(const uint4 *__restrict__ keys, const uint64_t *__restrict__ src, const uint32_t *__restrict__ len,
                                                  uint64_t n, uint64_t *__restrict__ s_src, uint32_t *__restrict__ s_len) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = keys[i].z;
  s_src[i] = src[k];
  s_len[i] = len[k];
}

__global__ void k_bs_range(const uint64_t *__restrict__ dst_off, uint64_t n, uint64_t a, uint64_t b, uint64_t *__restrict__ range) {
  if (blockIdx.x || threadIdx.x) return;
  uint64_t lo = 0, hi = n;   // the first i with dst_off[i + 1] > a
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (dst_off[mid + 1] > a) hi = mid; else lo = mid + 1;
  }
  range[0] = lo;
  lo = 0, hi = n;            // the first i with dst_off[i] >= b
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (dst_off[mid] >= b) hi = mid; else lo = mid + 1;
  }
  range[1] = lo;
}

// n bytes from src to dst by the G lanes of a group: a byte head up to dst's 16-byte boundary, 16-byte pieces (aligned stores;
// the loads take the source as it lies), a byte tail.  Reads and writes [0, n) only.
template <int G>
__device__ inline void copy_span(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t lane) {
  const uint64_t to_boundary = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
  const uint64_t head = n < to_boundary ? n : to_boundary;
  for (uint64_t b = lane; b < head; b += G) dst[b] = src[b];
  dst += head; src += head; n -= head;
  const uint64_t pieces = n >> 4;
  for (uint64_t p = lane; p < pieces; p += G) {
    const BsBytes16 v = *reinterpret_cast<const BsBytes16 *>(src + 16 * p);
    *reinterpret_cast<uint4 *>(dst + 16 * p) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
  }
  const uint64_t tail = n & 15u;
  for (uint64_t b = lane; b < tail; b += G) dst[16 * pieces + b] = src[16 * pieces + b];
}

template <int G>
__global__ __launch_bounds__(256) void k_bs_gather(const uint64_t *__restrict__ s_src, const uint64_t *__restrict__ dst_off, uint64_t i0, uint64_t i1,
                                                   uint64_t a, uint64_t b, uint8_t *__restrict__ out) {
  const uint64_t r = i0 + ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
  const uint32_t lane = threadIdx.x % G;
  if (r >= i1) return;
  const uint64_t o = dst_off[r], o1 = dst_off[r + 1];
  const uint64_t lo = o > a ? o : a, hi = o1 < b ? o1 : b;   // the slice's part of the record
  if (lo >= hi) return;
  const uint8_t *src = reinterpret_cast<const uint8_t *>((uintptr_t)s_src[r]);
  copy_span<G>(out + (lo - a), src + (lo - o), hi - lo, lane);
}

__device__ inline uint32_t reg2bin(uint64_t beg, uint64_t end) {
  end--;
  if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
  return 0;
}

__device__ inline uint64_t voff_at(const BamSortIndexIn &in, uint64_t o) {
  if (o >= in.total) return (in.header_clen + in.member_off[in.n_members]) << 16;   // the EOF member
  const uint64_t m = o / BGZF_MEMBER_IN;
  return (in.header_clen + in.member_off[m]) << 16 | (o % BGZF_MEMBER_IN);
}

__device__ inline uint32_t bin_of(const BamSortIndexIn &in, const uint4 k) {
  if (k.y >= in.n_ref || k.x == 0) return BAMSORT_NO_BIN;
  const uint64_t beg = k.x - 1u, span = in.meta[k.z] & ~BAMSORT_UNMAPPED;
  return reg2bin(beg, beg + span);
}

__global__ __launch_bounds__(256) void k_bs_index(BamSortIndexIn in, BamSortIndexOut out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= in.n) return;
  const uint4 k = in.keys[i];
  const uint32_t ref = k.y, bin = bin_of(in, k);
  uint4 kp = k;
  if (i) kp = in.keys[i - 1];
  out.head[i] = !i || kp.y != ref || bin_of(in, kp) != bin;
  if (ref >= in.n_ref) {
    if (!i || kp.y < in.n_ref) *out.first_no_coor = i;
    return;
  }
  const uint64_t sv = voff_at(in, in.dst_off[i]);
  if (!i || kp.y != ref) out.ref_first[ref] = sv;
  if (i + 1 == in.n || in.keys[i + 1].y != ref) out.ref_last[ref] = voff_at(in, in.dst_off[i + 1]);
  const uint32_t m = in.meta[k.z];
  atomicAdd((unsigned long long *)((m & BAMSORT_UNMAPPED) ? out.ref_unmapped : out.ref_mapped) + ref, 1ull);
  if (k.x == 0) return;
  const uint64_t w0 = in.win_off[ref], n_win = in.win_off[ref + 1] - w0;
  const uint64_t beg = k.x - 1u;
  uint64_t end = beg + (m & ~BAMSORT_UNMAPPED);
  if (end > n_win << 14) end = n_win << 14;   // (a record past its entry's end: refused before it gets here)
  if (end <= beg) return;
  atomicMax((unsigned long long *)out.ref_max_end + ref, (unsigned long long)end);
  for (uint64_t w = beg >> 14; w <= (end - 1) >> 14; w++) atomicMin((unsigned long long *)out.win + w0 + w, (unsigned long long)sv);
}

__global__ __launch_bounds__(256) void k_bs_runs(BamSortIndexIn in, const uint32_t *__restrict__ head, const uint32_t *__restrict__ run_at,
                                                 BamSortRun *__restrict__ runs) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= in.n || !head[i]) return;
  const uint4 k = in.keys[i];
  runs[run_at[i]] = BamSortRun{k.y < in.n_ref ? k.y : in.n_ref, bin_of(in, k), voff_at(in, in.dst_off[i])};
}

inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void bamsort_count_device(const uint8_t *data, const uint64_t *seg_off, uint64_t n_seg, uint64_t base, uint64_t end, uint32_t *cnt, hipStream_t s) {
  if (!n_seg) return;
  hipLaunchKernelGGL(k_bs_count, dim3(blocks_of(n_seg)), dim3(256), 0, s, data, seg_off, n_seg, base, end, cnt);
  HIPCHK(hipGetLastError());
}

void bamsort_write_device(const uint8_t *data, const uint64_t *seg_off, uint64_t n_seg, uint64_t base, uint64_t end, const uint32_t *first,
                          uint32_t n_ref, BamSortCols cols, hipStream_t s) {
  if (!n_seg) return;
  hipLaunchKernelGGL(k_bs_write, dim3(blocks_of(n_seg)), dim3(256), 0, s, data, seg_off, n_seg, base, end, first, n_ref, cols);
  HIPCHK(hipGetLastError());
}

void bamsort_keys_device(BamSortCols cols, const uint8_t *bytes, uint64_t n, uint64_t at, uint4 *keys, uint64_t *src, uint32_t *len, uint32_t *meta,
                         hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_bs_keys, dim3(blocks_of(n)), dim3(256), 0, s, cols, bytes, n, at, keys, src, len, meta);
  HIPCHK(hipGetLastError());
}

void bamsort_order_device(const uint4 *keys, const uint64_t *src, const uint32_t *len, uint64_t n, uint64_t *s_src, uint32_t *s_len, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_bs_order, dim3(blocks_of(n)), dim3(256), 0, s, keys, src, len, n, s_src, s_len);
  HIPCHK(hipGetLastError());
}

void bamsort_range_device(const uint64_t *dst_off, uint64_t n, uint64_t a, uint64_t b, uint64_t *range, hipStream_t s) {
  hipLaunchKernelGGL(k_bs_range, dim3(1), dim3(64), 0, s, dst_off, n, a, b, range);
  HIPCHK(hipGetLastError());
}

void bamsort_gather_device(const uint64_t *s_src, const uint64_t *dst_off, uint64_t i0, uint64_t i1, uint64_t a, uint64_t b, uint8_t *out, uint32_t lanes,
                           hipStream_t s) {
  if (i1 <= i0) return;
  const uint64_t n = i1 - i0;
  if (lanes == 1) hipLaunchKernelGGL(k_bs_gather<1>, dim3(blocks_of(n)), dim3(256), 0, s, s_src, dst_off, i0, i1, a, b, out);
  else if (lanes == 64) hipLaunchKernelGGL(k_bs_gather<64>, dim3(blocks_of(n * 64)), dim3(256), 0, s, s_src, dst_off, i0, i1, a, b, out);
  else hipLaunchKernelGGL(k_bs_gather<16>, dim3(blocks_of(n * 16)), dim3(256), 0, s, s_src, dst_off, i0, i1, a, b, out);
  HIPCHK(hipGetLastError());
}

void bamsort_index_device(const BamSortIndexIn &in, const BamSortIndexOut &out, hipStream_t s) {
  if (!in.n) return;
  hipLaunchKernelGGL(k_bs_index, dim3(blocks_of(in.n)), dim3(256), 0, s, in, out);
  HIPCHK(hipGetLastError());
}

void bamsort_runs_device(const BamSortIndexIn &in, const uint32_t *head, const uint32_t *run_at, BamSortRun *runs, hipStream_t s) {
  if (!in.n) return;
  hipLaunchKernelGGL(k_bs_runs, dim3(blocks_of(in.n)), dim3(256), 0, s, in, head, run_at, runs);
  HIPCHK(hipGetLastError());
}

}  // namespace kslam
