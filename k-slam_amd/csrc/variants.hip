// variants.hip -- the SNV table, piled up on the device (include/kslam_variants.h).
//
// When a lane has finished a batch, its final read pairs, their alignment-pair records, the overlap records those index, the
// CIGAR pool, the read bases and the entry bases lie in device memory.  A dense per-base allele array would cost four counters
// per base of the index (80 GB for 5 Gb), so the pileup is sparse: only what differs is recorded, plus the intervals that are
// covered.  The state is three append-only arrays of 8-byte keys whose numeric order is the rows' order:
//   events   (g << 3) | (alt << 1) | strand     g = g_off[entry] + pos, alt 0..3 = A C G T
//   begins   g of the first column of an M run
//   ends     g of its last column
// Per batch (variants_count_device, variants_write_device):
//   1. k_var_flag    one thread per alignment-pair RECORD, as coverage.hip's mark pass: its group by binary search, live iff it
//                    lies below first + count; a live record stores 1 at the overlap records it names (the same value from every
//                    thread: no atomic, and a record named three times is listed once)
//   2. scan + k_var_list   the marked overlap records as a list
//   3. k_var_walk<CountSink>   one thread per listed record: the CIGAR is checked whole against the read and the entry, then
//                    walked; events and intervals are counted
//   4. two scans     lay out the slots
//   5. the caller makes room (api_variants.hip: under the state's lock, so that appends from several lanes take their turns)
//   6. k_var_walk<WriteSink>   the same walk function writes the keys
// The walk is details.hip's: ONE loop over 16-column chunks whatever CIGAR operation a chunk belongs to (the lanes of a wave walk
// different CIGARs), one unaligned 16-byte load per chunk and stream; it carries no qualities, no probability chain and no MD
// bookkeeping, and it looks at the alphabet only on the columns that differ.
// On request (variants_take_device): radix_sort of the three arrays, run heads over the events ignoring the strand bit, a scan
// that numbers the runs, one thread per RUN that finds the strand split inside its run by binary search (a run of any length
// costs its thread ~log2 steps: no tile, no atomic, so one hot site is no slower than many cold ones), the depth of the sites
// that passed min_alt by two binary searches over the sorted interval keys, a scan of the keep flags and a compaction that
// resolves entry / pos / ref from the index.
// Bounds: a record is walked only after entry < n_entries, read < n_reads, its CIGAR slice inside the pool and every M, I and
// D run inside the read and the entry held; a 16-byte load may run up to 15 bytes past the last base of the arrays, inside the
// slack every DevBuf has, and those bytes are masked out; a load that would begin before the read array is done bytewise.
#include "common.h"
#include "../../include/kslam_variants.h"

namespace kslam {

namespace {

constexpr int VAR_BLOCK = 256;

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

__device__ inline uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

struct CountSink {
  uint32_t n_ev = 0, n_iv = 0;
  __device__ void event(uint64_t) { n_ev++; }
  __device__ void interval(uint64_t, uint64_t) { n_iv++; }
};
struct WriteSink {
  uint64_t *ev, *ib, *ie;
  __device__ void event(uint64_t key) { *ev++ = key; }
  __device__ void interval(uint64_t b, uint64_t e) { *ib++ = b; *ie++ = e; }
};

// false: the record is skipped (nothing was handed to the sink)
template <class Sink>
__device__ inline bool var_walk(const kslam_overlap &o, const VariantInputs &in, Sink &sink) {
  if (o.entry >= in.n_entries || o.cigar_len == 0 || o.ref_begin < 0) return false;
  // (kslam_variants_add refuses these before anything is launched, and a lane's records do not have them)
  if (o.read >= in.n_reads || o.cigar_off > in.n_cig || o.cigar_len > in.n_cig - o.cigar_off) return false;
  const uint64_t rb = in.roff[o.read];
  const int64_t L = (int64_t)(in.roff[o.read + 1] - rb);
  const uint64_t gb = in.goff[o.entry];
  const int64_t ref_len = (int64_t)(in.goff[o.entry + 1] - gb);
  const uint32_t *__restrict__ cig = in.pool + o.cigar_off;
  const int64_t q0 = o.query_begin > 0 ? o.query_begin : 0;
  {   // the whole CIGAR against the read and the entry, before anything is emitted
    int64_t rp = o.ref_begin, qp = q0;
    for (uint32_t k = 0; k < o.cigar_len; k++) {
      const uint32_t c = cig[k], op = c & 15u;
      const int64_t len = c >> 4;
      if (op == 0) {
        if (rp + len > ref_len || qp + len > L) return false;
        rp += len;
        qp += len;
      } else if (op == 1) {
        if (qp + len > L) return false;
        qp += len;
      } else if (op == 2) {
        if (rp + len > ref_len) return false;
        rp += len;
      }
    }
  }
  const uint8_t *__restrict__ ref = in.gbases + gb;
  const bool rc = o.revcomp != 0;
  int64_t rp = o.ref_begin, qp = q0;
  uint32_t k = 0, m_len = 0, i0 = 0;
  for (;;) {
    if (i0 >= m_len) {   // the M run is used up: operations until the next one (I and D on the way)
      bool got = false;
      while (k < o.cigar_len) {
        const uint32_t c = cig[k], len = c >> 4, op = c & 15u;
        k++;
        if (op == 0) {
          if (len) {
            sink.interval(gb + (uint64_t)rp, gb + (uint64_t)rp + len - 1);
            m_len = len;
            i0 = 0;
            got = true;
            break;
          }
        } else if (op == 1) {
          qp += len;
        } else if (op == 2) {
          rp += len;
        }
      }
      if (!got) break;
    }
    const uint32_t nn = min(16u, m_len - i0);
    const Bytes16 R = *reinterpret_cast<const Bytes16 *>(ref + rp + i0);
    // forward: the bytes from query position qp + i0 on; reverse: the 16 bytes ENDING at read index L - 1 - qp - i0, back to front
    const int64_t first = rc ? (int64_t)rb + (L - 1 - qp) - (int64_t)i0 - 15 : (int64_t)rb + qp + (int64_t)i0;
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
      const uint32_t b = byte_of(B, j), q = acgt(rc ? complement(b) : b);
      if (q < 4u && acgt(byte_of(R, j)) < 4u)
        sink.event(((gb + (uint64_t)rp + i0 + j) << 3) | (uint64_t)(q << 1) | (rc ? 1u : 0u));
    }
    i0 += 16;
    if (i0 >= m_len) {   // the run is done
      rp += m_len;
      qp += m_len;
    }
  }
  return true;
}

__global__ __launch_bounds__(VAR_BLOCK) void k_var_flag(VariantInputs in, uint32_t *__restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (i >= in.n_pairs || !in.n_groups) return;
  uint64_t lo = 0, hi = in.n_groups;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (in.groups[mid].first <= i) lo = mid;
    else hi = mid;
  }
  const uint64_t first = in.groups[lo].first;
  if (!(first <= i && i - first < in.groups[lo].count)) return;   // dead
  const uint32_t r1 = in.pairs[i].r1, r2 = in.pairs[i].r2;
  if (r1 != KSLAM_NO_OVERLAP && r1 < in.n_ov) flag[r1] = 1u;
  if (r2 != KSLAM_NO_OVERLAP && r2 < in.n_ov) flag[r2] = 1u;
}

__global__ __launch_bounds__(VAR_BLOCK) void k_var_list(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, uint64_t n,
                                                        uint32_t *__restrict__ list) {
  const uint64_t i = (uint64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (i < n && flag[i]) list[pos[i]] = (uint32_t)i;
}

__global__ __launch_bounds__(VAR_BLOCK) void k_var_count(VariantInputs in, const uint32_t *__restrict__ list, uint64_t n_list,
                                                         uint32_t *__restrict__ cnt_ev, uint32_t *__restrict__ cnt_iv,
                                                         unsigned long long *__restrict__ skipped) {
  const uint64_t x = (uint64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  uint64_t skip = 0;
  if (x < n_list) {
    const kslam_overlap o = in.ov[list[x]];
    CountSink sink;
    if (!var_walk(o, in, sink)) skip = 1;
    cnt_ev[x] = sink.n_ev;
    cnt_iv[x] = sink.n_iv;
  }
  skip = wave_sum(skip);
  if ((threadIdx.x & 63) == 0 && skip) atomicAdd(skipped, (unsigned long long)skip);
}

__global__ __launch_bounds__(VAR_BLOCK) void k_var_write(VariantInputs in, const uint32_t *__restrict__ list, uint64_t n_list,
                                                         const uint32_t *__restrict__ cnt_ev, const uint32_t *__restrict__ cnt_iv,
                                                         const uint64_t *__restrict__ off_ev, const uint64_t *__restrict__ off_iv,
                                                         uint64_t *__restrict__ ev, uint64_t *__restrict__ ib, uint64_t *__restrict__ ie) {
  const uint64_t x = (uint64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (x >= n_list || (cnt_ev[x] == 0 && cnt_iv[x] == 0)) return;   // (a skipped record counted nothing)
  const kslam_overlap o = in.ov[list[x]];
  WriteSink sink{ev + off_ev[x], ib + off_iv[x], ie + off_iv[x]};
  (void)var_walk(o, in, sink);
}

// ---- take ----

// the first i in [lo, hi) with a[i] >= v (hi when there is none)
__device__ inline uint64_t lower_bound(const uint64_t *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t v) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(VAR_BLOCK) void k_var_heads(const uint64_t *__restrict__ key, uint64_t n, uint32_t *__restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (i < n) head[i] = (i == 0 || (key[i] >> 1) != (key[i - 1] >> 1)) ? 1u : 0u;
}

__global__ __launch_bounds__(VAR_BLOCK) void k_var_starts(const uint32_t *__restrict__ head, const uint32_t *__restrict__ run, uint64_t n,
                                                          uint32_t *__restrict__ starts) {
  const uint64_t i = (uint64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (i < n && head[i]) starts[run[i]] = (uint32_t)i;
}

__global__ __launch_bounds__(VAR_BLOCK) void k_var_sites(const uint64_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ starts,
                                                         uint64_t n_sites, const uint64_t *__restrict__ begins,
                                                         const uint64_t *__restrict__ ends, uint64_t n_iv, uint32_t min_alt, uint32_t min_depth,
                                                         uint32_t *__restrict__ fwd, uint32_t *__restrict__ rev, uint32_t *__restrict__ depth,
                                                         uint32_t *__restrict__ keep) {
  const uint64_t r = (uint64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (r >= n_sites) return;
  const uint64_t s = starts[r], e = r + 1 < n_sites ? (uint64_t)starts[r + 1] : n;
  const uint64_t site = key[s] >> 1;                             // (g << 2) | alt
  const uint64_t split = lower_bound(key, s, e, (site << 1) | 1u);   // the forward strand's keys sort first
  const uint64_t f = split - s, v = e - split;
  bool k = f + v >= (uint64_t)min_alt;
  uint64_t d = 0;
  if (k) {   // the runs that began at or before the site less those that ended before it
    const uint64_t g = site >> 2;
    d = lower_bound(begins, 0, n_iv, g + 1) - lower_bound(ends, 0, n_iv, g);
    k = d >= (uint64_t)min_depth;
  }
  fwd[r] = (uint32_t)f;
  rev[r] = (uint32_t)v;
  depth[r] = (uint32_t)d;
  keep[r] = k ? 1u : 0u;
}

__global__ __launch_bounds__(VAR_BLOCK) void k_var_rows(const uint64_t *__restrict__ key, const uint32_t *__restrict__ starts, uint64_t n_sites,
                                                        const uint32_t *__restrict__ fwd, const uint32_t *__restrict__ rev,
                                                        const uint32_t *__restrict__ depth, const uint32_t *__restrict__ keep,
                                                        const uint32_t *__restrict__ out_at, const uint64_t *__restrict__ goff,
                                                        uint64_t n_entries, const uint8_t *__restrict__ gbases, kslam_variant_row *__restrict__ rows) {
  const uint64_t r = (uint64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (r >= n_sites || !keep[r]) return;
  const uint64_t site = key[starts[r]] >> 1, g = site >> 2;
  uint64_t lo = 0, hi = n_entries;   // the last entry that starts at or below g (entries of length 0 before it start there too)
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (goff[mid] <= g) lo = mid;
    else hi = mid;
  }
  kslam_variant_row out;
  out.entry = (uint32_t)lo;
  out.pos = (uint32_t)(g - goff[lo]);
  out.ref = gbases[g];
  out.alt = (uint8_t)((0x54474341u >> (8u * (uint32_t)(site & 3u))) & 0xFFu);   // "ACGT"
  out.pad[0] = out.pad[1] = 0;
  out.alt_fwd = fwd[r];
  out.alt_rev = rev[r];
  out.depth = depth[r];
  rows[out_at[r]] = out;
}

inline unsigned blocks(uint64_t n) { return (unsigned)((n + VAR_BLOCK - 1) / VAR_BLOCK); }

}  // namespace

uint64_t contributing_list_device(const VariantInputs &in, DevBuf &flag, DevBuf &pos, DevBuf &list, DevBuf &scan_tmp, DevBuf &totals, hipStream_t s) {
  totals.ensure(4 * sizeof(uint64_t));
  uint64_t *d_tot = totals.as<uint64_t>();
  HIPCHK(hipMemsetAsync(d_tot, 0, 4 * sizeof(uint64_t), s));
  if (!in.n_groups || !in.n_pairs || !in.n_ov) return 0;
  if (in.n_pairs >= (1ull << 39) || in.n_groups >= (1ull << 39)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^39 or more alignment pairs in one batch"};
  if (in.n_ov >= (1ull << 32)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^32 or more overlap records in one batch"};
  flag.ensure(in.n_ov * sizeof(uint32_t));
  pos.ensure(in.n_ov * sizeof(uint32_t));
  scan_tmp.ensure(scan_tmp_bytes(in.n_ov));
  HIPCHK(hipMemsetAsync(flag.p, 0, in.n_ov * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_var_flag, dim3(blocks(in.n_pairs)), dim3(VAR_BLOCK), 0, s, in, flag.as<uint32_t>());
  exclusive_scan_u32(flag.as<uint32_t>(), pos.as<uint32_t>(), in.n_ov, d_tot, scan_tmp.p, s);
  uint64_t n_list = 0;
  read_back(&n_list, d_tot, sizeof n_list, s);
  if (!n_list) return 0;
  list.ensure(n_list * sizeof(uint32_t));
  hipLaunchKernelGGL(k_var_list, dim3(blocks(in.n_ov)), dim3(VAR_BLOCK), 0, s, flag.as<uint32_t>(), pos.as<uint32_t>(), in.n_ov, list.as<uint32_t>());
  HIPCHK(hipGetLastError());
  return n_list;
}

void variants_count_device(const VariantInputs &in, VariantEmitWork &W, hipStream_t s) {
  W.ms = 0;
  W.n_list = W.n_ev = W.n_iv = W.n_skipped = 0;
  if (!W.ev[0])
    for (auto &e : W.ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventRecord(W.ev[0], s));
  if (!in.n_groups || !in.n_pairs || !in.n_ov) return;
  const uint64_t n_list = contributing_list_device(in, W.flag, W.pos, W.list, W.scan_tmp, W.totals, s);
  uint64_t *d_tot = W.totals.as<uint64_t>();
  W.n_list = n_list;
  if (!n_list) return;
  W.cnt_ev.ensure(n_list * sizeof(uint32_t));
  W.cnt_iv.ensure(n_list * sizeof(uint32_t));
  W.off_ev.ensure(n_list * sizeof(uint64_t));
  W.off_iv.ensure(n_list * sizeof(uint64_t));
  hipLaunchKernelGGL(k_var_count, dim3(blocks(n_list)), dim3(VAR_BLOCK), 0, s, in, W.list.as<uint32_t>(), n_list, W.cnt_ev.as<uint32_t>(),
                     W.cnt_iv.as<uint32_t>(), reinterpret_cast<unsigned long long *>(d_tot + 3));
  HIPCHK(hipGetLastError());
  exclusive_scan_u32_to_u64(W.cnt_ev.as<uint32_t>(), W.off_ev.as<uint64_t>(), n_list, d_tot + 1, W.scan_tmp.p, s);
  exclusive_scan_u32_to_u64(W.cnt_iv.as<uint32_t>(), W.off_iv.as<uint64_t>(), n_list, d_tot + 2, W.scan_tmp.p, s);
  uint64_t h[4] = {0, 0, 0, 0};
  read_back(h, d_tot, sizeof h, s);
  W.n_ev = h[1];
  W.n_iv = h[2];
  W.n_skipped = h[3];
}

void variants_write_device(const VariantInputs &in, VariantEmitWork &W, uint64_t *d_events, uint64_t *d_begins, uint64_t *d_ends, hipStream_t s) {
  if (W.n_list && (W.n_ev || W.n_iv))
    hipLaunchKernelGGL(k_var_write, dim3(blocks(W.n_list)), dim3(VAR_BLOCK), 0, s, in, W.list.as<uint32_t>(), W.n_list, W.cnt_ev.as<uint32_t>(),
                       W.cnt_iv.as<uint32_t>(), W.off_ev.as<uint64_t>(), W.off_iv.as<uint64_t>(), d_events, d_begins, d_ends);
  HIPCHK(hipEventRecord(W.ev[1], s));
  HIPCHK(hipGetLastError());
  HIPCHK(stream_wait(s));
  HIPCHK(hipEventElapsedTime(&W.ms, W.ev[0], W.ev[1]));
}

// sorts n keys of `buf` (scratch: `alt`, at least as large); the sorted keys end in `buf`
void sort_keys(DevBuf &buf, DevBuf &alt, uint64_t n, uint64_t max_key, SortWorkspace &ws, hipStream_t s) {
  if (n < 2) return;
  uint32_t bits = 1;
  while (bits < 64 && (max_key >> bits) != 0) bits++;
  SortPass passes[8];
  const int n_passes = (int)((bits + 7) / 8);   // from the largest key: 5 Gb of index needs 5 passes for intervals, 5 for events
  for (int p = 0; p < n_passes; p++) passes[p] = SortPass{(uint32_t)(p / 4), (uint32_t)(8 * (p % 4)), 0u};
  void *sorted = radix_sort(buf.p, alt.p, n, 2, passes, n_passes, ws, s, nullptr, nullptr, nullptr);
  if (sorted != buf.p) std::swap(buf, alt);
}

void variants_take_device(VariantTakeWork &T, DevBuf &events, uint64_t n_ev, DevBuf &begins, DevBuf &ends, uint64_t n_iv, bool sorted,
                          const uint64_t *d_goff, const uint8_t *d_gbases, uint64_t n_entries, uint64_t total_bases, uint32_t min_alt,
                          uint32_t min_depth, uint64_t *n_sites_out, uint64_t *n_rows_out, hipStream_t s) {
  *n_sites_out = *n_rows_out = 0;
  if (!n_ev) return;
  if (!sorted) {
    T.alt.ensure(std::max(events.cap, std::max(begins.cap, ends.cap)));
    sort_keys(events, T.alt, n_ev, total_bases << 3, T.sortws, s);
    T.alt.ensure(std::max(events.cap, std::max(begins.cap, ends.cap)));   // (a swap may have left the smaller block here)
    sort_keys(begins, T.alt, n_iv, total_bases, T.sortws, s);
    T.alt.ensure(std::max(events.cap, std::max(begins.cap, ends.cap)));
    sort_keys(ends, T.alt, n_iv, total_bases, T.sortws, s);
  }
  const uint64_t *key = events.as<uint64_t>();
  T.head.ensure(n_ev * sizeof(uint32_t));
  T.run.ensure(n_ev * sizeof(uint32_t));
  T.scan_tmp.ensure(scan_tmp_bytes(n_ev));
  T.totals.ensure(2 * sizeof(uint64_t));
  uint64_t *d_tot = T.totals.as<uint64_t>();
  hipLaunchKernelGGL(k_var_heads, dim3(blocks(n_ev)), dim3(VAR_BLOCK), 0, s, key, n_ev, T.head.as<uint32_t>());
  HIPCHK(hipGetLastError());
  exclusive_scan_u32(T.head.as<uint32_t>(), T.run.as<uint32_t>(), n_ev, d_tot, T.scan_tmp.p, s);
  uint64_t n_sites = 0;
  read_back(&n_sites, d_tot, sizeof n_sites, s);
  *n_sites_out = n_sites;
  if (!n_sites) return;
  for (DevBuf *b : {&T.starts, &T.fwd, &T.rev, &T.depth, &T.keep, &T.out_at}) b->ensure(n_sites * sizeof(uint32_t));
  hipLaunchKernelGGL(k_var_starts, dim3(blocks(n_ev)), dim3(VAR_BLOCK), 0, s, T.head.as<uint32_t>(), T.run.as<uint32_t>(), n_ev,
                     T.starts.as<uint32_t>());
  hipLaunchKernelGGL(k_var_sites, dim3(blocks(n_sites)), dim3(VAR_BLOCK), 0, s, key, n_ev, T.starts.as<uint32_t>(), n_sites,
                     begins.as<uint64_t>(), ends.as<uint64_t>(), n_iv, min_alt, min_depth, T.fwd.as<uint32_t>(), T.rev.as<uint32_t>(),
                     T.depth.as<uint32_t>(), T.keep.as<uint32_t>());
  HIPCHK(hipGetLastError());
  exclusive_scan_u32(T.keep.as<uint32_t>(), T.out_at.as<uint32_t>(), n_sites, d_tot + 1, T.scan_tmp.p, s);
  uint64_t n_rows = 0;
  read_back(&n_rows, d_tot + 1, sizeof n_rows, s);
  *n_rows_out = n_rows;
  if (!n_rows) return;
  T.rows.ensure(n_rows * sizeof(kslam_variant_row));
  hipLaunchKernelGGL(k_var_rows, dim3(blocks(n_sites)), dim3(VAR_BLOCK), 0, s, key, T.starts.as<uint32_t>(), n_sites, T.fwd.as<uint32_t>(),
                     T.rev.as<uint32_t>(), T.depth.as<uint32_t>(), T.keep.as<uint32_t>(), T.out_at.as<uint32_t>(), d_goff, n_entries, d_gbases,
                     T.rows.as<kslam_variant_row>());
  HIPCHK(hipGetLastError());
}

}  // namespace kslam
