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
//   2. scan + k_scatter_list   the marked overlap records as a list
//   3. k_var_count   one thread per listed record: walk_record (pileup_walk.h) checks the CIGAR whole against the read and the
//                    entry, then walks it into a VarSink<CountEmit>; events and intervals are counted
//   4. two scans     lay out the slots
//   5. the caller makes room (api_variants.hip: under the state's lock, so that appends from several lanes take their turns)
//   6. k_var_write   the same walk writes the keys through a VarSink<WriteEmit>
// Passes 1-2 (contributing_list_device), the shell around 3-4 and 6 (emit_count_device, emit_write_device), sort_keys and the
// run-head passes of the take are shared with depth.hip, consensus.hip and alignqc.hip (common.h); they are defined here.
// On request (variants_take_device): radix_sort of the three arrays, run heads over the events ignoring the strand bit, a scan
// that numbers the runs, one thread per RUN that finds the strand split inside its run by binary search (a run of any length
// costs its thread ~log2 steps: no tile, no atomic, so one hot site is no slower than many cold ones), the depth of the sites
// that passed min_alt by two binary searches over the sorted interval keys, a scan of the keep flags and a compaction that
// resolves entry / pos / ref from the index.
// Bounds: the walk's are stated in pileup_walk.h.  Every other kernel indexes arrays by thread number below their length, by a
// scanned slot below the scan's total, or by a binary search's result inside [0, n).
#include "pileup_walk.h"
#include "wave_add.h"
#include "../../include/kslam_variants.h"

namespace kslam {

namespace {

struct VariantKeys {              // where a batch's keys go
  uint64_t *ev, *ib, *ie;
};
struct CountEmit {
  uint32_t n[VAR_KINDS] = {0, 0};
  __device__ void event(uint64_t) { n[VAR_EV]++; }
  __device__ void interval(uint64_t, uint64_t) { n[VAR_IV]++; }
};
struct WriteEmit {
  VariantKeys at;
  __device__ void event(uint64_t key) { *at.ev++ = key; }
  __device__ void interval(uint64_t b, uint64_t e) { *at.ib++ = b; *at.ie++ = e; }
};
// the walk's sink (pileup_walk.h): an M run is a closed interval; an event needs both bytes in ACGT, and carries its strand
template <class Emit>
struct VarSink : Emit {
  static constexpr bool COLUMNS = true, INSERTIONS = false;
  __device__ void m_run(const kslam_overlap &, const RecordFrame &f, int64_t rp, uint32_t len) {
    Emit::interval(f.gb + (uint64_t)rp, f.gb + (uint64_t)rp + len - 1);
  }
  __device__ void d_run(const kslam_overlap &, const RecordFrame &, int64_t, uint32_t) {}
  __device__ void column(uint64_t g, uint32_t q, uint32_t r, bool rc) {
    const uint32_t alt = acgt(q);
    if (alt < 4u && acgt(r) < 4u) Emit::event((g << 3) | (uint64_t)(alt << 1) | (rc ? 1u : 0u));
  }
};

__global__ __launch_bounds__(PILEUP_BLOCK) void k_var_flag(VariantInputs in, uint32_t *__restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
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

__global__ __launch_bounds__(PILEUP_BLOCK) void k_scatter_list(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, uint64_t n,
                                                               uint32_t *__restrict__ list) {
  const uint64_t i = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
  if (i < n && flag[i]) list[pos[i]] = (uint32_t)i;
}

__global__ __launch_bounds__(PILEUP_BLOCK) void k_var_count(VariantInputs in, const uint32_t *__restrict__ list, uint64_t n_list,
                                                            uint32_t *__restrict__ cnt, unsigned long long *__restrict__ tallies) {
  const uint64_t x = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
  uint64_t skip = 0;
  if (x < n_list) {
    const kslam_overlap o = in.ov[list[x]];
    VarSink<CountEmit> sink;
    if (!walk_record(o, in, sink)) skip = 1;
    cnt[x] = sink.n[VAR_EV];
    cnt[n_list + x] = sink.n[VAR_IV];
  }
  skip = wave_sum(skip);
  if ((threadIdx.x & 63) == 0 && skip) atomicAdd(tallies, (unsigned long long)skip);
}

__global__ __launch_bounds__(PILEUP_BLOCK) void k_var_write(VariantInputs in, const uint32_t *__restrict__ list, uint64_t n_list,
                                                            const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off, VariantKeys at) {
  const uint64_t x = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
  if (x >= n_list || (cnt[x] == 0 && cnt[n_list + x] == 0)) return;   // (a skipped record counted nothing)
  const kslam_overlap o = in.ov[list[x]];
  const uint64_t o_ev = off[x], o_iv = off[n_list + x];
  VarSink<WriteEmit> sink{{VariantKeys{at.ev + o_ev, at.ib + o_iv, at.ie + o_iv}}};
  (void)walk_record(o, in, sink);
}

// ---- take ----

__global__ __launch_bounds__(PILEUP_BLOCK) void k_run_heads(const uint64_t *__restrict__ key, uint64_t n, uint32_t *__restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
  if (i < n) head[i] = (i == 0 || (key[i] >> 1) != (key[i - 1] >> 1)) ? 1u : 0u;
}

__global__ __launch_bounds__(PILEUP_BLOCK) void k_run_starts(const uint32_t *__restrict__ head, const uint32_t *__restrict__ run, uint64_t n,
                                                          uint32_t *__restrict__ starts) {
  const uint64_t i = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
  if (i < n && head[i]) starts[run[i]] = (uint32_t)i;
}

__global__ __launch_bounds__(PILEUP_BLOCK) void k_var_sites(const uint64_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ starts,
                                                         uint64_t n_sites, const uint64_t *__restrict__ begins,
                                                         const uint64_t *__restrict__ ends, uint64_t n_iv, uint32_t min_alt, uint32_t min_depth,
                                                         uint32_t *__restrict__ fwd, uint32_t *__restrict__ rev, uint32_t *__restrict__ depth,
                                                         uint32_t *__restrict__ keep) {
  const uint64_t r = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
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

__global__ __launch_bounds__(PILEUP_BLOCK) void k_var_rows(const uint64_t *__restrict__ key, const uint32_t *__restrict__ starts, uint64_t n_sites,
                                                        const uint32_t *__restrict__ fwd, const uint32_t *__restrict__ rev,
                                                        const uint32_t *__restrict__ depth, const uint32_t *__restrict__ keep,
                                                        const uint32_t *__restrict__ out_at, const uint64_t *__restrict__ goff,
                                                        uint64_t n_entries, const uint8_t *__restrict__ gbases, kslam_variant_row *__restrict__ rows) {
  const uint64_t r = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
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

}  // namespace

uint64_t contributing_list_device(const VariantInputs &in, DevBuf &flag, DevBuf &pos, DevBuf &list, DevBuf &scan_tmp, DevBuf &totals, hipStream_t s) {
  totals.ensure(EMIT_TOTALS * sizeof(uint64_t));
  uint64_t *d_tot = totals.as<uint64_t>();
  HIPCHK(hipMemsetAsync(d_tot, 0, EMIT_TOTALS * sizeof(uint64_t), s));
  if (!in.n_groups || !in.n_pairs || !in.n_ov) return 0;
  if (in.n_pairs >= (1ull << 39) || in.n_groups >= (1ull << 39)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^39 or more alignment pairs in one batch"};
  if (in.n_ov >= (1ull << 32)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^32 or more overlap records in one batch"};
  flag.ensure(in.n_ov * sizeof(uint32_t));
  pos.ensure(in.n_ov * sizeof(uint32_t));
  scan_tmp.ensure(scan_tmp_bytes(in.n_ov));
  HIPCHK(hipMemsetAsync(flag.p, 0, in.n_ov * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_var_flag, dim3(pileup_blocks(in.n_pairs)), dim3(PILEUP_BLOCK), 0, s, in, flag.as<uint32_t>());
  exclusive_scan_u32(flag.as<uint32_t>(), pos.as<uint32_t>(), in.n_ov, d_tot, scan_tmp.p, s);
  uint64_t n_list = 0;
  read_back(&n_list, d_tot, sizeof n_list, s);
  if (!n_list) return 0;
  list.ensure(n_list * sizeof(uint32_t));
  scatter_list_device(flag.as<uint32_t>(), pos.as<uint32_t>(), in.n_ov, list.as<uint32_t>(), s);
  return n_list;
}

void scatter_list_device(const uint32_t *flag, const uint32_t *pos, uint64_t n, uint32_t *list, hipStream_t s) {
  hipLaunchKernelGGL(k_scatter_list, dim3(pileup_blocks(n)), dim3(PILEUP_BLOCK), 0, s, flag, pos, n, list);
  HIPCHK(hipGetLastError());
}
void run_heads_device(const uint64_t *key, uint64_t n, uint32_t *head, hipStream_t s) {
  hipLaunchKernelGGL(k_run_heads, dim3(pileup_blocks(n)), dim3(PILEUP_BLOCK), 0, s, key, n, head);
  HIPCHK(hipGetLastError());
}
void run_starts_device(const uint32_t *head, const uint32_t *run, uint64_t n, uint32_t *starts, hipStream_t s) {
  hipLaunchKernelGGL(k_run_starts, dim3(pileup_blocks(n)), dim3(PILEUP_BLOCK), 0, s, head, run, n, starts);
  HIPCHK(hipGetLastError());
}

void emit_count_device(const VariantInputs &in, EmitWork &W, int kinds, EmitCountKernel count, hipStream_t s) {
  W.ms = 0;
  W.kinds = kinds;
  W.n_list = W.n_skipped = W.n_unanchored = W.n_unrepresentable = 0;
  for (auto &v : W.n) v = 0;
  if (!W.ev[0])
    for (auto &e : W.ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventRecord(W.ev[0], s));
  const uint64_t n_list = contributing_list_device(in, W.flag, W.pos, W.list, W.scan_tmp, W.totals, s);
  W.n_list = n_list;
  if (!n_list) return;
  uint64_t *d_tot = W.totals.as<uint64_t>();
  W.cnt.ensure(kinds * n_list * sizeof(uint32_t));
  W.off.ensure(kinds * n_list * sizeof(uint64_t));
  hipLaunchKernelGGL(count, dim3(pileup_blocks(n_list)), dim3(PILEUP_BLOCK), 0, s, in, W.list.as<uint32_t>(), n_list, W.cnt.as<uint32_t>(),
                     reinterpret_cast<unsigned long long *>(d_tot + 1 + EMIT_MAX_KINDS));
  HIPCHK(hipGetLastError());
  for (int kind = 0; kind < kinds; kind++)
    exclusive_scan_u32_to_u64(W.cnt.as<uint32_t>() + kind * n_list, W.off.as<uint64_t>() + kind * n_list, n_list, d_tot + 1 + kind, W.scan_tmp.p, s);
  uint64_t h[EMIT_TOTALS] = {0, 0, 0, 0, 0, 0, 0, 0};
  read_back(h, d_tot, sizeof h, s);
  for (int kind = 0; kind < kinds; kind++) W.n[kind] = h[1 + kind];
  W.n_skipped = h[1 + EMIT_MAX_KINDS];
  W.n_unanchored = h[2 + EMIT_MAX_KINDS];
  W.n_unrepresentable = h[3 + EMIT_MAX_KINDS];
}

void emit_written(EmitWork &W, hipStream_t s) {
  HIPCHK(hipEventRecord(W.ev[1], s));
  HIPCHK(hipGetLastError());
  HIPCHK(stream_wait(s));
  HIPCHK(hipEventElapsedTime(&W.ms, W.ev[0], W.ev[1]));
}

void variants_count_device(const VariantInputs &in, EmitWork &W, hipStream_t s) { emit_count_device(in, W, VAR_KINDS, k_var_count, s); }

void variants_write_device(const VariantInputs &in, EmitWork &W, uint64_t *d_events, uint64_t *d_begins, uint64_t *d_ends, hipStream_t s) {
  emit_write_device(in, W, k_var_write, VariantKeys{d_events, d_begins, d_ends}, s);
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
  run_heads_device(key, n_ev, T.head.as<uint32_t>(), s);
  exclusive_scan_u32(T.head.as<uint32_t>(), T.run.as<uint32_t>(), n_ev, d_tot, T.scan_tmp.p, s);
  uint64_t n_sites = 0;
  read_back(&n_sites, d_tot, sizeof n_sites, s);
  *n_sites_out = n_sites;
  if (!n_sites) return;
  for (DevBuf *b : {&T.starts, &T.fwd, &T.rev, &T.depth, &T.keep, &T.out_at}) b->ensure(n_sites * sizeof(uint32_t));
  run_starts_device(T.head.as<uint32_t>(), T.run.as<uint32_t>(), n_ev, T.starts.as<uint32_t>(), s);
  hipLaunchKernelGGL(k_var_sites, dim3(pileup_blocks(n_sites)), dim3(PILEUP_BLOCK), 0, s, key, n_ev, T.starts.as<uint32_t>(), n_sites,
                     begins.as<uint64_t>(), ends.as<uint64_t>(), n_iv, min_alt, min_depth, T.fwd.as<uint32_t>(), T.rev.as<uint32_t>(),
                     T.depth.as<uint32_t>(), T.keep.as<uint32_t>());
  HIPCHK(hipGetLastError());
  exclusive_scan_u32(T.keep.as<uint32_t>(), T.out_at.as<uint32_t>(), n_sites, d_tot + 1, T.scan_tmp.p, s);
  uint64_t n_rows = 0;
  read_back(&n_rows, d_tot + 1, sizeof n_rows, s);
  *n_rows_out = n_rows;
  if (!n_rows) return;
  T.rows.ensure(n_rows * sizeof(kslam_variant_row));
  hipLaunchKernelGGL(k_var_rows, dim3(pileup_blocks(n_sites)), dim3(PILEUP_BLOCK), 0, s, key, T.starts.as<uint32_t>(), n_sites, T.fwd.as<uint32_t>(),
                     T.rev.as<uint32_t>(), T.depth.as<uint32_t>(), T.keep.as<uint32_t>(), T.out_at.as<uint32_t>(), d_goff, n_entries, d_gbases,
                     T.rows.as<kslam_variant_row>());
  HIPCHK(hipGetLastError());
}

}  // namespace kslam
