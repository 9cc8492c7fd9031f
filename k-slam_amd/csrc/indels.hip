// indels.hip -- the indel table, normalised and piled up on the device (include/kslam_indels.h).
//
// What a lane holds after a batch is what variants.hip reads.  The pile-up is sparse, as there: one key per counted D run, one
// record per counted I run, plus the intervals that are covered.  Every event is shifted to its leftmost equivalent position
// against its entry's bases BEFORE it is keyed, so that the placements different alignments gave one haplotype change meet in
// one key.  The state is four append-only arrays whose numeric order is the rows' order:
//   begins, ends   g of the first / last column of an M run; g = g_off[entry] + pos
//   del            (g_anchor << 17) | ((len - 1) << 1) | strand
//   ins            two words per insertion: [0] the bases at 2 bits each, the first one highest;
//                  [1] (g_anchor << 7) | ((len - 1) << 1) | strand
// Per batch (indels_count_device, indels_write_device), through the shell the pile-up reports share (common.h):
//   1-2. variants.hip's flag / scan / list passes (contributing_list_device): the overlap records a live pair names, once each
//   3. k_indel_count   one thread per listed record: walk_record (pileup_walk.h) checks the CIGAR whole against the read and the
//                      entry, then walks it into an IndelSink<CountEmit> -- no columns, so the walk itself reads no bases; the
//                      sink counts M intervals, counted deletions, counted insertions and the D runs that are too long, and
//                      tallies the unanchored and the unrepresentable; the tallies are summed per wave before one atomic each
//   4. the scans       lay out the slots (the fourth kind, INDEL_LONG, is summed by its scan and gets no slot)
//   5. the caller makes room (api_indels.hip: under the state's lock)
//   6. k_indel_write   the same walk through an IndelSink<WriteEmit>: d_run normalises against the entry's bases and stores the
//                      key; i_run reads the inserted bases (insertion_bases, pileup_walk.h), normalises -- a rotation of the 2-bit
//                      word by two shifts and a mask per step -- and stores the record
// Which events are counted is decided by deletion_class / insertion_class, which both sinks call: the count and the write pass
// cannot disagree.  Normalisation moves an event and never drops one.
// One thread per record with a data-dependent loop: a wave waits for its longest shift.  Events inside repeats of thousands of
// bases are rare; the cost is stated in DESIGN.md.
// On request (indels_sort_device, indels_take_device, once per kind): sort_keys on the interval arrays and the deletion keys;
// the insertion records by the 4-word radix sort, least significant first: the strand bit, the bases, then word [1] from bit 1
// up -- the order (anchor, len, bases, strand), so that the records of one row are one run whose strands are split by a binary
// search; run heads ignoring the strand bit, a scan that numbers the runs, one thread per RUN: the split, and for the runs that
// pass min_alt the depth at the anchor by two binary searches over the sorted interval keys; a scan of the keep flags and a
// compaction that resolves entry and pos from g_off.  The two kinds' filtered rows are merged into the one order ON THE HOST
// (api_indels.hip: a std::merge over the rows that passed the filter; nothing else travels).
// Bounds: the walk's are stated in pileup_walk.h.  normalise_deletion reads ref[p - 1] with p >= 2, so never below ref[1], and
// ref[p + len - 1], which the fit check put inside the entry for the raw p and which only moves down with p.
// normalise_insertion reads ref[p - 1] with p >= 2 alone.  `ref` is the record's entry: neither loop reads below the entry's
// first byte or into another entry.  Every other kernel indexes arrays by thread number below their length, by a scanned slot
// below the scan's total, or by a binary search's result inside [0, n).
#include "pileup_walk.h"
#include "wave_add.h"
#include "../../include/kslam_indels.h"

namespace kslam {

namespace {

enum : uint32_t { EV_COUNTED = 0, EV_UNANCHORED = 1, EV_REFUSED = 2 };

// ---- which raw events are counted: the ONE decision of both passes ----
__device__ inline uint32_t deletion_class(const kslam_overlap &o, int64_t rp, uint32_t len) {
  return rp <= (int64_t)o.ref_begin ? EV_UNANCHORED : len > KSLAM_INDEL_MAX_DEL ? EV_REFUSED : EV_COUNTED;
}
// *bases: the oriented inserted bases of a counted insertion
__device__ inline uint32_t insertion_class(const kslam_overlap &o, const VariantInputs &in, const RecordFrame &f, int64_t rp, int64_t qp, uint32_t len,
                                           uint64_t *bases) {
  if (rp <= (int64_t)o.ref_begin) return EV_UNANCHORED;
  if (len > KSLAM_INDEL_MAX_INS || !insertion_bases(o, in, f, qp, len, bases)) return EV_REFUSED;
  return EV_COUNTED;
}

// ---- normalisation (include/kslam_indels.h): the leftmost equivalent position; ref: the entry's first byte ----
__device__ inline int64_t normalise_deletion(const uint8_t *__restrict__ ref, int64_t p, uint32_t len) {
  while (p >= 2) {
    const uint32_t a = ref[p - 1];
    if (a != (uint32_t)ref[p + (int64_t)len - 1] || acgt(a) >= 4u) break;
    p--;
  }
  return p;
}
__device__ inline int64_t normalise_insertion(const uint8_t *__restrict__ ref, int64_t p, uint32_t len, uint64_t *bases) {
  const uint32_t top = 2u * (len - 1u);
  const uint64_t mask = len >= 32u ? ~0ull : (1ull << (2u * len)) - 1ull;
  uint64_t s = *bases;
  while (p >= 2 && acgt(ref[p - 1]) == (uint32_t)(s & 3u)) {   // (a byte outside ACGT has code 4 and equals no base)
    s = ((s >> 2) | (s << top)) & mask;                        // the last base becomes the first
    p--;
  }
  *bases = s;
  return p;
}

struct CountEmit {
  uint32_t n[INDEL_KINDS] = {0, 0, 0, 0}, unanchored = 0, unrepresentable = 0;
  __device__ void interval(uint64_t, uint64_t) { n[INDEL_IV]++; }
  __device__ void deletion(uint32_t cls, const uint8_t *, uint64_t, int64_t, uint32_t, bool) {
    n[INDEL_DEL] += cls == EV_COUNTED ? 1u : 0u;
    n[INDEL_LONG] += cls == EV_REFUSED ? 1u : 0u;
    unanchored += cls == EV_UNANCHORED ? 1u : 0u;
  }
  __device__ void insertion(uint32_t cls, const uint8_t *, uint64_t, int64_t, uint32_t, uint64_t, bool) {
    n[INDEL_INS] += cls == EV_COUNTED ? 1u : 0u;
    unrepresentable += cls == EV_REFUSED ? 1u : 0u;
    unanchored += cls == EV_UNANCHORED ? 1u : 0u;
  }
};
struct WriteEmit {
  IndelKeys at;
  __device__ void interval(uint64_t b, uint64_t e) { *at.ib++ = b; *at.ie++ = e; }
  __device__ void deletion(uint32_t cls, const uint8_t *ref, uint64_t gb, int64_t p, uint32_t len, bool strand) {
    if (cls != EV_COUNTED) return;
    p = normalise_deletion(ref, p, len);
    *at.del++ = ((gb + (uint64_t)p - 1) << 17) | ((uint64_t)(len - 1u) << 1) | (strand ? 1u : 0u);
  }
  __device__ void insertion(uint32_t cls, const uint8_t *ref, uint64_t gb, int64_t p, uint32_t len, uint64_t bases, bool strand) {
    if (cls != EV_COUNTED) return;
    p = normalise_insertion(ref, p, len, &bases);
    at.ins[0] = bases;
    at.ins[1] = ((gb + (uint64_t)p - 1) << 7) | ((uint64_t)(len - 1u) << 1) | (strand ? 1u : 0u);
    at.ins += 2;
  }
};

// the walk's sink (pileup_walk.h): an M run is a closed interval; D and I runs are classified here, once for both passes
template <class Emit>
struct IndelSink : Emit {
  static constexpr bool COLUMNS = false, INSERTIONS = true;
  const uint8_t *__restrict__ gbases;
  __device__ void m_run(const kslam_overlap &, const RecordFrame &f, int64_t rp, uint32_t len) {
    Emit::interval(f.gb + (uint64_t)rp, f.gb + (uint64_t)rp + len - 1);
  }
  __device__ void d_run(const kslam_overlap &o, const RecordFrame &f, int64_t rp, uint32_t len) {
    Emit::deletion(deletion_class(o, rp, len), gbases + f.gb, f.gb, rp, len, o.revcomp != 0);
  }
  __device__ void i_run(const kslam_overlap &o, const VariantInputs &in, const RecordFrame &f, int64_t rp, int64_t qp, uint32_t len) {
    uint64_t w = 0;
    const uint32_t cls = insertion_class(o, in, f, rp, qp, len, &w);
    Emit::insertion(cls, gbases + f.gb, f.gb, rp, len, w, o.revcomp != 0);
  }
};

__global__ __launch_bounds__(PILEUP_BLOCK) void k_indel_count(VariantInputs in, const uint32_t *__restrict__ list, uint64_t n_list,
                                                              uint32_t *__restrict__ cnt, unsigned long long *__restrict__ tallies) {
  const uint64_t x = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
  uint64_t skip = 0, unanchored = 0, unrepresentable = 0;
  if (x < n_list) {
    const kslam_overlap o = in.ov[list[x]];
    IndelSink<CountEmit> sink;
    sink.gbases = in.gbases;
    if (!walk_record(o, in, sink)) skip = 1;
#pragma unroll
    for (int kind = 0; kind < INDEL_KINDS; kind++) cnt[(uint64_t)kind * n_list + x] = sink.n[kind];
    unanchored = sink.unanchored;
    unrepresentable = sink.unrepresentable;
  }
  skip = wave_sum(skip);
  unanchored = wave_sum(unanchored);
  unrepresentable = wave_sum(unrepresentable);
  if ((threadIdx.x & 63) == 0) {
    if (skip) atomicAdd(tallies + 0, (unsigned long long)skip);
    if (unanchored) atomicAdd(tallies + 1, (unsigned long long)unanchored);
    if (unrepresentable) atomicAdd(tallies + 2, (unsigned long long)unrepresentable);
  }
}

__global__ __launch_bounds__(PILEUP_BLOCK) void k_indel_write(VariantInputs in, const uint32_t *__restrict__ list, uint64_t n_list,
                                                              const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off, IndelKeys at) {
  const uint64_t x = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
  if (x >= n_list) return;
  if ((cnt[x] | cnt[n_list + x] | cnt[2 * n_list + x]) == 0) return;   // (a skipped record counted nothing; INDEL_LONG has no slot)
  const kslam_overlap o = in.ov[list[x]];
  const uint64_t o_iv = off[x], o_del = off[n_list + x], o_ins = off[2 * n_list + x];
  IndelSink<WriteEmit> sink;
  sink.at = IndelKeys{at.ib + o_iv, at.ie + o_iv, at.del + o_del, at.ins + 2 * o_ins};
  sink.gbases = in.gbases;
  (void)walk_record(o, in, sink);
}

// ---- take ----

// a kind's sorted keys as the take sees them: record i's key word, its bases, the fields inside the key
template <int KIND> struct KeyView;
template <> struct KeyView<KSLAM_INDEL_DEL> {
  static constexpr int STRIDE = 1, KEY_AT = 0;
  static constexpr uint32_t POS_SHIFT = 17, LEN_MASK = 0xFFFFu;
  __device__ static uint64_t bases(const uint64_t *, uint64_t) { return 0; }
};
template <> struct KeyView<KSLAM_INDEL_INS> {
  static constexpr int STRIDE = 2, KEY_AT = 1;
  static constexpr uint32_t POS_SHIFT = 7, LEN_MASK = 0x3Fu;
  __device__ static uint64_t bases(const uint64_t *rec, uint64_t i) { return rec[2 * i]; }
};

// head[i] = 1 where a run of insertion records that are equal but for their strand bit begins
__global__ __launch_bounds__(PILEUP_BLOCK) void k_ins_heads(const uint64_t *__restrict__ rec, uint64_t n, uint32_t *__restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
  if (i < n) head[i] = (i == 0 || rec[2 * i] != rec[2 * i - 2] || (rec[2 * i + 1] >> 1) != (rec[2 * i - 1] >> 1)) ? 1u : 0u;
}

template <int KIND>
__global__ __launch_bounds__(PILEUP_BLOCK) void k_indel_sites(const uint64_t *__restrict__ rec, uint64_t n, const uint32_t *__restrict__ starts,
                                                              uint64_t n_sites, const uint64_t *__restrict__ begins,
                                                              const uint64_t *__restrict__ ends, uint64_t n_iv, uint32_t min_alt, uint32_t min_depth,
                                                              uint32_t *__restrict__ fwd, uint32_t *__restrict__ rev, uint32_t *__restrict__ depth,
                                                              uint32_t *__restrict__ keep) {
  using V = KeyView<KIND>;
  const uint64_t r = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
  if (r >= n_sites) return;
  const uint64_t s = starts[r], e = r + 1 < n_sites ? (uint64_t)starts[r + 1] : n;
  const uint64_t key = rec[s * V::STRIDE + V::KEY_AT];
  const uint64_t split = lower_bound<V::STRIDE>(rec + V::KEY_AT, s, e, key | 1u);   // the forward strand's keys sort first
  const uint64_t f = split - s, v = e - split;
  bool k = f + v >= (uint64_t)min_alt;
  uint64_t d = 0;
  if (k) {   // the M runs that began at or before the anchor less those that ended before it
    const uint64_t g = key >> V::POS_SHIFT;
    d = lower_bound(begins, 0, n_iv, g + 1) - lower_bound(ends, 0, n_iv, g);
    k = d >= (uint64_t)min_depth;
  }
  fwd[r] = (uint32_t)f;
  rev[r] = (uint32_t)v;
  depth[r] = (uint32_t)d;
  keep[r] = k ? 1u : 0u;
}

template <int KIND>
__global__ __launch_bounds__(PILEUP_BLOCK) void k_indel_rows(const uint64_t *__restrict__ rec, const uint32_t *__restrict__ starts, uint64_t n_sites,
                                                             const uint32_t *__restrict__ fwd, const uint32_t *__restrict__ rev,
                                                             const uint32_t *__restrict__ depth, const uint32_t *__restrict__ keep,
                                                             const uint32_t *__restrict__ out_at, const uint64_t *__restrict__ goff,
                                                             uint64_t n_entries, kslam_indel_row *__restrict__ rows) {
  using V = KeyView<KIND>;
  const uint64_t r = (uint64_t)blockIdx.x * PILEUP_BLOCK + threadIdx.x;
  if (r >= n_sites || !keep[r]) return;
  const uint64_t s = starts[r], key = rec[s * V::STRIDE + V::KEY_AT], g = key >> V::POS_SHIFT;
  uint64_t lo = 0, hi = n_entries;   // the last entry that starts at or below g (entries of length 0 before it start there too)
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (goff[mid] <= g) lo = mid;
    else hi = mid;
  }
  kslam_indel_row out;
  out.entry = (uint32_t)lo;
  out.pos = (uint32_t)(g - goff[lo]);
  out.kind = (uint8_t)KIND;
  out.pad[0] = out.pad[1] = out.pad[2] = 0;
  out.len = (uint32_t)((key >> 1) & V::LEN_MASK) + 1u;
  out.bases = V::bases(rec, s);
  out.alt_fwd = fwd[r];
  out.alt_rev = rev[r];
  out.depth = depth[r];
  out.pad2 = 0;
  rows[out_at[r]] = out;
}

// sorts n insertion records of `buf` into the order (word [1] >> 1, bases, strand): stable runs of the radix sort, the least
// significant digits first.  No digit straddles a 32-bit word: word [1]'s bits 1 .. 31 are four digits, its upper half four more.
void sort_insertions(DevBuf &buf, DevBuf &alt, uint64_t n, uint64_t max_key, SortWorkspace &ws, hipStream_t s) {
  if (n < 2) return;
  SortPass passes[8];
  auto run = [&](int n_passes) {
    void *sorted = radix_sort(buf.p, alt.p, n, 4, passes, n_passes, ws, s, nullptr, nullptr, nullptr);
    if (sorted != buf.p) std::swap(buf, alt);
  };
  passes[0] = SortPass{2u, 0u, 0u};   // the strand bit (the digit's other bits are sorted again below)
  run(1);
  for (int p = 0; p < 8; p++) passes[p] = SortPass{(uint32_t)(p / 4), (uint32_t)(8 * (p % 4)), 0u};
  run(8);
  uint32_t bits = 1;
  while (bits < 64 && (max_key >> bits) != 0) bits++;
  int n_passes = 0;
  for (uint32_t at = 1; at < bits && n_passes < 8; n_passes++) {
    passes[n_passes] = at < 32 ? SortPass{2u, at, 0u} : SortPass{3u, at - 32u, 0u};
    at = at < 25 ? at + 8 : at == 25 ? 32 : at + 8;
  }
  if (n_passes) run(n_passes);
}

template <int KIND>
void take_kind(VariantTakeWork &T, const uint64_t *rec, uint64_t n, const uint64_t *begins, const uint64_t *ends, uint64_t n_iv, const uint64_t *d_goff,
               uint64_t n_entries, uint32_t min_alt, uint32_t min_depth, uint64_t *n_sites_out, uint64_t *n_rows_out, hipStream_t s) {
  *n_sites_out = *n_rows_out = 0;
  if (!n) return;
  T.head.ensure(n * sizeof(uint32_t));
  T.run.ensure(n * sizeof(uint32_t));
  T.scan_tmp.ensure(scan_tmp_bytes(n));
  T.totals.ensure(2 * sizeof(uint64_t));
  uint64_t *d_tot = T.totals.as<uint64_t>();
  if constexpr (KIND == KSLAM_INDEL_DEL) {
    run_heads_device(rec, n, T.head.as<uint32_t>(), s);
  } else {
    hipLaunchKernelGGL(k_ins_heads, dim3(pileup_blocks(n)), dim3(PILEUP_BLOCK), 0, s, rec, n, T.head.as<uint32_t>());
    HIPCHK(hipGetLastError());
  }
  exclusive_scan_u32(T.head.as<uint32_t>(), T.run.as<uint32_t>(), n, d_tot, T.scan_tmp.p, s);
  uint64_t n_sites = 0;
  read_back(&n_sites, d_tot, sizeof n_sites, s);
  *n_sites_out = n_sites;
  if (!n_sites) return;
  for (DevBuf *b : {&T.starts, &T.fwd, &T.rev, &T.depth, &T.keep, &T.out_at}) b->ensure(n_sites * sizeof(uint32_t));
  run_starts_device(T.head.as<uint32_t>(), T.run.as<uint32_t>(), n, T.starts.as<uint32_t>(), s);
  hipLaunchKernelGGL(k_indel_sites<KIND>, dim3(pileup_blocks(n_sites)), dim3(PILEUP_BLOCK), 0, s, rec, n, T.starts.as<uint32_t>(), n_sites, begins, ends,
                     n_iv, min_alt, min_depth, T.fwd.as<uint32_t>(), T.rev.as<uint32_t>(), T.depth.as<uint32_t>(), T.keep.as<uint32_t>());
  HIPCHK(hipGetLastError());
  exclusive_scan_u32(T.keep.as<uint32_t>(), T.out_at.as<uint32_t>(), n_sites, d_tot + 1, T.scan_tmp.p, s);
  uint64_t n_rows = 0;
  read_back(&n_rows, d_tot + 1, sizeof n_rows, s);
  *n_rows_out = n_rows;
  if (!n_rows) return;
  T.rows.ensure(n_rows * sizeof(kslam_indel_row));
  hipLaunchKernelGGL(k_indel_rows<KIND>, dim3(pileup_blocks(n_sites)), dim3(PILEUP_BLOCK), 0, s, rec, T.starts.as<uint32_t>(), n_sites, T.fwd.as<uint32_t>(),
                     T.rev.as<uint32_t>(), T.depth.as<uint32_t>(), T.keep.as<uint32_t>(), T.out_at.as<uint32_t>(), d_goff, n_entries,
                     T.rows.as<kslam_indel_row>());
  HIPCHK(hipGetLastError());
  HIPCHK(stream_wait(s));
}

}  // namespace

void indels_count_device(const VariantInputs &in, EmitWork &W, hipStream_t s) { emit_count_device(in, W, INDEL_KINDS, k_indel_count, s); }

void indels_write_device(const VariantInputs &in, EmitWork &W, const IndelKeys &at, hipStream_t s) {
  const uint64_t n_long = W.n[INDEL_LONG];
  W.n[INDEL_LONG] = 0;   // (nothing is written for it: a batch that holds nothing else launches nothing)
  emit_write_device(in, W, k_indel_write, at, s);
  W.n[INDEL_LONG] = n_long;
}

void indels_sort_device(VariantTakeWork &T, DevBuf &begins, DevBuf &ends, uint64_t n_iv, DevBuf &dels, uint64_t n_del, DevBuf &ins, uint64_t n_ins,
                        uint64_t total_bases, hipStream_t s) {
  auto room = [&] {   // (a swap may have left a smaller block in T.alt)
    size_t cap = ins.cap;
    for (const DevBuf *b : {&begins, &ends, &dels}) cap = std::max(cap, b->cap);
    T.alt.ensure(cap);
  };
  room();
  sort_keys(begins, T.alt, n_iv, total_bases, T.sortws, s);
  room();
  sort_keys(ends, T.alt, n_iv, total_bases, T.sortws, s);
  room();
  sort_keys(dels, T.alt, n_del, total_bases << 17, T.sortws, s);
  room();
  sort_insertions(ins, T.alt, n_ins, total_bases << 7, T.sortws, s);
}

void indels_take_device(VariantTakeWork &T, int kind, const uint64_t *keys, uint64_t n_keys, const uint64_t *begins, const uint64_t *ends, uint64_t n_iv,
                        const uint64_t *d_goff, uint64_t n_entries, uint32_t min_alt, uint32_t min_depth, uint64_t *n_sites_out, uint64_t *n_rows_out,
                        hipStream_t s) {
  if (kind == KSLAM_INDEL_DEL)
    take_kind<KSLAM_INDEL_DEL>(T, keys, n_keys, begins, ends, n_iv, d_goff, n_entries, min_alt, min_depth, n_sites_out, n_rows_out, s);
  else
    take_kind<KSLAM_INDEL_INS>(T, keys, n_keys, begins, ends, n_iv, d_goff, n_entries, min_alt, min_depth, n_sites_out, n_rows_out, s);
}

}  // namespace kslam
