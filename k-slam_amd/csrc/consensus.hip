// consensus.hip -- the consensus caller, piled up and called on the device (include/kslam_consensus.h).
//
// What a lane holds after a batch is what variants.hip reads.  A dense per-base vote array would cost six counters per base of
// the index, so the pile-up is sparse, as there: only what differs from the entry is recorded, plus the intervals that are
// covered.  The state is six append-only arrays whose numeric order is the order the call pass reads them in:
//   ev        (g << 3) | code       one per M column whose query byte differs from the entry's; g = g_off[entry] + pos
//   mb, me    g of the first / last column of an M run
//   db, de    of a D run
//   ins       two words per stored insertion: [0] the bases at 2 bits each, the first one highest; [1] (anchor << 6) | (len - 1)
// Per batch (consensus_count_device, consensus_write_device):
//   1-2. variants.hip's flag / scan / list passes (contributing_list_device): the overlap records a live pair names, once each
//   3. k_cns_count   one thread per listed record: walk_record (pileup_walk.h) checks the CIGAR whole against the read and the
//                    entry, then walks it into a CnsSink<CountEmit>; what it would emit of each kind is counted, and the I runs
//                    that are not stored are tallied
//   4. four scans    lay out the slots
//   5. the caller makes room (api_consensus.hip: under the state's lock)
//   6. k_cns_write   the same walk writes the keys through a CnsSink<WriteEmit>
// The walk is the SNV table's and the depth track's, with the widest sink: every differing column, the D runs, and the I runs,
// whose bases (at most 32) are read bytewise (insertion_bases, shared with indels.hip).
// On request (consensus_sort_device, consensus_take_device): radix_sort of the six arrays; one thread per ENTRY marks the entries
// holding an M or D run, a scan lists them; the host cuts the list into slices of whole entries; per slice
//   k_cns_call    one thread per position: m and dl by two binary searches each over the sorted interval arrays, the position's
//                 events and the insertion runs at the anchor by further searches, the call, the output length (0 .. 33) and
//                 what the write pass needs; the entry's counters are combined inside the wavefront (wave_add.h)
//   a scan        places the bytes
//   k_cns_write_seq   stores them, for the reported entries alone, where the host laid their sequences out
// Bounds: the walk's are stated in pileup_walk.h; an I run's bytes lie inside the read (the fit check covered them).  The call
// pass indexes positions of touched entries only, below g_off[n_entries].
#include "consensus.h"
#include "pileup_walk.h"
#include "wave_add.h"

namespace kslam {

namespace {

constexpr int CNS_BLOCK = PILEUP_BLOCK;
constexpr uint32_t NO_INS = 0xFFFFFFFFu;
constexpr uint64_t NOT_REPORTED = ~0ull;

// an I run is unanchored (no reference position consumed before it), stored, or unrepresentable (too long, or a base outside
// ACGT).  (Counted with sums, not one increment per case: three branches that each add 1 to another counter are merged into
// one add through a pointer, which takes the counters out of registers.)
struct CountEmit {
  uint32_t n[CNS_KINDS] = {0, 0, 0, 0}, unanchored = 0, unrepresentable = 0;
  __device__ void event(uint64_t) { n[CNS_EV]++; }
  __device__ void m(uint64_t, uint64_t) { n[CNS_M]++; }
  __device__ void d(uint64_t, uint64_t) { n[CNS_D]++; }
  __device__ void insertion(bool anchored, bool stored, uint64_t, uint64_t) {
    n[CNS_INS] += stored ? 1u : 0u;
    unanchored += anchored ? 0u : 1u;
    unrepresentable += anchored && !stored ? 1u : 0u;
  }
};
struct WriteEmit {
  ConsensusKeys at;
  __device__ void event(uint64_t key) { *at.ev++ = key; }
  __device__ void m(uint64_t b, uint64_t e) { *at.mb++ = b; *at.me++ = e; }
  __device__ void d(uint64_t b, uint64_t e) { *at.db++ = b; *at.de++ = e; }
  __device__ void insertion(bool, bool stored, uint64_t key, uint64_t bases) {
    if (!stored) return;
    at.ins[0] = bases;
    at.ins[1] = key;
    at.ins += 2;
  }
};

// the walk's sink (pileup_walk.h): M and D runs as closed intervals, every differing column with its code 0 .. 4, and the I runs,
// whose bases insertion_bases (pileup_walk.h) reads
template <class Emit>
struct CnsSink : Emit {
  static constexpr bool COLUMNS = true, INSERTIONS = true;
  __device__ void m_run(const kslam_overlap &, const RecordFrame &f, int64_t rp, uint32_t len) { Emit::m(f.gb + (uint64_t)rp, f.gb + (uint64_t)rp + len - 1); }
  __device__ void d_run(const kslam_overlap &, const RecordFrame &f, int64_t rp, uint32_t len) { Emit::d(f.gb + (uint64_t)rp, f.gb + (uint64_t)rp + len - 1); }
  __device__ void column(uint64_t g, uint32_t q, uint32_t, bool) { Emit::event((g << 3) | (uint64_t)acgt(q)); }
  __device__ void i_run(const kslam_overlap &o, const VariantInputs &in, const RecordFrame &f, int64_t rp, int64_t qp, uint32_t len) {
    const bool anchored = rp > (int64_t)o.ref_begin;
    uint64_t w = 0;
    const bool stored = anchored && len <= KSLAM_CONSENSUS_MAX_INS && insertion_bases(o, in, f, qp, len, &w);
    Emit::insertion(anchored, stored, ((f.gb + (uint64_t)rp - 1) << 6) | (uint64_t)(len - 1), w);
  }
};

__global__ __launch_bounds__(CNS_BLOCK) void k_cns_count(VariantInputs in, const uint32_t *__restrict__ list, uint64_t n_list,
                                                         uint32_t *__restrict__ cnt, unsigned long long *__restrict__ tallies) {
  const uint64_t x = (uint64_t)blockIdx.x * CNS_BLOCK + threadIdx.x;
  uint64_t skip = 0, unanchored = 0, unrepresentable = 0;
  if (x < n_list) {
    const kslam_overlap o = in.ov[list[x]];
    CnsSink<CountEmit> sink;
    if (!walk_record(o, in, sink)) skip = 1;
#pragma unroll
    for (int kind = 0; kind < CNS_KINDS; kind++) cnt[(uint64_t)kind * n_list + x] = sink.n[kind];
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

__global__ __launch_bounds__(CNS_BLOCK) void k_cns_write(VariantInputs in, const uint32_t *__restrict__ list, uint64_t n_list,
                                                         const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off, ConsensusKeys at) {
  const uint64_t x = (uint64_t)blockIdx.x * CNS_BLOCK + threadIdx.x;
  if (x >= n_list) return;
  if ((cnt[x] | cnt[n_list + x] | cnt[2 * n_list + x] | cnt[3 * n_list + x]) == 0) return;   // (a skipped record counted nothing)
  const kslam_overlap o = in.ov[list[x]];
  const uint64_t o_ev = off[x], o_m = off[n_list + x], o_d = off[2 * n_list + x], o_ins = off[3 * n_list + x];
  CnsSink<WriteEmit> sink{{ConsensusKeys{at.ev + o_ev, at.mb + o_m, at.me + o_m, at.db + o_d, at.de + o_d, at.ins + 2 * o_ins}}};
  (void)walk_record(o, in, sink);
}

// ---- take ----

// touched: the entry holds at least one M or D run (a run lies inside one entry, so its first column decides)
__global__ __launch_bounds__(CNS_BLOCK) void k_cns_touched(const uint64_t *__restrict__ goff, uint64_t n_entries, const uint64_t *__restrict__ mb,
                                                           uint64_t n_m, const uint64_t *__restrict__ db, uint64_t n_d, uint32_t *__restrict__ flag) {
  const uint64_t e = (uint64_t)blockIdx.x * CNS_BLOCK + threadIdx.x;
  if (e >= n_entries) return;
  const uint64_t b = goff[e], end = goff[e + 1];
  bool t = false;
  if (end > b) {
    const uint64_t i = lower_bound(mb, 0, n_m, b);
    t = i < n_m && mb[i] < end;
    if (!t) {
      const uint64_t j = lower_bound(db, 0, n_d, b);
      t = j < n_d && db[j] < end;
    }
  }
  flag[e] = t ? 1u : 0u;
}

struct SliceView {                 // touched entries [t0, t1) and their npos positions
  const uint32_t *tlist;
  const uint64_t *tstart;
  uint64_t t0, t1, npos;
};
// the touched entry that position x of the slice lies in (touched entries have a length above 0)
__device__ inline uint64_t slice_entry(const SliceView &S, uint64_t x) {
  const uint64_t p = S.tstart[S.t0] + x;
  uint64_t lo = S.t0, hi = S.t1;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (S.tstart[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(CNS_BLOCK) void k_cns_call(SliceView S, ConsensusKeys K, uint64_t n_ev, uint64_t n_m, uint64_t n_d, uint64_t n_ins,
                                                        const uint64_t *__restrict__ goff, const uint8_t *__restrict__ gbases,
                                                        kslam_consensus_params P, uint32_t *__restrict__ out_len, uint8_t *__restrict__ out_call,
                                                        uint32_t *__restrict__ out_ins, unsigned long long *__restrict__ counters) {
  const uint64_t x = (uint64_t)blockIdx.x * CNS_BLOCK + threadIdx.x;
  const bool has = x < S.npos;
  uint32_t key = 0, len = 0, ins_len = 0;
  bool covered = false, subst = false, deleted = false, ambiguous = false;
  if (has) {
    const uint64_t t = slice_entry(S, x);
    key = (uint32_t)(t - S.t0);
    const uint64_t g = goff[S.tlist[t]] + (S.tstart[S.t0] + x - S.tstart[t]);
    const uint32_t refb = gbases[g];
    // the runs that began at or before g less those that ended before it
    const uint64_t m = lower_bound(K.mb, 0, n_m, g + 1) - lower_bound(K.me, 0, n_m, g);
    const uint64_t dl = lower_bound(K.db, 0, n_d, g + 1) - lower_bound(K.de, 0, n_d, g);
    const uint64_t d = m + dl;
    uint32_t call = 0, win_ins = NO_INS;
    if (d < (uint64_t)P.min_depth) {
      call = P.fill == KSLAM_CONSENSUS_FILL_REF ? refb : (uint32_t)'N';
      len = 1;
    } else {
      covered = true;
      const uint64_t need = d * (uint64_t)P.call_permille;
      // the position's events: [b[c], b[c + 1]) are those with code c
      uint64_t b[6];
      b[0] = lower_bound(K.ev, 0, n_ev, g << 3);
      b[5] = lower_bound(K.ev, b[0], n_ev, (g + 1) << 3);
#pragma unroll
      for (uint32_t c = 1; c < 5; c++) b[c] = b[5] > b[0] ? lower_bound(K.ev, b[c - 1], b[5], (g << 3) | c) : b[0];
      const uint64_t refc = m - (b[5] - b[0]);
      const uint32_t rcode = acgt(refb);
      uint32_t won = 5;   // 0 .. 3: that base; 4: deletion; 5: nothing
#pragma unroll
      for (uint32_t c = 0; c < 4; c++) {
        const uint64_t vote = (b[c + 1] - b[c]) + (rcode == c ? refc : 0ull);
        if (vote * 1000ull > need) won = c;
      }
      if (dl * 1000ull > need) won = 4;
      if (won < 4) {
        call = (0x54474341u >> (8u * won)) & 0xFFu;   // "ACGT"
        len = 1;
        subst = call != refb;
      } else if (won == 4) {
        deleted = true;
      } else {
        call = (uint32_t)'N';
        len = 1;
        ambiguous = true;
      }
      // the stored insertions anchored here: runs of equal records, ascending by length, then by their bases
      if (n_ins) {
        uint64_t i = lower_bound<2>(K.ins + 1, 0, n_ins, g << 6);
        const uint64_t hi = lower_bound<2>(K.ins + 1, i, n_ins, (g + 1) << 6);
        while (i < hi && (hi - i) * 1000ull > need) {   // (fewer records left than a winner needs: none can win)
          const uint64_t k0 = K.ins[2 * i], k1 = K.ins[2 * i + 1];
          uint64_t a = i + 1, e = hi;
          while (a < e) {
            const uint64_t mid = a + (e - a) / 2;
            if (K.ins[2 * mid + 1] == k1 && K.ins[2 * mid] == k0) a = mid + 1;
            else e = mid;
          }
          if ((a - i) * 1000ull > need) {
            win_ins = (uint32_t)i;
            ins_len = (uint32_t)(k1 & 63u) + 1u;
            break;
          }
          i = a;
        }
      }
    }
    len += ins_len;
    out_len[x] = len;
    out_call[x] = (uint8_t)call;
    out_ins[x] = win_ins;
  }
  // per entry: table A = covered, sequence bytes, substitutions, deleted; table B = insertions, inserted bases, ambiguous, -
  unsigned long long *A = counters, *B = counters + 4ull * (S.t1 - S.t0);
  wave_add(has, key, covered, len, A, 0, 1);
  wave_add(has, key, subst, deleted ? 1ull : 0ull, A, 2, 3);
  wave_add(has, key, ins_len != 0, ins_len, B, 0, 1);
  wave_add(has, key, ambiguous, 0ull, B, 2, 3);
}

__global__ __launch_bounds__(CNS_BLOCK) void k_cns_write_seq(SliceView S, const uint64_t *__restrict__ ins, const uint32_t *__restrict__ out_len,
                                                             const uint64_t *__restrict__ out_off, const uint8_t *__restrict__ out_call,
                                                             const uint32_t *__restrict__ out_ins, const uint64_t *__restrict__ obase,
                                                             uint8_t *__restrict__ seq) {
  const uint64_t x = (uint64_t)blockIdx.x * CNS_BLOCK + threadIdx.x;
  if (x >= S.npos) return;
  const uint32_t n = out_len[x];
  if (!n) return;
  const uint64_t t = slice_entry(S, x);
  const uint64_t base = obase[t - S.t0];
  if (base == NOT_REPORTED) return;
  uint8_t *dst = seq + base + (out_off[x] - out_off[S.tstart[t] - S.tstart[S.t0]]);
  const uint32_t idx = out_ins[x];
  uint32_t il = 0;
  uint64_t w = 0;
  if (idx != NO_INS) {
    w = ins[2ull * idx];
    il = (uint32_t)(ins[2ull * idx + 1] & 63u) + 1u;
  }
  if (n > il) *dst++ = out_call[x];
  for (uint32_t i = 0; i < il; i++) dst[i] = (uint8_t)((0x54474341u >> (8u * (uint32_t)((w >> (2u * (il - 1u - i))) & 3u))) & 0xFFu);
}

// sorts n insertion records of `buf` by (key, bases): two stable runs of the radix sort, the less significant word first
void sort_insertions(DevBuf &buf, DevBuf &alt, uint64_t n, uint64_t max_key, SortWorkspace &ws, hipStream_t s) {
  if (n < 2) return;
  SortPass passes[8];
  for (int p = 0; p < 8; p++) passes[p] = SortPass{(uint32_t)(p / 4), (uint32_t)(8 * (p % 4)), 0u};
  void *sorted = radix_sort(buf.p, alt.p, n, 4, passes, 8, ws, s, nullptr, nullptr, nullptr);
  if (sorted != buf.p) std::swap(buf, alt);
  uint32_t bits = 1;
  while (bits < 64 && (max_key >> bits) != 0) bits++;
  const int n_passes = (int)((bits + 7) / 8);
  for (int p = 0; p < n_passes; p++) passes[p] = SortPass{(uint32_t)(2 + p / 4), (uint32_t)(8 * (p % 4)), 0u};
  sorted = radix_sort(buf.p, alt.p, n, 4, passes, n_passes, ws, s, nullptr, nullptr, nullptr);
  if (sorted != buf.p) std::swap(buf, alt);
}

}  // namespace

void consensus_count_device(const VariantInputs &in, EmitWork &W, hipStream_t s) { emit_count_device(in, W, CNS_KINDS, k_cns_count, s); }

void consensus_write_device(const VariantInputs &in, EmitWork &W, const ConsensusKeys &at, hipStream_t s) { emit_write_device(in, W, k_cns_write, at, s); }

void consensus_sort_device(ConsensusTakeWork &T, DevBuf &ev, DevBuf &mb, DevBuf &me, DevBuf &db, DevBuf &de, DevBuf &ins, const uint64_t n[CNS_KINDS],
                           uint64_t total_bases, hipStream_t s) {
  auto room = [&] {   // (a swap may have left a smaller block in T.alt)
    size_t cap = ins.cap;
    for (const DevBuf *b : {&ev, &mb, &me, &db, &de}) cap = std::max(cap, b->cap);
    T.alt.ensure(cap);
  };
  room();
  sort_keys(ev, T.alt, n[CNS_EV], total_bases << 3, T.sortws, s);
  room();
  sort_keys(mb, T.alt, n[CNS_M], total_bases, T.sortws, s);
  room();
  sort_keys(me, T.alt, n[CNS_M], total_bases, T.sortws, s);
  room();
  sort_keys(db, T.alt, n[CNS_D], total_bases, T.sortws, s);
  room();
  sort_keys(de, T.alt, n[CNS_D], total_bases, T.sortws, s);
  room();
  sort_insertions(ins, T.alt, n[CNS_INS], total_bases << 6, T.sortws, s);
}

void consensus_take_device(ConsensusTakeWork &T, const ConsensusKeys &K, const uint64_t n[CNS_KINDS], const uint64_t *d_goff, const uint8_t *d_gbases,
                           const std::vector<uint64_t> &h_goff, uint64_t n_entries, const kslam_consensus_params &P, uint64_t slice,
                           ConsensusCall &out, hipStream_t s) {
  out.rows.clear();
  out.seq_bytes = out.n_touched = 0;
  if (!n_entries || (!n[CNS_M] && !n[CNS_D])) return;
  // ---- the touched entries, as a list ----
  T.tflag.ensure(n_entries * sizeof(uint32_t));
  T.tpos.ensure(n_entries * sizeof(uint32_t));
  T.scan_tmp.ensure(scan_tmp_bytes(n_entries));
  T.totals.ensure(2 * sizeof(uint64_t));
  uint64_t *d_tot = T.totals.as<uint64_t>();
  hipLaunchKernelGGL(k_cns_touched, dim3(pileup_blocks(n_entries)), dim3(CNS_BLOCK), 0, s, d_goff, n_entries, K.mb, n[CNS_M], K.db, n[CNS_D], T.tflag.as<uint32_t>());
  HIPCHK(hipGetLastError());
  exclusive_scan_u32(T.tflag.as<uint32_t>(), T.tpos.as<uint32_t>(), n_entries, d_tot, T.scan_tmp.p, s);
  uint64_t n_touched = 0;
  read_back(&n_touched, d_tot, sizeof n_touched, s);
  out.n_touched = n_touched;
  if (!n_touched) return;
  T.tlist.ensure(n_touched * sizeof(uint32_t));
  scatter_list_device(T.tflag.as<uint32_t>(), T.tpos.as<uint32_t>(), n_entries, T.tlist.as<uint32_t>(), s);
  std::vector<uint32_t> tlist(n_touched);
  HIPCHK(hipMemcpyAsync(tlist.data(), T.tlist.p, n_touched * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(stream_wait(s));
  std::vector<uint64_t> tstart(n_touched + 1, 0);
  for (uint64_t t = 0; t < n_touched; t++) tstart[t + 1] = tstart[t] + (h_goff[tlist[t] + 1] - h_goff[tlist[t]]);
  T.tstart.ensure((n_touched + 1) * sizeof(uint64_t));
  HIPCHK(hipMemcpyAsync(T.tstart.p, tstart.data(), (n_touched + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  HIPCHK(stream_wait(s));
  // ---- slice by slice ----
  const uint64_t min_covered = P.min_covered ? P.min_covered : 1;
  std::vector<uint64_t> counters, obase;
  for (uint64_t t0 = 0; t0 < n_touched;) {
    uint64_t t1 = t0 + 1;
    while (t1 < n_touched && tstart[t1 + 1] - tstart[t0] <= slice) t1++;
    const uint64_t nt = t1 - t0, npos = tstart[t1] - tstart[t0];
    const SliceView S{T.tlist.as<uint32_t>(), T.tstart.as<uint64_t>(), t0, t1, npos};
    T.len.ensure(npos * sizeof(uint32_t));
    T.off.ensure(npos * sizeof(uint64_t));
    T.call.ensure(npos);
    T.insidx.ensure(npos * sizeof(uint32_t));
    T.counters.ensure(8 * nt * sizeof(uint64_t));
    T.scan_tmp.ensure(scan_tmp_bytes(npos));
    HIPCHK(hipMemsetAsync(T.counters.p, 0, 8 * nt * sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_cns_call, dim3(pileup_blocks(npos)), dim3(CNS_BLOCK), 0, s, S, K, n[CNS_EV], n[CNS_M], n[CNS_D], n[CNS_INS], d_goff, d_gbases, P,
                       T.len.as<uint32_t>(), T.call.as<uint8_t>(), T.insidx.as<uint32_t>(), T.counters.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    exclusive_scan_u32_to_u64(T.len.as<uint32_t>(), T.off.as<uint64_t>(), npos, d_tot + 1, T.scan_tmp.p, s);
    counters.resize(8 * nt);
    HIPCHK(hipMemcpyAsync(counters.data(), T.counters.p, 8 * nt * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
    // which entries are reported, and where their sequences go
    obase.assign(nt, NOT_REPORTED);
    const uint64_t seq_before = out.seq_bytes;
    for (uint64_t i = 0; i < nt; i++) {
      const uint64_t *A = counters.data() + 4 * i, *B = counters.data() + 4 * nt + 4 * i;
      if (A[0] < min_covered) continue;
      kslam_consensus_row r;
      memset(&r, 0, sizeof r);
      r.entry = tlist[t0 + i];
      r.seq_off = out.seq_bytes;
      r.seq_len = A[1];
      r.entry_len = tstart[t0 + i + 1] - tstart[t0 + i];
      r.covered = A[0];
      r.substitutions = A[2];
      r.deleted = A[3];
      r.insertions = B[0];
      r.inserted_bases = B[1];
      r.ambiguous = B[2];
      out.rows.push_back(r);
      obase[i] = out.seq_bytes;
      out.seq_bytes += r.seq_len;
    }
    if (out.seq_bytes > seq_before) {
      if (out.seq_bytes > T.seq.cap) {   // grow, keeping the sequences of the slices before
        DevBuf grown;
        grown.ensure(out.seq_bytes + out.seq_bytes / 2);
        if (seq_before) HIPCHK(hipMemcpyAsync(grown.p, T.seq.p, seq_before, hipMemcpyDeviceToDevice, s));
        HIPCHK(stream_wait(s));
        std::swap(T.seq, grown);
      }
      T.obase.ensure(nt * sizeof(uint64_t));
      HIPCHK(hipMemcpyAsync(T.obase.p, obase.data(), nt * sizeof(uint64_t), hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(k_cns_write_seq, dim3(pileup_blocks(npos)), dim3(CNS_BLOCK), 0, s, S, K.ins, T.len.as<uint32_t>(), T.off.as<uint64_t>(),
                         T.call.as<uint8_t>(), T.insidx.as<uint32_t>(), T.obase.as<uint64_t>(), T.seq.as<uint8_t>());
      HIPCHK(hipGetLastError());
      HIPCHK(stream_wait(s));   // (obase is the host's vector, reused by the next slice)
    }
    t0 = t1;
  }
}

}  // namespace kslam
