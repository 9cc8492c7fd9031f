// alignqc.hip -- the alignment QC report's tables, tallied on the device (include/kslam_alignqc.h).
//
// When a lane has finished a batch, its final read pairs, their alignment-pair records, the overlap records those index, the
// CIGAR pool, the read bases, the quality column (text route) and the entry bases lie in device memory.  The contributing set
// is the variants' (contributing_list_device: k_var_flag, scan, k_scatter_list -- called, not copied), so a record named by three
// live pairs is counted once.  Several lanes count into one state from their own streams, so every update of the global tables
// is a device-scope atomic; every accumulator is an integer add, so the result does not depend on who counted what in which
// order.
//
// Count pass (k_aq_count<true>): a WAVEFRONT per listed record, lane = column.  The usual record is one M run of the read's
// length; a wave-uniform loop walks the CIGAR words, and inside an M run the wave takes 64 consecutive columns per step: lane j
// loads entry[g + j], the read byte at the cycle of q + j and its quality byte.  A forward record reads ascending addresses, a
// reverse one descending ones; both are contiguous, so the loads coalesce at any alignment.  Lane j holds cycle c0 +- j: two lanes
// of one instruction never share a per-cycle row below C.  The whole CIGAR is checked first by the same wave (record_frame,
// pileup_walk.h: a uniform loop), and that check decides skip-or-count before any counter moves.  The walk is ONE template, aq_walk<WAVE>: the instantiation
// with WAVE = false is the one-thread-per-record baseline (a column at a time, every add an atomic of its own), kept to be
// measured against (KSLAM_ALIGNQC_WALK=thread selects it; tools/alignqc_bench.py); the product uses WAVE = true.
//   tile         grid = (runs of the list, tiles of AQ_TILE cycle rows, streams).  A workgroup owns AQ_TILE consecutive cycle
//                rows of ONE stream's tables and a run of the list, of which it takes the records of its stream; its LDS does
//                not depend on C.  The grid has as many tiles as the longest read of the batch needs (one for reads of 150
//                bases).  A workgroup passes over the 64-column steps none of whose cycles it owns; tile 0 walks everything (it
//                owns the per-record sums).
//   cq_compared, cq_mismatch   the hot table and its rare twin share s_q[row][95] in LDS: a 32-bit cell holds the compared
//                columns in its low half and the mismatches in its high half, so ONE ds add that returns nothing counts both
//                (1, or 0x10001 for a mismatch).  The row stride of 95 words is odd: when every lane adds to the same quality
//                value -- binned qualities -- lane i hits bank (q +- i) mod 32.
//   cycle[.][0], [.][1]   compared columns and mismatches by cycle: s_c[row], packed the same way, one word per row
//                (consecutive lanes, consecutive banks).
//   row C        the pooled row is hit by MANY lanes of one instruction, so it is reduced inside the wave first: a ballot for
//                the compared columns (and one for the mismatches among them), equal quality values combined the way
//                readqc.hip does (one LDS add per distinct value and step).  Its counters are 64-bit LDS words.  The last
//                tile of the grid owns it.
//   per record   compared and mismatches are ballots and population counts carried in wave-uniform registers, as are the four
//                ballots per step that count the matches on subst's diagonal; the twelve scalars and the diagonal are kept per
//                wave and go to 64-bit LDS words once, at the wave's end.
//   rare things  an inserted base, a deletion: their per-cycle cells (cycle columns 2 and 3) go STRAIGHT to global 64-bit
//                atomics -- below row C the lanes of an instruction hold distinct cells, in row C they are combined inside the
//                wave first.  One read in some hundred has one.  The first version sent the mismatches' per-cycle cells the
//                same way; at 1 % mismatches most 64-column steps then issue a global atomic, which (so the supposition: loads
//                and atomics share one outstanding-memory counter) the next step's loads wait for.  That version (with tiles of 128 rows, 512 threads
//                and no prefetch of the next record besides) took 9.26 ms for the batch of profiles/alignqc.json against this
//                one's 7.28 ms, and 3.95 against 1.73 ms at 8 % mismatches, where the atomics weigh most.
//                The FEW-cell tables (off-diagonal subst: 12 cells; nm: 65; identity: 101; ins_len, del_len: 65 each) go to small
//                LDS tables, combined inside the wave where several lanes can meet (subst): every workgroup would hammer the same
//                handful of global addresses otherwise (nm[0] and identity[100] take one add per clean record).
//   latency      five loads stand one behind the other between a record's place in the list and its counts; the next record is loaded
//                while this one is walked, and the list's entry of the one after.  The offsets, the CIGAR and the columns of
//                a record are still fetched one after the other: the pass is bound by those latencies, not by issue or LDS.
//   flush        once per workgroup: every non-zero LDS cell is added to its 64-bit global counter(s).
// Counter widths: a 16-bit half of a cell of s_q / s_c receives at most 1 per record the workgroup takes (the walk's query
// position only grows, so a record meets a cycle once) and a workgroup takes at most AQ_MAX_RECORDS = 65 535 records (a longer
// list gets more workgroups), so no half passes 2^16 - 1 and none carries into the other; s_nm / s_id receive exactly 1 per
// record.  Everything one record can feed more than once (row C, the scalars, subst, the length histograms: one add per run) is
// 64 bits wide.
// Occupancy: AQ_BLOCK = 1024 threads (16 waves); LDS = 160 * 96 * 4 (s_q, s_c) + 2 * 96 * 8 (row C) + (12 + 16 + 130) * 8 +
// 166 * 4 = 64 944 bytes, so two workgroups fit the 160 KB of a CU: 32 waves, 8 per SIMD, which leaves 64 VGPRs per lane; the
// wave instantiation needs 47.  (The baseline instantiation needs 105 and gets one workgroup per CU.)
// Pair pass (k_aq_pairs): one thread per alignment-pair RECORD, liveness as k_var_flag finds it; the three pair counters are
// ballots, insert_sum a wave sum (wave_add.h), equal insert bins are combined inside the wave before the atomic.  n_read_pairs
// is a ballot over the groups (k_aq_groups).
// Bounds: a record is walked only after record_frame held (pileup_walk.h: read < n_reads, entry < n_entries, its CIGAR slice inside
// the pool and every M, I and D run inside the read and the entry); a lane loads entry[rp + j] and read / quality[cycle] only for j below the run's
// length, so every index lies inside the entry and the read; a row index below C is < row_end <= C; the bins are clamped.
#include "pileup_walk.h"
#include "wave_add.h"
#include "../../include/kslam_alignqc.h"

namespace kslam {

namespace {

constexpr int AQ_BLOCK = 1024;                // 16 waves share one tile
constexpr int AQ_WAVES = AQ_BLOCK / 64;
constexpr int AQ_PAIR_BLOCK = 256;
constexpr uint32_t AQ_TILE = 160;              // cycle rows per workgroup: a read of 150 bases needs one tile
constexpr uint32_t AQ_QS = KSLAM_ALIGN_QC_QUAL_COLS;   // 95: the quality row's stride
constexpr uint32_t AQ_MAX_BLOCKS = 512;        // runs of the list: two workgroups per CU
constexpr uint64_t AQ_RECORDS = 256;           // the fewest records a workgroup takes (more when the grid is full) ...
constexpr uint64_t AQ_MAX_RECORDS = 65535;     // ... and the most: the 16-bit halves of an LDS cell
constexpr uint32_t AQ_NONE = 0xFFFFFFFFu;
constexpr uint32_t NQ = KSLAM_ALIGN_QC_QUAL_COLS, NC = KSLAM_ALIGN_QC_CYCLE_COLS, NL = KSLAM_ALIGN_QC_LEN_BINS, NN = KSLAM_ALIGN_QC_NM_BINS,
                   NI = KSLAM_ALIGN_QC_IDENTITY_BINS, NS = KSLAM_ALIGN_QC_INSERT_BINS, NSC = KSLAM_ALIGN_QC_SCALARS;

// a stream's words (include/kslam_alignqc.h)
__host__ __device__ inline uint64_t aq_stream(uint32_t C, uint32_t z) { return KSLAM_ALIGN_QC_REPORT_WORDS + (uint64_t)z * KSLAM_ALIGN_QC_STREAM_WORDS(C); }
constexpr uint64_t AQ_SUBST = NSC, AQ_ILEN = AQ_SUBST + 16, AQ_DLEN = AQ_ILEN + NL, AQ_NM = AQ_DLEN + NL, AQ_ID = AQ_NM + NN, AQ_CYCLE = AQ_ID + NI;
__host__ __device__ inline uint64_t aq_cqc(uint32_t C) { return AQ_CYCLE + ((uint64_t)C + 1) * NC; }
__host__ __device__ inline uint64_t aq_cqm(uint32_t C) { return aq_cqc(C) + ((uint64_t)C + 1) * NQ; }

__device__ inline uint32_t qual_col(uint32_t q) { return q - 33u <= 93u ? q - 33u : 94u; }

// how many of the group's lanes hold p: the wavefront's, or the one thread's
template <bool WAVE>
__device__ inline uint32_t cnt(bool p) {
  if constexpr (WAVE) return (uint32_t)__popcll(__ballot(p));
  else return p ? 1u : 0u;
}
// tab[key] += 1 for every lane with `has`; lanes that share a key go to memory as one add
template <bool WAVE>
__device__ inline void keyed_add(bool has, uint32_t key, unsigned long long *tab, int lane) {
  if constexpr (WAVE) {
    uint64_t pending = __ballot(has);
    while (pending) {
      const int leader = __ffsll((long long)pending) - 1;
      const uint32_t k0 = __shfl(key, leader);
      const uint64_t m = __ballot(has && key == k0);
      if (lane == leader) atomicAdd(tab + k0, (unsigned long long)__popcll(m));
      pending &= ~m;
    }
  } else if (has) {
    atomicAdd(tab + key, 1ull);
  }
}

struct AqShared {                 // the workgroup's LDS
  uint32_t *q, *c;                // [AQ_TILE * 95], [AQ_TILE]: compared in the low half of a cell, mismatches in the high half
  unsigned long long *tail, *tailm;   // row C, compared and mismatches: [0] the row's count, then its 95 quality columns
  unsigned long long *scal, *subst, *ilen, *dlen;   // [12], [16], [65], [65]
  uint32_t *nm, *id;              // [65], [101]
};
struct AqTile {                   // what this workgroup owns
  uint32_t C;
  uint64_t row0, row_end;         // ordinary rows [row0, row_end)
  bool owns_tail, owns_rec;
  unsigned long long *g_cycle;    // the stream's cycle table (global)
};
struct AqAcc {                    // per wave (per thread in the baseline): uniform registers
  unsigned long long s[NSC] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long diag[4] = {0, 0, 0, 0};
};

// One record, by the 64 lanes of a wavefront together (WAVE) or by one thread.  Every lane of the wavefront calls it with the
// same record.
template <bool WAVE>
__device__ inline void aq_walk(const kslam_overlap &o, const VariantInputs &in, const uint8_t *__restrict__ rqual, const AqShared &S, const AqTile &T,
                               AqAcc &acc, int lane) {
  constexpr uint32_t STEP = WAVE ? 64u : 1u;
  const bool lead = WAVE ? lane == 0 : true;
  const uint32_t C = T.C;
  if (T.owns_rec) {
    acc.s[0]++;
    if (!rqual) acc.s[3]++;
  }
  RecordFrame f;   // (every lane holds the same record: the return is wave-uniform)
  if (!record_frame(o, in, f)) {
    if (T.owns_rec) acc.s[2]++;
    return;
  }
  const uint32_t *__restrict__ cig = f.cig;
  const uint64_t rb = f.rb, gb = f.gb;
  const int64_t L = f.L, q0 = f.q0;
  const uint8_t *__restrict__ ref = in.gbases + gb;
  const uint8_t *__restrict__ read = in.rbases + rb;
  const uint8_t *__restrict__ qual = rqual ? rqual + rb : nullptr;
  const bool rc = o.revcomp != 0, have_q = qual != nullptr;
  // does this workgroup own a row that the cycles of query positions [qa, qb] reach?
  auto reaches = [&](int64_t qa, int64_t qb) {
    if (T.owns_rec) return true;
    const int64_t lo = rc ? L - 1 - qb : qa, hi = rc ? L - 1 - qa : qb;
    return (lo < (int64_t)T.row_end && hi >= (int64_t)T.row0) || (T.owns_tail && hi >= (int64_t)C);
  };
  auto mine = [&](int64_t cyc) { return cyc < (int64_t)C ? (cyc >= (int64_t)T.row0 && cyc < (int64_t)T.row_end) : T.owns_tail; };
  uint64_t mcols = 0, compared = 0, miss = 0, ins = 0, del = 0;
  int64_t rp = o.ref_begin, qp = q0;
  for (uint32_t k = 0; k < o.cigar_len; k++) {
    const uint32_t c = cig[k], op = c & 15u;
    const int64_t len = c >> 4;
    if (op == 0) {
      for (int64_t i0 = 0; i0 < len; i0 += STEP) {
        const int64_t i1 = i0 + STEP < len ? i0 + STEP : len;   // the step's columns: [i0, i1)
        if (!reaches(qp + i0, qp + i1 - 1)) continue;
        const int64_t j = i0 + lane;
        const bool ok = j < len;
        const int64_t cyc = ok ? (rc ? L - 1 - (qp + j) : qp + j) : 0;
        const uint32_t r = ok ? ref[rp + j] : 0u, b = ok ? read[cyc] : 0u;
        const uint32_t qc = qual_col(ok && have_q ? qual[cyc] : 0u);
        const uint32_t rk = acgt(r), qk = acgt(rc ? complement(b) : b);
        const bool cmp = ok && rk < 4u && qk < 4u, mis = cmp && rk != qk;
        const bool own = ok && mine(cyc), low = cyc < (int64_t)C;
        if (cmp && own && low) {   // one add counts the column and, in the cell's high half, its mismatch
          const uint32_t row = (uint32_t)(cyc - (int64_t)T.row0), one = mis ? 0x10001u : 1u;
          atomicAdd(&S.c[row], one);
          if (have_q) atomicAdd(&S.q[row * AQ_QS + qc], one);
        }
        if (T.owns_tail) {   // row C: many lanes of one instruction
          const bool t = cmp && !low;
          const uint32_t n = cnt<WAVE>(t);
          if (n) {
            if (lead) atomicAdd(&S.tail[0], (unsigned long long)n);
            if (have_q) keyed_add<WAVE>(t, qc, S.tail + 1, lane);
            const bool tm = mis && !low;
            const uint32_t n_tm = cnt<WAVE>(tm);
            if (n_tm) {
              if (lead) atomicAdd(&S.tailm[0], (unsigned long long)n_tm);
              if (have_q) keyed_add<WAVE>(tm, qc, S.tailm + 1, lane);
            }
          }
        }
        const uint32_t n_mis = cnt<WAVE>(mis);
        if (n_mis && T.owns_rec) keyed_add<WAVE>(mis, rc ? 4u * (3u - rk) + (3u - qk) : 4u * rk + qk, S.subst, lane);
        if (T.owns_rec) {
          compared += cnt<WAVE>(cmp);
          miss += n_mis;
#pragma unroll
          for (uint32_t x = 0; x < 4; x++) acc.diag[x] += cnt<WAVE>(cmp && !mis && (rc ? 3u - rk : rk) == x);
        }
      }
      mcols += (uint64_t)len;
      rp += len;
      qp += len;
    } else if (op == 1) {
      if (len) {
        for (int64_t i0 = 0; i0 < len; i0 += STEP) {
          const int64_t i1 = i0 + STEP < len ? i0 + STEP : len;
          if (!reaches(qp + i0, qp + i1 - 1)) continue;
          const int64_t j = i0 + lane;
          const bool ok = j < len;
          const int64_t cyc = ok ? (rc ? L - 1 - (qp + j) : qp + j) : 0;
          const bool own = ok && mine(cyc), low = cyc < (int64_t)C;
          if (own && low) atomicAdd(T.g_cycle + (uint64_t)cyc * NC + 2, 1ull);
          if (T.owns_tail) {
            const uint32_t n = cnt<WAVE>(ok && !low);
            if (n && lead) atomicAdd(T.g_cycle + (uint64_t)C * NC + 2, (unsigned long long)n);
          }
        }
        if (T.owns_rec) {
          acc.s[7]++;
          if (lead) atomicAdd(&S.ilen[(len < (int64_t)NL ? len : (int64_t)NL) - 1], 1ull);
        }
      }
      ins += (uint64_t)len;
      qp += len;
    } else if (op == 2) {
      if (len) {
        if (L > 0) {   // at the cycle where the walk stands
          const int64_t qd = qp < L - 1 ? qp : L - 1, cyc = rc ? L - 1 - qd : qd;
          if (lead && mine(cyc)) atomicAdd(T.g_cycle + (uint64_t)(cyc < (int64_t)C ? cyc : (int64_t)C) * NC + 3, 1ull);
        }
        if (T.owns_rec) {
          acc.s[9]++;
          if (lead) atomicAdd(&S.dlen[(len < (int64_t)NL ? len : (int64_t)NL) - 1], 1ull);
        }
      }
      del += (uint64_t)len;
      rp += len;
    }
  }
  if (T.owns_rec) {
    if (rc) acc.s[1]++;
    acc.s[4] += mcols;
    acc.s[5] += compared;
    acc.s[6] += miss;
    acc.s[8] += ins;
    acc.s[10] += del;
    acc.s[11] += (uint64_t)L - mcols - ins;
    if (lead) {
      const uint64_t edits = miss + ins + del, den = compared + ins + del;
      atomicAdd(&S.nm[edits < NN - 1 ? edits : NN - 1], 1u);
      if (den) atomicAdd(&S.id[100 * (compared - miss) / den], 1u);
    }
  }
}

// Workgroup x takes the rpb records from x * rpb on of the list, those of stream blockIdx.z; blockIdx.y is its tile.  tail_tile:
// the tile that owns row C (AQ_NONE: no read of the batch is longer than C).  half: the first read of stream 1 (all ones when
// the batch is single-end: no read reaches it).
template <bool WAVE>
__global__ __launch_bounds__(AQ_BLOCK) void k_aq_count(VariantInputs in, const uint8_t *__restrict__ rqual, const uint32_t *__restrict__ list,
                                                       uint64_t n_list, uint64_t rpb, AlignQcTable G, uint64_t half, uint32_t tail_tile) {
  __shared__ uint32_t s_q[AQ_TILE * AQ_QS];
  __shared__ uint32_t s_c[AQ_TILE];
  __shared__ unsigned long long s_tail[1 + NQ], s_tailm[1 + NQ];
  __shared__ unsigned long long s_scal[NSC], s_subst[16], s_ilen[NL], s_dlen[NL];
  __shared__ uint32_t s_nm[NN], s_id[NI];

  const uint32_t C = G.C, tile = blockIdx.y, stream = blockIdx.z;
  unsigned long long *const W = G.words + aq_stream(C, stream);
  AqTile T;
  T.C = C;
  T.row0 = (uint64_t)tile * AQ_TILE;
  T.row_end = T.row0 + AQ_TILE < C ? T.row0 + AQ_TILE : C;
  T.owns_tail = tile == tail_tile;
  T.owns_rec = tile == 0;
  T.g_cycle = W + AQ_CYCLE;
  const AqShared S{s_q, s_c, s_tail, s_tailm, s_scal, s_subst, s_ilen, s_dlen, s_nm, s_id};
  uint64_t b_lo = (uint64_t)blockIdx.x * rpb, b_hi = b_lo + rpb;
  if (b_lo > n_list) b_lo = n_list;
  if (b_hi > n_list) b_hi = n_list;

  for (uint32_t i = threadIdx.x; i < AQ_TILE * AQ_QS; i += AQ_BLOCK) s_q[i] = 0;
  if (threadIdx.x < AQ_TILE) s_c[threadIdx.x] = 0;
  if (threadIdx.x < 1 + NQ) s_tail[threadIdx.x] = s_tailm[threadIdx.x] = 0;
  if (threadIdx.x < NSC) s_scal[threadIdx.x] = 0;
  if (threadIdx.x < 16) s_subst[threadIdx.x] = 0;
  if (threadIdx.x < NL) s_ilen[threadIdx.x] = s_dlen[threadIdx.x] = 0;
  if (threadIdx.x < NN) s_nm[threadIdx.x] = 0;
  if (threadIdx.x < NI) s_id[threadIdx.x] = 0;
  __syncthreads();

  const int lane = WAVE ? (int)(threadIdx.x & 63) : 0;
  const uint32_t unit = WAVE ? (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x;
  constexpr uint32_t UNITS = WAVE ? AQ_WAVES : AQ_BLOCK;
  AqAcc acc;
  // Five loads stand one behind the other between a record's place in the list and its counts (the list, the record, its
  // offsets, its CIGAR, its columns), and a read of 150 bases is three steps of work: so the record after this one is loaded
  // while this one is walked, and the list's entry of the one after that.
  uint64_t x = b_lo + unit;
  kslam_overlap o;
  if (x < b_hi) o = in.ov[list[x]];
  uint32_t idx_next = x + UNITS < b_hi ? list[x + UNITS] : 0u;
  for (; x < b_hi; x += UNITS) {
    kslam_overlap o_next;
    if (x + UNITS < b_hi) o_next = in.ov[idx_next];
    if (x + 2 * UNITS < b_hi) idx_next = list[x + 2 * UNITS];
    if ((o.read >= half ? 1u : 0u) == stream) aq_walk<WAVE>(o, in, rqual, S, T, acc, lane);
    o = o_next;
  }
  if (T.owns_rec && (WAVE ? lane == 0 : true)) {
#pragma unroll
    for (uint32_t k = 0; k < NSC; k++)
      if (acc.s[k]) atomicAdd(&s_scal[k], acc.s[k]);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
      if (acc.diag[k]) atomicAdd(&s_subst[5 * k], acc.diag[k]);
  }
  __syncthreads();

  // the flush: non-zero cells only
  unsigned long long *const g_cqc = W + aq_cqc(C), *const g_cqm = W + aq_cqm(C);
  for (uint32_t i = threadIdx.x; i < AQ_TILE * AQ_QS; i += AQ_BLOCK) {
    const uint32_t v = s_q[i];
    const uint64_t row = T.row0 + i / AQ_QS;
    if (v && row < T.row_end) {
      atomicAdd(g_cqc + row * NQ + i % AQ_QS, (unsigned long long)(v & 0xFFFFu));
      if (v >> 16) atomicAdd(g_cqm + row * NQ + i % AQ_QS, (unsigned long long)(v >> 16));
    }
  }
  if (threadIdx.x < AQ_TILE) {
    const uint32_t v = s_c[threadIdx.x];
    const uint64_t row = T.row0 + threadIdx.x;
    if (v && row < T.row_end) {
      atomicAdd(T.g_cycle + row * NC, (unsigned long long)(v & 0xFFFFu));
      if (v >> 16) atomicAdd(T.g_cycle + row * NC + 1, (unsigned long long)(v >> 16));
    }
  }
  if (T.owns_tail && threadIdx.x < 1 + NQ) {
    const unsigned long long v = s_tail[threadIdx.x], m = s_tailm[threadIdx.x];
    if (threadIdx.x == 0) {
      if (v) atomicAdd(T.g_cycle + (uint64_t)C * NC, v);
      if (m) atomicAdd(T.g_cycle + (uint64_t)C * NC + 1, m);
    } else {
      if (v) atomicAdd(g_cqc + (uint64_t)C * NQ + (threadIdx.x - 1), v);
      if (m) atomicAdd(g_cqm + (uint64_t)C * NQ + (threadIdx.x - 1), m);
    }
  }
  if (T.owns_rec) {
    if (threadIdx.x < NSC && s_scal[threadIdx.x]) atomicAdd(W + threadIdx.x, s_scal[threadIdx.x]);
    if (threadIdx.x < 16 && s_subst[threadIdx.x]) atomicAdd(W + AQ_SUBST + threadIdx.x, s_subst[threadIdx.x]);
    if (threadIdx.x < NL && s_ilen[threadIdx.x]) atomicAdd(W + AQ_ILEN + threadIdx.x, s_ilen[threadIdx.x]);
    if (threadIdx.x < NL && s_dlen[threadIdx.x]) atomicAdd(W + AQ_DLEN + threadIdx.x, s_dlen[threadIdx.x]);
    if (threadIdx.x < NN && s_nm[threadIdx.x]) atomicAdd(W + AQ_NM + threadIdx.x, (unsigned long long)s_nm[threadIdx.x]);
    if (threadIdx.x < NI && s_id[threadIdx.x]) atomicAdd(W + AQ_ID + threadIdx.x, (unsigned long long)s_id[threadIdx.x]);
  }
}

// one thread per alignment-pair record; every lane stays to the end (the wave sums need them all)
__global__ __launch_bounds__(AQ_PAIR_BLOCK) void k_aq_pairs(VariantInputs in, unsigned long long *__restrict__ words) {
  const uint64_t i = (uint64_t)blockIdx.x * AQ_PAIR_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool live = false;
  if (i < in.n_pairs && in.n_groups) {
    uint64_t lo = 0, hi = in.n_groups;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (in.groups[mid].first <= i) lo = mid;
      else hi = mid;
    }
    const uint64_t first = in.groups[lo].first;
    live = first <= i && i - first < in.groups[lo].count;
  }
  uint32_t r1 = KSLAM_NO_OVERLAP, r2 = KSLAM_NO_OVERLAP, isz = 0;
  if (live) {
    r1 = in.pairs[i].r1;
    r2 = in.pairs[i].r2;
    isz = in.pairs[i].insert_size;
  }
  const bool h1 = r1 != KSLAM_NO_OVERLAP, h2 = r2 != KSLAM_NO_OVERLAP, both = h1 && h2;
  const uint32_t n_both = cnt<true>(both), n_1 = cnt<true>(h1 && !h2), n_2 = cnt<true>(h2 && !h1);
  if (!(n_both | n_1 | n_2)) return;   // (uniform)
  const uint64_t sum = n_both ? wave_sum(both ? (uint64_t)isz : 0ull) : 0ull;
  if (lane == 0) {
    if (n_both) atomicAdd(words + 1, (unsigned long long)n_both);
    if (n_1) atomicAdd(words + 2, (unsigned long long)n_1);
    if (n_2) atomicAdd(words + 3, (unsigned long long)n_2);
    if (sum) atomicAdd(words + 4, (unsigned long long)sum);
  }
  keyed_add<true>(both, isz < NS - 1 ? isz : NS - 1, words + 6, lane);
}

__global__ __launch_bounds__(AQ_PAIR_BLOCK) void k_aq_groups(const kslam_read_pair *__restrict__ groups, uint64_t n, unsigned long long *__restrict__ words) {
  const uint64_t i = (uint64_t)blockIdx.x * AQ_PAIR_BLOCK + threadIdx.x;
  const uint32_t m = cnt<true>(i < n && groups[i].count != 0);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(words, (unsigned long long)m);
}

inline unsigned pair_blocks(uint64_t n) { return (unsigned)((n + AQ_PAIR_BLOCK - 1) / AQ_PAIR_BLOCK); }

}  // namespace

void alignqc_zero_device(const AlignQcTable &T, hipStream_t s) { HIPCHK(hipMemsetAsync(T.words, 0, KSLAM_ALIGN_QC_WORDS(T.C) * sizeof(uint64_t), s)); }

void alignqc_count_device(const VariantInputs &in, const uint8_t *d_quality, bool paired, uint64_t max_len, const AlignQcTable &T, AlignQcWork &W,
                          bool timed, bool thread_per_record, hipStream_t s) {
  if (timed) {
    W.ms = 0;
    if (!W.ev[0])
      for (auto &e : W.ev) HIPCHK(hipEventCreate(&e));
  }
  // the pairs and the groups
  if (in.n_groups) {
    if (in.n_pairs >= (1ull << 39) || in.n_groups >= (1ull << 39)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^39 or more alignment pairs in one batch"};
    hipLaunchKernelGGL(k_aq_groups, dim3(pair_blocks(in.n_groups)), dim3(AQ_PAIR_BLOCK), 0, s, in.groups, in.n_groups, T.words);
    if (in.n_pairs) hipLaunchKernelGGL(k_aq_pairs, dim3(pair_blocks(in.n_pairs)), dim3(AQ_PAIR_BLOCK), 0, s, in, T.words);
    HIPCHK(hipGetLastError());
  }
  // the contributing records, as the variants list them
  const uint64_t n_list = contributing_list_device(in, W.flag, W.pos, W.list, W.scan_tmp, W.totals, s);
  if (timed) HIPCHK(hipEventRecord(W.ev[0], s));
  if (n_list) {
    const uint32_t C = T.C;
    // tiles: the ordinary rows the longest read reaches; with a read longer than C all of them, and the last one owns row C
    const uint64_t reach = max_len < C ? max_len : C;
    uint32_t n_tiles = (uint32_t)((reach + AQ_TILE - 1) / AQ_TILE);
    if (!n_tiles) n_tiles = 1;
    const uint32_t tail_tile = max_len > C ? n_tiles - 1 : AQ_NONE;
    uint64_t rpb = (n_list + AQ_MAX_BLOCKS - 1) / AQ_MAX_BLOCKS;
    if (rpb < AQ_RECORDS) rpb = AQ_RECORDS;
    if (rpb > AQ_MAX_RECORDS) rpb = AQ_MAX_RECORDS;   // (more workgroups instead: no half of a cell passes 2^16 - 1)
    const dim3 grid((unsigned)((n_list + rpb - 1) / rpb), n_tiles, paired ? 2 : 1);
    const uint64_t half = paired ? in.n_reads / 2 : ~0ull;
    if (thread_per_record)
      hipLaunchKernelGGL(k_aq_count<false>, grid, dim3(AQ_BLOCK), 0, s, in, d_quality, W.list.as<uint32_t>(), n_list, rpb, T, half, tail_tile);
    else
      hipLaunchKernelGGL(k_aq_count<true>, grid, dim3(AQ_BLOCK), 0, s, in, d_quality, W.list.as<uint32_t>(), n_list, rpb, T, half, tail_tile);
    HIPCHK(hipGetLastError());
  }
  if (timed) {
    HIPCHK(hipEventRecord(W.ev[1], s));
    HIPCHK(stream_wait(s));
    HIPCHK(hipEventElapsedTime(&W.ms, W.ev[0], W.ev[1]));
  }
}

}  // namespace kslam
