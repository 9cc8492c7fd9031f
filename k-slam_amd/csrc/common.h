// common.h -- shared declarations of the HIP implementation (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <time.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "../../include/kslam.h"

namespace kslam {

constexpr int WAVE = 64;

struct HipError {
  hipError_t code;
  const char *what;
  const char *file;
  int line;
};

#define HIPCHK(expr)                                                      \
  do {                                                                    \
    hipError_t _e = (expr);                                               \
    if (_e != hipSuccess) throw ::kslam::HipError{_e, #expr, __FILE__, __LINE__}; \
  } while (0)

struct StatusError {
  kslam_status st;
  std::string msg;
};

// The KSLAM_* environment switches.  They are read ONCE per context, when
// kslam_create builds it (kslam_reload_tuning re-reads them: variant tests and tuning scripts), never on
// the batch path, and none of them changes a result.  The measurement-only ablations that DO change
// results (parts of kernels switched off) only exist in a -DKSLAM_ABLATE build (make ABLATE=1).
struct Tuning {
  bool debug = false;                 // KSLAM_DEBUG: per-stage counts on stderr
  bool sw_full = false;               // KSLAM_SW_FULL=1: every candidate on the full-matrix scoring kernel
  bool sw_no48 = false, sw_no96 = false;   // KSLAM_SW_NO48 / _NO96: drop a band tier
  int sw_unknown_nd = 0;              // KSLAM_SW_UNKNOWN_ND: where gapped candidates start (0: by read length)
  int cigar_sys_mask = 0xF8;          // KSLAM_CIGAR_SYS: band-width bins (cigar.hip: cig_bin) that run on the systolic kernel, one bit each
  bool cigar_reg = true;              // KSLAM_CIGAR_REG=0: no band-in-registers kernel
  int bucket_bits_max = 27;           // KSLAM_BUCKET_BITS
  int bucket_bits_exact = 0;          // KSLAM_BUCKET_BITS_EXACT (0: sized from the index)
  int filter_bits = -1;               // KSLAM_FILTER_BITS (-1: sized from the index, 0: no filter)
  int sort_bytes = -1;                // KSLAM_SORT_BYTES (-1: what the bucket table needs)
  bool sort_digit_bytes = true;       // KSLAM_SORT_DIGIT_BYTES=0: histograms re-read the records
  int lanes = 2;                      // KSLAM_LANES
  bool eager_cigar = false;           // KSLAM_EAGER_CIGAR
  bool lane_waits_yield = false;      // KSLAM_LANE_WAITS=yield: the pipeline lanes poll + sleep instead of busy-waiting for the GPU (stream_wait)
  bool pageable_columns = false;      // KSLAM_PAGEABLE_COLUMNS
  bool details_in_token = true;       // KSLAM_DETAILS_IN_TOKEN=0 (A/B): the per-row walk outside the lanes' compute token
  int plan_blocks_per_cu = 64;        // KSLAM_PLAN_BLOCKS: workgroups of k_sw_plan per CU (its waves walk through the candidates)
  int join_group_order = 1;           // KSLAM_JOIN_GROUP_ORDER=0: the overlap keys go through all their radix passes (join.hip: group_order)
  bool sweep_room = true;             // KSLAM_SWEEP_ROOM=0 (tests): the CIGAR bins' and SW tiers' launches get NO room for what earlier ones send
                                      // on, so that every such candidate takes the left-over rounds
  int join_merge = 0;                 // KSLAM_JOIN=merge: k_join_merge instead of the probe k_join_fill (join.hip)
  bool filter_build_sorted = true;    // KSLAM_FILTER_BUILD=atomics: the membership filter by scattered atomics instead of block by block (filter.hip)
  int pseudo_cap = 0;                 // KSLAM_PSEUDO_CAP (tests): alignment pairs of one entry beyond which pseudo-assembly is left to the host; 0 = 262144
#ifdef KSLAM_ABLATE
  uint32_t sw_ablate = 0, cigar_variant = 0, filter_ablate = 0;   // KSLAM_SW_ABLATE / _CIGAR_VARIANT / _FILTER_ABLATE
#endif
};
Tuning read_tuning();   // kslam_api.hip

// grow-only device buffer that owns its block.  No copy-assignment: `a = b` would free the block twice.  A buffer
// several contexts read is shared through the object holding it (GenomeIndex, context.h), never through a second DevBuf.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  ~DevBuf() { if (p) (void)hipFree(p); }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p; cap = o.cap;
      o.p = nullptr; o.cap = 0;
    }
    return *this;
  }
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    release();
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      throw StatusError{KSLAM_ERR_OOM, "hipMalloc of " + std::to_string(want) + " bytes failed"};
    }
    cap = want;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// ---- base coding shared by the SW and cigar kernels (branch-free) ---------------------------
#ifdef __HIPCC__
// kBaseTranslation (reference src/ssw_cpp.cpp:11-23): A/a 0, C/c 1, G/g 2, T/t 3, U/u 0, else 4
__device__ inline uint32_t ssw_code(uint32_t c) {
  const uint32_t idx = c & 31u;                                        // A 1, C 3, G 7, T 20, U 21
  const bool known = ((c & 0xC0u) == 0x40u) && ((0x0030008Au >> idx) & 1u);
  const uint32_t code = (uint32_t)(((1ull << 6) | (2ull << 14) | (3ull << 40)) >> (2u * idx)) & 3u;
  return known ? code : 4u;
}
// the same after inPlaceReverseComplement's per-base step (reference src/sequenceTools.h:98-116):
// only UPPER-case A/C/G/T are complemented, every other character is left as it is
__device__ inline uint32_t ssw_code_complemented(uint32_t c) {
  const uint32_t idx = c & 31u;
  const uint32_t code = ssw_code(c);
  const bool upper_acgt = ((c & 0xE0u) == 0x40u) && ((0x0010008Au >> idx) & 1u);
  return upper_acgt ? 3u - code : code;
}
#endif

// ---------------------------------------------------------------- scan.hip
// exclusive scan of n u32 values; out may be u32 or u64. total (u64) is
// written to d_total[0].  tmp must hold scan_tmp_bytes(n).
size_t scan_tmp_bytes(uint64_t n);
void exclusive_scan_u32(const uint32_t *d_in, uint32_t *d_out, uint64_t n,
                        uint64_t *d_total, void *d_tmp, hipStream_t s);
void exclusive_scan_u32_to_u64(const uint32_t *d_in, uint64_t *d_out, uint64_t n,
                               uint64_t *d_total, void *d_tmp, hipStream_t s);

// Lists of candidate numbers by bin that grow while kernels run: the SW tiers (sw.hip) and the CIGAR band-width bins
// (cigar.hip).  A kernel of one bin appends what it does not finish to the list of a later bin.
struct BinLists {
  uint32_t *list[8];   // list[b]: the numbers in bin b (nullptr: a bin that cannot occur)
  uint32_t *count;     // [8] entries of each list (nullptr: nothing is appended)
};
// Stable 8-way partition of the element numbers 0..n-1 by d_bins[i] (bins >= 8 are left out):
// B.list[k] receives bin k's numbers in order, B.count[k] its size.
void partition_bins(const uint8_t *d_bins, uint64_t n, const BinLists &B, DevBuf &pos, hipStream_t s);
// The entries [first, first + cap) of a list that one launch covers.  With count_dev, cap is a CAPACITY: the list was
// still growing when the host sized the launch, and its workgroups read its real length when they run.  The first
// `sure` entries of the slice existed when the host looked; a workgroup inside them does not wait for that load.
struct ListSlice {
  const uint32_t *list;
  uint32_t first, cap, sure;
  const uint32_t *count_dev;
};
#ifdef __HIPCC__
// entries of the slice that exist, for a workgroup whose entries end before hi (counted from `first`)
__device__ inline uint32_t live_len(const ListSlice &S, uint32_t hi) {
  if (!S.count_dev || hi <= S.sure) return S.cap;
  const uint32_t tot = *S.count_dev;
  return min(S.cap, tot > S.first ? tot - S.first : 0u);
}
// wave-aggregated append of v to a list (one atomic per wave)
__device__ inline void wave_append(bool want, uint32_t v, uint32_t *list, uint32_t *count) {
  const uint64_t m = __ballot(want);
  if (!m) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t leader = (uint32_t)__builtin_ctzll(m);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = __shfl((int)base, (int)leader, 64);
  if (want) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = v;
}
// the same into the list of bin `dest` (< 0: nothing; lanes of a wave may differ in it): one atomic per wave and bin
__device__ inline void wave_append_to_bin(const BinLists &B, int dest, uint32_t v) {
  if (!B.count) return;
  for (;;) {
    const uint64_t m = __ballot(dest >= 0);
    if (!m) break;
    const int d0 = __shfl(dest, (int)__builtin_ctzll(m), 64);
    wave_append(dest == d0, v, B.list[d0], B.count + d0);
    if (dest == d0) dest = -1;
  }
}
#endif
// The sweep over bins 0 .. n_bins - 1 of such lists, with as few read-backs as it can.  Pass one launches every bin with
// first_cap[b] > 0 at once, sized for that capacity, with the list's counter (count_dev) for its workgroups to read:
// when the host queues a bin it cannot know what the bins before it will append.  Then rounds, each after one read-back
// of the counters into h (h_bytes of them): a round first calls `round_hook` (a list of the caller's own, outside the
// bins: true if it launched something), then launches, per bin, the entries nobody has launched yet (count_dev nullptr:
// m is exact), until a round finds nothing new.  `step`: no pass one, and a read-back after every launch, so that each
// bin runs once, whole (a caller that has nothing to size the capacities from).  h must hold the counters on entry
// and holds them on return.  launch(bin, m, first, count_dev, sure, round): round -1 is pass one.
using SweepLaunch = std::function<void(uint32_t bin, uint64_t m, uint32_t first, const uint32_t *count_dev, uint32_t sure, int round)>;
void sweep_lists(uint32_t n_bins, const uint32_t *d_counts, uint32_t *h, size_t h_bytes, const uint64_t *first_cap, bool step,
                 const SweepLaunch &launch, const std::function<bool(int round)> &round_hook, hipStream_t s);

// ------------------------------------------------------------- extract.hip
struct SegEntry {   // one wave-sized unit of extraction work
  uint32_t seq;     // sequence index (read id / entry id)
  uint32_t q0;      // first k-mer index of the segment inside the sequence
  uint64_t out;     // record index of k-mer q0 in the output
};
constexpr uint32_t SEG_KMERS = 128;  // k-mers per segment
constexpr uint32_t MAX_GAP = 64;

struct ExtractPlan {
  uint64_t n_seqs = 0;
  uint64_t n_kmers = 0;
  uint64_t n_segs = 0;
};
// Sizes the work (device scans) and fills the segment table.
// d_nk / d_nseg: u32[n] scratch; d_rec_start: u64[n]; d_seg_start: u64[n]
void extract_plan(const uint64_t *d_offsets, uint64_t n_seqs, uint32_t gap,
                  uint32_t *d_nk, uint32_t *d_nseg, uint64_t *d_rec_start,
                  uint64_t *d_seg_start, uint64_t *d_totals /*[2]*/, void *d_scan_tmp,
                  hipStream_t s);
void extract_fill_segments(const uint32_t *d_nk, const uint64_t *d_rec_start,
                           const uint64_t *d_seg_start, uint64_t n_seqs, uint32_t gap,
                           SegEntry *d_segs, hipStream_t s, uint64_t n_segs = ~0ull);
// AoS output (reference record layout); id_base is added to the sequence index.  d_digits != nullptr: also the digit of
// *first_pass of every record, one byte at the record's index (the first histogram of the sort that follows reads those
// instead of the records: radix_sort.hip, SortWorkspace::first_digits_ready)
struct SortPass;
void extract_kmers_launch(const uint8_t *d_bases, const uint64_t *d_offsets,
                          const SegEntry *d_segs, uint64_t n_segs, uint32_t gap,
                          int is_gb, uint32_t id_base, uint4 *d_out, hipStream_t s,
                          uint8_t *d_digits = nullptr, const SortPass *first_pass = nullptr);

// -------------------------------------------------------------- filter.hip
// Blocked Bloom filter over the genome k-mer set (2^log2_bits bits, 128-byte lines chosen by the
// k-mer's minimizer) and the read extraction kernel that keeps only the k-mers the filter lets through.
size_t filter_bytes(uint32_t log2_bits);
void filter_build(const uint64_t *d_sorted_keys, uint32_t n, uint32_t log2_bits, void *d_filter, hipStream_t s);
// the same filter, built from the keys' probe words ordered by 32 KB filter block, each block assembled in LDS (filter.hip);
// d_words_a / _b: n + 1 u64 each; d_block_start: (filter bytes / 32 KB) + 2 u32
struct SortWorkspace;
void filter_build_sorted(const uint64_t *d_sorted_keys, uint32_t n, uint32_t log2_bits, void *d_filter, void *d_words_a, void *d_words_b,
                         uint32_t *d_block_start, SortWorkspace &ws, hipStream_t s, bool words_ready = false);
// One pass over the sorted genome records for all of: the key column, the {meta, offset} column, the bucket table (2^bucket_bits + 1
// lower bounds) and the filter's probe words in d_words (+ their first sort digit in ws.digits) -- then filter_build_sorted(...,
// words_ready = true).  false: not applicable (empty list, filter smaller than a block), nothing was done.
bool split_columns_and_tables(const void *d_sorted_recs, uint32_t n, uint64_t *d_key, void *d_meta_off, uint32_t bucket_bits, uint32_t *d_bucket,
                              uint32_t log2_bits, void *d_words, SortWorkspace &ws, hipStream_t s);
// reads d_off[0..n_reads] (gap 1, ids = position in d_off): surviving records appended at *d_cursor
// (which ends as their number); nothing is written beyond `cap` (the caller reruns with a larger buffer)
// d_digits != nullptr: also byte digit_word / digit_shift of every record written (the first radix pass's digit), at
// the record's index
void extract_filtered(const uint8_t *d_bases, const uint64_t *d_off, uint32_t n_reads, const void *d_filter,
                      uint32_t log2_bits, uint4 *d_out, uint64_t *d_cursor, uint64_t cap, const Tuning &tune, hipStream_t s,
                      uint8_t *d_digits = nullptr, uint32_t digit_word = 0, uint32_t digit_shift = 0);

// ---------------------------------------------------------- radix_sort.hip
struct SortPass {
  uint32_t word;    // which 32-bit word of the record holds the digit
  uint32_t shift;   // bit shift inside the word
  uint32_t invert;  // XOR mask applied to the word first (descending keys)
  // a digit made of TWO bit fields of the word (hi_bits > 0): bits [shift, shift + 8 - hi_bits) below bits
  // [hi_shift, hi_shift + hi_bits) -- the meta word's high id bits and its revComp bit in one pass (kslam_api.hip: build_index)
  uint32_t hi_shift = 0, hi_bits = 0;
};
#ifdef __HIPCC__
__host__ __device__ inline uint32_t sort_pass_digit(uint32_t word_value, const SortPass &p) {
  const uint32_t v = word_value ^ p.invert;
  if (p.hi_bits == 0) return (v >> p.shift) & 0xFFu;
  const uint32_t lo_bits = 8u - p.hi_bits;
  return ((v >> p.shift) & ((1u << lo_bits) - 1u)) | (((v >> p.hi_shift) & ((1u << p.hi_bits) - 1u)) << lo_bits);
}
#endif
// Waiting for a stream.  hipStreamSynchronize spins on the completion signal: the fastest wake-up, and what a caller
// that has nothing else to do wants (kslam_align_batch, the resident bench).  A pipeline lane waits while the host
// stage of an earlier batch needs every CPU the process may use (a 16-CPU cgroup quota on the bench boxes), and its
// ~40 waits per batch add up to most of the batch's GPU time: measured with tools/cpu_sampler.c, the two lanes spent
// 1.1 CPUs inside the runtime's busy-wait loop -- with hipEventBlockingSync events too, which this runtime spins on
// just the same.  With KSLAM_LANE_WAITS=yield a lane thread sets `yield`, and its waits poll an event with
// hipEventQuery: at once, after a few short spins, then between sleeps of 20-80 microseconds (lane CPU 1.3 -> 0.2 s
// per 20 batches; the GPU-bound pipelined ABI path loses 1 ms per batch to the later wake-ups, and on the bench box the
// end-to-end loop did not get faster for the freed CPU, so the default stays the spin).
struct WaitMode {
  bool yield = false;
  hipEvent_t ev = nullptr;
  ~WaitMode() { if (ev) (void)hipEventDestroy(ev); }
};
inline WaitMode &wait_mode() {
  static thread_local WaitMode w;
  return w;
}
inline hipError_t stream_wait(hipStream_t s) {
  WaitMode &w = wait_mode();
  if (!w.yield) return hipStreamSynchronize(s);
  hipError_t e = hipSuccess;
  if (!w.ev) e = hipEventCreateWithFlags(&w.ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(w.ev, s);
  if (e != hipSuccess) return e;
  for (int spin = 0;; spin++) {
    e = hipEventQuery(w.ev);
    if (e != hipErrorNotReady) return e;
    if (spin < 8) continue;
    const long us = spin < 40 ? 20 : 80;
    struct timespec ts = {0, us * 1000};
    nanosleep(&ts, nullptr);
  }
}

// Device -> host copy of a few bytes the host has to look at before it can launch the next kernel
// (list sizes, counts).  Through a small page-locked buffer: a copy into pageable memory goes through
// the runtime's staging path and costs tens of microseconds more per look, with the GPU idle.
inline void read_back(void *dst, const void *d_src, size_t bytes, hipStream_t s) {
  static thread_local void *pinned = nullptr;
  constexpr size_t CAP = 256;
  if (bytes > CAP) throw StatusError{KSLAM_ERR_INTERNAL, "read_back: more than 256 bytes"};
  if (!pinned) HIPCHK(hipHostMalloc(&pinned, CAP, hipHostMallocDefault));
  HIPCHK(hipMemcpyAsync(pinned, d_src, bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(stream_wait(s));
  memcpy(dst, pinned, bytes);
}

constexpr int SORT_TILE = 4096;
struct SortWorkspace {
  DevBuf hist;      // u32 [chunks][256] per-chunk digit totals -> bases
  DevBuf status;    // u32 [tiles][256] per-tile digit counts -> in-chunk prefixes
  DevBuf tickets;   // u32 [256] per-digit totals -> global bin bases
  DevBuf digits;    // u8 [n] the next pass's digit of every record, written by the scatter (radix_sort.hip)
  bool use_digit_bytes = true;   // KSLAM_SORT_DIGIT_BYTES=0: every histogram re-reads the records (A/B)
  bool first_digits_ready = false;   // `digits` already holds the FIRST pass's digit of every record (the producer of the
                                     // records wrote them: extract_filtered); the caller sets and clears it around one sort
  bool meta_digits_in_runs = false;  // set around the one-time sort of genome records when entries hold many k-mers each: the meta word's
                                     // digits then come in long runs of few values, and their histograms take the kernel made for that
  hipEvent_t *ev_sc0 = nullptr, *ev_sc1 = nullptr;   // optional per-pass events around k_scatter
  uint32_t epoch = 0;
};
// Sorts n records of REC_WORDS 32-bit words (4 = k-mer record, 2 = u64 key) by
// the given passes (LSD order: passes[0] is the least significant digit).
// Result ends in `a` if the number of passes is even, else in `b`; returns the
// pointer holding the sorted data.  ev0/ev1 bracket the scatter passes.
void *radix_sort(void *a, void *b, uint64_t n, int rec_words, const SortPass *passes,
                 int n_passes, SortWorkspace &ws, hipStream_t s, hipEvent_t ev_scatter0,
                 hipEvent_t ev_scatter1, uint32_t *n_launches, bool setup = false);   // setup: one-time sort (kernel names *_setup)

// ---------------------------------------------------------------- join.hip
struct GenomeIndexDev {
  const uint64_t *key;   // sorted genome k-mers
  const uint2 *mo;       // {ID_isFromGB_RC, offset} of the key at the same position: ONE 8-byte gather per hit (two 4-byte
                         // columns cost two cache lines per hit; the join is bound by the lines it touches, not by ALU work)
  const uint32_t *bucket;  // [2^bits + 1] lower bounds by top `bits` bits of the key
  uint32_t bucket_bits;
  uint32_t n;
};
struct OverlapKeyLayout {  // packed u64 overlap: read | entry | rel + bias | revcomp
  uint32_t bits_read, bits_entry, bits_rel;
  uint32_t rel_bias;
};
constexpr int JOIN_TILE = 1024;
void build_bucket_table(const uint64_t *d_keys, uint32_t n, uint32_t bits, uint32_t *d_bucket,
                        hipStream_t s);
// lower bounds of the nb values `key >> shift` takes (keys ordered by it): d_table[0 .. nb]
void build_offsets_table(const uint64_t *d_keys, uint32_t n, uint32_t shift, uint32_t nb, uint32_t *d_table, hipStream_t s);
// single-pass join: output ranges reserved with one atomic per workgroup; *d_cursor ends as the
// total number of overlaps; nothing beyond `cap` is written (caller reruns with a larger buffer)
void join_fill_single_pass(const uint4 *d_read_recs, uint32_t n_r, GenomeIndexDev g, const uint32_t *d_read_len,
                           uint64_t *d_cursor, uint64_t cap, OverlapKeyLayout lay, uint64_t *d_out, hipStream_t s);
// the same contract by a merge (join.hip: k_join_merge): the read records must be ordered by their top `sorted_top_bits` key bits
void join_fill_merge(const uint4 *d_read_recs, uint32_t n_r, GenomeIndexDev g, uint32_t sorted_top_bits, const uint32_t *d_read_len,
                     uint64_t *d_cursor, uint64_t cap, OverlapKeyLayout lay, uint64_t *d_out, hipStream_t s);
// overlap keys radix-sorted by the bits above rel / revComp only: finish every (read, entry) group -- order its few keys by the
// low bits, apply std::unique's "within 3 of the last kept" (Overlap.h:79-85) -- writing ordered keys and flags (join.hip).
// *d_big is set when a group holds more than 64 keys (a read in a tandem repeat): d_out / d_flags are then incomplete and the
// caller sorts the chunk the long way from d_keys, which is only read here.
void group_order(const uint64_t *d_keys, uint64_t n, OverlapKeyLayout lay, uint64_t *d_out, uint32_t *d_flags, uint32_t *d_big, hipStream_t s);
void dedupe_flags(const uint64_t *d_keys, uint64_t n, OverlapKeyLayout lay, uint32_t *d_flags,
                  hipStream_t s);
void dedupe_compact(const uint64_t *d_keys, const uint32_t *d_flags, const uint32_t *d_pos,
                    uint64_t n, OverlapKeyLayout lay, uint32_t read_id_base, kslam_overlap *d_out,
                    hipStream_t s);

// --------------------------------------------------------------- merge.hip
constexpr uint32_t MERGE_MAX_SHARDS = 256;
struct MergeShard {            // one read shard of a batch, as the collecting device sees it
  uint64_t pair_lo, pair_hi;   // the batch's pairs [lo, hi) this shard aligned (local ids: R1 block | R2 block)
  uint64_t row_base, n_rows;   // its rows inside the gathered row array
  uint64_t pool_base;          // its CIGAR pool inside the gathered pools
  uint64_t n_r1, out_r1, out_r2;   // filled on the device: rows of its R1 block, output positions of its two blocks
};
// d_shards: n_shards entries with the host-known fields set.  d_out / d_pool_out receive the batch-global
// result in the reference's order with the pool in row order; *d_total ends as the number of CIGAR ops.
void merge_shards(const kslam_overlap *d_rows, uint64_t n_rows, const uint32_t *d_pool_in, MergeShard *d_shards,
                  uint32_t n_shards, uint64_t n_pairs, kslam_overlap *d_out, uint32_t *d_pool_out, uint32_t *d_lens,
                  uint64_t *d_new_off, uint64_t *d_total, void *d_scan_tmp, hipStream_t s);

// d_out2[0] = rows of the R1 block, d_out2[1] = CIGAR words of those rows
void shard_counts(const kslam_overlap *d_rows, uint64_t n, uint32_t n_local_pairs, uint64_t n_cigar, uint64_t *d_out2,
                  hipStream_t s);
void export_rows(const kslam_overlap *d_rows, uint64_t n, uint64_t n_r1, uint32_t n_local_pairs, uint64_t pair_lo,
                 uint64_t n_pairs_total, uint64_t n_cigar_r1, uint64_t pool_base_r1, uint64_t pool_base_r2,
                 kslam_overlap *d_out_r1, kslam_overlap *d_out_r2, hipStream_t s);

// ------------------------------------------------------------------ sw.hip
// ---- 48-byte records, a wave at a time ----------------------------------------------------------------------------
// kslam_overlap is 48 bytes and a thread that loads "its" record issues three 16-byte loads at a 48-byte stride: every
// instruction of the wave touches 64 different pieces spread over 3 KB.  These helpers move the 64 records of a wave
// (3072 contiguous bytes) with three fully coalesced 16-byte accesses per lane and transpose them through 3 KB of LDS
// per wave.  All 64 lanes must call; records at or beyond n are not read / written (their lanes get zeros).
static_assert(sizeof(kslam_overlap) == 48, "the record helpers move 48-byte records");
__device__ inline kslam_overlap wave_load_records(const kslam_overlap *rows, uint64_t first, uint64_t n, uint4 *lds_wave) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint4 *src = reinterpret_cast<const uint4 *>(rows + first);
  const uint64_t pieces = first < n ? (n - first < 64 ? (n - first) * 3 : 192) : 0;   // 16-byte pieces that exist
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    const uint32_t x = lane + 64u * k;
    lds_wave[x] = x < pieces ? src[x] : make_uint4(0u, 0u, 0u, 0u);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  union { uint4 q[3]; kslam_overlap o; } u;
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) u.q[k] = lds_wave[3u * lane + k];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return u.o;
}
__device__ inline void wave_store_records(kslam_overlap *rows, uint64_t first, uint64_t n, const kslam_overlap &mine, uint4 *lds_wave) {
  const uint32_t lane = threadIdx.x & 63u;
  union { uint4 q[3]; kslam_overlap o; } u;
  u.o = mine;
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) lds_wave[3u * lane + k] = u.q[k];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  uint4 *dst = reinterpret_cast<uint4 *>(rows + first);
  const uint64_t pieces = first < n ? (n - first < 64 ? (n - first) * 3 : 192) : 0;
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    const uint32_t x = lane + 64u * k;
    if (x < pieces) dst[x] = lds_wave[x];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the kept records of a wave into consecutive slots: lane `keep`s record `mine` for slot base + rank (rank = number of
// kept lanes below it); `count` = kept lanes of the wave.  All 64 lanes must call.
__device__ inline void wave_store_records_compact(kslam_overlap *rows, uint64_t base, uint32_t count, bool keep, uint32_t rank,
                                                  const kslam_overlap &mine, uint4 *lds_wave) {
  const uint32_t lane = threadIdx.x & 63u;
  union { uint4 q[3]; kslam_overlap o; } u;
  u.o = mine;
  if (keep) {
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) lds_wave[3u * rank + k] = u.q[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  uint4 *dst = reinterpret_cast<uint4 *>(rows + base);
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    const uint32_t x = lane + 64u * k;
    if (x < 3u * count) dst[x] = lds_wave[x];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct SwParams {
  int32_t match, mismatch, gap_open, gap_extend;
  uint32_t score_threshold;
  int32_t report_cigar;
  int32_t striped = 0;   // scoring outside the envelope: every candidate through k_sw_striped + the literal banded_sw
                         // (sw_scores sets it for a long chunk of any scoring in which match x longest read can pass 32767)
#ifdef KSLAM_ABLATE
  uint32_t ablate = 0;   // KSLAM_SW_ABLATE (measurement only): 1 = no sweep, 2 = no staging either, 3 = one turn, result accepted
#else
  static constexpr uint32_t ablate = 0;   // the ablations are compiled out of the product build
#endif
};
struct SwInputs {
  const uint8_t *read_bases;
  const uint64_t *read_off;   // [n_reads + 1]
  const uint8_t *genome_bases;
  const uint64_t *genome_off; // [n_entries + 1]
  // the same two arrays as base codes (encode_bases): what the SW kernels stage from
  const uint8_t *read_codes = nullptr;
  const uint8_t *genome_codes = nullptr;
};
// One byte per base: bits 0..2 = SSW code 0..4 (ssw_code), bit 3 = "upper-case A/C/G/T", i.e. the
// bases inPlaceReverseComplement complements (ssw_code_complemented(c) = bit 3 ? 3 - code : code).
// Done once per index and once per read batch so that no SW kernel decodes ASCII again.
void encode_bases(const uint8_t *d_src, uint8_t *d_dst, uint64_t n, hipStream_t s);
// forward + reverse passes for n candidates (in place on d_ov: window-relative,
// unflipped coordinates); d_band0[i] = initial band width for banded_sw
// (0 = no cigar wanted, ssw.c:924-927)
struct SwWork {
  DevBuf flags, pos, list, totals, tier_list[6];
  // what the last chunk's tiers received from the tiers before them (sw.hip: the one sweep over the tiers is sized from it)
  uint64_t last_n = 0;
  uint32_t last_inflow[6] = {0, 0, 0, 0, 0, 0};
  int last_tiers = 0, last_lm = -1;
};
// *n_full_out: candidates that needed the full-matrix kernel (the rest ran in a proven band)
void sw_scores(kslam_overlap *d_ov, uint64_t n, SwInputs in, SwParams p, uint32_t max_read_len,
               uint32_t *d_band0, SwWork &W, uint64_t *n_full_out, const Tuning &tune, hipStream_t s,
               bool long_reads = false);   // long_reads: the chunk's reads exceed the packed kernels (sw.hip: k_sw_long)

// --------------------------------------------------------------- cigar.hip
struct CigarWork {
  DevBuf flags, pos, list, bmax, needbig, scan_tmp, totals, cig_off, tmp, tmp_big, big_pos, scratch, cls, cls_list[8],
      special, counters, tb_list;
};
constexpr uint32_t CIG_CAP = 24;  // ops per small temp cigar slot
// allocates and clears the per-candidate cigar state; call before sw_scores
void cigar_prepare(CigarWork &W, uint64_t n, hipStream_t s);
// the records as cigar_finalize will leave them, cigars aside, into d_out (for the pairing between SW and the cigar stage);
// and: no cigar for the rows whose d_referenced flag is 0
void final_coords_copy(const kslam_overlap *d_ov, uint64_t n, SwInputs in, kslam_overlap *d_out, hipStream_t s);
void drop_unreferenced_cigars(kslam_overlap *d_ov, uint32_t *d_bw, const uint32_t *d_referenced, uint64_t n, hipStream_t s);
// banded DP + traceback into temp slots; returns the total number of cigar ops
// and the number of "Trace back error" cases (reference would abort there)
void cigar_traceback(kslam_overlap *d_ov, uint64_t n, SwInputs in, SwParams p, uint32_t lmax, uint32_t *d_bw,
                     CigarWork &W, uint64_t *n_cigar_out, uint32_t *n_tb_err, const Tuning &tune, hipStream_t s);
// un-flip + absolute coordinates, cigar gather into pool[pool_base ...)
void cigar_finalize(kslam_overlap *d_ov, uint64_t n, SwInputs in, uint32_t lmax, CigarWork &W,
                    const uint32_t *d_bw, uint32_t *d_pool, uint64_t pool_base, uint64_t *d_cells, hipStream_t s);

// ------------------------------------------------------------- details.hip
struct DetailWork {
  DevBuf lens, off, slots, scan_tmp, totals, md_pool;
};
// NM / log-probability / MD text of every row (see details.hip); d_tables = matchTable[100] then
// misMatchTable[100] of reference src/SAM.h:33-48, computed by the host
void row_details(const kslam_overlap *d_ov, uint64_t n, const uint32_t *d_pool, const uint8_t *d_rbases,
                 const uint8_t *d_rqual, const uint64_t *d_roff, const uint8_t *d_gbases, const uint64_t *d_goff,
                 const double *d_tables, kslam_row_detail *d_out, DetailWork &W, uint8_t **d_md_pool_out,
                 uint64_t *n_md_out, uint32_t *flags_out, hipStream_t s, const uint32_t *d_rows = nullptr,
                 uint64_t n_list = 0);   // d_rows: only these rows are walked, the others get zero records

// --------------------------------------------------------------- pairs.hip
struct PairWork {
  DevBuf recs, count, base, inserts, flags, gpos, rpos, scan_tmp, totals, groups, dense, sort_a, sort_b, idx, picked, row_list, row_start, gaps;
  DevBuf route_a, route_b, route_heads, route_counts, route_scores;   // pseudo_route / pseudo_owned (entries partitioned over ranks)
  const void *route_sorted = nullptr;   // {destination, record} of this rank's records in sending order (route_a or route_b)
  uint64_t route_n = ~0ull;             // records routed by the last pseudo_route, ~0 when none is outstanding
  uint32_t route_world = 0;
  uint64_t units = 0, mid = 0;   // between pair_phase_a and pair_phase_b: read pairs (or reads) of the batch, its R1 block
  uint32_t pseudo_cap = 0;       // 0 = the default (pairs.hip: PSEUDO_CAP_GLOBAL); tests lower it to reach the host fallback
  int paired = 0;
};
struct PairResult {
  uint64_t n_overlaps_screened, n_paired_initial, n_insert_sizes, n_read_pairs, n_pairs;
  uint64_t n_pairs_left;                 // what the groups' counts add up to: n_pairs until the second score screen shrinks groups in place
  uint32_t max_insert_size;
  uint32_t stages_done;                  // KSLAM_TAIL_* bits of the stages the device ran
  const kslam_read_pair *d_groups;       // n_read_pairs, `first` indexes d_pairs
  const kslam_paired_overlap *d_pairs;   // n_pairs, dense
};
// score screen + pairing + insert-size limit + the two per-read-pair screens (see pairs.hip); d_ov in
// alignToDatabase order, d_read_len[read]; blocks on the stream (small read-backs between the kernels)
void pair_and_screen(const kslam_overlap *d_ov, uint64_t n, const uint32_t *d_read_len, uint64_t n_reads, int paired,
                     uint32_t score_threshold, double score_fraction, int do_insert, int do_score, PairWork &W,
                     SortWorkspace &sortws, PairResult *res, hipStream_t s);

// --------------------------------------------------------- fastq_index.hip
// one FASTQ stream of an indexed batch: its text and line-terminator list on the device (fastq_lines.h: line_span)
struct FqStream {
  const uint8_t *text;   // the stream's first byte (device)
  uint64_t len;
  const uint64_t *ev;    // terminator positions
  uint64_t terminated;   // their number
  uint64_t rest_start;   // text after the last terminator
  uint64_t n;            // records taken
  uint64_t shift;        // position of the stream inside [r1 | r2]
  uint64_t first;        // number of its first record in the batch
};
struct FastqWork {
  DevBuf tile_count, tile_base, scan_tmp, totals, ev[2], bases_at, quality_at, blen, id_at, id_len, bases_off, ids_off, ids;
  FqStream st[2]{};      // the two streams of the last fastq_index_device: valid, like ev, until the next one (readsplit.hip)
};
struct FastqIndexResult {
  uint64_t n_reads, bases_total, ids_total;
  uint64_t consumed[2];
  const uint64_t *d_bases_at, *d_quality_at;   // n_reads: positions in [r1 | r2]
  const uint64_t *d_bases_off, *d_ids_off;     // n_reads + 1
  const uint8_t *d_ids;                        // ids_total bytes
};
// d_text = [r1 | r2] on the device; h_last1 / h_last2: the streams' last bytes on the host (or nullptr for
// an empty stream).  Semantics of host/fastq.cpp's index (kslam_fastq_index_pair).
void fastq_index_device(const uint8_t *d_text, uint64_t len1, uint64_t len2, const uint8_t *h_last1, const uint8_t *h_last2,
                        uint64_t max_pairs, bool at_eof, FastqWork &W, FastqIndexResult *res, hipStream_t s, bool single = false);

// pair_and_screen in its two halves, for read pairs sharded over several GPUs: phase A pairs per
// read pair and collects the shard's insert sizes (W.inserts, res->n_insert_sizes); the caller gathers every shard's
// insert sizes and computes the batch's limit from all of them (insert_limit_device: the statistic is batch-global,
// src/PairedOverlap.h:314-360); phase B screens with that limit.  pseudo_merged: pseudo-assembly on the dense
// alignment-pair records of ALL shards (d_all, gathered in rank order; this shard's are [own_base, own_base + n_pairs)),
// new scores copied back into this shard's records, second screen on them.
void pair_phase_a(const kslam_overlap *d_ov, uint64_t n, const uint32_t *d_read_len, uint64_t n_reads, int paired,
                  uint32_t score_threshold, PairWork &W, PairResult *res, hipStream_t s);
uint32_t insert_limit_device(const int32_t *d_ins, uint64_t n, PairWork &W, SortWorkspace &sortws, hipStream_t s);
void pair_phase_b(const kslam_overlap *d_ov, uint32_t limit, double score_fraction, int do_insert, int do_score, PairWork &W,
                  PairResult *res, hipStream_t s);
bool pseudo_merged(PairWork &W, PairResult *res, void *d_all, uint64_t n_all, uint64_t own_base, double score_fraction,
                   SortWorkspace &sortws, hipStream_t s);

// the overlap records the result's alignment pairs refer to, ascending, as a list in W (valid until the next pairs call)
void referenced_rows(PairWork &W, const PairResult *res, uint64_t n_rows, const uint32_t **d_list, uint64_t *n_list, hipStream_t s);

// pseudoAssembly + the second score screen on pair_and_screen's result, in place; false (nothing changed)
// when an entry has more spans than a workgroup's LDS holds: the host then runs that stage itself
bool pseudo_and_rescreen(PairWork &W, PairResult *res, double score_fraction, SortWorkspace &sortws, hipStream_t s);
// the same stage with the ENTRIES partitioned over the ranks of a sharded batch (pairs.hip, bottom): route -> all-to-all ->
// owned -> all-to-all back -> return
void pseudo_route(PairWork &W, const PairResult *res, uint32_t world, const void **d_heads, uint64_t *counts, SortWorkspace &sortws,
                  hipStream_t s);
bool pseudo_owned(PairWork &W, void *d_heads, uint64_t n, const uint32_t **d_scores, SortWorkspace &sortws, hipStream_t s);
void pseudo_return(PairWork &W, PairResult *res, const uint32_t *d_scores, uint64_t n, double score_fraction, hipStream_t s);

// test hook for wave_gnu_sort.h (kslam_debug_wave_sort)
void debug_wave_sort(const int32_t *keys, const uint64_t *seg_off, uint64_t n_seg, uint32_t *perm, hipStream_t s);

// bases / quality columns cut out of FASTQ text on the device: read i = text[bases_at[i] ..) and
// text[quality_at[i] ..), d_off[i + 1] - d_off[i] bytes each, to d_bases / d_quality + d_off[i]
void gather_fields(const uint8_t *d_text, const uint64_t *d_bases_at, const uint64_t *d_quality_at, const uint64_t *d_off,
                   uint64_t n_reads, uint8_t *d_bases, uint8_t *d_quality, hipStream_t s);

// ----------------------------------------------------------- readsplit.hip
// The batch's records split by outcome (include/kslam_readsplit.h): streams 0 / 1 = classified R1 / R2, 2 / 3 = unclassified.
struct ReadSplitWork {
  DevBuf flag, len_sel, len_unsel, src, off_sel, off_unsel, scan_tmp, totals, out[4];
  hipEvent_t ev[4]{};          // around the flag + length + scan launches, and around the copy launches
  float kernel_ms = 0;         // their device time, last batch (tools/readsplit_bench.py)
  uint64_t bytes_moved = 0;    // text bytes the copy kernels read + wrote, last batch
  ReadSplitWork() = default;
  ReadSplitWork(const ReadSplitWork &) = delete;
  ReadSplitWork &operator=(const ReadSplitWork &) = delete;
  ~ReadSplitWork() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
// st: FastqWork::st of the batch; d_groups: its final read pairs; which: KSLAM_READS_OUT_* bits.  Leaves stream k in W.out[k],
// bytes[k] long, n_records[0] classified and n_records[1] unclassified records per stream.  Waits for the stream (the sizes are read back).
void read_split_device(const FqStream st[2], bool single, const kslam_read_pair *d_groups, uint64_t n_groups, uint32_t which,
                       ReadSplitWork &W, uint64_t bytes[4], uint64_t n_records[2], hipStream_t s);
// The same in two halves, for a caller that flags the records itself (taxreads.hip): read_split_prepare sizes the buffers,
// zeroes W.flag (one byte per record of the batch, [R1 | R2]) and the totals and returns the number of records; the caller
// records W.ev[0], runs its flag pass on s and calls read_split_flagged for the lengths, scans and copy (flagged records are
// the "classified" streams).
uint64_t read_split_prepare(const FqStream st[2], bool single, ReadSplitWork &W, hipStream_t s);
void read_split_flagged(const FqStream st[2], bool single, uint32_t which, ReadSplitWork &W, uint64_t bytes[4], uint64_t n_records[2],
                        hipStream_t s);

// ------------------------------------------------------------ taxreads.hip
// The reads of chosen taxa (include/kslam_taxreads.h).  The selection belongs to the context kslam_set_taxon_reads was called
// on (context.h: kslam_ctx::TaxReads); its lanes only read it.
struct TaxReadsSel {               // what the flag pass sees
  const uint32_t *keys;           // [n_nodes] the tree's taxonomy ids, ascending
  const uint32_t *nodes;          // [n_nodes] the node of keys[i]
  uint64_t n_nodes;
  const uint8_t *mask;            // [n_nodes] 1: the node's id is in S
  const uint32_t *unknown;        // [n_unknown] the chosen ids the tree does not know, ascending and distinct
  uint64_t n_unknown;
  int all_nonzero;                // id 1 chosen with CHILDREN: every non-zero id is in S
};
struct TaxReadsMaskWork {
  SortWorkspace sortws;
  DevBuf ids, seed, items_a, items_b, head, run, cursor, scan_tmp, totals;
};
struct TaxReadsFlagWork {
  DevBuf count;                   // matched read pairs of the batch: 32 counters on cache lines of their own, and their sum
  hipEvent_t ev[2]{};             // around the flag launch
  float ms = 0;                   // its device time, last batch
  uint64_t n_matched = 0;
  TaxReadsFlagWork() = default;
  TaxReadsFlagWork(const TaxReadsFlagWork &) = delete;
  TaxReadsFlagWork &operator=(const TaxReadsFlagWork &) = delete;
  ~TaxReadsFlagWork() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
// S from n chosen ids (host memory, none of them 0): d_mask[0 .. n_nodes) is written, the unknown chosen ids go to `unknown`
// (u32, ascending, distinct; *n_unknown of them), *all_nonzero as in TaxReadsSel.  ev: two events around the launches.  Waits
// for the stream.
void taxreads_mask_device(const uint32_t *h_ids, uint64_t n, uint32_t mode, const uint32_t *d_keys, const uint32_t *d_nodes, uint64_t n_nodes,
                          const uint32_t *d_up, const uint32_t *d_depth, TaxReadsMaskWork &W, uint8_t *d_mask, DevBuf &unknown,
                          uint64_t *n_unknown, int *all_nonzero, hipEvent_t ev[2], hipStream_t s);
// flag[r1_read] = flag[r2_read] = 1 for every read pair g whose d_ids[g] is in S; n_total: the records of the batch (the
// flag array's length).  Does not wait: W.n_matched and W.ms are read by taxreads_flag_finish once the stream has been waited for.
void taxreads_flag_device(const kslam_read_pair *d_groups, const uint32_t *d_ids, uint64_t n_groups, int paired, uint64_t n_total,
                          const TaxReadsSel &S, uint8_t *d_flag, TaxReadsFlagWork &W, hipStream_t s);
void taxreads_flag_finish(TaxReadsFlagWork &W, hipStream_t s);

// ------------------------------------------------------------ coverage.hip
// The per-entry coverage table (include/kslam_coverage.h).  CoverageState belongs to the context the switch was set on; its
// lanes mark into it from their own streams (every update a device-scope atomic), each with a CoverageMarkWork of its own.
struct CoverageTable {            // what the kernels see
  unsigned long long *bitmap;    // one bit per base; entry e's words start at word_off[e]
  unsigned long long *rows;      // 4 per entry: alignments, unique_read_pairs, aligned_bases, covered_bases
  unsigned long long *skipped;   // mates that contributed nothing
  const uint64_t *word_off;      // [n_entries + 1]
  const uint64_t *g_off;         // [n_entries + 1]: the index's entry offsets (lengths)
  uint64_t n_entries, n_words;
};
struct CoverageMarkWork {
  DevBuf gflag;                  // per read pair: bit 0 = a live record's entry differs from the first record's
  hipEvent_t ev[2]{};            // around the mark launches
  float ms = 0;                  // their device time, last batch
  CoverageMarkWork() = default;
  CoverageMarkWork(const CoverageMarkWork &) = delete;
  CoverageMarkWork &operator=(const CoverageMarkWork &) = delete;
  ~CoverageMarkWork() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
constexpr int COV_MARK_BLOCK = 256;   // threads per workgroup of the mark pass (one alignment-pair record each)
// one batch into the table: d_ov the overlap records d_pairs' r1 / r2 index; waits for the stream (the events are read)
void coverage_mark_device(const kslam_overlap *d_ov, uint64_t n_ov, const kslam_read_pair *d_groups, uint64_t n_groups,
                          const kslam_paired_overlap *d_pairs, uint64_t n_pairs, const CoverageTable &T, CoverageMarkWork &W, hipStream_t s);
// covered_bases of every row, counted from the bitmap (the column is cleared first); ev: two events around the launches
void coverage_count_device(const CoverageTable &T, hipEvent_t ev[2], hipStream_t s);

// ------------------------------------------------------------- kreport.hip
// The Kraken-style report's counts (include/kslam_kreport.h).  The state belongs to the context the switch was set on
// (context.h: kslam_ctx::Kreport); its lanes count into it from their own streams (every update a device-scope atomic), each
// with a KreportCountWork of its own, and append their unknown-id items under the state's lock.
struct KreportTable {             // what the count pass sees
  unsigned long long *direct;    // [n_nodes] reads whose id is this node's
  const uint32_t *keys;          // [n_nodes] the tree's taxonomy ids, ascending
  const uint32_t *nodes;         // [n_nodes] the node of keys[i]
  uint64_t n_nodes;
};
struct KreportCountWork {
  DevBuf items, cursor;          // the call's unknown-id items (id << 32 | count), and how many there are
  uint64_t n_new = 0;            // ... read back
  hipEvent_t ev[2]{};            // around the count launches
  float ms = 0;                  // their device time, last batch
  KreportCountWork() = default;
  KreportCountWork(const KreportCountWork &) = delete;
  KreportCountWork &operator=(const KreportCountWork &) = delete;
  ~KreportCountWork() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
struct KreportTakeWork {
  SortWorkspace sortws;
  DevBuf clade, flag, pos;       // per node: u64 clade sum, u32 clade > 0, u32 place among the rows
  DevBuf keys_a, keys_b, head, run;   // per unknown-id item: the sort's two buffers, run head, heads before it
  DevBuf rows, scan_tmp, totals;
};
// n ids into the table; the unknown ids' items into W.items[0 .. W.n_new).  dry: nothing is written but W.n_new (what the call
// WOULD append).  Waits for the stream (the cursor and the events are read).
void kreport_count_device(const uint32_t *d_ids, uint64_t n, const KreportTable &T, KreportCountWork &W, bool dry, hipStream_t s);
// clade sums, then the rows (kslam_kreport_row) into W.rows: *n_known rows of nodes in node order, *n_unknown of unknown ids in id
// order behind them.  ev: two events around the launches.  Waits for the stream for the two counts, not for the row kernels.
void kreport_take_device(const KreportTable &T, const uint32_t *d_up, const uint32_t *d_depth, const uint32_t *d_node_tax, const uint64_t *d_items,
                         uint64_t n_items, KreportTakeWork &W, uint64_t *n_known, uint64_t *n_unknown, hipEvent_t ev[2], hipStream_t s);

// --------------------------------------------------------------- genes.hip
// The per-gene abundance table (include/kslam_genes.h).  The state -- the lookup index, four 64-bit counters per gene and four
// statistics counters -- belongs to the context the switch was set on (context.h: kslam_ctx::Genes); its lanes count into it
// from their own streams (every update a device-scope atomic), each with a GenesCountWork of its own.
struct GeneTable {                // what the kernels see
  uint64_t n_entries, n_genes;
  const uint64_t *gene_first;    // [n_entries + 1], ascending from 0 to n_genes (checked at switch-on)
  const int32_t *gene_start, *gene_stop;   // [n_genes] the annotation columns, in gene-index order
  // the lookup index: per entry, its genes ordered by (start, gene index); position p lies in the entry's own slice
  // [gene_first[e], gene_first[e + 1])
  const uint32_t *order;         // [n_genes] the gene at position p
  const int32_t *sstart, *sstop; // [n_genes] its start and stop
  const int32_t *runmax;         // [n_genes] the largest stop among the entry's positions <= p
  unsigned long long *rows;      // 4 per gene: unused, alignments, unique_read_pairs, overlap_bases
  unsigned long long *stats;     // n_alignments, n_in_gene, n_no_gene, n_skipped
};
struct GenesCountWork {
  DevBuf gene;                   // u32 per alignment-pair record: its gene, GENE_NONE or GENE_SKIPPED (live records only)
  DevBuf gflag;                  // u32 per read pair: a live record's gene differs from the first record's, or is no gene
  hipEvent_t ev[2]{};            // around the count launches
  float ms = 0;                  // their device time, last batch
  GenesCountWork() = default;
  GenesCountWork(const GenesCountWork &) = delete;
  GenesCountWork &operator=(const GenesCountWork &) = delete;
  ~GenesCountWork() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
struct GenesTakeWork {
  DevBuf flag, pos, rows, scan_tmp, totals;   // u32 per gene: alignments > 0, its place among the rows; the compacted rows
};
constexpr int GENES_BLOCK = 256;      // threads per workgroup of the count pass (one alignment-pair record each)
// the lookup index of n_genes genes from the three annotation columns into the four arrays (each n_genes long); *ms: the device
// time of the launches.  Waits for the stream.
void genes_build_device(uint64_t n_entries, uint64_t n_genes, const uint64_t *d_gene_first, const int32_t *d_gene_start, const int32_t *d_gene_stop,
                        uint32_t *d_order, int32_t *d_sstart, int32_t *d_sstop, int32_t *d_runmax, float *ms, hipStream_t s);
// one batch into the table; linear: the walk over all genes of the entry instead of the indexed lookup (the same result).
// Waits for the stream (the events are read).
void genes_count_device(const kslam_read_pair *d_groups, uint64_t n_groups, const kslam_paired_overlap *d_pairs, uint64_t n_pairs,
                        const GeneTable &T, GenesCountWork &W, bool linear, hipStream_t s);
// the rows with alignments > 0 (kslam_gene_row) into W.rows in gene order; ev: two events around the launches.  Waits for the
// stream for *n_rows, not for the row kernel.
void genes_take_device(const GeneTable &T, GenesTakeWork &W, uint64_t *n_rows, hipEvent_t ev[2], hipStream_t s);
// n triples through the count pass's device function: d_gene_out / d_shared_out as kslam_genes_lookup describes them
void genes_lookup_device(const uint32_t *d_entries, const int32_t *d_starts, const int32_t *d_stops, uint64_t n, const GeneTable &T, bool linear,
                         int64_t *d_gene_out, int64_t *d_shared_out, hipStream_t s);

// -------------------------------------------------------------- readqc.hip
// The read QC report's tables (include/kslam_readqc.h).  The state -- two streams of 64-bit words in the header's layout --
// belongs to the context the switch was set on (context.h: kslam_ctx::ReadQc); its lanes count into it from their own streams
// (every update a device-scope atomic), each with a ReadQcWork of its own.
struct ReadQcTable {              // what the count pass sees
  unsigned long long *words;     // [2 * n_words]: stream 0's words, then stream 1's
  uint64_t n_words;              // KSLAM_READ_QC_WORDS(C)
  uint32_t C;                    // cycle rows without the pooled one
};
struct ReadQcWork {
  hipEvent_t ev[2]{};            // around the count launches
  float ms = 0;                  // their device time, last batch counted with `timed`
  uint64_t bytes = 0;            // bases + quality bytes that batch held
  ReadQcWork() = default;
  ReadQcWork(const ReadQcWork &) = delete;
  ReadQcWork &operator=(const ReadQcWork &) = delete;
  ~ReadQcWork() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
constexpr uint64_t RQ_READS = 256;   // the fewest reads a workgroup of the count pass takes (more when the grid is full)
// n reads (read i = d_bases / d_quality[d_off[i] .. d_off[i + 1])) into the table; paired: the first n / 2 are stream 0, the
// rest stream 1.  max_len: no read is longer (it sizes the grid's tiles).  timed: events around the launches, and the call
// waits for the stream and reads them; else it does not wait.
void readqc_count_device(const uint8_t *d_bases, const uint8_t *d_quality, const uint64_t *d_off, uint64_t n, bool paired, uint64_t max_len,
                         const ReadQcTable &T, ReadQcWork &W, bool timed, hipStream_t s);
// a zeroed table: every word 0, the two min_len words all ones (the take turns an untouched one into 0)
void readqc_zero_device(const ReadQcTable &T, hipStream_t s);

// ------------------------------------------------------------ variants.hip
// The SNV table (include/kslam_variants.h).  The state -- three arrays of 8-byte keys -- belongs to the context the switch was
// set on (context.h: kslam_ctx::Variants); each lane counts its batch with an EmitWork of its own and appends under the
// state's lock.
struct VariantInputs {            // one batch as the kernels see it
  const kslam_overlap *ov;
  uint64_t n_ov;
  const kslam_read_pair *groups;
  uint64_t n_groups;
  const kslam_paired_overlap *pairs;
  uint64_t n_pairs;
  const uint32_t *pool;          // the CIGAR pool
  uint64_t n_cig;
  const uint8_t *rbases;         // read i: rbases[roff[i] .. roff[i + 1])
  const uint64_t *roff;
  uint64_t n_reads;
  const uint8_t *gbases;         // the index's entries
  const uint64_t *goff;
  uint64_t n_entries;
};
// What the emit passes of the three pile-up reports share (variants.hip, depth.hip, consensus.hip): the contributing list, what
// each listed record emits of each KIND of key (SNV table: events, intervals; depth track: M runs; consensus: consensus.h), the
// scans that lay out the slots, the batch's totals.
constexpr int PILEUP_BLOCK = 256;   // threads per workgroup of the three reports' emit and take passes
inline unsigned pileup_blocks(uint64_t n) { return (unsigned)((n + PILEUP_BLOCK - 1) / PILEUP_BLOCK); }
constexpr int EMIT_MAX_KINDS = 4;
constexpr int EMIT_TOTALS = 8;   // u64: [0] the list's length, [1 + kind] the kind's sum, [5] skipped, [6] unanchored, [7] unrepresentable
struct EmitWork {
  DevBuf flag, pos, list;        // u32 per overlap record: named by a live pair, its place in the list; the list
  DevBuf cnt;                    // u32 [kinds][n_list]: what each listed record emits of each kind
  DevBuf off;                    // u64 [kinds][n_list]: its first slot
  DevBuf scan_tmp, totals;
  int kinds = 0;                 // of the batch counted last, as what follows
  uint64_t n_list = 0, n[EMIT_MAX_KINDS] = {0, 0, 0, 0}, n_skipped = 0;
  uint64_t n_unanchored = 0, n_unrepresentable = 0;   // (insertions the consensus does not store; 0 for the others)
  hipEvent_t ev[2]{};            // before the first pass, after the last
  float ms = 0;
  EmitWork() = default;
  EmitWork(const EmitWork &) = delete;
  EmitWork &operator=(const EmitWork &) = delete;
  ~EmitWork() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
// one thread per listed record x: cnt[kind * n_list + x] = what it emits of each kind; tallies[0 .. 2] += skipped, unanchored,
// unrepresentable
using EmitCountKernel = void (*)(VariantInputs in, const uint32_t *list, uint64_t n_list, uint32_t *cnt, unsigned long long *tallies);
// the contributing list, the counting walk and one scan per kind; fills W.n_list / n / n_skipped / ... (waits for the stream)
void emit_count_device(const VariantInputs &in, EmitWork &W, int kinds, EmitCountKernel count, hipStream_t s);
// after the write kernel: waits for the stream and fills W.ms
void emit_written(EmitWork &W, hipStream_t s);
// the writing walk of the batch counted last, unless it emits nothing: write(in, list, n_list, cnt, off, at), one thread per
// listed record, the keys from `at` on (the caller made room for W.n[kind] of each); waits for the stream and fills W.ms
template <class Out>
void emit_write_device(const VariantInputs &in, EmitWork &W, void (*write)(VariantInputs, const uint32_t *, uint64_t, const uint32_t *, const uint64_t *, Out),
                       const Out &at, hipStream_t s) {
  uint64_t any = 0;
  for (int kind = 0; kind < W.kinds; kind++) any |= W.n[kind];
  if (W.n_list && any)
    hipLaunchKernelGGL(write, dim3(pileup_blocks(W.n_list)), dim3(PILEUP_BLOCK), 0, s, in, W.list.as<uint32_t>(), W.n_list, W.cnt.as<uint32_t>(),
                       W.off.as<uint64_t>(), at);
  emit_written(W, s);
}
enum { VAR_EV = 0, VAR_IV = 1, VAR_KINDS = 2 };   // the SNV table's kinds
struct VariantTakeWork {
  SortWorkspace sortws;
  DevBuf alt;                    // the sort's second buffer
  DevBuf head, run;              // u32 per event: starts a (g, alt) run; the run's number
  DevBuf starts, fwd, rev, depth, keep, out_at;   // u32 per run
  DevBuf rows, scan_tmp, totals;
};
// passes 1-4: flags, list, counting walk, scans; fills W.n_list / n[VAR_EV] / n[VAR_IV] / n_skipped (waits for the stream)
void variants_count_device(const VariantInputs &in, EmitWork &W, hipStream_t s);
// pass 6: the keys of the batch counted last, from d_events / d_begins / d_ends on (the caller made room for W.n[VAR_EV] /
// W.n[VAR_IV]); waits for the stream and fills W.ms
void variants_write_device(const VariantInputs &in, EmitWork &W, uint64_t *d_events, uint64_t *d_begins, uint64_t *d_ends, hipStream_t s);
// sorts the three arrays in place unless `sorted`, then the rows that pass the filter into T.rows (device); waits for the stream
void variants_take_device(VariantTakeWork &T, DevBuf &events, uint64_t n_ev, DevBuf &begins, DevBuf &ends, uint64_t n_iv, bool sorted,
                          const uint64_t *d_goff, const uint8_t *d_gbases, uint64_t n_entries, uint64_t total_bases, uint32_t min_alt,
                          uint32_t min_depth, uint64_t *n_sites_out, uint64_t *n_rows_out, hipStream_t s);
// passes 1-2 alone, shared by every report that walks the contributing records: the overlap records a live pair names as a list
// in `list`; returns its length (waits for the stream).  totals: EMIT_TOTALS u64, zeroed here; [0] ends as the list's length
uint64_t contributing_list_device(const VariantInputs &in, DevBuf &flag, DevBuf &pos, DevBuf &list, DevBuf &scan_tmp, DevBuf &totals, hipStream_t s);
// sorts n u64 keys of `buf` (scratch: `alt`, at least as large) with as many radix passes as max_key needs; the sorted keys end in `buf`
void sort_keys(DevBuf &buf, DevBuf &alt, uint64_t n, uint64_t max_key, SortWorkspace &ws, hipStream_t s);
// list[pos[i]] = i for every i < n with flag[i] (pos: the exclusive scan of the flags)
void scatter_list_device(const uint32_t *flag, const uint32_t *pos, uint64_t n, uint32_t *list, hipStream_t s);
// over n sorted keys: head[i] = 1 where a run of keys that are equal but for their low bit begins
void run_heads_device(const uint64_t *key, uint64_t n, uint32_t *head, hipStream_t s);
// starts[run[i]] = i for every i < n with head[i] (run: the exclusive scan of the heads)
void run_starts_device(const uint32_t *head, const uint32_t *run, uint64_t n, uint32_t *starts, hipStream_t s);

// ------------------------------------------------------------- indels.hip
// The indel table (include/kslam_indels.h).  The state -- the interval arrays, 8-byte deletion keys and 16-byte insertion
// records -- belongs to the context the switch was set on (context.h: kslam_ctx::Indels); the emit shell and the take's buffers
// are the SNV table's.  INDEL_LONG is a kind for the shell's sake alone: the anchored D runs that are too long are summed by its
// scan and nothing is written for them.
enum { INDEL_IV = 0, INDEL_DEL = 1, INDEL_INS = 2, INDEL_LONG = 3, INDEL_KINDS = 4 };
struct IndelKeys {                // where a batch's keys go
  uint64_t *ib, *ie, *del, *ins;  // ins: two words per record
};
// the list, the counting walk and the scans; fills W.n_list / n[kind] / n_skipped / n_unanchored / n_unrepresentable (waits)
void indels_count_device(const VariantInputs &in, EmitWork &W, hipStream_t s);
// the writing walk of the batch counted last (the caller made room for W.n[kind] of each); waits for the stream and fills W.ms
void indels_write_device(const VariantInputs &in, EmitWork &W, const IndelKeys &at, hipStream_t s);
// sorts the four arrays in place: the rows' order
void indels_sort_device(VariantTakeWork &T, DevBuf &begins, DevBuf &ends, uint64_t n_iv, DevBuf &dels, uint64_t n_del, DevBuf &ins, uint64_t n_ins,
                        uint64_t total_bases, hipStream_t s);
// the rows of ONE kind (KSLAM_INDEL_DEL: keys = the sorted deletion keys, KSLAM_INDEL_INS: the sorted insertion records) that
// pass the filter into T.rows (device, kslam_indel_row); waits for the stream
void indels_take_device(VariantTakeWork &T, int kind, const uint64_t *keys, uint64_t n_keys, const uint64_t *begins, const uint64_t *ends, uint64_t n_iv,
                        const uint64_t *d_goff, uint64_t n_entries, uint32_t min_alt, uint32_t min_depth, uint64_t *n_sites_out, uint64_t *n_rows_out,
                        hipStream_t s);

// ------------------------------------------------------------ alignqc.hip
// The alignment QC report (include/kslam_alignqc.h).  The state -- one block of 64-bit counters -- belongs to the context the
// switch was set on (context.h: kslam_ctx::AlignQc); each lane counts its batch with an AlignQcWork of its own.
struct AlignQcTable {             // what the passes see
  unsigned long long *words;     // [KSLAM_ALIGN_QC_WORDS(C)]: the report's words, stream 0's, stream 1's
  uint32_t C;                    // cycle rows without the pooled one
};
struct AlignQcWork {
  DevBuf flag, pos, list;        // as EmitWork
  DevBuf scan_tmp, totals;
  hipEvent_t ev[2]{};            // around the count pass
  float ms = 0;                  // its device time, last batch counted with `timed`
  AlignQcWork() = default;
  AlignQcWork(const AlignQcWork &) = delete;
  AlignQcWork &operator=(const AlignQcWork &) = delete;
  ~AlignQcWork() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
// one batch into the table: the pair pass, the contributing list (variants.hip's) and the count pass.  d_quality: the quality
// column laid out as in.rbases, or null; paired: reads below in.n_reads / 2 are stream 0, the others stream 1; max_len: no read
// is longer (it sizes the grid's tiles).  timed: events around the count pass, and the call reads them after waiting for the
// stream; it waits for the stream in any case (the list's length is read back).  thread_per_record: the baseline instantiation.
void alignqc_count_device(const VariantInputs &in, const uint8_t *d_quality, bool paired, uint64_t max_len, const AlignQcTable &T, AlignQcWork &W,
                          bool timed, bool thread_per_record, hipStream_t s);
void alignqc_zero_device(const AlignQcTable &T, hipStream_t s);

// ------------------------------------------------------------ depth.hip
// The per-base depth track (include/kslam_depth.h).  Boundaries live in a key space with ONE SPARE position per entry,
// key = g_off[entry] + entry + pos, so that the boundary after the last base of entry e is not the first base of entry e + 1.
// Pending: u64 (key << 1) | is_end, two per M run, appended per batch.  Compacted: distinct keys ascending with their net change
// (i64: begins less ends; a count must hold 2^32 - 1, which a signed 32-bit change does not), none of them 0.
struct DepthWork {                // compaction and take; used under the state's lock
  SortWorkspace sortws;
  DevBuf alt;                    // the sort's second buffer
  DevBuf head, run, starts;      // u32 per pending key: starts a run of one boundary; the run's number; per run: its first key
  DevBuf pkey, pnet;             // the pending keys reduced: one record per distinct boundary
  DevBuf mkey, mnet;             // the merge of the reduced and the compacted list (a boundary at most twice)
  DevBuf keep, at;               // u32 per merged record / per compacted boundary: kept; its slot
  DevBuf nkey, nnet;             // the new compacted list (swapped in)
  DevBuf tile_sum, depth;        // take: i64 per scan tile; u32 per boundary: the depth from it on
  DevBuf rows, scan_tmp, totals;
};
// the list, the counting walk and the scan; fills W.n_list / n[0] (M runs) / n_skipped (waits for the stream).  in.rbases /
// in.gbases are not read
void depth_count_device(const VariantInputs &in, EmitWork &W, hipStream_t s);
// the writing walk: 2 * W.n[0] pending keys from d_pending on (the caller made room); waits for the stream and fills W.ms
void depth_write_device(const VariantInputs &in, EmitWork &W, uint64_t *d_pending, hipStream_t s);
// sort, reduce, merge, drop: n_pend pending keys into the compacted list (ckey / cnet, *n_keys of them).  Throws
// KSLAM_ERR_UNSUPPORTED before the compacted list is touched when the merge would pass 2^32 - 1 records.  Waits for the stream.
void depth_compact_device(DepthWork &T, DevBuf &pending, uint64_t n_pend, DevBuf &ckey, DevBuf &cnet, uint64_t *n_keys, uint64_t max_key, hipStream_t s);
// the rows of the compacted list that reach min_depth into T.rows (device); out[0..3] = rows before the filter, covered bases,
// the largest depth, rows after the filter.  Waits for the stream.
void depth_take_device(DepthWork &T, const uint64_t *d_ckey, const int64_t *d_cnet, uint64_t n_keys, const uint64_t *d_goff, uint64_t n_entries,
                       uint32_t min_depth, uint64_t out[4], hipStream_t s);

}  // namespace kslam
