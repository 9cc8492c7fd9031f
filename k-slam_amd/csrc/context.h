// context.h -- what the translation units behind the C ABI (include/kslam.h) share: the context itself and the internal
// helpers that cross file boundaries.  The ABI's host side was one file of 2 650 lines until round 6 (kslam_api.hip); it is now split
// by phase:
//   api_core.hip   context life cycle, tuning switches, page-locked pools, loading reads, fetching results, the operator entry
//   api_index.hip  kslam_set_index: extraction + the one-time sort + tables (build_index), and the stage-level entry points
//   api_align.hip  alignToDatabase on the resident batch (the chunk loop: extract -> sort -> join -> dedupe -> SW -> CIGAR)
//   api_tail.hip   the widened path on the device: qualities, per-row details, pairing / screens / pseudo-assembly, SAM text
//   api_lanes.hip  the pipelined entry (worker lanes, FASTQ text in)
//   api_multi.hip  several devices: shard export / merge, kslam_multi_*
//   api_readsplit.hip  the reads split by outcome, cut out of the uploaded text
//   api_taxreads.hip   the reads of chosen taxa, likewise
//   api_gunzip.hip     plain gzip input: the stages of gunzip.hip in order, in rounds
//   api_coverage.hip, api_variants.hip, api_indels.hip, api_depth.hip, api_kreport.hip, api_genes.hip, api_readqc.hip, api_alignqc.hip,
//   api_consensus.hip, api_bamsort.hip
//                  the opt-in reports the lanes feed, one file each; what they share is in api_reports.h (included below)
#pragma once
#include <sys/mman.h>

#include "common.h"
#include "samtext.h"
#include "bgzf.h"
#include "inflate.h"
#include "gunzip.h"
#include "consensus.h"
#include "../../include/kslam_samtext.h"
#include "../../include/kslam_bgzf.h"
#include "../../include/kslam_inflate.h"
#include "../../include/kslam_gunzip.h"
#include "../../include/kslam_bam.h"
#include "../../include/kslam_samseq.h"
#include "../../include/kslam_samunmapped.h"
#include "../../include/kslam_readsplit.h"
#include "../../include/kslam_coverage.h"
#include "../../include/kslam_variants.h"
#include "../../include/kslam_indels.h"
#include "../../include/kslam_depth.h"
#include "../../include/kslam_kreport.h"
#include "../../include/kslam_readqc.h"
#include "../../include/kslam_taxreads.h"
#include "../../include/kslam_genes.h"
#include "../../include/kslam_alignqc.h"
#include "../../include/kslam_bamsort.h"
#include "../host/workers.hpp"
#include "../host/inflate.hpp"
#include "../host/batch_check.hpp"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <sys/prctl.h>
#include <thread>

using namespace kslam;

namespace kslam {
struct BamSortState;   // bamsort.h
struct BamSortWork;
}  // namespace kslam

// The resident genome index (const GenbankIndex&): what build_index makes, never changed after.  The context that built it,
// its worker lanes and its siblings share it; kslam_set_index builds a new one and leaves the old one to whoever still holds it.
struct GenomeIndex {
  kslam_index_stats stats{};     // phases of the build
  uint64_t n_entries = 0;
  uint64_t max_entry_len = 0;
  std::vector<uint64_t> h_goff;  // [n_entries + 1]
  DevBuf g_bases, g_off, g_codes;   // g_codes: encode_bases(g_bases)
  uint64_t n_gk = 0;
  DevBuf gk_key, gk_meta, g_bucket;
  uint32_t bucket_bits = 8;
  DevBuf g_filter;            // membership filter over the genome k-mers (filter.hip); filter_bits = 0: off
  uint32_t filter_bits = 0;
};

// One batch's arrays on the device, as a report's kslam_*_add got them from the host.  Every report state holds one of its own:
// the adds of different reports hold different mutexes and may run at the same time.
struct BatchUpload {
  enum Columns { no_columns, bases, bases_and_quality };   // of the reads, besides their offsets
  DevBuf ov, groups, pairs, pool, rbases, rqual, roff;

  // Uploads what `level` checked (kslam_batch::check) -- the groups and the pairs; from Level::pairs the overlap records; from
  // Level::records the CIGAR pool and the read offsets -- and the reads' columns asked for, on s, and waits: the caller's arrays
  // are free again.  What the report does not take stays null in the batch handed back; the entries' bases come with the reads'.
  VariantInputs upload(const kslam_batch::Arrays &a, kslam_batch::Level level, const uint32_t *cigar_pool, Columns columns, const char *read_bases,
                       const char *read_quality, const GenomeIndex *ix, hipStream_t s) {
    const bool with_ov = level >= kslam_batch::Level::pairs, with_records = level >= kslam_batch::Level::records;
    const uint64_t n_rbytes = columns != no_columns && a.n_reads ? a.read_offsets[a.n_reads] : 0;
    if (with_ov) ov.ensure((a.n_overlaps + 1) * sizeof(kslam_overlap));
    groups.ensure((a.n_read_pairs + 1) * sizeof(kslam_read_pair));
    pairs.ensure((a.n_pairs + 1) * sizeof(kslam_paired_overlap));
    if (with_records) pool.ensure((a.n_cigar + 1) * sizeof(uint32_t));
    if (columns != no_columns) rbases.ensure(n_rbytes + 64);
    if (columns == bases_and_quality) rqual.ensure(n_rbytes + 64);
    if (with_records) roff.ensure((a.n_reads + 1) * sizeof(uint64_t));
    if (with_ov && a.n_overlaps) HIPCHK(hipMemcpyAsync(ov.p, a.overlaps, a.n_overlaps * sizeof(kslam_overlap), hipMemcpyHostToDevice, s));
    if (a.n_read_pairs) HIPCHK(hipMemcpyAsync(groups.p, a.read_pairs, a.n_read_pairs * sizeof(kslam_read_pair), hipMemcpyHostToDevice, s));
    if (a.n_pairs) HIPCHK(hipMemcpyAsync(pairs.p, a.pairs, a.n_pairs * sizeof(kslam_paired_overlap), hipMemcpyHostToDevice, s));
    if (with_records && a.n_cigar) HIPCHK(hipMemcpyAsync(pool.p, cigar_pool, a.n_cigar * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (n_rbytes) HIPCHK(hipMemcpyAsync(rbases.p, read_bases, n_rbytes, hipMemcpyHostToDevice, s));
    if (n_rbytes && columns == bases_and_quality && read_quality) HIPCHK(hipMemcpyAsync(rqual.p, read_quality, n_rbytes, hipMemcpyHostToDevice, s));
    if (with_records && a.n_reads) HIPCHK(hipMemcpyAsync(roff.p, a.read_offsets, (a.n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(stream_wait(s));   // (pageable sources)
    const bool with_bases = columns != no_columns;
    return VariantInputs{with_ov ? ov.as<kslam_overlap>() : nullptr,
                         with_ov ? a.n_overlaps : 0,
                         groups.as<kslam_read_pair>(),
                         a.n_read_pairs,
                         pairs.as<kslam_paired_overlap>(),
                         a.n_pairs,
                         with_records ? pool.as<uint32_t>() : nullptr,
                         with_records ? a.n_cigar : 0,
                         with_bases ? rbases.as<uint8_t>() : nullptr,
                         with_records ? roff.as<uint64_t>() : nullptr,
                         with_records ? a.n_reads : 0,
                         ix && with_bases ? ix->g_bases.as<uint8_t>() : nullptr,
                         ix ? ix->g_off.as<uint64_t>() : nullptr,
                         ix ? ix->n_entries : 0};
  }
  void release_all() {
    for (DevBuf *b : {&ov, &groups, &pairs, &pool, &rbases, &rqual, &roff}) b->release();
  }
};

struct kslam_ctx {
  kslam_params prm{};
  Tuning tune;                   // the KSLAM_* environment switches as they stood at kslam_create
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  hipEvent_t ev[16]{};
  hipEvent_t evs0[12]{}, evs1[12]{};   // per-pass events around the k-mer scatter kernel

  // ---- index ----
  // null: no index (kslam_set_index not called, or it failed).  Whatever drops the last reference frees device memory: it runs
  // with this context's device current (inside guarded() or kslam_destroy).
  std::shared_ptr<const GenomeIndex> index;
  const GenomeIndex &need_index() const {
    if (!index) throw StatusError{KSLAM_ERR_STATE, "kslam_set_index has not been called"};
    return *index;
  }
  uint32_t group_route_pause = 0;    // chunks left on the long route after a chunk's overlap keys held a (read, entry) group too
                                     // long for join.hip's group_order (a read in a tandem repeat): such data comes in stretches,
                                     // and a chunk that tries the short route in vain pays for 4 radix passes too many
  uint64_t kept_last = 0;     // survivors of the last chunk (sizes the next chunk's record buffers)

  // ---- resident read batch ----
  bool have_reads = false;
  uint64_t n_reads = 0;
  uint32_t max_read_len = 0;
  // reads the packed SW / extraction kernels cannot hold (more than short_cap bases) are aligned in chunks of their own,
  // by the plain kernels (sw.hip: k_sw_long): class_runs = the read numbers at which the class (short / long) changes
  uint32_t short_cap = 511, max_short_len = 0;
  std::vector<uint64_t> class_runs;
  std::vector<uint64_t> h_roff;  // [n_reads + 1]
  std::vector<uint64_t> h_kpre, h_spre;   // [n_reads + 1] k-mers / extraction segments of the reads before i (chunk planning)
  DevBuf r_bases, r_off, r_len, r_codes;

  // ---- work buffers ----
  DevBuf nk, nseg, rec_start, seg_start, segs, scan_tmp, totals;
  DevBuf recs_a, recs_b, block_tot, block_base, ovk_a, ovk_b, flags, pos, band0;
  SortWorkspace sortws;
  CigarWork cig;
  SwWork sww;
  DevBuf cells;

  // ---- pinned host staging (host-pointer entry point): reused across batches ----
  // kslam_free_batch may run on another thread than the one taking results (a host-tail worker
  // hands buffers back while the main thread takes the next batch's): the pool has its own lock
  struct Pinned { void *p; size_t cap; bool in_use; };
  std::vector<Pinned> pinned;
  std::mutex pin_mu;

  // ---- per-row details for the SAM writer (details.hip) ----
  DevBuf r_qual, d_tables, res_det;
  DevBuf fq_text, fq_bases_at, fq_qual_at;   // kslam_submit_batch_fastq: the uploaded texts and field positions
  FastqWork fqw;                              // kslam_submit_batch_fastq_text: the record index built on the device
  bool have_qual = false, have_details = false;
  uint8_t *d_md_pool = nullptr;   // inside detw.md_pool
  uint64_t n_md = 0;
  uint32_t det_flags = 0;
  DetailWork detw;

  // ---- SAM records / per-read lines on the device (samtext.hip, include/kslam_samtext.h) ----
  SamAnnot annot{};               // device pointers; the primary context owns the buffers, its lanes read them
  std::vector<DevBuf> annot_bufs;
  bool have_annot = false;
  SamWork samw;
  struct { bool sam = false, per_read = false, bgzf = false, bam = false, seq = false, unmapped = false; uint32_t num_alignments = 10; int sam_xa = 0;
           int deflate = KSLAM_BGZF_DEFLATE_FIXED; } samtext;   // for the lanes; deflate: kslam_set_bgzf_deflate, also for kslam_bgzf_compress
  // ---- the coordinate-sorted BAM (bamsort.hip, include/kslam_bamsort.h): the state behind a pointer (bamsort.h), made by the
  // switch on the context it was set on; its lanes append their batches' records to it instead of compressing them
  std::atomic<bool> bsort_on{false};
  kslam::BamSortState *bsort = nullptr;
  kslam::BamSortWork *bsort_w = nullptr;   // this context's own record-index passes (a lane's batches); made by the thread that uses it
  struct { int on = 0, bai_fd = -1; } bsort_stream;   // kslam_stream_set_bam_sort

  // the rows of the reads without alignment (samunmapped.hip, include/kslam_samunmapped.h): this context's own passes, and what
  // kslam_sam_unmapped_kernel_ms reports -- the last batch formatted here or on one of this context's lanes (under as_mu)
  SamUnmappedWork sumw;
  struct { double ms = 0; uint64_t bytes = 0, n_rows = 0; } unmapped_last;
  const uint8_t *d_ids = nullptr;       // read identifiers of the loaded batch (fqw.ids, or ids_buf)
  const uint64_t *d_ids_off = nullptr;
  DevBuf ids_buf, ids_off_buf;
  bool have_ids = false;
  // ---- BGZF (bgzf.hip, include/kslam_bgzf.h): the scratch, the compressed bytes, kslam_bgzf_compress's upload ----
  BgzfWork bgzfw;
  DevBuf bgzf_out, bgzf_in;
  InflateWork inflw;              // kslam_bgzf_inflate (inflate.hip, include/kslam_inflate.h): one round's bytes, text and members
  double inflate_kernel_ms = 0;   // device time of the last kslam_bgzf_inflate's kernels, by events around each round's launch
  // ---- plain gzip (gunzip.hip, include/kslam_gunzip.h): the scratch, the two sizes (0: the default), the last call's figures ----
  GunzipWork gzw;
  struct { uint64_t chunk = 0, round = 0; kslam_gunzip_stats stats{}; } gz;
  bool in_multi = false;          // one of a kslam_multi's contexts
  // ---- the reads split by outcome (readsplit.hip, include/kslam_readsplit.h) ----
  ReadSplitWork rsw;
  struct { uint32_t which = 0; bool bgzf = false; int fds[4] = {-1, -1, -1, -1}; } reads_out;   // for the lanes; fds: kslam_stream_set_reads_out
  struct ReadsOutEntry { bool supported = false; kslam_reads_out out{}; };
  std::map<uint64_t, ReadsOutEntry> ro_ready;   // by ticket: collected batches whose streams kslam_collect_reads_out has not taken (under as_mu)

  // ---- the per-entry coverage table (coverage.hip, include/kslam_coverage.h) ----
  struct Coverage {               // on the context the switch was set on; its lanes mark into it (lane_main)
    std::atomic<bool> on{false};
    uint64_t n_entries = 0, n_words = 0;
    DevBuf bitmap, rows, skipped, word_off;
    BatchUpload up;               // kslam_coverage_add's
    hipEvent_t ev_count[2]{};
    double count_ms = 0;
    int stream_fd = -1;           // kslam_stream_set_coverage
    std::mutex mu;                // add / take / reset / bitmap / the switch: one at a time
  } cov;
  CoverageMarkWork covw;          // this context's own mark passes (a lane's batches; on the primary: kslam_coverage_add)

  // ---- the SNV table (variants.hip, include/kslam_variants.h) ----
  struct Variants {               // on the context the switch was set on; its lanes append to it (lane_main)
    std::atomic<bool> on{false};
    uint64_t n_entries = 0, total_bases = 0;
    DevBuf events, begins, ends;  // u64 keys, append-only between two resets; n_ev / n_iv of them are in use
    uint64_t n_ev = 0, n_iv = 0, n_records = 0, n_skipped = 0;
    bool sorted = false;          // nothing was appended since kslam_variants_take sorted the arrays
    VariantTakeWork tw;
    BatchUpload up;               // kslam_variants_add's
    hipEvent_t ev_take[2]{};
    double take_ms = 0;
    int stream_fd = -1;           // kslam_stream_set_variants
    uint32_t stream_min_alt = 2, stream_min_depth = 1;
    std::mutex mu;                // append / take / reset / the switch: one at a time
  } var;
  EmitWork varw;                  // this context's own emit passes (a lane's batches; on the primary: kslam_variants_add)

  // ---- the indel table (indels.hip, include/kslam_indels.h) ----
  struct Indels {                 // on the context the switch was set on; its lanes append to it (lane_main)
    std::atomic<bool> on{false};
    uint64_t n_entries = 0, total_bases = 0;
    DevBuf begins, ends, dels, ins;   // u64 keys (ins: two per record), append-only between two resets; n[kind] of them are in use
    uint64_t n[INDEL_KINDS] = {0, 0, 0, 0};   // n[INDEL_LONG]: the D runs too long to be counted (nothing is stored for them)
    uint64_t n_records = 0, n_skipped = 0, n_unanchored = 0, n_unrepresentable = 0;
    bool sorted = false;          // nothing was appended since kslam_indels_take sorted the arrays
    VariantTakeWork tw;
    BatchUpload up;               // kslam_indels_add's
    hipEvent_t ev_take[2]{};
    double take_ms = 0;
    int stream_fd = -1;           // kslam_stream_set_indels
    uint32_t stream_min_alt = 2, stream_min_depth = 1;
    std::mutex mu;                // append / take / reset / the switch: one at a time
  } ind;
  EmitWork indw;                  // this context's own emit passes (a lane's batches; on the primary: kslam_indels_add)

  // ---- the consensus caller (consensus.hip, include/kslam_consensus.h) ----
  struct Consensus {              // on the context the switch was set on; its lanes append to it (lane_main)
    std::atomic<bool> on{false};
    uint64_t n_entries = 0, total_bases = 0;
    DevBuf ev, mb, me, db, de, ins;   // the keys, append-only between two resets; n[kind] of them are in use
    uint64_t n[CNS_KINDS] = {0, 0, 0, 0}, n_records = 0, n_skipped = 0, n_unanchored = 0, n_unrepresentable = 0;
    bool sorted = false;          // nothing was appended since kslam_consensus_take sorted the arrays
    uint64_t slice = KSLAM_CONSENSUS_DEFAULT_SLICE;   // kslam_consensus_set_slice
    ConsensusTakeWork tw;
    BatchUpload up;               // kslam_consensus_add's
    hipEvent_t ev_take[2]{};
    double take_ms = 0;
    int stream_fd = -1;           // kslam_stream_set_consensus
    kslam_consensus_params stream_params{1, 500, KSLAM_CONSENSUS_FILL_N, 1};
    std::mutex mu;                // append / take / reset / the switch: one at a time
  } cns;
  EmitWork cnsw;                  // this context's own emit passes (a lane's batches; on the primary: kslam_consensus_add)

  // ---- the depth track (depth.hip, include/kslam_depth.h) ----
  struct Depth {                  // on the context the switch was set on; its lanes append to it (lane_main)
    std::atomic<bool> on{false};
    uint64_t n_entries = 0, max_key = 0;   // max_key: total bases + entries (one spare position per entry)
    DevBuf pending;               // u64 (key << 1) | is_end, appended per batch; n_pend of them are in use
    DevBuf ckey, cnet;            // the compacted list: n_keys distinct boundaries ascending, their net change (i64, never 0)
    uint64_t n_pend = 0, n_keys = 0, n_records = 0, n_skipped = 0, n_iv = 0;
    uint64_t compact_at = 0;      // kslam_depth_set_compact_at; 0: the default
    DepthWork tw;
    BatchUpload up;               // kslam_depth_add's
    hipEvent_t ev[4]{};           // around a compaction, around a take
    double compact_ms = 0, take_ms = 0;
    int stream_fd = -1;           // kslam_stream_set_depth
    uint32_t stream_min_depth = 1;
    std::mutex mu;                // append / compact / take / reset / the switch: one at a time
  } dep;
  EmitWork depw;                  // this context's own emit passes (a lane's batches; on the primary: kslam_depth_add)

  // ---- the Kraken-style report's counts (kreport.hip, include/kslam_kreport.h) ----
  struct Kreport {                // on the context the switch was set on; its lanes count into it (lane_main)
    std::atomic<bool> on{false};
    uint64_t n_nodes = 0;         // of the device tree the state was laid out for
    DevBuf direct, keys, nodes;   // u64 per node; the id -> node table
    DevBuf items;                 // u64 (id << 32 | count) per unknown-id item; n_items of them are in use
    uint64_t n_items = 0;
    DevBuf up_ids;                // kslam_kreport_add's upload
    KreportTakeWork tw;
    hipEvent_t ev_take[2]{};
    double take_ms = 0;
    int stream_fd = -1;           // kslam_stream_set_kreport
    std::mutex mu;                // add / take / reset / the lanes' appends / the switch: one at a time
  } kr;
  KreportCountWork krw;           // this context's own count passes (a lane's batches; on the primary: kslam_kreport_add)

  // ---- the per-gene abundance table (genes.hip, include/kslam_genes.h) ----
  struct Genes {                  // on the context the switch was set on; its lanes count into it (lane_main)
    std::atomic<bool> on{false};
    uint64_t n_entries = 0, n_genes = 0;   // of the annotations the state was laid out for
    DevBuf order, sstart, sstop, runmax;   // the lookup index: 16 bytes per gene
    DevBuf rows, stats;           // u64 [4 * n_genes], u64 [4]
    BatchUpload up;               // kslam_genes_add's
    DevBuf lk_in, lk_out;         // kslam_genes_lookup's triples and answers
    GenesTakeWork tw;
    hipEvent_t ev_take[2]{};
    double build_ms = 0, take_ms = 0;
    int stream_fd = -1;           // kslam_stream_set_genes
    std::mutex mu;                // add / take / reset / lookup / the switch: one at a time
  } gen;
  GenesCountWork genw;            // this context's own count passes (a lane's batches; on the primary: kslam_genes_add)

  // ---- the read QC report's tables (readqc.hip, include/kslam_readqc.h) ----
  struct ReadQc {                 // on the context the switch was set on; its lanes count into it (lane_main)
    std::atomic<bool> on{false};
    uint32_t C = 0;               // cycle rows, resolved
    uint64_t n_words = 0;         // a stream's words
    DevBuf words;                 // u64 [2 * n_words]
    bool paired = false;          // a batch counted since the last reset was paired
    DevBuf up_bases, up_qual, up_off;   // kslam_read_qc_add's uploads
    int stream_fd = -1;           // kslam_stream_set_read_qc
    uint32_t stream_cycles = 0;
    std::mutex mu;                // add / take / reset / the lanes' launches / the switch: one at a time
  } rq;
  ReadQcWork rqw;                 // this context's own count passes (a lane's batches; on the primary: kslam_read_qc_add)

  // ---- the alignment QC report's tables (alignqc.hip, include/kslam_alignqc.h) ----
  struct AlignQc {                // on the context the switch was set on; its lanes count into it (lane_main)
    std::atomic<bool> on{false};
    uint32_t C = 0;               // cycle rows, resolved
    uint64_t n_entries = 0;       // of the index the switch was set for
    DevBuf words;                 // u64 [KSLAM_ALIGN_QC_WORDS(C)]
    bool paired = false;          // a batch counted since the last reset was paired
    BatchUpload up;               // kslam_align_qc_add's
    int stream_fd = -1;           // kslam_stream_set_align_qc
    uint32_t stream_cycles = 0;
    std::mutex mu;                // add / take / reset / the lanes' launches / the switch: one at a time
  } aq;
  AlignQcWork aqw;                // this context's own count passes (a lane's batches; on the primary: kslam_align_qc_add)

  // ---- the reads of chosen taxa (taxreads.hip, include/kslam_taxreads.h) ----
  struct TaxReads {               // on the context kslam_set_taxon_reads was called on; its lanes read it (lane_main)
    std::atomic<bool> on{false};
    std::vector<uint32_t> ids;    // the chosen ids as they were set
    uint32_t mode = 0;
    uint64_t n_nodes = 0;         // of the device tree the mask was laid out for
    DevBuf keys, nodes;           // the id -> node table
    DevBuf mask, unknown;         // one byte per node; the unknown chosen ids (u32, ascending, distinct), n_unknown of them
    uint64_t n_unknown = 0;
    int all_nonzero = 0;
    TaxReadsMaskWork mw;
    DevBuf up_groups, up_ids;     // kslam_taxon_reads_text's uploads
    hipEvent_t ev_mask[2]{};
    double mask_ms = 0, flag_ms = 0, copy_ms = 0;   // kslam_taxon_reads_kernel_ms
    uint64_t bytes_moved = 0;
    int fds[2] = {-1, -1};        // kslam_stream_set_taxon_reads
    std::mutex mu;                // the switch and the mask's read-back: one at a time
  } tr;
  ReadSplitWork tr_rsw;           // this context's own selections (a lane's batches; on the primary: kslam_taxon_reads_text):
  TaxReadsFlagWork trw;           // apart from rsw, so that the split and the selection of one batch do not share a buffer
  std::map<uint64_t, ReadsOutEntry> tr_ready;   // by ticket, as ro_ready: for kslam_collect_taxon_reads (under as_mu)

  // ---- device pairing / screens (pairs.hip) ----
  PairWork pw;
  PairResult pres{};
  bool have_pairs = false;        // c->pres holds pairs (of res_ov, or of records handed in)
  bool pairs_of_result = false;   // ... and they index the rows of the current res_ov (kslam_pair_screen / the lane hook)
  bool phase_a_done = false;      // kslam_pair_phase_a ran on the current result, kslam_pair_phase_b has not yet
  DevBuf pr_ov, pr_len;          // kslam_pair_screen_overlaps: the records and read lengths handed in
  struct { int paired = 1; uint32_t thr = 0; double fraction = 0.95; uint32_t stages = 0; } pairing;   // for the lanes

  // ---- pipelined entry (kslam_align_batch_async): worker lanes, each a sibling context that shares this context's index ----
  bool holds_hook = false;       // this context counts towards the page-locked column allocator being installed
  struct AsyncJob {                   // what was submitted ...
    uint64_t ticket = 0;
    uint64_t n_reads = 0;
    char *cat = nullptr;              // pinned, from the lane context's pool
    char *qcat = nullptr;             // the quality strings, same layout (optional)
    bool borrowed = false;            // cat / qcat / off_ptr are the caller's columns (kslam_submit_batch_columns)
    const uint64_t *off_ptr = nullptr;
    // kslam_submit_batch_fastq: the two texts (cat = r1, qcat = r2) and where the fields lie in [r1 | r2]
    bool fastq = false, fastq_text = false;   // fastq_text: the index is built on the device too
    bool single = false;                      // fastq_text with ONE stream (r2 == NULL): single-end reads
    uint64_t max_pairs = 0; int at_eof = 1;
    uint64_t len1 = 0, len2 = 0;
    const uint64_t *bases_at = nullptr, *quality_at = nullptr;
    std::vector<uint64_t> off;
    // ... and what became of it: the lane writes the result where kslam_collect_batch hands it out from
    bool done = false;
    kslam_status st = KSLAM_OK;
    std::string err;
    kslam_batch_result res{};
    bool ro_on = false, ro_supported = false;   // kslam_set_reads_out was on when the lane ran the batch; it came as FASTQ text
    kslam_reads_out ro{};
    bool tr_on = false, tr_supported = false;   // the same for kslam_set_taxon_reads
    kslam_reads_out tr{};
  };
  struct AsyncLane {
    kslam_ctx *c = nullptr;
    std::thread th;
    std::deque<AsyncJob *> q;     // of the jobs `jobs` owns: a job leaves the map only when it is done
  };
  std::vector<AsyncLane *> lanes;
  std::mutex as_mu, as_compute;
  std::condition_variable as_cv;
  std::map<uint64_t, std::unique_ptr<AsyncJob>> jobs;   // submitted, not yet waited for
  uint64_t next_ticket = 0;
  bool as_stop = false;

  // ---- merge of gathered shard results (merge.hip) ----
  DevBuf mg_shards, mg_lens, mg_off, mg_scan;

  // ---- results of the last align ----
  DevBuf res_ov, res_cig, res_tmp, fin_copy, band0_all;
  uint64_t n_res = 0, n_cig = 0;
  kslam_timings tm{};
};

struct kslam_multi {
  std::vector<kslam_ctx *> ctx;
  std::string err;
  DevBuf rows_out, pool_out;     // on ctx[0]'s device: the batch-global result
  std::vector<DevBuf> send;      // per shard, on its own device: its records in batch terms, ready to copy
};

namespace kslam_api {

template <typename F> kslam_status guarded(kslam_ctx *ctx, F &&f) {
  if (!ctx) return KSLAM_ERR_ARG;
  try {
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
      ctx->err = std::string("hipSetDevice failed: ") + hipGetErrorString(e);
      return KSLAM_ERR_NO_DEVICE;
    }
    f();
    return KSLAM_OK;
  } catch (const StatusError &se) {
    ctx->err = se.msg;
    return se.st;
  } catch (const HipError &he) {
    ctx->err = std::string("HIP error ") + hipGetErrorString(he.code) + " at " + he.file + ":" +
               std::to_string(he.line) + " in " + he.what;
    (void)hipGetLastError();
    return he.code == hipErrorOutOfMemory ? KSLAM_ERR_OOM : KSLAM_ERR_NO_DEVICE;
  } catch (const std::bad_alloc &) {
    ctx->err = "host allocation failed";
    return KSLAM_ERR_OOM;
  }
}

// ---- api_core.hip
uint32_t bits_for(uint64_t max_value);
// grow a device buffer while keeping its first `used` bytes
void ensure_keep(DevBuf &b, size_t bytes, size_t used, hipStream_t s);
void *pinned_alloc(size_t bytes);
void pinned_free(void *p, size_t bytes);
// pinned host buffers from a small per-context pool (pinning is expensive; reuse across batches)
void *pinned_get(kslam_ctx *c, size_t bytes);
bool pinned_put(kslam_ctx *c, void *p);
bool scoring_in_envelope(const kslam_params &p);
// a sibling context shares the primary's index and pairing settings
void share_index(kslam_ctx *dst, const kslam_ctx *src);

// ---- api_index.hip
// extraction of n sequences d_off[0..n] into d_out (AoS records) [+ the first radix pass's digit of every record]
void run_extract(kslam_ctx *c, const uint8_t *d_bases, const uint64_t *d_off, uint64_t n, uint32_t gap, int is_gb,
                 uint64_t n_segs, uint4 *d_out, uint8_t *d_digits = nullptr, const SortPass *first_pass = nullptr);

// ---- api_align.hip
void finish_load_reads(kslam_ctx *c);
float ev_ms(hipEvent_t a, hipEvent_t b);
struct PairingHook {
  int paired;
  uint32_t thr;
  double fraction;
  uint32_t stages;
  bool ran = false;    // false: the batch had several chunks (or nothing to pair): the caller pairs afterwards
};
// the hot path on the resident reads; stop_after_join: only rows a-3..a-6
void align_resident(kslam_ctx *c, bool stop_after_join, uint64_t *n_raw_out, PairingHook *hook = nullptr);

// ---- api_tail.hip

struct SamStage {   // one batch's way through the stage
  SamInputs in;
  SamParams P;
  kslam_paired_overlap *d_recs = nullptr;
  const kslam_read_pair *d_groups = nullptr;
  uint64_t n_groups = 0, n_vals = 0, n_segs = 0, text_bytes = 0, pr_bytes = 0;
  const void *d_sam = nullptr;    // where sam_stage_fetch copies the SAM bytes from (nullptr: samw.text)
  bool bam = false;               // BAM records instead of SAM lines (include/kslam_bam.h)
  bool seq = false;               // SEQ and QUAL on the rows without flag 0x100 (include/kslam_samseq.h)
  bool unmapped = false;          // rows for the reads without alignment behind the others (include/kslam_samunmapped.h)
  double *h_vals = nullptr;       // pinned
  uint32_t *h_seg = nullptr;      // pinned
  uint8_t *h_mapq = nullptr;      // pinned
};

void sam_stage_free(kslam_ctx *c, SamStage &S);
void sam_stage_plan(kslam_ctx *c, const kslam_ctx *owner, int paired, uint32_t num_alignments, int sam_xa, bool sort_groups, SamStage &S);
void sam_stage_mapq(SamStage &S);
void sam_stage_kernels(kslam_ctx *c, const kslam_ctx *owner, SamStage &S, bool want_sam, bool want_per_read);

void sam_stage_fetch(kslam_ctx *c, SamStage &S, bool want_sam, bool want_per_read, char **sam_text, uint64_t *sam_len, char **pr_text,
                     uint64_t *pr_len, uint32_t **tax, uint64_t *n_tax);
void fill_pair_stats(const PairResult &r, kslam_pair_stats *st);
void unmapped_note(kslam_ctx *owner, const kslam_ctx *lane);

// ---- api_lanes.hip
void stop_lanes(kslam_ctx *c);

// ---- api_readsplit.hip
// the split of the batch resident on c (indexed by fastq_index_device: c->fqw) by d_groups; blocks from c's page-locked pool
void split_resident(kslam_ctx *c, bool single, const kslam_read_pair *d_groups, uint64_t n_groups, uint32_t which, bool bgzf, int deflate,
                    kslam_reads_out *out);
void free_reads_out(kslam_ctx *c, kslam_reads_out *out);

}  // namespace kslam_api

#include "api_reports.h"

using namespace kslam_api;
