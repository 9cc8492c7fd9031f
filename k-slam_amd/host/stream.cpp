// stream.cpp -- include/kslam_stream.h: the reference's batch loop (metagenomicAnalysis_Low_Mem, src/SLAM.h:193-250)
// over this library's own C ABI.  Plain C++: every stage it calls is an exported entry point, so a k-SLAM host
// could write the same loop itself (INTEGRATION.md shows it); this file is that loop, tested and timed.
//
//   main thread:  cut batch k+d (kslam_fastq_batch_end) -> kslam_submit_batch_fastq_text ... kslam_collect_batch(k)
//   worker:       host stage of batch k-1: the SAM records and the per-read lines arrive WRITTEN (include/kslam_samtext.h: on the
//                 GPU, inside the lane) and go to kslam_sam_writer (its own thread) / per_read_fd as they are; what is left for
//                 the CPUs is kslam_taxreport_add_batch.  A batch whose text the device left to the host (pseudo-assembly
//                 fallback), or KSLAM_HOST_SAM_TEXT=1: kslam_tail_finish_prepare -> kslam_tail_finish_write_rows,
//                 kslam_tail_classify
// Each opt-in file report is described ONCE, below (struct Report and the eight after it): how it is armed for a call, what a batch
// that no lane fed adds to it, how its file is written behind the last batch and how it is put away.  The loop arms, feeds,
// finishes and disarms them in loops and knows nothing else about a report; a new one is one more description and one more
// entry in Run::reports.
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../../include/kslam_fastq.h"
#include "../../include/kslam_stream.h"
#include "../../include/kslam_samtext.h"
#include "../../include/kslam_bgzf.h"
#include "../../include/kslam_bam.h"
#include "../../include/kslam_samseq.h"
#include "../../include/kslam_samunmapped.h"
#include "../../include/kslam_readsplit.h"
#include "../../include/kslam_coverage.h"
#include "../../include/kslam_alignqc.h"
#include "../../include/kslam_genes.h"
#include "../../include/kslam_kreport.h"
#include "../../include/kslam_readqc.h"
#include "../../include/kslam_taxreads.h"
#include "../../include/kslam_variants.h"
#include "../../include/kslam_indels.h"
#include "../../include/kslam_consensus.h"
#include "../../include/kslam_bamsort.h"
#include "../../include/kslam_depth.h"
#include "workers.hpp"

namespace {
using namespace kslam_host;

bool write_all(int fd, const char *p, uint64_t n) {
  while (n) {
    const ssize_t w = ::write(fd, p, (size_t)std::min<uint64_t>(n, 1ull << 30));
    if (w < 0) {
      if (errno == EINTR) continue;
      return false;
    }
    p += w;
    n -= (uint64_t)w;
  }
  return true;
}

struct Window { uint64_t p1, e1, p2, e2; };   // one batch's stretch of the two texts

// The lanes keep the read bases and qualities on the device, so whoever needs them for a batch handled on the host has the batch's
// window parsed into columns (host/fastq.cpp, the same records the device indexed): once per batch, on first use.
struct Columns {
  const char *r1, *r2;
  Window win;
  bool paired;
  int32_t threads;
  const kslam_batch_result &res;
  kslam_reads_columns cols{};
  bool parsed = false;
  const kslam_reads_columns &get() {
    if (parsed) return cols;
    uint64_t c1 = 0, c2 = 0;
    const kslam_status q = paired ? kslam_fastq_parse_pair(r1 + win.p1, win.e1 - win.p1, r2 + win.p2, win.e2 - win.p2, 0, 1, threads, &cols, &c1, &c2)
                                  : kslam_fastq_parse(r1 + win.p1, win.e1 - win.p1, 0, 1, threads, &cols, &c1);
    if (q != KSLAM_OK) fail(q, kslam_tail_last_error());
    if (cols.n_reads != res.n_reads || memcmp(cols.bases_off, res.reads_bases_off, sizeof(uint64_t) * (res.n_reads + 1)) != 0)
      fail(KSLAM_ERR_INTERNAL, "the host's parse of a batch differs from the device's index");
    parsed = true;
    return cols;
  }
  ~Columns() { kslam_reads_free(&cols); }
};

// what the writers behind the last batch need of the call
struct Ending { kslam_ctx *ctx; const kslam_index_view *index; const kslam_taxdb *taxdb; int paired; uint64_t n_pairs; };

inline void taken(kslam_ctx *ctx, kslam_status s) { if (s != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx)); }
inline void written(kslam_status w) { if (w != KSLAM_OK) fail(w, kslam_tail_last_error()); }
// rows taken from the context, handed back when the writer is done with them
template <typename T> struct Pinned {
  kslam_ctx *ctx;
  T *p = nullptr;
  ~Pinned() { kslam_free_pinned(ctx, p); }
};

struct Report {
  int fd = -1;          // kslam_stream_set_*: where the file goes; the report is wanted when it is >= 0
  bool armed = false;   // this call switched the report on, so this call switches it off
  virtual ~Report() = default;
  virtual void want(kslam_ctx *ctx) = 0;      // kslam_stream_get_*: the descriptor and the parameters
  virtual void arm(kslam_ctx *ctx) = 0;       // kslam_set_* and kslam_*_reset, through started(), when the report is wanted
  // the batch from the host, for a report that counts final alignment pairs: a lane fed it the batch unless the batch's
  // pseudo-assembly was left to the host stage
  virtual void add(kslam_ctx *, const kslam_batch_result &, Columns &) {}
  virtual void finish(const Ending &e) = 0;   // take, write to fd, free
  virtual void disarm(kslam_ctx *ctx) = 0;    // off if armed; kslam_stream_set_* back to "none" (they hold for one call) if ctx

  static void got(kslam_status s) { if (s != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context"); }
  // switched on -- `armed` tells disarm to switch it off again -- and emptied of what an earlier call left
  void started(kslam_ctx *ctx, kslam_status switched_on, kslam_status (*reset)(kslam_ctx *)) {
    if (switched_on != KSLAM_OK) fail(KSLAM_ERR_UNSUPPORTED, kslam_last_error(ctx));
    armed = true;
    if (reset(ctx) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
  }
};

// the per-entry coverage table (include/kslam_coverage.h): the lanes mark what they finish
struct CoverageReport : Report {
  void want(kslam_ctx *ctx) override { got(kslam_stream_get_coverage(ctx, &fd)); }
  void arm(kslam_ctx *ctx) override { if (fd >= 0) started(ctx, kslam_set_coverage(ctx, 1), kslam_coverage_reset); }
  void disarm(kslam_ctx *ctx) override { if (armed) kslam_set_coverage(ctx, 0); if (ctx) kslam_stream_set_coverage(ctx, -1); }
  void add(kslam_ctx *ctx, const kslam_batch_result &res, Columns &) override {
    taken(ctx, kslam_coverage_add(ctx, res.overlaps, res.n_overlaps, res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs));
  }
  void finish(const Ending &e) override {
    Pinned<kslam_entry_coverage> rows{e.ctx};
    uint64_t n_rows = 0, n_skipped = 0;
    taken(e.ctx, kslam_coverage_take(e.ctx, &rows.p, &n_rows, &n_skipped));
    written(kslam_coverage_write(e.index, rows.p, n_rows, fd));
  }
};

// the per-gene abundance table (include/kslam_genes.h): the lanes count what they finish.  Armed behind the annotations: they
// bring the gene columns, and setting them drops the table.
struct GenesReport : Report {
  void want(kslam_ctx *ctx) override { got(kslam_stream_get_genes(ctx, &fd)); }
  void arm(kslam_ctx *ctx) override { if (fd >= 0) started(ctx, kslam_set_genes(ctx, 1), kslam_genes_reset); }
  void disarm(kslam_ctx *ctx) override { if (armed) kslam_set_genes(ctx, 0); if (ctx) kslam_stream_set_genes(ctx, -1); }
  void add(kslam_ctx *ctx, const kslam_batch_result &res, Columns &) override {
    taken(ctx, kslam_genes_add(ctx, res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs));
  }
  void finish(const Ending &e) override {
    Pinned<kslam_gene_row> rows{e.ctx};
    uint64_t n_rows = 0;
    kslam_gene_stats gs;
    taken(e.ctx, kslam_genes_take(e.ctx, &rows.p, &n_rows, &gs));
    written(kslam_genes_write(e.index, rows.p, n_rows, fd));
  }
};

// the Kraken-style report (include/kslam_kreport.h): the lanes count the taxonomy ids they make; a batch classified on the host
// goes in by its ids (add_ids), not through add.  Armed behind the annotations: they bring the device tree.
struct KrakenReport : Report {
  void want(kslam_ctx *ctx) override { got(kslam_stream_get_kreport(ctx, &fd)); }
  void arm(kslam_ctx *ctx) override { if (fd >= 0) started(ctx, kslam_set_kreport(ctx, 1), kslam_kreport_reset); }
  void disarm(kslam_ctx *ctx) override { if (armed) kslam_set_kreport(ctx, 0); if (ctx) kslam_stream_set_kreport(ctx, -1); }
  void add_ids(kslam_ctx *ctx, const uint32_t *ids, uint64_t n) { taken(ctx, kslam_kreport_add(ctx, ids, n)); }
  void finish(const Ending &e) override {
    Pinned<kslam_kreport_row> rows{e.ctx};
    uint64_t n_rows = 0;
    kslam_kreport_stats ks;
    taken(e.ctx, kslam_kreport_take(e.ctx, &rows.p, &n_rows, &ks));
    written(kslam_kreport_write(e.taxdb, rows.p, n_rows, e.n_pairs, fd));
  }
};

// the SNV table (include/kslam_variants.h): the lanes pile up what they finish; the host's batch needs the read bases
struct VariantsReport : Report {
  uint32_t min_alt = 2, min_depth = 1;
  void want(kslam_ctx *ctx) override { got(kslam_stream_get_variants(ctx, &fd, &min_alt, &min_depth)); }
  void arm(kslam_ctx *ctx) override { if (fd >= 0) started(ctx, kslam_set_variants(ctx, 1), kslam_variants_reset); }
  void disarm(kslam_ctx *ctx) override { if (armed) kslam_set_variants(ctx, 0); if (ctx) kslam_stream_set_variants(ctx, -1, 2, 1); }
  void add(kslam_ctx *ctx, const kslam_batch_result &res, Columns &columns) override {
    const kslam_reads_columns &rc = columns.get();
    taken(ctx, kslam_variants_add(ctx, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar, rc.bases, rc.bases_off, rc.n_reads,
                                  res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs));
  }
  void finish(const Ending &e) override {
    Pinned<kslam_variant_row> rows{e.ctx};
    uint64_t n_rows = 0;
    kslam_variant_stats vs;
    taken(e.ctx, kslam_variants_take(e.ctx, min_alt, min_depth, &rows.p, &n_rows, &vs));
    written(kslam_variants_write(e.index, rows.p, n_rows, &vs, fd));
  }
};

// the indel table (include/kslam_indels.h): as the SNV table
struct IndelsReport : Report {
  uint32_t min_alt = 2, min_depth = 1;
  void want(kslam_ctx *ctx) override { got(kslam_stream_get_indels(ctx, &fd, &min_alt, &min_depth)); }
  void arm(kslam_ctx *ctx) override { if (fd >= 0) started(ctx, kslam_set_indels(ctx, 1), kslam_indels_reset); }
  void disarm(kslam_ctx *ctx) override { if (armed) kslam_set_indels(ctx, 0); if (ctx) kslam_stream_set_indels(ctx, -1, 2, 1); }
  void add(kslam_ctx *ctx, const kslam_batch_result &res, Columns &columns) override {
    const kslam_reads_columns &rc = columns.get();
    taken(ctx, kslam_indels_add(ctx, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar, rc.bases, rc.bases_off, rc.n_reads,
                                res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs));
  }
  void finish(const Ending &e) override {
    Pinned<kslam_indel_row> rows{e.ctx};
    uint64_t n_rows = 0;
    kslam_indel_stats is;
    taken(e.ctx, kslam_indels_take(e.ctx, min_alt, min_depth, &rows.p, &n_rows, &is));
    written(kslam_indels_write(e.index, rows.p, n_rows, &is, fd));
  }
};

// the consensus caller (include/kslam_consensus.h): the lanes pile up what they finish; the host's batch needs the read bases
struct ConsensusReport : Report {
  kslam_consensus_params params{1, 500, KSLAM_CONSENSUS_FILL_N, 1};
  void want(kslam_ctx *ctx) override { got(kslam_stream_get_consensus(ctx, &fd, &params)); }
  void arm(kslam_ctx *ctx) override { if (fd >= 0) started(ctx, kslam_set_consensus(ctx, 1), kslam_consensus_reset); }
  void disarm(kslam_ctx *ctx) override { if (armed) kslam_set_consensus(ctx, 0); if (ctx) kslam_stream_set_consensus(ctx, -1, nullptr); }
  void add(kslam_ctx *ctx, const kslam_batch_result &res, Columns &columns) override {
    const kslam_reads_columns &rc = columns.get();
    taken(ctx, kslam_consensus_add(ctx, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar, rc.bases, rc.bases_off, rc.n_reads,
                                   res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs));
  }
  void finish(const Ending &e) override {
    Pinned<kslam_consensus_row> rows{e.ctx};
    Pinned<char> seq{e.ctx};
    uint64_t n_rows = 0;
    kslam_consensus_stats cs;
    taken(e.ctx, kslam_consensus_take(e.ctx, &params, &rows.p, &n_rows, &seq.p, &cs));
    written(kslam_consensus_write(e.index, rows.p, n_rows, seq.p, fd));
  }
};

// the read QC report (include/kslam_readqc.h): the lanes count the columns of every batch they take in, so the host never feeds
// it.  It needs neither the tree nor the pairing.
struct ReadQcReport : Report {
  uint32_t cycles = 0;
  void want(kslam_ctx *ctx) override { got(kslam_stream_get_read_qc(ctx, &fd, &cycles)); }
  void arm(kslam_ctx *ctx) override { if (fd >= 0) started(ctx, kslam_set_read_qc(ctx, 1, cycles), kslam_read_qc_reset); }
  void disarm(kslam_ctx *ctx) override { if (armed) kslam_set_read_qc(ctx, 0, 0); if (ctx) kslam_stream_set_read_qc(ctx, -1, 0); }
  void finish(const Ending &e) override {
    kslam_read_qc_tables qt;
    taken(e.ctx, kslam_read_qc_take(e.ctx, &qt));
    qt.paired = e.paired;   // (a run that ends before its first batch is still the kind of run it was asked to be)
    const kslam_status w = kslam_read_qc_write(&qt, fd);
    kslam_read_qc_release(e.ctx, &qt);
    written(w);
  }
};

// the alignment QC report (include/kslam_alignqc.h): the lanes count what they finish; the host's batch needs the read bases and
// the quality column
struct AlignQcReport : Report {
  uint32_t cycles = 0;
  void want(kslam_ctx *ctx) override { got(kslam_stream_get_align_qc(ctx, &fd, &cycles)); }
  void arm(kslam_ctx *ctx) override { if (fd >= 0) started(ctx, kslam_set_align_qc(ctx, 1, cycles), kslam_align_qc_reset); }
  void disarm(kslam_ctx *ctx) override { if (armed) kslam_set_align_qc(ctx, 0, 0); if (ctx) kslam_stream_set_align_qc(ctx, -1, 0); }
  void add(kslam_ctx *ctx, const kslam_batch_result &res, Columns &columns) override {
    const kslam_reads_columns &rc = columns.get();
    if (memcmp(rc.quality_off, rc.bases_off, sizeof(uint64_t) * (res.n_reads + 1)) != 0)
      fail(KSLAM_ERR_INTERNAL, "the host's parse of a batch differs from the device's index");
    taken(ctx, kslam_align_qc_add(ctx, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar, rc.bases, rc.bases_off, rc.n_reads,
                                  res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs, rc.quality, columns.paired ? 1 : 0));
  }
  void finish(const Ending &e) override {
    kslam_align_qc_tables at;
    taken(e.ctx, kslam_align_qc_take(e.ctx, &at));
    at.paired = e.paired;   // (likewise)
    const kslam_status w = kslam_align_qc_write(&at, fd);
    kslam_align_qc_release(e.ctx, &at);
    written(w);
  }
};

// the depth track (include/kslam_depth.h): the lanes add what they finish; the host's batch needs the reads' lengths alone, which
// came back with the batch (no parse)
struct DepthReport : Report {
  uint32_t min_depth = 1;
  void want(kslam_ctx *ctx) override { got(kslam_stream_get_depth(ctx, &fd, &min_depth)); }
  void arm(kslam_ctx *ctx) override { if (fd >= 0) started(ctx, kslam_set_depth(ctx, 1), kslam_depth_reset); }
  void disarm(kslam_ctx *ctx) override { if (armed) kslam_set_depth(ctx, 0); if (ctx) kslam_stream_set_depth(ctx, -1, 1); }
  void add(kslam_ctx *ctx, const kslam_batch_result &res, Columns &) override {
    taken(ctx, kslam_depth_add(ctx, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar, res.reads_bases_off, res.n_reads,
                               res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs));
  }
  void finish(const Ending &e) override {
    Pinned<kslam_depth_row> rows{e.ctx};
    uint64_t n_rows = 0;
    kslam_depth_stats ds;
    taken(e.ctx, kslam_depth_take(e.ctx, min_depth, &rows.p, &n_rows, &ds));
    written(kslam_depth_write(e.index, rows.p, n_rows, fd));
  }
};

// One collected batch: its result, its two read splits and its window.  Whoever holds it releases it; handing it to the worker
// moves it.  (A block the SAM writer adopts is taken out with res.sam_text = nullptr.)
struct Batch {
  kslam_ctx *ctx;
  kslam_batch_result res{};
  kslam_reads_out ro{}, tro{};
  Window win{};
  uint64_t seq = 0;   // the batch's place in submission order (the sorted BAM's ordinal)
  explicit Batch(kslam_ctx *c) : ctx(c) {}
  Batch(Batch &&o) noexcept : ctx(o.ctx), res(o.res), ro(o.ro), tro(o.tro), win(o.win), seq(o.seq) { o.ctx = nullptr; }
  ~Batch() {
    if (!ctx) return;
    kslam_release_reads_out(ctx, &tro);
    kslam_release_reads_out(ctx, &ro);
    kslam_release_batch(ctx, &res);
  }
};

// The steps of one batch on one thread: each runs only if all before it succeeded; the first failure and that thread's
// thread-local message are kept.
struct Steps {
  kslam_status s = KSLAM_OK;
  std::string err;
  template <typename F> void run(bool wanted, F &&f) {
    if (s != KSLAM_OK || !wanted) return;
    s = guarded(f);
    if (s != KSLAM_OK) err = g_err;
  }
};

// One kslam_stream_classify call.  The main thread writes everything here except what the worker (host_stage, one thread per batch,
// joined before the next starts) and its optional second thread (taxonomy) write:
//   worker:    worker_status, worker_error; of st: batches_pseudo_on_host, seconds_sam_text, n_alignment_pairs,
//              n_read_pairs_aligned, n_overlaps, first_max_insert_size, n_batches, n_pairs, sam_bytes
//   taxonomy:  all_ids (grown and filled); of st: per_read_bytes, seconds_classify, seconds_report
// The main thread reads them only behind the join.
struct Run {
  kslam_ctx *const ctx;
  const kslam_index_view *const index;
  const kslam_taxdb *const taxdb;
  kslam_taxreport *const report;
  const char *const r1, *const r2;
  const uint64_t len1, len2;
  const kslam_stream_params *const P;
  const int pool_cap = P && P->pool_threads ? (int)P->pool_threads : std::max(2, usable_cpus() - 4);
  // KSLAM_HOST_SAM_TEXT=1 keeps the host formatter and the host twins of the splits for every batch (A/B, and the route of a
  // batch the device hands back without text)
  const bool host_text = getenv("KSLAM_HOST_SAM_TEXT") && getenv("KSLAM_HOST_SAM_TEXT")[0] == '1';
  bool paired = false;
  uint32_t depth = 3;
  kslam_stream_stats st{};
  kslam_sam_writer *writer = nullptr;
  std::thread worker;
  kslam_status worker_status = KSLAM_OK;
  std::string worker_error;
  std::deque<uint64_t> tickets;
  std::deque<Window> windows;   // of the tickets, in their order
  std::vector<uint32_t> all_ids;
  bool pairing_set = false, text_set = false, reads_out_set = false, taxreads_on = false, taxreads_set = false;
  int ro_fds[4] = {-1, -1, -1, -1};   // kslam_stream_set_reads_out: where the classified / unclassified records go
  uint32_t ro_which = 0;
  int ro_bgzf = 0;
  int tr_fds[2] = {-1, -1};           // kslam_stream_set_taxon_reads: where the selected R1 / R2 records go
  std::vector<uint32_t> tr_ids;       // the chosen ids and the mode, as kslam_set_taxon_reads was given them before this call
  uint32_t tr_mode = 0;
  int tr_bgzf = 0;
  int bgzf = 0, bam = 0, seq = 0, unmapped = 0;
  // kslam_stream_set_bam_sort (include/kslam_bamsort.h): the SAM file as a coordinate-sorted BAM, written whole behind the last batch
  int sorted = 0, bai_fd = -1;
  bool sort_armed = false;
  uint64_t first_ticket = 0;
  bool any_ticket = false;
  kslam_tail_params host_all, host_write, host_sorted;   // what the host stage still has to run
  // batch boundaries, found ahead of the submission (src/SLAM.h:193, 201-206)
  uint64_t p1 = 0, p2 = 0, done_pairs = 0;
  uint32_t passes_left = 0;
  bool exhausted = false;
  CoverageReport coverage; VariantsReport variants; IndelsReport indels; ConsensusReport consensus; DepthReport depth_track; ReadQcReport read_qc; AlignQcReport align_qc;
  GenesReport genes; KrakenReport kreport;   // armed behind the annotations, which drop them
  // in the order they are fed and finished: it decides which error is reported if two fail
  Report *const reports[9] = {&coverage, &genes, &kreport, &variants, &indels, &consensus, &read_qc, &align_qc, &depth_track};

  void check_arguments(const kslam_stream_stats *stats, uint32_t *const *tax_ids_out) {
    if (!ctx || !index || !P || !stats) fail(KSLAM_ERR_ARG, "null argument");
    if ((len1 && !r1) || (len2 && !r2)) fail(KSLAM_ERR_ARG, "null text");
    paired = P->tail.paired != 0;
    if (!paired && (r2 || len2)) fail(KSLAM_ERR_ARG, "single-end data (tail.paired == 0) is ONE text: r2 must be NULL");
    if (P->pairs_per_batch == 0) fail(KSLAM_ERR_ARG, "pairs_per_batch must be positive");
    if (taxdb && !tax_ids_out) fail(KSLAM_ERR_ARG, "tax_ids output missing");
    depth = P->depth ? P->depth : 3;
    if (const char *e = getenv("KSLAM_STREAM_DEPTH")) depth = (uint32_t)std::max(1, std::min(8, atoi(e)));   // A/B
    passes_left = P->passes > 1 ? P->passes - 1 : 0;
    host_all = host_write = host_sorted = P->tail;
    host_write.pseudo_assembly = 0;
    host_sorted.pseudo_assembly = 0;
    host_sorted.stages = (P->tail.stages ? P->tail.stages : KSLAM_TAIL_ALL) | KSLAM_TAIL_GROUPS_SORTED;
  }

  // The pairing, the two read splits, the reports and the device text, switched on for this call in the one order that works:
  // the annotations drop the chosen taxa, the gene table and the Kraken report, so those are armed behind them.
  void arm() {
    const uint32_t stages = KSLAM_TAIL_INSERT_SCREEN | KSLAM_TAIL_SCORE_SCREEN | (P->tail.pseudo_assembly ? KSLAM_TAIL_PSEUDO_ASM : 0u);
    if (kslam_set_pairing(ctx, paired ? 1 : 0, P->tail.score_threshold, P->tail.score_fraction, stages) != KSLAM_OK)
      fail(KSLAM_ERR_UNSUPPORTED, kslam_last_error(ctx));
    pairing_set = true;
    // the reads themselves, split by outcome (include/kslam_readsplit.h): the lanes cut each batch's streams on the device
    if (kslam_stream_get_reads_out(ctx, ro_fds) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    if (!paired) ro_fds[1] = ro_fds[3] = -1;
    ro_which = ((ro_fds[0] >= 0 || ro_fds[1] >= 0) ? KSLAM_READS_OUT_CLASSIFIED : 0u) |
               ((ro_fds[2] >= 0 || ro_fds[3] >= 0) ? KSLAM_READS_OUT_UNCLASSIFIED : 0u);
    if (ro_which) {
      if (kslam_set_reads_out(ctx, ro_which) != KSLAM_OK || kslam_get_reads_out_bgzf(ctx, &ro_bgzf) != KSLAM_OK)
        fail(KSLAM_ERR_UNSUPPORTED, kslam_last_error(ctx));
      reads_out_set = true;
    }
    // the reads of chosen taxa (include/kslam_taxreads.h): the ids are read NOW -- the annotations set below drop the selection
    // with the old tree -- and set again behind them
    if (kslam_stream_get_taxon_reads(ctx, tr_fds) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    if (!paired) tr_fds[1] = -1;
    taxreads_on = tr_fds[0] >= 0 || tr_fds[1] >= 0;
    if (taxreads_on) {
      if (!taxdb) fail(KSLAM_ERR_STATE, "the reads of chosen taxa need a taxonomy tree (not available with --just-align)");
      uint32_t *ids = nullptr;
      uint64_t n_ids = 0;
      if (kslam_get_taxon_reads(ctx, &ids, &n_ids, &tr_mode) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      tr_ids.assign(ids, ids + n_ids);
      kslam_free(ids);
      if (tr_ids.empty()) fail(KSLAM_ERR_STATE, "kslam_stream_set_taxon_reads without chosen ids: call kslam_set_taxon_reads first");
      if (kslam_get_reads_out_bgzf(ctx, &tr_bgzf) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    }
    // the sorted BAM: switched on (and emptied) ahead of the first ticket, which becomes ordinal 0
    if (kslam_stream_get_bam_sort(ctx, &sorted, &bai_fd) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    if (sorted) {
      if (P->sam_fd < 0) fail(KSLAM_ERR_ARG, "kslam_stream_set_bam_sort needs a SAM file (sam_fd)");
      if (kslam_set_bam_sort(ctx, 1) != KSLAM_OK) fail(KSLAM_ERR_UNSUPPORTED, kslam_last_error(ctx));
      sort_armed = true;
      if (kslam_bam_sort_reset(ctx) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
    }
    Report *const ahead_of_the_annotations[] = {&coverage, &variants, &indels, &consensus, &depth_track, &read_qc, &align_qc};
    for (Report *r : ahead_of_the_annotations) {
      r->want(ctx);
      r->arm(ctx);
    }
    // the SAM records and the per-read lines written on the GPU (include/kslam_samtext.h)
    const bool device_text = !host_text && (P->sam_fd >= 0 || taxdb);
    if (device_text) {
      if (kslam_set_sam_annotations(ctx, index, taxdb) != KSLAM_OK ||
          kslam_set_sam_text(ctx, P->sam_fd >= 0 ? 1 : 0, taxdb ? 1 : 0, P->tail.num_sam_alignments, P->tail.sam_xa) != KSLAM_OK)
        fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      text_set = true;
    }
    kreport.want(ctx);
    if (kreport.fd >= 0 && !taxdb) fail(KSLAM_ERR_STATE, "the Kraken-style report needs a taxonomy tree (not available with --just-align)");
    genes.want(ctx);
    if ((kreport.fd >= 0 || taxreads_on || genes.fd >= 0) && !device_text && kslam_set_sam_annotations(ctx, index, taxdb) != KSLAM_OK)
      fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
    genes.arm(ctx);
    kreport.arm(ctx);
    // the chosen taxa again, on the tree that is on the device now: the lanes select the batches whose ids they make, the others
    // go through kslam_tail_taxon_reads behind the classification on this side
    if (taxreads_on) {
      if (kslam_set_taxon_reads(ctx, tr_ids.data(), tr_ids.size(), tr_mode) != KSLAM_OK) fail(KSLAM_ERR_UNSUPPORTED, kslam_last_error(ctx));
      taxreads_set = true;
    }
  }

  static void give_back(void *user, void *data) { kslam_free_pinned(static_cast<kslam_ctx *>(user), data); }
  uint64_t enqueue_compressed(const char *text, uint64_t len) {
    char *z = nullptr;
    uint64_t zlen = 0;
    if (kslam_bgzf_compress(ctx, text, len, &z, &zlen) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
    if (kslam_sam_writer_enqueue(writer, z, zlen, &give_back, ctx) != KSLAM_OK) fail(KSLAM_ERR_ARG, kslam_tail_last_error());
    return zlen;
  }

  // BGZF (include/kslam_bgzf.h): every SAM byte goes to the writer compressed -- the lanes compress what they format, the
  // header and any host-formatted batch go through kslam_bgzf_compress here; the EOF marker ends the file.
  // BAM (include/kslam_bam.h): the same file framing, with kslam_bam_header's bytes and BAM records inside the members
  void open_writer() {
    if (kslam_get_sam_bgzf(ctx, &bgzf) != KSLAM_OK || kslam_get_sam_bam(ctx, &bam) != KSLAM_OK || kslam_get_sam_seq(ctx, &seq) != KSLAM_OK ||
        kslam_get_sam_unmapped(ctx, &unmapped) != KSLAM_OK)
      fail(KSLAM_ERR_ARG, "null context");
    if (sorted) bam = 1;
    if (bam) bgzf = 1;
    if (P->sam_fd < 0) return;
    if (kslam_sam_writer_open(P->sam_fd, &writer) != KSLAM_OK) fail(KSLAM_ERR_ARG, "could not start the SAM writer");
    if (sorted) return;   // (the header goes out with the records, behind the last batch: finish)
    if (bam) {
      char *h = nullptr;
      uint64_t hlen = 0;
      if (kslam_bam_header(index, P->sam_header, P->sam_header ? P->sam_header_len : 0, &h, &hlen) != KSLAM_OK)
        fail(KSLAM_ERR_ARG, kslam_tail_last_error());
      std::unique_ptr<char, decltype(&free)> own(h, &free);
      enqueue_compressed(h, hlen);
    } else if (bgzf && P->sam_header && P->sam_header_len)
      enqueue_compressed(P->sam_header, P->sam_header_len);
    else if (P->sam_header && P->sam_header_len && kslam_write_queued(writer, P->sam_header, P->sam_header_len) != 0)
      fail(KSLAM_ERR_ARG, "writing the SAM header failed");
  }

  bool next_window(Window *w) {
    if ((exhausted || !(p1 < len1 || p2 < len2)) && passes_left && len1 && (len2 || !paired)) {   // the texts once more
      passes_left--;
      p1 = p2 = 0;
      exhausted = false;
    }
    if (exhausted || !(p1 < len1 || p2 < len2)) return false;
    uint64_t want = P->pairs_per_batch;
    if (P->max_pairs_total) {
      if (done_pairs >= P->max_pairs_total) return false;
      want = std::min(want, P->max_pairs_total - done_pairs);   // readsPerGoTemp
    }
    uint64_t e1 = 0, e2 = 0;
    int c1 = 0, c2 = 0;
    const double tc = now_ms();
    if (kslam_fastq_batch_end(r1 + p1, len1 - p1, want, 1, P->tail.threads, &e1, &c1) != KSLAM_OK ||
        (paired && kslam_fastq_batch_end(r2 + p2, len2 - p2, want, 1, P->tail.threads, &e2, &c2) != KSLAM_OK))
      fail(KSLAM_ERR_ARG, kslam_tail_last_error());
    st.seconds_cutting += (now_ms() - tc) * 1e-3;
    *w = Window{p1, p1 + e1, p2, p2 + e2};
    done_pairs += want;
    p1 += e1;
    p2 += e2;
    // R1 decides when the stream is over (src/FASTQsequence.h:114-116: no read from R1, no batch).  R2 running out first does not:
    // the next window then holds R1's records and nothing of R2, and the batch is refused as the reference refuses it (:118-122)
    // -- also when R2 ends exactly where a batch ends.
    if (p1 >= len1) exhausted = true;
    return true;
  }

  // keeps `depth` batches in flight
  void submit_ahead() {
    Window w;
    while (tickets.size() < depth && next_window(&w)) {
      uint64_t tk = 0;
      const double tsub = now_ms();
      // "at end of stream" for inner windows too: a window ends right after a terminator (kslam_fastq_batch_end looked at
      // the byte behind a closing "\r"), so the end-of-stream rule adds nothing and keeps that "\r" a whole terminator
      // (single end: r2 == NULL is how the library is told that there is one stream)
      if (kslam_submit_batch_fastq_text(ctx, r1 + w.p1, w.e1 - w.p1, paired ? r2 + w.p2 : nullptr, paired ? w.e2 - w.p2 : 0, 0, 1, &tk) != KSLAM_OK)
        fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      st.seconds_submitting += (now_ms() - tsub) * 1e-3;
      if (!any_ticket) first_ticket = tk;
      any_ticket = true;
      tickets.push_back(tk);
      windows.push_back(w);
    }
  }

  // The oldest ticket's batch into `b`, and the worker of the batch before it joined.  false: an empty batch ends the loop
  // (src/SLAM.h:207).
  bool collect(Batch &b) {
    const double ta = now_ms();
    const uint64_t tk = tickets.front();
    tickets.pop_front();
    b.win = windows.front();
    b.seq = tk - first_ticket;
    windows.pop_front();
    const kslam_status cs = kslam_collect_batch(ctx, tk, &b.res);
    const double tb = now_ms();
    st.seconds_waiting_for_gpu += (tb - ta) * 1e-3;
    if (worker.joinable()) worker.join();
    st.seconds_waiting_for_host_stage += (now_ms() - tb) * 1e-3;
    if (cs != KSLAM_OK) fail(cs, kslam_last_error(ctx));
    const kslam_status rs = ro_which ? kslam_collect_reads_out(ctx, tk, &b.ro) : KSLAM_OK;
    if (rs != KSLAM_OK) fail(rs, kslam_last_error(ctx));
    const kslam_status ts = taxreads_set ? kslam_collect_taxon_reads(ctx, tk, &b.tro) : KSLAM_OK;
    if (ts != KSLAM_OK) fail(ts, kslam_last_error(ctx));
    if (worker_status != KSLAM_OK) fail(worker_status, worker_error);
    if (b.res.n_reads == 0) return false;
    if (!b.res.read_pairs && b.res.n_overlaps) fail(KSLAM_ERR_INTERNAL, "the lane returned no device pairing");
    return true;
  }

  // ---- The host stage of one batch, on the worker thread (it owns the batch), in the reference's order (src/SLAM.h:228-246):
  //   (1) everything that CHANGES res.read_pairs / res.pairs: what the device left of pseudo-assembly + the second score
  //       screen, then writeSAMOutputPairs' per-pair sort (only when there is a SAM file: without one the reference does
  //       not sort, and the classification sees the unsorted order) -- prepare;
  //   (2) the SAM text on this thread and the taxonomy part (per-read LCA, <out>_PerRead, the report's records) on a
  //       second one at the same time.  From here on both only READ `res`; the pool shares its workers between their
  //       loops, and the serial stretches of one (offsets, buffer growth, the per-read file's write) run under the
  //       other's loops instead of leaving the workers idle.
  void prepare(const kslam_batch_result &res, const kslam_reads_view &reads, bool pseudo_left) {
    if (pseudo_left) st.batches_pseudo_on_host++;
    const kslam_tail_params *tp = pseudo_left ? &host_all : &host_write;
    kslam_tail_stats ps;
    memset(&ps, 0, sizeof ps);
    const double t0 = now_ms();
    if (res.text_flags & KSLAM_TEXT_PAIRS_SORTED) {   // the device finished every stage and ran the per-pair sort: nothing to change
      ps.n_read_pairs = res.n_read_pairs;
      for (uint64_t g = 0; g < res.n_read_pairs; g++) ps.n_paired_final += res.read_pairs[g].count;
    } else {
      const kslam_status a = kslam_tail_finish_prepare(tp, &reads, res.overlaps, res.n_overlaps, res.read_pairs, res.n_read_pairs, res.pairs,
                                                       res.n_pairs, writer ? 1 : 0, &ps);
      if (a != KSLAM_OK) fail(a, kslam_tail_last_error());
    }
    st.seconds_sam_text += (now_ms() - t0) * 1e-3;
    st.n_alignment_pairs += ps.n_paired_final;
    st.n_read_pairs_aligned += ps.n_read_pairs;
    st.n_overlaps += res.n_overlaps;
    if (st.n_batches == 0) st.first_max_insert_size = res.pair_stats.max_insert_size;
    st.n_batches++;
    st.n_pairs += P->tail.paired ? res.n_reads / 2 : res.n_reads;
  }

  // The taxonomy part: the batch's ids behind all_ids, its per-read lines to their file, its records to the XML report.
  // Returns the ids when kslam_tail_classify made them here (no lane counted or selected by them), else NULL.
  const uint32_t *taxonomy(const kslam_batch_result &res, const kslam_reads_view &reads) {
    const uint32_t *host_ids = nullptr;
    const double t1 = now_ms();
    const size_t base = all_ids.size();
    all_ids.resize(base + res.n_read_pairs);
    uint64_t tlen = 0;
    bool wrote = true;
    if (res.text_flags & KSLAM_TEXT_PER_READ) {   // taxonomy ids and lines came with the batch (GPU)
      if (res.n_read_pairs) memcpy(all_ids.data() + base, res.tax_ids, sizeof(uint32_t) * res.n_read_pairs);
      tlen = res.per_read_len;
      wrote = P->per_read_fd < 0 || write_all(P->per_read_fd, res.per_read_text, tlen);
    } else {
      char *text = nullptr;
      const kslam_status b = kslam_tail_classify(&host_write, &reads, index, taxdb, res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs,
                                                 all_ids.data() + base, &text, &tlen);
      if (b != KSLAM_OK) fail(b, kslam_tail_last_error());
      host_ids = all_ids.data() + base;
      wrote = P->per_read_fd < 0 || write_all(P->per_read_fd, text, tlen);
      kslam_free(text);
    }
    if (!wrote) fail(KSLAM_ERR_ARG, std::string("writing the per-read file failed: ") + strerror(errno));
    st.per_read_bytes += tlen;
    const double t2 = now_ms();
    st.seconds_classify += (t2 - t1) * 1e-3;
    if (report) {
      const kslam_status c = kslam_taxreport_add_batch(report, &reads, index, res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs,
                                                       all_ids.data() + base);
      if (c != KSLAM_OK) fail(c, kslam_tail_last_error());
      st.seconds_report += (now_ms() - t2) * 1e-3;
    }
    return host_ids;
  }

  // The batch's SAM text as the GPU wrote it: the page-locked block joins the writer's queue as it is and goes back to the
  // context's pool once it is in the file.
  void device_text_route(kslam_batch_result &res) {
    const double t0 = now_ms();
    if (bam && !(res.text_flags & KSLAM_TEXT_SAM_BAM))   // (a batch formatted before the switch went on: text, not records)
      fail(KSLAM_ERR_STATE, "kslam_set_sam_bam was switched on while a batch was in flight");
    if ((seq != 0) != ((res.text_flags & KSLAM_TEXT_SAM_SEQ) != 0))   // (host-formatted batches follow `seq`: one file, one form)
      fail(KSLAM_ERR_STATE, "kslam_set_sam_seq was changed while kslam_stream_classify was running");
    if ((unmapped != 0) != ((res.text_flags & KSLAM_TEXT_SAM_UNMAPPED) != 0))   // (host-formatted batches follow `unmapped`)
      fail(KSLAM_ERR_STATE, "kslam_set_sam_unmapped was changed while kslam_stream_classify was running");
    if (sorted) {   // the lane holds the records in the sort's store: nothing travels, nothing is written yet
      if (!(res.text_flags & KSLAM_TEXT_SAM_HELD)) fail(KSLAM_ERR_STATE, "kslam_set_bam_sort was switched off while kslam_stream_classify was running");
      st.seconds_sam_text += (now_ms() - t0) * 1e-3;
      return;
    }
    if (bgzf && !(res.text_flags & KSLAM_TEXT_SAM_BGZF)) {   // (the switch went on after the batch was formatted)
      st.sam_bytes += enqueue_compressed(res.sam_text, res.sam_text_len);
    } else {
      char *block = res.sam_text;
      const uint64_t len = res.sam_text_len;
      res.sam_text = nullptr;   // the writer owns it now
      if (kslam_sam_writer_enqueue(writer, block, len, &give_back, ctx) != KSLAM_OK) fail(KSLAM_ERR_ARG, kslam_tail_last_error());
      st.sam_bytes += len;
    }
    st.seconds_sam_text += (now_ms() - t0) * 1e-3;
  }

  // The batch's SAM text formatted here, by the host twins of what the lanes run.
  void host_text_route(const kslam_batch_result &res, const kslam_reads_view &reads, Columns &columns, uint64_t ordinal) {
    kslam_tail_stats ts;
    memset(&ts, 0, sizeof ts);
    const double t0 = now_ms();
    // BGZF: the batch's text is gathered whole and compressed like a device-formatted one (same members, same bytes)
    std::string text;
    static const kslam_write_fn append = [](void *user, const char *data, uint64_t len) -> int {
      static_cast<std::string *>(user)->append(data, len);
      return 0;
    };
    // BAM: the same stage writing records (kslam_tail_finish_write_rows_bam), gathered and compressed the same way
    // SEQ / QUAL (include/kslam_samseq.h): the twin with the switch on, either record kind, over the batch's parsed
    // columns; the rows then read what the device's rows read.
    kslam_reads_view seq_reads = reads;
    if (seq) {
      const kslam_reads_columns &rc = columns.get();
      seq_reads.bases = rc.bases;
      seq_reads.quality = rc.quality;
      seq_reads.quality_off = rc.quality_off;
    }
    const kslam_write_fn wr = bgzf ? append : kslam_write_queued;
    void *const wu = bgzf ? (void *)&text : (void *)writer;
    const kslam_status a =
        seq ? kslam_tail_finish_write_rows_seq(&host_sorted, &seq_reads, index, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar,
                                               res.details, res.md_pool, res.n_md, res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs, bam,
                                               wr, wu, &ts)
            : (bam ? kslam_tail_finish_write_rows_bam : kslam_tail_finish_write_rows)(
                  &host_sorted, &reads, index, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar, res.details, res.md_pool, res.n_md,
                  res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs, wr, wu, &ts);
    if (a != KSLAM_OK) fail(a, kslam_tail_last_error());
    // (include/kslam_samunmapped.h) the rows of the reads without alignment behind the batch's rows, by the host twin
    if (unmapped) {
      char *rows = nullptr;
      uint64_t rows_len = 0;
      const kslam_status u = kslam_tail_sam_unmapped(&P->tail, &seq_reads, res.read_pairs, res.n_read_pairs,
                                                     paired ? res.n_reads / 2 : res.n_reads, bam, seq, &rows, &rows_len);
      if (u != KSLAM_OK) fail(u, kslam_tail_last_error());
      std::unique_ptr<char, decltype(&kslam_free)> own(rows, &kslam_free);
      if (rows_len && wr(wu, rows, rows_len) != 0) fail(KSLAM_ERR_ARG, "writing the SAM rows of the unaligned reads failed");
      if (!bgzf) ts.sam_bytes += rows_len;
    }
    if (sorted) {   // the batch's records join the lanes' in the sort's store, under the batch's ordinal
      if (kslam_bam_sort_add(ctx, ordinal, text.data(), text.size()) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
    } else
      st.sam_bytes += bgzf ? enqueue_compressed(text.data(), text.size()) : ts.sam_bytes;
    st.seconds_sam_text += (now_ms() - t0) * 1e-3;
  }

  // One batch's split streams to their files, on the host stage's thread (batch order; not behind the SAM writer's queue);
  // plain blocks are compressed like the device's when the files are BGZF, so that both routes write the same file.
  void write_split(const kslam_reads_out &out, const int *fds, int n_fds, int to_bgzf, const char *noun) {
    for (int k = 0; k < n_fds; k++) {
      if (fds[k] < 0 || !out.len[k]) continue;
      bool ok;
      if (to_bgzf && !(out.flags & KSLAM_READS_OUT_BGZF)) {
        char *z = nullptr;
        uint64_t zlen = 0;
        if (kslam_bgzf_compress(ctx, out.data[k], out.len[k], &z, &zlen) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
        ok = write_all(fds[k], z, zlen);
        kslam_free_pinned(ctx, z);
      } else {
        if (!to_bgzf && (out.flags & KSLAM_READS_OUT_BGZF)) fail(KSLAM_ERR_STATE, "kslam_set_reads_out_bgzf was changed while kslam_stream_classify was running");
        ok = write_all(fds[k], out.data[k], out.len[k]);
      }
      if (!ok) fail(KSLAM_ERR_ARG, std::string("writing ") + noun + " failed: " + strerror(errno));
    }
  }
  // After the stage that finishes res.read_pairs: a batch the device left without streams is split here by the host twin.
  void write_reads_out(Batch &b) {
    const Window &w = b.win;
    if ((b.ro.flags & KSLAM_READS_OUT_LEFT_TO_HOST) || host_text) {
      kslam_release_reads_out(ctx, &b.ro);
      if (kslam_tail_split_reads(r1 + w.p1, w.e1 - w.p1, paired ? r2 + w.p2 : nullptr, paired ? w.e2 - w.p2 : 0, 0, 1, b.res.read_pairs,
                                 b.res.n_read_pairs, ro_which, &b.ro) != KSLAM_OK)
        fail(KSLAM_ERR_ARG, kslam_tail_last_error());
    }
    write_split(b.ro, ro_fds, 4, ro_bgzf, "a reads-out file");
  }
  // Likewise the selected records; `ids`: the batch's taxonomy ids, final by now.
  void write_taxon_reads(Batch &b, const uint32_t *ids) {
    const Window &w = b.win;
    if ((b.tro.flags & KSLAM_READS_OUT_LEFT_TO_HOST) || host_text) {
      kslam_release_reads_out(ctx, &b.tro);
      if (kslam_tail_taxon_reads(taxdb, tr_ids.data(), tr_ids.size(), tr_mode, r1 + w.p1, w.e1 - w.p1, paired ? r2 + w.p2 : nullptr,
                                 paired ? w.e2 - w.p2 : 0, 0, 1, b.res.read_pairs, ids, b.res.n_read_pairs, &b.tro) != KSLAM_OK)
        fail(KSLAM_ERR_ARG, kslam_tail_last_error());
    }
    write_split(b.tro, tr_fds, 2, tr_bgzf, "a file of selected reads");
  }

  void host_stage(Batch b) {
    name_thread("kslam-host");
    kslam_batch_result &res = b.res;
    const size_t ids_base = all_ids.size();   // where the taxonomy part puts this batch's ids
    const kslam_reads_view reads = {res.n_reads, nullptr, res.reads_bases_off, nullptr, res.reads_bases_off, res.reads_ids, res.reads_ids_off};
    // the batch's pseudo-assembly was left to this stage: no lane fed it to the reports that count final alignment pairs
    const bool pseudo_left = P->tail.pseudo_assembly && !(res.pair_stats.stages_done & KSLAM_TAIL_PSEUDO_ASM);
    Columns columns{r1, r2, b.win, paired, P->tail.threads, res};
    Steps main, tax;
    const uint32_t *host_ids = nullptr;
    std::thread tax_thread;
    main.run(true, [this, &res, &reads, pseudo_left] { prepare(res, reads, pseudo_left); });
    const auto tax_part = [this, &tax, &res, &reads, &host_ids] {
      tax.run(true, [this, &res, &reads, &host_ids] { host_ids = taxonomy(res, reads); });
    };
    if (main.s == KSLAM_OK && taxdb && P->host_threads != 1) tax_thread = std::thread([&tax_part] { name_thread("kslam-tax"); tax_part(); });
    main.run(ro_which != 0, [this, &b] { write_reads_out(b); });
    // the reports that count final alignment pairs: this stage has just finished the batch's, where no lane did
    for (Report *r : reports) main.run(r->armed && pseudo_left, [this, r, &res, &columns] { r->add(ctx, res, columns); });
    if (writer && (res.text_flags & KSLAM_TEXT_SAM)) main.run(true, [this, &res] { device_text_route(res); });
    else main.run(writer != nullptr, [this, &b, &res, &reads, &columns] { host_text_route(res, reads, columns, b.seq); });
    if (tax_thread.joinable()) tax_thread.join();
    else if (taxdb && main.s == KSLAM_OK) tax_part();
    if (main.s == KSLAM_OK && tax.s != KSLAM_OK) main = tax;
    // the Kraken report: a lane counted the batch unless its ids were made by the classification above
    main.run(kreport.armed && host_ids, [this, &res, host_ids] { kreport.add_ids(ctx, host_ids, res.n_read_pairs); });
    // the selection: behind the classification, whose ids the host twin needs for a batch no lane selected
    main.run(taxreads_set, [this, &b, ids_base] { write_taxon_reads(b, all_ids.data() + ids_base); });
    if (main.s != KSLAM_OK && worker_status == KSLAM_OK) {
      worker_status = main.s;
      worker_error = main.err;            // (the failing thread's thread-local message)
    }
  }

  // behind the last batch and its host stage: the end markers of the compressed files, then every armed report's file
  void finish() {
    if (worker.joinable()) worker.join();
    if (worker_status != KSLAM_OK) fail(worker_status, worker_error);
    if (writer && sorted) {   // every batch is in: the whole sorted file and its index, in front of the other report files
      kslam_bam_sort_stats bs;
      int fd = bai_fd;
      if (kslam_bam_sort_take(ctx, P->sam_header, P->sam_header ? P->sam_header_len : 0, kslam_write_queued, writer, bai_fd >= 0 ? kslam_write_fd : nullptr,
                              &fd, &bs) != KSLAM_OK)
        fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      st.sam_bytes = bs.compressed_bytes;
    } else if (writer && bgzf && kslam_write_queued(writer, KSLAM_BGZF_EOF, KSLAM_BGZF_EOF_LEN) != 0)
      fail(KSLAM_ERR_ARG, "writing the BGZF EOF marker failed");
    if (ro_which && ro_bgzf)
      for (int k = 0; k < 4; k++)
        if (ro_fds[k] >= 0 && !write_all(ro_fds[k], KSLAM_BGZF_EOF, KSLAM_BGZF_EOF_LEN)) fail(KSLAM_ERR_ARG, "writing a reads-out file's BGZF EOF marker failed");
    if (taxreads_set && tr_bgzf)
      for (int k = 0; k < 2; k++)
        if (tr_fds[k] >= 0 && !write_all(tr_fds[k], KSLAM_BGZF_EOF, KSLAM_BGZF_EOF_LEN)) fail(KSLAM_ERR_ARG, "writing the BGZF EOF marker of a file of selected reads failed");
    const Ending e{ctx, index, taxdb, paired ? 1 : 0, st.n_pairs};
    for (Report *r : reports)
      if (r->armed) r->finish(e);
  }

  // whatever happens: the worker joined, the tickets collected and released, the writer closed, and everything this call switched
  // on switched off; the descriptors and parameters held for this call alone go back to their defaults
  kslam_status wind_down() {
    if (worker.joinable()) worker.join();
    for (uint64_t tk : tickets) {
      kslam_batch_result r;
      if (kslam_collect_batch(ctx, tk, &r) == KSLAM_OK) kslam_release_batch(ctx, &r);
    }
    tickets.clear();
    kslam_status w = KSLAM_OK;
    if (writer) {
      uint64_t bytes = 0;
      double sec = 0;
      w = kslam_sam_writer_close(writer, &bytes, &sec);
      st.seconds_in_write = sec;
      writer = nullptr;
    }
    if (text_set) kslam_set_sam_text(ctx, 0, 0, 10, 0);
    if (reads_out_set) kslam_set_reads_out(ctx, 0);
    for (Report *r : reports) r->disarm(ctx);
    if (sort_armed) kslam_set_bam_sort(ctx, 0);
    if (ctx) kslam_stream_set_bam_sort(ctx, 0, -1);
    if (taxreads_set) kslam_set_taxon_reads(ctx, nullptr, 0, 0);
    if (ctx) kslam_stream_set_taxon_reads(ctx, nullptr);
    if (ctx) kslam_stream_set_reads_out(ctx, nullptr);
    if (pairing_set) kslam_set_pairing(ctx, 1, 0, 0.95, 0);
    Pool::get().remove_cap(pool_cap);
    return w;
  }
};

}  // namespace

extern "C" kslam_status kslam_stream_classify(kslam_ctx *ctx, const kslam_index_view *index, const kslam_taxdb *taxdb,
                                              kslam_taxreport *report, const char *r1, uint64_t len1, const char *r2,
                                              uint64_t len2, const kslam_stream_params *P, uint32_t **tax_ids_out,
                                              uint64_t *n_tax_ids, kslam_stream_stats *stats) {
  if (tax_ids_out) *tax_ids_out = nullptr;
  if (n_tax_ids) *n_tax_ids = 0;
  const double t_begin = now_ms();
  Run run{ctx, index, taxdb, report, r1, r2, len1, len2, P};
  run.st.first_max_insert_size = 0xFFFFFFFFu;
  Pool::get().add_cap(run.pool_cap);
  const kslam_status status = guarded([&run, stats, tax_ids_out] {
    run.check_arguments(stats, tax_ids_out);
    run.arm();
    run.open_writer();
    for (;;) {
      run.submit_ahead();
      if (run.tickets.empty()) break;
      Batch b(run.ctx);
      if (!run.collect(b)) break;   // (the host stage of the batch before has ended in there)
      run.worker = std::thread(&Run::host_stage, &run, std::move(b));
    }
    run.finish();
  });
  const double t_close = now_ms();
  const kslam_status closing = run.wind_down();
  run.st.seconds_closing = (now_ms() - t_close) * 1e-3;
  run.st.seconds = (now_ms() - t_begin) * 1e-3;
  if (stats) *stats = run.st;
  if (status != KSLAM_OK) return status;
  if (closing != KSLAM_OK) return closing;
  if (taxdb && tax_ids_out) {
    uint32_t *out = (uint32_t *)malloc(sizeof(uint32_t) * (run.all_ids.size() + 1));
    if (!out) return KSLAM_ERR_OOM;
    if (!run.all_ids.empty()) memcpy(out, run.all_ids.data(), sizeof(uint32_t) * run.all_ids.size());
    *tax_ids_out = out;
    if (n_tax_ids) *n_tax_ids = run.all_ids.size();
  }
  return KSLAM_OK;
}
