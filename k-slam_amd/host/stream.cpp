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
#include "../../include/kslam_consensus.h"
#include "../../include/kslam_depth.h"
#include "workers.hpp"

namespace {
using namespace kslam_host;

struct Window { uint64_t p1, e1, p2, e2; };

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

}  // namespace

extern "C" kslam_status kslam_stream_classify(kslam_ctx *ctx, const kslam_index_view *index, const kslam_taxdb *taxdb,
                                              kslam_taxreport *report, const char *r1, uint64_t len1, const char *r2,
                                              uint64_t len2, const kslam_stream_params *P, uint32_t **tax_ids_out,
                                              uint64_t *n_tax_ids, kslam_stream_stats *stats) {
  if (tax_ids_out) *tax_ids_out = nullptr;
  if (n_tax_ids) *n_tax_ids = 0;
  kslam_stream_stats st;
  memset(&st, 0, sizeof st);
  st.first_max_insert_size = 0xFFFFFFFFu;
  const double t_begin = now_ms();
  kslam_sam_writer *writer = nullptr;
  std::thread worker;
  kslam_status worker_status = KSLAM_OK;
  std::string worker_error;
  std::deque<uint64_t> tickets;
  std::vector<uint32_t> all_ids;
  bool pairing_set = false, text_set = false, reads_out_set = false;
  int ro_fds[4] = {-1, -1, -1, -1};   // kslam_stream_set_reads_out: where the classified / unclassified records go
  uint32_t ro_which = 0;
  int ro_bgzf = 0;
  int cov_fd = -1;                    // kslam_stream_set_coverage: where the coverage report goes
  bool coverage_set = false;
  int gen_fd = -1;                    // kslam_stream_set_genes: where the per-gene table goes
  bool genes_set = false;
  int var_fd = -1;                   // kslam_stream_set_variants: where the VCF file goes
  uint32_t var_min_alt = 2, var_min_depth = 1;
  bool variants_set = false;
  int cns_fd = -1;                   // kslam_stream_set_consensus: where the consensus FASTA goes
  kslam_consensus_params cns_params{1, 500, KSLAM_CONSENSUS_FILL_N, 1};
  bool consensus_set = false;
  int dep_fd = -1;                    // kslam_stream_set_depth: where the bedGraph file goes
  uint32_t dep_min = 1;
  bool depth_set = false;
  int kr_fd = -1;                     // kslam_stream_set_kreport: where the Kraken-style report goes
  bool kreport_set = false;
  int qc_fd = -1;                     // kslam_stream_set_read_qc: where the read QC report goes
  uint32_t qc_cycles = 0;
  bool read_qc_set = false;
  int aq_fd = -1;                     // kslam_stream_set_align_qc: where the alignment QC report goes
  uint32_t aq_cycles = 0;
  bool align_qc_set = false;
  int tr_fds[2] = {-1, -1};           // kslam_stream_set_taxon_reads: where the selected R1 / R2 records go
  bool taxreads_on = false, taxreads_set = false;
  std::vector<uint32_t> tr_ids;       // the chosen ids and the mode, as kslam_set_taxon_reads was given them before this call
  uint32_t tr_mode = 0;
  int tr_bgzf = 0;

  const int pool_cap = P && P->pool_threads ? (int)P->pool_threads : std::max(2, usable_cpus() - 4);
  Pool::get().add_cap(pool_cap);
  // whatever happens: the worker joined, the tickets collected and released, the writer closed, the pairing switched off
  auto wind_down = [&]() -> kslam_status {
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
    if (coverage_set) kslam_set_coverage(ctx, 0);
    if (ctx) kslam_stream_set_coverage(ctx, -1);          // held for this call alone, like the descriptors below
    if (genes_set) kslam_set_genes(ctx, 0);
    if (ctx) kslam_stream_set_genes(ctx, -1);
    if (variants_set) kslam_set_variants(ctx, 0);
    if (ctx) kslam_stream_set_variants(ctx, -1, 2, 1);
    if (consensus_set) kslam_set_consensus(ctx, 0);
    if (ctx) kslam_stream_set_consensus(ctx, -1, nullptr);
    if (depth_set) kslam_set_depth(ctx, 0);
    if (ctx) kslam_stream_set_depth(ctx, -1, 1);
    if (kreport_set) kslam_set_kreport(ctx, 0);
    if (ctx) kslam_stream_set_kreport(ctx, -1);
    if (read_qc_set) kslam_set_read_qc(ctx, 0, 0);
    if (ctx) kslam_stream_set_read_qc(ctx, -1, 0);
    if (align_qc_set) kslam_set_align_qc(ctx, 0, 0);
    if (ctx) kslam_stream_set_align_qc(ctx, -1, 0);
    if (taxreads_set) kslam_set_taxon_reads(ctx, nullptr, 0, 0);
    if (ctx) kslam_stream_set_taxon_reads(ctx, nullptr);
    if (ctx) kslam_stream_set_reads_out(ctx, nullptr);   // the descriptors held for this call alone
    if (pairing_set) kslam_set_pairing(ctx, 1, 0, 0.95, 0);
    Pool::get().remove_cap(pool_cap);
    return w;
  };

  const kslam_status status = guarded([&] {
    if (!ctx || !index || !P || !stats) fail(KSLAM_ERR_ARG, "null argument");
    if ((len1 && !r1) || (len2 && !r2)) fail(KSLAM_ERR_ARG, "null text");
    const bool paired = P->tail.paired != 0;
    if (!paired && (r2 || len2)) fail(KSLAM_ERR_ARG, "single-end data (tail.paired == 0) is ONE text: r2 must be NULL");
    if (P->pairs_per_batch == 0) fail(KSLAM_ERR_ARG, "pairs_per_batch must be positive");
    if (taxdb && !tax_ids_out) fail(KSLAM_ERR_ARG, "tax_ids output missing");
    uint32_t depth = P->depth ? P->depth : 3;
    if (const char *e = getenv("KSLAM_STREAM_DEPTH")) depth = (uint32_t)std::max(1, std::min(8, atoi(e)));   // A/B
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
    // a report for this call: switched on -- `set` tells wind_down to switch it off again -- and emptied of what an earlier call left
    auto started = [&](kslam_status switched_on, bool &set, kslam_status (*reset)(kslam_ctx *)) {
      if (switched_on != KSLAM_OK) fail(KSLAM_ERR_UNSUPPORTED, kslam_last_error(ctx));
      set = true;
      if (reset(ctx) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
    };
    // the per-entry coverage table (include/kslam_coverage.h): the lanes mark what they finish; the report follows the last batch
    if (kslam_stream_get_coverage(ctx, &cov_fd) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    if (cov_fd >= 0) started(kslam_set_coverage(ctx, 1), coverage_set, kslam_coverage_reset);
    // the SNV table (include/kslam_variants.h): the lanes pile up what they finish; the VCF file follows the last batch
    if (kslam_stream_get_variants(ctx, &var_fd, &var_min_alt, &var_min_depth) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    if (var_fd >= 0) started(kslam_set_variants(ctx, 1), variants_set, kslam_variants_reset);
    // the consensus caller (include/kslam_consensus.h): the lanes pile up what they finish; the FASTA file follows the last batch
    if (kslam_stream_get_consensus(ctx, &cns_fd, &cns_params) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    if (cns_fd >= 0) started(kslam_set_consensus(ctx, 1), consensus_set, kslam_consensus_reset);
    // the depth track (include/kslam_depth.h): the lanes add what they finish; the bedGraph file follows the last batch
    if (kslam_stream_get_depth(ctx, &dep_fd, &dep_min) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    if (dep_fd >= 0) started(kslam_set_depth(ctx, 1), depth_set, kslam_depth_reset);
    // the read QC report (include/kslam_readqc.h): the lanes count the columns of every batch they take in; the file follows the
    // last batch.  It needs neither the tree nor the pairing.
    if (kslam_stream_get_read_qc(ctx, &qc_fd, &qc_cycles) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    if (qc_fd >= 0) started(kslam_set_read_qc(ctx, 1, qc_cycles), read_qc_set, kslam_read_qc_reset);
    // the alignment QC report (include/kslam_alignqc.h): the lanes count what they finish; the file follows the last batch
    if (kslam_stream_get_align_qc(ctx, &aq_fd, &aq_cycles) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    if (aq_fd >= 0) started(kslam_set_align_qc(ctx, 1, aq_cycles), align_qc_set, kslam_align_qc_reset);
    const bool host_split = getenv("KSLAM_HOST_SAM_TEXT") && getenv("KSLAM_HOST_SAM_TEXT")[0] == '1';   // (A/B: the host twin for every batch)
    // the SAM records and the per-read lines written on the GPU (include/kslam_samtext.h); KSLAM_HOST_SAM_TEXT=1 keeps the
    // host formatter for everything (A/B, and the route of a batch the device hands back without text)
    const bool device_text = !(getenv("KSLAM_HOST_SAM_TEXT") && getenv("KSLAM_HOST_SAM_TEXT")[0] == '1') && (P->sam_fd >= 0 || taxdb);
    if (device_text) {
      if (kslam_set_sam_annotations(ctx, index, taxdb) != KSLAM_OK ||
          kslam_set_sam_text(ctx, P->sam_fd >= 0 ? 1 : 0, taxdb ? 1 : 0, P->tail.num_sam_alignments, P->tail.sam_xa) != KSLAM_OK)
        fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      text_set = true;
    }
    // the Kraken-style report (include/kslam_kreport.h): the lanes count the taxonomy ids they make, the batches classified here
    // go in through kslam_kreport_add; the file follows the last batch.  Behind the annotations: they bring the device tree.
    if (kslam_stream_get_kreport(ctx, &kr_fd) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    if (kr_fd >= 0 && !taxdb) fail(KSLAM_ERR_STATE, "the Kraken-style report needs a taxonomy tree (not available with --just-align)");
    if (kslam_stream_get_genes(ctx, &gen_fd) != KSLAM_OK) fail(KSLAM_ERR_ARG, "null context");
    if ((kr_fd >= 0 || taxreads_on || gen_fd >= 0) && !device_text && kslam_set_sam_annotations(ctx, index, taxdb) != KSLAM_OK)
      fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
    // the per-gene abundance table (include/kslam_genes.h): the lanes count what they finish; the file follows the last batch.
    // Behind the annotations: they bring the gene columns, and setting them drops the table.
    if (gen_fd >= 0) started(kslam_set_genes(ctx, 1), genes_set, kslam_genes_reset);
    if (kr_fd >= 0) started(kslam_set_kreport(ctx, 1), kreport_set, kslam_kreport_reset);
    // the chosen taxa again, on the tree that is on the device now: the lanes select the batches whose ids they make, the others
    // go through kslam_tail_taxon_reads behind the classification on this side
    if (taxreads_on) {
      if (kslam_set_taxon_reads(ctx, tr_ids.data(), tr_ids.size(), tr_mode) != KSLAM_OK) fail(KSLAM_ERR_UNSUPPORTED, kslam_last_error(ctx));
      taxreads_set = true;
    }
    // BGZF (include/kslam_bgzf.h): every SAM byte goes to the writer compressed -- the lanes compress what they format, the
    // header and any host-formatted batch go through kslam_bgzf_compress here; the EOF marker ends the file
    int bgzf = 0, bam = 0, seq = 0, unmapped = 0;
    if (kslam_get_sam_bgzf(ctx, &bgzf) != KSLAM_OK || kslam_get_sam_bam(ctx, &bam) != KSLAM_OK || kslam_get_sam_seq(ctx, &seq) != KSLAM_OK ||
        kslam_get_sam_unmapped(ctx, &unmapped) != KSLAM_OK)
      fail(KSLAM_ERR_ARG, "null context");
    // BAM (include/kslam_bam.h): the same file framing, with kslam_bam_header's bytes and BAM records inside the members
    if (bam) bgzf = 1;
    static const auto give_back = [](void *user, void *data) { kslam_free_pinned(static_cast<kslam_ctx *>(user), data); };
    auto enqueue_compressed = [&](const char *text, uint64_t len) -> uint64_t {
      char *z = nullptr;
      uint64_t zlen = 0;
      if (kslam_bgzf_compress(ctx, text, len, &z, &zlen) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      if (kslam_sam_writer_enqueue(writer, z, zlen, +give_back, ctx) != KSLAM_OK) fail(KSLAM_ERR_ARG, kslam_tail_last_error());
      return zlen;
    };
    if (P->sam_fd >= 0) {
      if (kslam_sam_writer_open(P->sam_fd, &writer) != KSLAM_OK) fail(KSLAM_ERR_ARG, "could not start the SAM writer");
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
    kslam_tail_params host_all = P->tail, host_write = P->tail, host_sorted = P->tail;   // what the host stage still has to run
    host_write.pseudo_assembly = 0;
    host_sorted.pseudo_assembly = 0;
    host_sorted.stages = (P->tail.stages ? P->tail.stages : KSLAM_TAIL_ALL) | KSLAM_TAIL_GROUPS_SORTED;

    // ---- batch boundaries, found ahead of the submission (src/SLAM.h:193, 201-206) ----
    uint64_t p1 = 0, p2 = 0, done_pairs = 0;
    uint32_t passes_left = P->passes > 1 ? P->passes - 1 : 0;
    bool exhausted = false;
    auto next_window = [&](Window *w) -> bool {
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
      if (p1 >= len1 || (paired && p2 >= len2)) exhausted = true;
      return true;
    };

    // The host stage of one batch, on the worker thread (it owns `res`), in the reference's order (src/SLAM.h:228-246):
    //   (1) everything that CHANGES res.read_pairs / res.pairs: what the device left of pseudo-assembly + the second score
    //       screen, then writeSAMOutputPairs' per-pair sort (only when there is a SAM file: without one the reference does
    //       not sort, and the classification sees the unsorted order) -- kslam_tail_finish_prepare;
    //   (2) the SAM text on this thread and the taxonomy part (per-read LCA, <out>_PerRead, the report's records) on a
    //       second one at the same time.  From here on both only READ `res`; the pool shares its workers between their
    //       loops, and the serial stretches of one (offsets, buffer growth, the per-read file's write) run under the
    //       other's loops instead of leaving the workers idle.
    // One batch's streams to their files, on the host stage's thread (batch order; not behind the SAM writer's queue).  After
    // the stage that finishes res.read_pairs: a batch the device left without streams is split here by the host twin, and its
    // blocks compressed like the device's, so that both routes write the same file.
    auto write_reads_out = [&](const kslam_batch_result &res, kslam_reads_out &ro, Window win) {
      if ((ro.flags & KSLAM_READS_OUT_LEFT_TO_HOST) || host_split) {
        kslam_release_reads_out(ctx, &ro);
        if (kslam_tail_split_reads(r1 + win.p1, win.e1 - win.p1, paired ? r2 + win.p2 : nullptr, paired ? win.e2 - win.p2 : 0, 0, 1,
                                   res.read_pairs, res.n_read_pairs, ro_which, &ro) != KSLAM_OK)
          fail(KSLAM_ERR_ARG, kslam_tail_last_error());
      }
      for (int k = 0; k < 4; k++) {
        if (ro_fds[k] < 0 || !ro.len[k]) continue;
        bool ok;
        if (ro_bgzf && !(ro.flags & KSLAM_READS_OUT_BGZF)) {
          char *z = nullptr;
          uint64_t zlen = 0;
          if (kslam_bgzf_compress(ctx, ro.data[k], ro.len[k], &z, &zlen) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
          ok = write_all(ro_fds[k], z, zlen);
          kslam_free_pinned(ctx, z);
        } else {
          if (!ro_bgzf && (ro.flags & KSLAM_READS_OUT_BGZF)) fail(KSLAM_ERR_STATE, "kslam_set_reads_out_bgzf was changed while kslam_stream_classify was running");
          ok = write_all(ro_fds[k], ro.data[k], ro.len[k]);
        }
        if (!ok) fail(KSLAM_ERR_ARG, std::string("writing a reads-out file failed: ") + strerror(errno));
      }
    };
    // The selected records of one batch to their files, likewise; `ids`: the batch's taxonomy ids, final by now.
    auto write_taxon_reads = [&](const kslam_batch_result &res, kslam_reads_out &tro, Window win, const uint32_t *ids) {
      if ((tro.flags & KSLAM_READS_OUT_LEFT_TO_HOST) || host_split) {
        kslam_release_reads_out(ctx, &tro);
        if (kslam_tail_taxon_reads(taxdb, tr_ids.data(), tr_ids.size(), tr_mode, r1 + win.p1, win.e1 - win.p1, paired ? r2 + win.p2 : nullptr,
                                   paired ? win.e2 - win.p2 : 0, 0, 1, res.read_pairs, ids, res.n_read_pairs, &tro) != KSLAM_OK)
          fail(KSLAM_ERR_ARG, kslam_tail_last_error());
      }
      for (int k = 0; k < 2; k++) {
        if (tr_fds[k] < 0 || !tro.len[k]) continue;
        bool ok;
        if (tr_bgzf && !(tro.flags & KSLAM_READS_OUT_BGZF)) {
          char *z = nullptr;
          uint64_t zlen = 0;
          if (kslam_bgzf_compress(ctx, tro.data[k], tro.len[k], &z, &zlen) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
          ok = write_all(tr_fds[k], z, zlen);
          kslam_free_pinned(ctx, z);
        } else {
          if (!tr_bgzf && (tro.flags & KSLAM_READS_OUT_BGZF)) fail(KSLAM_ERR_STATE, "kslam_set_reads_out_bgzf was changed while kslam_stream_classify was running");
          ok = write_all(tr_fds[k], tro.data[k], tro.len[k]);
        }
        if (!ok) fail(KSLAM_ERR_ARG, std::string("writing a file of selected reads failed: ") + strerror(errno));
      }
    };
    auto host_stage = [&](kslam_batch_result res, kslam_reads_out ro, kslam_reads_out tro, Window win) {
      name_thread("kslam-host");
      const size_t ids_base = all_ids.size();   // where tax_part puts this batch's ids
      kslam_reads_view reads = {res.n_reads, nullptr, res.reads_bases_off, nullptr, res.reads_bases_off, res.reads_ids, res.reads_ids_off};
      kslam_status tax_status = KSLAM_OK;
      std::string tax_error;
      std::thread tax_thread;
      const uint32_t *host_ids = nullptr;   // the batch's taxonomy ids when kslam_tail_classify made them here
      // the batch's pseudo-assembly was left to this stage: no lane fed it to the reports that count final alignment pairs
      const bool pseudo_left = P->tail.pseudo_assembly && !(res.pair_stats.stages_done & KSLAM_TAIL_PSEUDO_ASM);
      // The lanes keep the read bases and qualities on the device, so whoever needs them for a batch handled here has the batch's
      // window parsed into columns (host/fastq.cpp, the same records the device indexed): once per batch, on first use.
      kslam_reads_columns cols;
      memset(&cols, 0, sizeof cols);
      struct Release { kslam_reads_columns *c; ~Release() { kslam_reads_free(c); } } release{&cols};
      bool parsed = false;
      auto columns = [&]() -> const kslam_reads_columns & {
        if (parsed) return cols;
        uint64_t c1 = 0, c2 = 0;
        const kslam_status q = paired ? kslam_fastq_parse_pair(r1 + win.p1, win.e1 - win.p1, r2 + win.p2, win.e2 - win.p2, 0, 1,
                                                               P->tail.threads, &cols, &c1, &c2)
                                      : kslam_fastq_parse(r1 + win.p1, win.e1 - win.p1, 0, 1, P->tail.threads, &cols, &c1);
        if (q != KSLAM_OK) fail(q, kslam_tail_last_error());
        if (cols.n_reads != res.n_reads || memcmp(cols.bases_off, res.reads_bases_off, sizeof(uint64_t) * (res.n_reads + 1)) != 0)
          fail(KSLAM_ERR_INTERNAL, "the host's parse of a batch differs from the device's index");
        parsed = true;
        return cols;
      };
      auto tax_part = [&] {
          tax_status = guarded([&] {
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
              const kslam_status b = kslam_tail_classify(&host_write, &reads, index, taxdb, res.read_pairs, res.n_read_pairs, res.pairs,
                                                         res.n_pairs, all_ids.data() + base, &text, &tlen);
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
              const kslam_status c = kslam_taxreport_add_batch(report, &reads, index, res.read_pairs, res.n_read_pairs, res.pairs,
                                                               res.n_pairs, all_ids.data() + base);
              if (c != KSLAM_OK) fail(c, kslam_tail_last_error());
              st.seconds_report += (now_ms() - t2) * 1e-3;
            }
          });
          if (tax_status != KSLAM_OK) tax_error = g_err;
      };
      kslam_status s = guarded([&] {
        if (pseudo_left) st.batches_pseudo_on_host++;
        const kslam_tail_params *tp = pseudo_left ? &host_all : &host_write;
        kslam_tail_stats ps;
        memset(&ps, 0, sizeof ps);
        const double t0 = now_ms();
        if (res.text_flags & KSLAM_TEXT_PAIRS_SORTED) {   // the device finished every stage and ran the per-pair sort: nothing to change
          ps.n_read_pairs = res.n_read_pairs;
          for (uint64_t g = 0; g < res.n_read_pairs; g++) ps.n_paired_final += res.read_pairs[g].count;
        } else {
          const kslam_status a = kslam_tail_finish_prepare(tp, &reads, res.overlaps, res.n_overlaps, res.read_pairs, res.n_read_pairs,
                                                           res.pairs, res.n_pairs, writer ? 1 : 0, &ps);
          if (a != KSLAM_OK) fail(a, kslam_tail_last_error());
        }
        st.seconds_sam_text += (now_ms() - t0) * 1e-3;
        st.n_alignment_pairs += ps.n_paired_final;
        st.n_read_pairs_aligned += ps.n_read_pairs;
        st.n_overlaps += res.n_overlaps;
        if (st.n_batches == 0) st.first_max_insert_size = res.pair_stats.max_insert_size;
        st.n_batches++;
        st.n_pairs += P->tail.paired ? res.n_reads / 2 : res.n_reads;
      });
      std::string err = s != KSLAM_OK ? g_err : std::string();
      const bool two_threads = P->host_threads != 1;
      if (s == KSLAM_OK && taxdb && two_threads) tax_thread = std::thread([&] { name_thread("kslam-tax"); tax_part(); });
      if (s == KSLAM_OK && ro_which) {
        s = guarded([&] { write_reads_out(res, ro, win); });
        if (s != KSLAM_OK) err = g_err;
      }
      // The reports that count final alignment pairs: a lane fed them the batch unless its pseudo-assembly was left to this stage,
      // which has just finished its read pairs.
      auto add = [&](bool report_set, auto &&call) {
        if (s != KSLAM_OK || !report_set || !pseudo_left) return;
        s = guarded(call);
        if (s != KSLAM_OK) err = g_err;
      };
      add(coverage_set, [&] {
        if (kslam_coverage_add(ctx, res.overlaps, res.n_overlaps, res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs) != KSLAM_OK)
          fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      });
      add(genes_set, [&] {
        if (kslam_genes_add(ctx, res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      });
      // the variants need the read bases
      add(variants_set, [&] {
        const kslam_reads_columns &rc = columns();
        if (kslam_variants_add(ctx, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar, rc.bases, rc.bases_off, rc.n_reads, res.read_pairs,
                               res.n_read_pairs, res.pairs, res.n_pairs) != KSLAM_OK)
          fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      });
      // the consensus caller likewise
      add(consensus_set, [&] {
        const kslam_reads_columns &rc = columns();
        if (kslam_consensus_add(ctx, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar, rc.bases, rc.bases_off, rc.n_reads, res.read_pairs,
                                res.n_read_pairs, res.pairs, res.n_pairs) != KSLAM_OK)
          fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      });
      // the alignment QC report the quality column as well
      add(align_qc_set, [&] {
        const kslam_reads_columns &rc = columns();
        if (memcmp(rc.quality_off, rc.bases_off, sizeof(uint64_t) * (res.n_reads + 1)) != 0)
          fail(KSLAM_ERR_INTERNAL, "the host's parse of a batch differs from the device's index");
        if (kslam_align_qc_add(ctx, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar, rc.bases, rc.bases_off, rc.n_reads, res.read_pairs,
                               res.n_read_pairs, res.pairs, res.n_pairs, rc.quality, paired ? 1 : 0) != KSLAM_OK)
          fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      });
      // the depth track the reads' lengths alone, which came back with the batch
      add(depth_set, [&] {
        if (kslam_depth_add(ctx, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar, res.reads_bases_off, res.n_reads, res.read_pairs,
                            res.n_read_pairs, res.pairs, res.n_pairs) != KSLAM_OK)
          fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      });
      if (s == KSLAM_OK && writer && (res.text_flags & KSLAM_TEXT_SAM)) {
        s = guarded([&] {   // written on the GPU: the page-locked block joins the writer's queue as it is and goes back to the
                            // context's pool once it is in the file
          const double t0 = now_ms();
          if (bam && !(res.text_flags & KSLAM_TEXT_SAM_BAM))   // (a batch formatted before the switch went on: text, not records)
            fail(KSLAM_ERR_STATE, "kslam_set_sam_bam was switched on while a batch was in flight");
          if ((seq != 0) != ((res.text_flags & KSLAM_TEXT_SAM_SEQ) != 0))   // (host-formatted batches follow `seq`: one file, one form)
            fail(KSLAM_ERR_STATE, "kslam_set_sam_seq was changed while kslam_stream_classify was running");
          if ((unmapped != 0) != ((res.text_flags & KSLAM_TEXT_SAM_UNMAPPED) != 0))   // (host-formatted batches follow `unmapped`)
            fail(KSLAM_ERR_STATE, "kslam_set_sam_unmapped was changed while kslam_stream_classify was running");
          if (bgzf && !(res.text_flags & KSLAM_TEXT_SAM_BGZF)) {   // (the switch went on after the batch was formatted)
            st.sam_bytes += enqueue_compressed(res.sam_text, res.sam_text_len);
          } else {
            char *block = res.sam_text;
            const uint64_t len = res.sam_text_len;
            res.sam_text = nullptr;   // the writer owns it now
            if (kslam_sam_writer_enqueue(writer, block, len, +give_back, ctx) != KSLAM_OK) fail(KSLAM_ERR_ARG, kslam_tail_last_error());
            st.sam_bytes += len;
          }
          st.seconds_sam_text += (now_ms() - t0) * 1e-3;
        });
        if (s != KSLAM_OK) err = g_err;
      } else if (s == KSLAM_OK && writer) {
        s = guarded([&] {
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
            const kslam_reads_columns &rc = columns();
            seq_reads.bases = rc.bases;
            seq_reads.quality = rc.quality;
            seq_reads.quality_off = rc.quality_off;
          }
          const kslam_write_fn wr = bgzf ? append : kslam_write_queued;
          void *const wu = bgzf ? (void *)&text : (void *)writer;
          const kslam_status a =
              seq ? kslam_tail_finish_write_rows_seq(&host_sorted, &seq_reads, index, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar,
                                                     res.details, res.md_pool, res.n_md, res.read_pairs, res.n_read_pairs, res.pairs,
                                                     res.n_pairs, bam, wr, wu, &ts)
                  : (bam ? kslam_tail_finish_write_rows_bam : kslam_tail_finish_write_rows)(
                        &host_sorted, &reads, index, res.overlaps, res.n_overlaps, res.cigar_pool, res.n_cigar, res.details, res.md_pool,
                        res.n_md, res.read_pairs, res.n_read_pairs, res.pairs, res.n_pairs, wr, wu, &ts);
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
          st.sam_bytes += bgzf ? enqueue_compressed(text.data(), text.size()) : ts.sam_bytes;
          st.seconds_sam_text += (now_ms() - t0) * 1e-3;
        });
        if (s != KSLAM_OK) err = g_err;
      }
      if (tax_thread.joinable()) tax_thread.join();
      else if (taxdb && s == KSLAM_OK) tax_part();
      if (s == KSLAM_OK && tax_status != KSLAM_OK) {
        s = tax_status;
        err = tax_error;
      }
      // the report: a lane counted the batch unless its ids were made by the classification above
      if (s == KSLAM_OK && kreport_set && host_ids) {
        s = guarded([&] {
          if (kslam_kreport_add(ctx, host_ids, res.n_read_pairs) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
        });
        if (s != KSLAM_OK) err = g_err;
      }
      // the selection: behind the classification, whose ids the host twin needs for a batch no lane selected
      if (s == KSLAM_OK && taxreads_set) {
        s = guarded([&] { write_taxon_reads(res, tro, win, all_ids.data() + ids_base); });
        if (s != KSLAM_OK) err = g_err;
      }
      kslam_release_reads_out(ctx, &tro);
      kslam_release_reads_out(ctx, &ro);
      kslam_release_batch(ctx, &res);
      if (s != KSLAM_OK && worker_status == KSLAM_OK) {
        worker_status = s;
        worker_error = err;            // (the failing thread's thread-local message)
      }
    };

    std::deque<Window> windows;   // of the tickets, in their order
    for (;;) {
      Window w;
      while (tickets.size() < depth && next_window(&w)) {
        uint64_t tk = 0;
        const double tsub = now_ms();
        // "at end of stream" for inner windows too: a window ends right after a terminator (kslam_fastq_batch_end looked at
        // the byte behind a closing "\r"), so the end-of-stream rule adds nothing and keeps that "\r" a whole terminator
        // (single end: r2 == NULL is how the library is told that there is one stream)
        if (kslam_submit_batch_fastq_text(ctx, r1 + w.p1, w.e1 - w.p1, paired ? r2 + w.p2 : nullptr, paired ? w.e2 - w.p2 : 0, 0, 1,
                                          &tk) != KSLAM_OK)
          fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
        st.seconds_submitting += (now_ms() - tsub) * 1e-3;
        tickets.push_back(tk);
        windows.push_back(w);
      }
      if (tickets.empty()) break;
      const double ta = now_ms();
      kslam_batch_result res;
      const uint64_t tk = tickets.front();
      tickets.pop_front();
      const Window win = windows.front();
      windows.pop_front();
      const kslam_status cs = kslam_collect_batch(ctx, tk, &res);
      const double tb = now_ms();
      st.seconds_waiting_for_gpu += (tb - ta) * 1e-3;
      if (worker.joinable()) worker.join();
      st.seconds_waiting_for_host_stage += (now_ms() - tb) * 1e-3;
      if (cs != KSLAM_OK) fail(cs, kslam_last_error(ctx));
      kslam_reads_out ro;
      memset(&ro, 0, sizeof ro);
      const kslam_status rs = ro_which ? kslam_collect_reads_out(ctx, tk, &ro) : KSLAM_OK;
      if (rs != KSLAM_OK) {
        kslam_release_batch(ctx, &res);
        fail(rs, kslam_last_error(ctx));
      }
      kslam_reads_out tro;
      memset(&tro, 0, sizeof tro);
      const kslam_status ts = taxreads_set ? kslam_collect_taxon_reads(ctx, tk, &tro) : KSLAM_OK;
      if (ts != KSLAM_OK) {
        kslam_release_reads_out(ctx, &ro);
        kslam_release_batch(ctx, &res);
        fail(ts, kslam_last_error(ctx));
      }
      if (worker_status != KSLAM_OK) {
        kslam_release_reads_out(ctx, &tro);
        kslam_release_reads_out(ctx, &ro);
        kslam_release_batch(ctx, &res);
        fail(worker_status, worker_error);
      }
      if (res.n_reads == 0) {          // an empty batch ends the loop (src/SLAM.h:207)
        kslam_release_reads_out(ctx, &tro);
        kslam_release_reads_out(ctx, &ro);
        kslam_release_batch(ctx, &res);
        break;
      }
      if (!res.read_pairs && res.n_overlaps) {
        kslam_release_reads_out(ctx, &tro);
        kslam_release_reads_out(ctx, &ro);
        kslam_release_batch(ctx, &res);
        fail(KSLAM_ERR_INTERNAL, "the lane returned no device pairing");
      }
      worker = std::thread(host_stage, res, ro, tro, win);
    }
    if (worker.joinable()) worker.join();
    if (worker_status != KSLAM_OK) fail(worker_status, worker_error);
    if (writer && bgzf && kslam_write_queued(writer, KSLAM_BGZF_EOF, KSLAM_BGZF_EOF_LEN) != 0) fail(KSLAM_ERR_ARG, "writing the BGZF EOF marker failed");
    if (ro_which && ro_bgzf)
      for (int k = 0; k < 4; k++)
        if (ro_fds[k] >= 0 && !write_all(ro_fds[k], KSLAM_BGZF_EOF, KSLAM_BGZF_EOF_LEN)) fail(KSLAM_ERR_ARG, "writing a reads-out file's BGZF EOF marker failed");
    if (taxreads_set && tr_bgzf)
      for (int k = 0; k < 2; k++)
        if (tr_fds[k] >= 0 && !write_all(tr_fds[k], KSLAM_BGZF_EOF, KSLAM_BGZF_EOF_LEN)) fail(KSLAM_ERR_ARG, "writing the BGZF EOF marker of a file of selected reads failed");
    if (coverage_set) {
      kslam_entry_coverage *rows = nullptr;
      uint64_t n_rows = 0, n_skipped = 0;
      if (kslam_coverage_take(ctx, &rows, &n_rows, &n_skipped) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      const kslam_status w = kslam_coverage_write(index, rows, n_rows, cov_fd);
      kslam_free_pinned(ctx, rows);
      if (w != KSLAM_OK) fail(w, kslam_tail_last_error());
    }
    if (genes_set) {
      kslam_gene_row *rows = nullptr;
      uint64_t n_rows = 0;
      kslam_gene_stats gs;
      if (kslam_genes_take(ctx, &rows, &n_rows, &gs) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      const kslam_status w = kslam_genes_write(index, rows, n_rows, gen_fd);
      kslam_free_pinned(ctx, rows);
      if (w != KSLAM_OK) fail(w, kslam_tail_last_error());
    }
    if (kreport_set) {
      kslam_kreport_row *rows = nullptr;
      uint64_t n_rows = 0;
      kslam_kreport_stats ks;
      if (kslam_kreport_take(ctx, &rows, &n_rows, &ks) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      const kslam_status w = kslam_kreport_write(taxdb, rows, n_rows, st.n_pairs, kr_fd);
      kslam_free_pinned(ctx, rows);
      if (w != KSLAM_OK) fail(w, kslam_tail_last_error());
    }
    if (variants_set) {
      kslam_variant_row *rows = nullptr;
      uint64_t n_rows = 0;
      kslam_variant_stats vs;
      if (kslam_variants_take(ctx, var_min_alt, var_min_depth, &rows, &n_rows, &vs) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      const kslam_status w = kslam_variants_write(index, rows, n_rows, &vs, var_fd);
      kslam_free_pinned(ctx, rows);
      if (w != KSLAM_OK) fail(w, kslam_tail_last_error());
    }
    if (consensus_set) {
      kslam_consensus_row *rows = nullptr;
      uint64_t n_rows = 0;
      char *seq = nullptr;
      kslam_consensus_stats cs;
      if (kslam_consensus_take(ctx, &cns_params, &rows, &n_rows, &seq, &cs) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      const kslam_status w = kslam_consensus_write(index, rows, n_rows, seq, cns_fd);
      kslam_free_pinned(ctx, rows);
      kslam_free_pinned(ctx, seq);
      if (w != KSLAM_OK) fail(w, kslam_tail_last_error());
    }
    if (read_qc_set) {
      kslam_read_qc_tables qt;
      if (kslam_read_qc_take(ctx, &qt) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      qt.paired = paired ? 1 : 0;   // (a run that ends before its first batch is still the kind of run it was asked to be)
      const kslam_status w = kslam_read_qc_write(&qt, qc_fd);
      kslam_read_qc_release(ctx, &qt);
      if (w != KSLAM_OK) fail(w, kslam_tail_last_error());
    }
    if (align_qc_set) {
      kslam_align_qc_tables at;
      if (kslam_align_qc_take(ctx, &at) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      at.paired = paired ? 1 : 0;   // (a run that ends before its first batch is still the kind of run it was asked to be)
      const kslam_status w = kslam_align_qc_write(&at, aq_fd);
      kslam_align_qc_release(ctx, &at);
      if (w != KSLAM_OK) fail(w, kslam_tail_last_error());
    }
    if (depth_set) {
      kslam_depth_row *rows = nullptr;
      uint64_t n_rows = 0;
      kslam_depth_stats ds;
      if (kslam_depth_take(ctx, dep_min, &rows, &n_rows, &ds) != KSLAM_OK) fail(KSLAM_ERR_STATE, kslam_last_error(ctx));
      const kslam_status w = kslam_depth_write(index, rows, n_rows, dep_fd);
      kslam_free_pinned(ctx, rows);
      if (w != KSLAM_OK) fail(w, kslam_tail_last_error());
    }
  });

  const double t_close = now_ms();
  const kslam_status closing = wind_down();
  st.seconds_closing = (now_ms() - t_close) * 1e-3;
  st.seconds = (now_ms() - t_begin) * 1e-3;
  if (stats) *stats = st;
  if (status != KSLAM_OK) return status;
  if (closing != KSLAM_OK) return closing;
  if (taxdb && tax_ids_out) {
    uint32_t *out = (uint32_t *)malloc(sizeof(uint32_t) * (all_ids.size() + 1));
    if (!out) return KSLAM_ERR_OOM;
    if (!all_ids.empty()) memcpy(out, all_ids.data(), sizeof(uint32_t) * all_ids.size());
    *tax_ids_out = out;
    if (n_tax_ids) *n_tax_ids = all_ids.size();
  }
  return KSLAM_OK;
}
