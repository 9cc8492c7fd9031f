// api_lanes.hip -- the C ABI, part 5: the operator pipelined.  Batches go round-robin to the worker lanes (KSLAM_LANES of them, two
// unless set; a host thread + a sibling context that shares the index each); columns, FASTQ fields or whole FASTQ texts in, results
// (+ pairs, details, SAM text) out through kslam_wait_batch / kslam_collect_batch.
#include "context.h"
#include <type_traits>

namespace kslam_api {

using AsyncJob = kslam_ctx::AsyncJob;

// the two FASTQ texts one behind the other on the device, 64 zero bytes behind them
static void upload_fastq_texts(kslam_ctx *c, const char *r1, uint64_t len1, const char *r2, uint64_t len2, hipStream_t s) {
  c->fq_text.ensure(len1 + len2 + 64);
  if (len1) HIPCHK(hipMemcpyAsync(c->fq_text.p, r1, len1, hipMemcpyHostToDevice, s));
  if (len2) HIPCHK(hipMemcpyAsync(c->fq_text.as<uint8_t>() + len1, r2, len2, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(c->fq_text.as<uint8_t>() + len1 + len2, 0, 64, s));
}

// the tail of both FASTQ forms: 64 zero bytes behind either column, then the host's part of a load.  arriving (the text form): the
// read offsets are still on their way to the host -- the stream is waited for and c->h_roff taken from them first
static void finish_fastq_columns(kslam_ctx *c, uint64_t total, hipStream_t s, const uint64_t *arriving = nullptr) {
  HIPCHK(hipMemsetAsync(c->r_bases.as<uint8_t>() + total, 0, 64, s));
  HIPCHK(hipMemsetAsync(c->r_qual.as<uint8_t>() + total, 0, 64, s));
  if (arriving) {
    HIPCHK(stream_wait(s));
    c->h_roff.assign(arriving, arriving + c->n_reads + 1);
  }
  finish_load_reads(c);
  c->have_qual = true;
}

kslam_status load_reads_from_fastq(kslam_ctx *c, uint64_t n_reads, const char *r1, uint64_t len1, const char *r2,
                                   uint64_t len2, const uint64_t *offsets, const uint64_t *bases_at,
                                   const uint64_t *quality_at) {
  return guarded(c, [&] {
    if (n_reads && (!offsets || !bases_at || !quality_at || (len1 && !r1) || (len2 && !r2)))
      throw StatusError{KSLAM_ERR_ARG, "null argument"};
    hipStream_t s = c->stream;
    c->have_reads = false;
    c->n_reads = n_reads;
    c->h_roff.assign(n_reads + 1, 0);
    const uint64_t o0 = n_reads ? offsets[0] : 0;
    for (uint64_t i = 0; i <= n_reads && n_reads; i++) c->h_roff[i] = offsets[i] - o0;
    const uint64_t total = c->h_roff[n_reads];
    upload_fastq_texts(c, r1, len1, r2, len2, s);
    c->fq_bases_at.ensure((n_reads + 1) * sizeof(uint64_t));
    c->fq_qual_at.ensure((n_reads + 1) * sizeof(uint64_t));
    c->r_off.ensure((n_reads + 1) * sizeof(uint64_t));
    if (n_reads) {
      HIPCHK(hipMemcpyAsync(c->fq_bases_at.p, bases_at, n_reads * sizeof(uint64_t), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(c->fq_qual_at.p, quality_at, n_reads * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(c->r_off.p, c->h_roff.data(), (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    c->r_bases.ensure(total + 64);
    c->r_qual.ensure(total + 64);
    // a field that reaches past the end of the texts would be a broken index: check on the host
    for (uint64_t i = 0; i < n_reads; i++) {
      const uint64_t len = c->h_roff[i + 1] - c->h_roff[i];
      if (bases_at[i] + len > len1 + len2 || quality_at[i] + len > len1 + len2)
        throw StatusError{KSLAM_ERR_ARG, "field " + std::to_string(i) + " lies outside the FASTQ texts"};
    }
    gather_fields(c->fq_text.as<uint8_t>(), c->fq_bases_at.as<uint64_t>(), c->fq_qual_at.as<uint64_t>(),
                  c->r_off.as<uint64_t>(), n_reads, c->r_bases.as<uint8_t>(), c->r_qual.as<uint8_t>(), s);
    finish_fastq_columns(c, total, s);
  });
}

// kslam_submit_batch_fastq_text: texts up, record index + columns on the device, the host's columns back
kslam_status load_reads_from_fastq_text(kslam_ctx *c, AsyncJob *job) {
  return guarded(c, [&] {
    const char *r1 = job->cat, *r2 = job->qcat;
    const uint64_t len1 = job->len1, len2 = job->len2;
    kslam_batch_result &res = job->res;
    if ((len1 && !r1) || (len2 && !r2)) throw StatusError{KSLAM_ERR_ARG, "null text"};
    hipStream_t s = c->stream;
    c->have_reads = false;
    upload_fastq_texts(c, r1, len1, r2, len2, s);
    FastqIndexResult ix;
    fastq_index_device(c->fq_text.as<uint8_t>(), len1, len2, len1 ? (const uint8_t *)r1 + len1 - 1 : nullptr,
                       len2 ? (const uint8_t *)r2 + len2 - 1 : nullptr, job->max_pairs, job->at_eof != 0, c->fqw, &ix, s, job->single);
    const uint64_t n = ix.n_reads;
    // the host's columns: offsets (= lengths), identifiers
    res.n_reads = n;
    res.reads_bases_off = (uint64_t *)pinned_get(c, (n + 2) * sizeof(uint64_t));
    res.reads_ids_off = (uint64_t *)pinned_get(c, (n + 2) * sizeof(uint64_t));
    res.reads_ids = (char *)pinned_get(c, ix.ids_total + 64);
    HIPCHK(hipMemcpyAsync(res.reads_bases_off, ix.d_bases_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(res.reads_ids_off, ix.d_ids_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (ix.ids_total) HIPCHK(hipMemcpyAsync(res.reads_ids, ix.d_ids, ix.ids_total, hipMemcpyDeviceToHost, s));
    res.consumed1 = ix.consumed[0];
    res.consumed2 = ix.consumed[1];
    // the device's columns
    c->n_reads = n;
    c->r_off.ensure((n + 1) * sizeof(uint64_t));
    HIPCHK(hipMemcpyAsync(c->r_off.p, ix.d_bases_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    c->r_bases.ensure(ix.bases_total + 64);
    c->r_qual.ensure(ix.bases_total + 64);
    gather_fields(c->fq_text.as<uint8_t>(), ix.d_bases_at, ix.d_quality_at, c->r_off.as<uint64_t>(), n,
                  c->r_bases.as<uint8_t>(), c->r_qual.as<uint8_t>(), s);
    finish_fastq_columns(c, ix.bases_total, s, res.reads_bases_off);
    res.reads_ids[ix.ids_total] = 0;
    c->d_ids = ix.d_ids;                 // in c->fqw: valid until this context indexes its next batch
    c->d_ids_off = ix.d_ids_off;
    c->have_ids = true;
    job->n_reads = n;
  });
}

namespace {

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One batch on its way through a lane, like Run in host/stream.cpp: the stages below in lane_main's order, one status that the
// first failure sets and that every later step looks at (run), the result written straight into the job's kslam_batch_result.
struct LaneBatch {
  kslam_ctx *const primary;         // the context the batch was submitted on: the settings, the switches, the reports' owners
  kslam_ctx *const c;               // the lane's own context: its stream, work buffers and page-locked pool
  AsyncJob *const job;
  kslam_batch_result &res;          // job->res
  kslam_status st = KSLAM_OK;
  SamStage sam;
  const uint32_t stages;            // of kslam_set_pairing; 0: the device pairing is off
  const bool has_qual;              // qualities came along, as columns or in FASTQ text: the batch gets row details
  bool details_wanted = false;      // ... and they are still to be made (compute / details_outside_token)
  bool text_wanted = false;         // rows, pairs and details are there for the SAM text (or no CIGAR is reported, so that none are needed)
  bool pseudo_left = false;         // the device left the pseudo-assembly to the host: the batch's scores and pairs are not final yet
  bool sam_planned = false;         // sam_stage_plan went through: the device writes this batch's text
  bool held = false, bam = false, bgzf = false;   // the form of the SAM records (sam_text)
  double t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;

  LaneBatch(kslam_ctx *primary_, kslam_ctx *c_, AsyncJob *job_)
      : primary(primary_), c(c_), job(job_), res(job_->res), stages(primary_->pairing.stages), has_qual(job_->qcat || job_->fastq) {}

  bool ok() const { return st == KSLAM_OK; }
  // every guarded step: it runs only while the batch's status is still OK.  A step that returns a status is a call of the C ABI
  // (which has left its message in c->err); one that returns nothing reports by throwing (guarded)
  template <typename F> void run(F &&step) {
    if (!ok()) return;
    if constexpr (std::is_void_v<decltype(step())>) st = guarded(c, step);
    else st = step();
  }

  void load() {
    t0 = now_ms();
    if (job->fastq_text)
      st = load_reads_from_fastq_text(c, job);
    else if (job->fastq)
      st = load_reads_from_fastq(c, job->n_reads, job->cat, job->len1, job->qcat, job->len2, job->off_ptr, job->bases_at, job->quality_at);
    else
      st = kslam_load_reads(c, job->n_reads, job->cat, job->borrowed ? job->off_ptr : job->off.data());
    if (job->qcat && !job->fastq)
      run([&] { return kslam_load_qualities(c, job->borrowed && job->n_reads ? job->qcat + job->off_ptr[0] : job->qcat); });
    if (job->qcat && !job->borrowed) pinned_put(c, job->qcat);
    t1 = now_ms();
    if (!job->borrowed) pinned_put(c, job->cat);
    job->cat = nullptr;
  }

  // the per-row walk, once per batch: inside the token (compute) or behind it (details_outside_token)
  void row_details() {
    if (!details_wanted) return;
    st = stages ? kslam_row_details_of_pairs(c, nullptr) : kslam_row_details(c, nullptr);
    details_wanted = false;
    if (!ok()) text_wanted = false;
  }

  void compute(std::mutex &as_compute) {
    if (!ok()) return;
    // one lane computes at a time: the kernels of a batch fill the chip, so two batches computing at
    // once only time-slice -- and, worse, fall into step, both lanes copying while the GPU idles and
    // both computing afterwards (measured: 32.6 ms per batch against 27.3 resident).  With the token
    // the lanes run in anti-phase: one computes while the other downloads its last result and
    // uploads its next batch.
    std::lock_guard<std::mutex> token(as_compute);
    t2 = now_ms();
    PairingHook hook{primary->pairing.paired, primary->pairing.thr, primary->pairing.fraction, stages};
    const bool eager = primary->tune.eager_cigar;   // A/B: every CIGAR, pairing afterwards
    const bool use_hook = stages && has_qual && !eager;
    run([&] { align_resident(c, false, nullptr, use_hook ? &hook : nullptr); });
    if (stages && ok() && hook.ran) fill_pair_stats(c->pres, &res.pair_stats);
    else if (stages) run([&] { return kslam_pair_screen(c, primary->pairing.paired, primary->pairing.thr, primary->pairing.fraction, stages, &res.pair_stats); });
    pseudo_left = (stages & 4u) && !(res.pair_stats.stages_done & 4u);
    details_wanted = ok() && has_qual;
    text_wanted = ok() && (has_qual || !c->prm.report_cigar);
    if (primary->tune.details_in_token) row_details();   // default; KSLAM_DETAILS_IN_TOKEN=0 moves it out (measured: 40.5 against 43.1 M reads/s)
  }

  // (KSLAM_DETAILS_IN_TOKEN=0, A/B: the per-row walk outside the token as well -- slower: its 150-byte windows of the index
  // compete with the other lane's staging for L2)
  void details_outside_token() { row_details(); }

  // The SAM records / per-read lines on the device (kslam_set_sam_text): the reference's per-pair sort (in place: the pairs
  // go back to the host in that order), the rows to report, the log-probabilities the host evaluates with its libm, then the
  // text.  OUTSIDE the compute token: these kernels are bound by the latency of dependent gathers (samtext.hip), not by
  // ALU work or bandwidth, so they run next to the other lane's alignment kernels instead of in front of them.
  // Not for a batch whose pseudo-assembly the device left to the host: its scores are not final yet.
  void sam_text() {
    const auto &T = primary->samtext;
    if (!(text_wanted && (T.sam || T.per_read) && stages && c->have_ids && !pseudo_left)) return;
    run([&] { sam_stage_plan(c, primary, primary->pairing.paired, T.num_alignments, T.sam_xa, T.sam, sam); });
    sam_planned = ok();
    if (!sam_planned) return;
    sam_stage_mapq(sam);   // pow / log10 / ceil with the host's libm
    // (kslam_set_sam_bgzf) compressed before the copy; (kslam_set_sam_bam) BAM records, which are always compressed
    // (kslam_set_bam_sort) BAM records that stay on the device: neither compressed nor fetched, held for the sort at the end
    held = T.sam && primary->bsort_on.load(std::memory_order_acquire);
    bam = T.sam && (T.bam || held);
    bgzf = T.sam && (T.bgzf || bam) && !held;
    sam.bam = bam;
    sam.seq = T.sam && T.seq;             // (kslam_set_sam_seq) SEQ and QUAL on the primary rows
    sam.unmapped = T.sam && T.unmapped;   // (kslam_set_sam_unmapped) rows for the reads without alignment
    run([&] { sam_write(); });
    run([&] { sam_stage_fetch(c, sam, T.sam, T.per_read, &res.sam_text, &res.sam_text_len, &res.per_read_text, &res.per_read_len, &res.tax_ids, nullptr); });
    if (!ok()) return;
    res.text_flags = (T.sam ? (KSLAM_TEXT_PAIRS_SORTED | KSLAM_TEXT_SAM) : 0u) | (T.per_read ? KSLAM_TEXT_PER_READ : 0u) | (bgzf ? KSLAM_TEXT_SAM_BGZF : 0u) |
                     (bam ? KSLAM_TEXT_SAM_BAM : 0u) | (held ? KSLAM_TEXT_SAM_HELD : 0u) | (sam.seq ? KSLAM_TEXT_SAM_SEQ : 0u) |
                     (sam.unmapped ? KSLAM_TEXT_SAM_UNMAPPED : 0u);
    if (sam.unmapped) unmapped_note(primary, c);
    // (kslam_set_kreport) this lane has just made the batch's taxonomy ids: they go into the owner's per-taxon counters from
    // where they lie, on this lane's stream and outside the compute token like the marks below.  A batch without the
    // per-read stage gets its ids on the host, which hands them to kslam_kreport_add.
    if (T.per_read && primary->kr.on.load(std::memory_order_acquire)) run([&] { kreport_count_resident(primary, c, sam.n_groups); });
  }

  // the text's kernels, and what becomes of the records where they lie (throws)
  void sam_write() {
    sam_stage_kernels(c, primary, sam, primary->samtext.sam, primary->samtext.per_read);
    if (held) {
      // into the owner's store on this lane's stream, outside the compute token like the reports below; the unmapped rows lie
      // behind the mapped ones (sam_stage_kernels), c->sumw.bytes of them
      const uint64_t behind = sam.unmapped ? c->sumw.bytes : 0;
      const uint64_t n_records = primary->pairing.paired ? c->n_reads / 2 : c->n_reads;
      bamsort_append_resident(primary, c, job->ticket, sam.n_groups, sam.text_bytes - behind, sam.unmapped ? n_records : 0, sam.text_bytes);
      sam.text_bytes = 0;   // nothing travels
    } else if (bgzf) {
      bgzf_compress_device(c->samw.text.as<char>(), sam.text_bytes, primary->samtext.deflate, c->bgzfw, c->bgzf_out, &sam.text_bytes, c->stream);
      sam.d_sam = c->bgzf_out.p;
    }
  }

  // (kslam_set_taxon_reads) the records of the read pairs whose taxonomy id is in the chosen set, cut out of the text this lane
  // uploaded: on this lane's stream and outside the compute token, like the split below.  The flag pass reads samw.tax_ids
  // and the groups k_lca saw (sam.d_groups); both are device buffers of this lane that live until its next batch
  // (sam_stage_free hands back only the page-locked host blocks), but the call stands in front of it all the same.  A batch
  // whose ids this lane did not make -- pseudo-assembly left to the host, the host's text, no per-read stage -- is left to
  // the host twin.
  void taxon_reads() {
    if (!primary->tr.on.load(std::memory_order_acquire)) return;
    job->tr_on = true;
    job->tr_supported = job->fastq_text && stages != 0;
    if (!ok() || !job->tr_supported) return;
    if (!(sam_planned && primary->samtext.per_read)) job->tr.flags = KSLAM_READS_OUT_LEFT_TO_HOST;
    else run([&] {
      taxreads_resident(primary, c, job->single, sam.d_groups, c->samw.tax_ids.as<uint32_t>(), sam.n_groups, primary->reads_out.bgzf,
                        primary->samtext.deflate, &job->tr);
    });
  }

  // (kslam_set_read_qc) the batch's reads into the owner's per-cycle tables, from the bases and quality columns this lane cut
  // out of the text it uploaded: a streaming pass on this lane's stream, outside the compute token like the split below, and
  // it does not wait.  It asks for no alignment result, so every batch of the text route is counted, whatever became of it.
  void read_qc() {
    if (job->fastq_text && primary->rq.on.load(std::memory_order_acquire)) run([&] { readqc_count_resident(primary, c, job->single); });
  }

  // (kslam_set_reads_out) the records split by outcome, cut out of the text this lane uploaded.  Outside the compute token as
  // well: a streaming copy next to the other lane's alignment kernels.  A batch whose pseudo-assembly is left to the host
  // has no final read pairs yet: the host twin splits it.
  void reads_out() {
    const uint32_t which = primary->reads_out.which;
    if (!which) return;
    job->ro_on = true;
    job->ro_supported = job->fastq_text && stages != 0;
    if (!ok() || !job->ro_supported) return;
    if (pseudo_left) job->ro.flags = KSLAM_READS_OUT_LEFT_TO_HOST;
    else run([&] {
      split_resident(c, job->single, c->pres.d_groups, c->pres.n_read_pairs, which, primary->reads_out.bgzf, primary->samtext.deflate, &job->ro);
    });
  }

  // The reports fed by the batch's final alignment pairs: a report that is switched on sees the batch when everything before
  // went well and this lane holds the final pairs.  (The report looks at its switch again under its own lock.)
  template <typename F> void feed(const std::atomic<bool> &on, F &&pass) {
    if (on.load(std::memory_order_acquire) && stages && !pseudo_left && c->have_pairs) run(pass);
  }
  void reports() {
    // (kslam_set_coverage) the batch's final alignment pairs into the owner's coverage table: bit and counter atomics on this
    // lane's stream, outside the compute token like the split above.  A batch whose pseudo-assembly is left to the host goes
    // in through kslam_coverage_add after the host stage.
    feed(primary->cov.on, [&] { coverage_mark_resident(primary, c); });
    // (kslam_set_variants) the batch's mismatch events and covered intervals into the owner's state, on this lane's stream and
    // outside the compute token as well; the batches left to the host go in through kslam_variants_add after the host stage
    feed(primary->var.on, [&] { variants_emit_resident(primary, c); });
    // (kslam_set_indels) the batch's normalised deletions and insertions and its covered intervals into the owner's state, likewise
    feed(primary->ind.on, [&] { indels_emit_resident(primary, c); });
    // (kslam_set_consensus) the batch's intervals, events and insertions into the owner's state, likewise
    feed(primary->cns.on, [&] { consensus_emit_resident(primary, c); });
    // (kslam_set_depth) the batch's M runs as interval boundaries into the owner's state, likewise
    feed(primary->dep.on, [&] { depth_emit_resident(primary, c); });
    // (kslam_set_genes) the batch's final alignment pairs into the owner's per-gene counters, likewise
    feed(primary->gen.on, [&] { genes_count_resident(primary, c); });
    // (kslam_set_align_qc) the batch's contributing records and live pairs into the owner's per-cycle tables, likewise; the batches
    // left to the host go in through kslam_align_qc_add after the host stage
    feed(primary->aq.on, [&] { alignqc_count_resident(primary, c, job->single); });
  }

  void download() {
    t3 = now_ms();
    // with the SAM records written on the device the host has no use for the rows, the CIGAR pool, the per-row details and
    // the MD text (0.7 GB per batch of configs[1]): they stay where they are, only their counts travel
    const bool text_sam = (res.text_flags & KSLAM_TEXT_SAM) != 0;
    if (!text_sam) run([&] { return kslam_take_results(c, &res.overlaps, &res.n_overlaps, &res.cigar_pool, &res.n_cigar); });
    else if (ok()) { res.n_overlaps = c->n_res; res.n_cigar = c->n_cig; }
    t4 = now_ms();
    if (has_qual && !text_sam) run([&] { return kslam_take_row_details(c, &res.details, &res.md_pool, &res.n_md); });
    t5 = now_ms();
    if (stages) run([&] { return kslam_take_pairs(c, &res.read_pairs, &res.n_read_pairs, &res.pairs, &res.n_pairs); });
  }

  // the collector may take the job away as soon as `done` is set: nothing of it is touched after that
  void publish(const kslam_ctx::AsyncLane *lane) {
    if (primary->tune.debug) {
      fprintf(stderr, "[kslam]   align phases: extract %.2f sort %.2f join %.2f sw %.2f cigar %.2f total %.2f ms\n", c->tm.ms_extract,
              c->tm.ms_sort, c->tm.ms_join, c->tm.ms_sw, c->tm.ms_cigar, c->tm.ms_total);
      fprintf(stderr, "[kslam] t=%.1f lane %p ticket %llu: upload %.2f, token wait %.2f, align %.2f, download %.2f (rows %.2f, details %.2f, pairs %.2f) ms\n",
              fmod(t0, 100000.0), (const void *)lane, (unsigned long long)job->ticket, t1 - t0, t2 - t1, t3 - t2, now_ms() - t3, t4 - t3, t5 - t4, now_ms() - t5);
    }
    {
      std::lock_guard<std::mutex> lk(primary->as_mu);
      job->st = st;
      if (!ok()) job->err = c->err;
      job->done = true;
    }
    primary->as_cv.notify_all();
  }
};

}  // namespace

void lane_main(kslam_ctx *primary, kslam_ctx::AsyncLane *lane) {
  kslam_host::name_thread("kslam-lane");
  wait_mode().yield = primary->tune.lane_waits_yield;   // common.h: stream_wait
  if (wait_mode().yield) (void)prctl(PR_SET_TIMERSLACK, 5000UL, 0, 0, 0);   // its 20 us sleeps mean 25, not 70
  for (;;) {
    AsyncJob *job = nullptr;
    {
      std::unique_lock<std::mutex> lk(primary->as_mu);
      primary->as_cv.wait(lk, [&] { return primary->as_stop || !lane->q.empty(); });
      if (lane->q.empty()) return;   // stop requested and nothing left
      job = lane->q.front();
      lane->q.pop_front();
    }
    LaneBatch b(primary, lane->c, job);
    b.load();
    b.compute(primary->as_compute);
    b.details_outside_token();
    b.sam_text();
    b.taxon_reads();
    sam_stage_free(lane->c, b.sam);   // on every path, and here: the blocks it hands back are the ones the stages below take
    b.read_qc();
    b.reads_out();
    b.reports();
    b.download();
    b.publish(lane);
  }
}

void ensure_lanes(kslam_ctx *c) {
  if (!c->lanes.empty()) return;
  const int n_lanes = c->tune.lanes;
  // built aside and published only when every lane has its context AND its thread: a failure half way
  // (page-locked or device memory) must not leave lanes without workers behind, to which the next
  // submit would queue a job nobody ever runs
  std::vector<kslam_ctx::AsyncLane *> fresh;
  auto undo = [&] {
    for (auto *l : fresh) { kslam_destroy(l->c); delete l; }
    fresh.clear();
  };
  for (int k = 0; k < n_lanes; k++) {
    kslam_ctx *lc = nullptr;
    const kslam_status s1 = kslam_create(&c->prm, &lc);
    if (s1 != KSLAM_OK) {
      const std::string msg = lc ? lc->err : "lane context";
      kslam_destroy(lc);
      undo();
      throw StatusError{s1, msg};
    }
    lc->tune = c->tune;
    lc->pw.pseudo_cap = (uint32_t)c->tune.pseudo_cap;
    share_index(lc, c);
    auto *l = new kslam_ctx::AsyncLane();
    l->c = lc;
    fresh.push_back(l);
  }
  size_t started = 0;
  try {
    for (auto *l : fresh) { l->th = std::thread(lane_main, c, l); started++; }
  } catch (const std::exception &e) {
    { std::lock_guard<std::mutex> lk(c->as_mu); c->as_stop = true; }
    c->as_cv.notify_all();
    for (size_t k = 0; k < started; k++) fresh[k]->th.join();
    c->as_stop = false;
    undo();
    throw StatusError{KSLAM_ERR_OOM, std::string("could not start a lane thread: ") + e.what()};
  }
  c->lanes = std::move(fresh);
}

void stop_lanes(kslam_ctx *c) {
  { std::lock_guard<std::mutex> lk(c->as_mu); c->as_stop = true; }
  c->as_cv.notify_all();
  for (auto *l : c->lanes) {
    if (l->th.joinable()) l->th.join();
    kslam_destroy(l->c);
    delete l;
  }
  c->lanes.clear();
  c->jobs.clear();       // results nobody waited for
  c->ro_ready.clear();   // (their blocks went with the lanes' page-locked pools)
  c->tr_ready.clear();
  c->as_stop = false;
}

// The way into the queue, first half (inside guarded): what every form checks before it has a job to fill in
static std::unique_ptr<AsyncJob> make_job(kslam_ctx *c, bool null_argument, const char *what) {
  if (null_argument) throw StatusError{KSLAM_ERR_ARG, what};
  c->need_index();
  ensure_lanes(c);
  return std::make_unique<AsyncJob>();
}

// ... and second half: the ticket, the job into c->jobs (its owner until it is collected) and into the queue of the ticket's lane,
// the lanes woken.  taken: the ticket kslam_submit_batch took beforehand; the other forms take theirs here, in one step with the
// publication, so that a lane's queue is in ticket order
static void enqueue(kslam_ctx *c, std::unique_ptr<AsyncJob> job, uint64_t *ticket, const uint64_t *taken = nullptr) {
  {
    std::lock_guard<std::mutex> lk(c->as_mu);
    const uint64_t tk = taken ? *taken : c->next_ticket++;
    job->ticket = tk;
    c->lanes[tk % c->lanes.size()]->q.push_back(job.get());
    c->jobs[tk] = std::move(job);
    *ticket = tk;
  }
  c->as_cv.notify_all();
}

// kslam_submit_batch: the reads leave the caller's memory (parallel gather into page-locked buffers of the lane that will run the
// batch); a failure hands the buffers back to that lane's pool
static void gather_reads(kslam_ctx *lane_c, AsyncJob *job, const char *const *bases, const char *const *quality, const uint32_t *lens) {
  const uint64_t n_reads = job->n_reads;
  try {
    job->cat = (char *)pinned_get(lane_c, job->off[n_reads] + 64);
    if (quality) job->qcat = (char *)pinned_get(lane_c, job->off[n_reads] + 64);
    unsigned nt = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (n_reads < 100000) nt = 1;
    std::vector<std::thread> th;
    char *cat = job->cat, *qcat = job->qcat;
    const std::vector<uint64_t> &off = job->off;
    for (unsigned t = 0; t < nt; t++) {
      const uint64_t lo = n_reads * t / nt, hi = n_reads * (t + 1) / nt;
      auto work = [=, &off] {
        for (uint64_t i = lo; i < hi; i++) memcpy(cat + off[i], bases[i], lens[i]);
        if (qcat) for (uint64_t i = lo; i < hi; i++) memcpy(qcat + off[i], quality[i], lens[i]);
      };
      if (nt == 1) work(); else th.emplace_back(work);
    }
    for (auto &x : th) x.join();
  } catch (...) {
    if (job->cat) pinned_put(lane_c, job->cat);
    if (job->qcat) pinned_put(lane_c, job->qcat);
    throw;
  }
}

// (kslam_set_reads_out / kslam_set_taxon_reads) a collected batch's streams wait for their own collect call, the last 16 batches'
static void keep_reads_out(kslam_ctx *c, std::map<uint64_t, kslam_ctx::ReadsOutEntry> &ready, uint64_t ticket, bool supported,
                           const kslam_reads_out &out) {
  std::lock_guard<std::mutex> lk(c->as_mu);
  while (ready.size() >= 16) {
    free_reads_out(c, &ready.begin()->second.out);
    ready.erase(ready.begin());
  }
  ready[ticket] = kslam_ctx::ReadsOutEntry{supported, out};
}

}  // namespace kslam_api

extern "C" {

// ---- the operator, pipelined: batches go round-robin to the worker lanes (a host thread + a sibling
// context with its own stream and work buffers each), so the upload of batch k+1 and the download of
// batch k-1 run under the kernels of batch k, and one lane's host read-backs are covered by the other
// lanes' kernels ----
kslam_status kslam_align_batch_async(kslam_ctx *c, uint64_t n_reads, const char *const *bases, const uint32_t *lens,
                                     uint64_t *ticket) {
  return kslam_submit_batch(c, n_reads, bases, nullptr, lens, ticket);
}

kslam_status kslam_submit_batch(kslam_ctx *c, uint64_t n_reads, const char *const *bases, const char *const *quality,
                                const uint32_t *lens, uint64_t *ticket) {
  if (!c || !ticket) return KSLAM_ERR_ARG;
  return guarded(c, [&] {
    auto job = make_job(c, n_reads && (!bases || !lens), "null bases/lens");
    job->n_reads = n_reads;
    job->off.assign(n_reads + 1, 0);
    for (uint64_t i = 0; i < n_reads; i++) job->off[i + 1] = job->off[i] + lens[i];
    // the caller may reuse its buffers as soon as this call returns: the reads are gathered now, into the pool of the lane the
    // ticket names -- so the ticket comes first
    uint64_t tk;
    { std::lock_guard<std::mutex> lk(c->as_mu); tk = c->next_ticket++; }
    gather_reads(c->lanes[tk % c->lanes.size()]->c, job.get(), bases, quality, lens);
    enqueue(c, std::move(job), ticket, &tk);
  });
}

kslam_status kslam_submit_batch_columns(kslam_ctx *c, uint64_t n_reads, const char *bases, const char *quality,
                                        const uint64_t *offsets, uint64_t *ticket) {
  if (!c || !ticket) return KSLAM_ERR_ARG;
  return guarded(c, [&] {
    auto job = make_job(c, n_reads && (!bases || !offsets), "null bases/offsets");
    job->n_reads = n_reads;
    job->borrowed = true;
    job->cat = const_cast<char *>(bases);
    job->qcat = const_cast<char *>(quality);
    job->off_ptr = offsets;
    enqueue(c, std::move(job), ticket);
  });
}

kslam_status kslam_submit_batch_fastq(kslam_ctx *c, const char *r1, uint64_t len1, const char *r2, uint64_t len2,
                                      uint64_t n_reads, const uint64_t *offsets, const uint64_t *bases_at,
                                      const uint64_t *quality_at, uint64_t *ticket) {
  if (!c || !ticket) return KSLAM_ERR_ARG;
  return guarded(c, [&] {
    auto job = make_job(c, n_reads && (!offsets || !bases_at || !quality_at), "null layout");
    job->n_reads = n_reads;
    job->borrowed = true;
    job->fastq = true;
    job->cat = const_cast<char *>(r1);
    job->qcat = const_cast<char *>(r2);
    job->len1 = len1; job->len2 = len2;
    job->off_ptr = offsets;
    job->bases_at = bases_at; job->quality_at = quality_at;
    enqueue(c, std::move(job), ticket);
  });
}

kslam_status kslam_submit_batch_fastq_text(kslam_ctx *c, const char *r1, uint64_t len1, const char *r2, uint64_t len2,
                                           uint64_t max_pairs, int at_eof, uint64_t *ticket) {
  if (!c || !ticket) return KSLAM_ERR_ARG;
  return guarded(c, [&] {
    auto job = make_job(c, (len1 && !r1) || (len2 && !r2), "null text");
    job->borrowed = true;
    job->fastq = true;
    job->fastq_text = true;
    job->cat = const_cast<char *>(r1);
    job->qcat = const_cast<char *>(r2);
    job->len1 = len1; job->len2 = len2;
    job->max_pairs = max_pairs; job->at_eof = at_eof;
    job->single = r2 == nullptr && len2 == 0;
    enqueue(c, std::move(job), ticket);
  });
}

// the one list of a batch's page-locked blocks
void kslam_release_batch(kslam_ctx *c, kslam_batch_result *r) {
  if (!c || !r) return;
  kslam_free_batch(c, r->overlaps, r->cigar_pool);
  kslam_free_pinned(c, r->details);
  kslam_free_pinned(c, r->md_pool);
  kslam_free_pinned(c, r->read_pairs);
  kslam_free_pinned(c, r->pairs);
  kslam_free_pinned(c, r->reads_bases_off);
  kslam_free_pinned(c, r->reads_ids_off);
  kslam_free_pinned(c, r->reads_ids);
  kslam_free_pinned(c, r->sam_text);
  kslam_free_pinned(c, r->per_read_text);
  kslam_free_pinned(c, r->tax_ids);
  memset(r, 0, sizeof *r);
}

kslam_status kslam_collect_batch(kslam_ctx *c, uint64_t ticket, kslam_batch_result *res) {
  if (!c || !res) return KSLAM_ERR_ARG;
  memset(res, 0, sizeof *res);
  std::unique_ptr<AsyncJob> job;
  {
    std::unique_lock<std::mutex> lk(c->as_mu);
    auto it = c->jobs.find(ticket);
    if (it == c->jobs.end()) { c->err = "no such ticket (already waited for?)"; return KSLAM_ERR_ARG; }
    c->as_cv.wait(lk, [&] { return it->second->done; });
    job = std::move(it->second);
    c->jobs.erase(it);
  }
  if (job->st != KSLAM_OK) {
    c->err = job->err;
    kslam_release_batch(c, &job->res);
    free_reads_out(c, &job->ro);
    free_reads_out(c, &job->tr);
    return job->st;
  }
  *res = job->res;
  if (job->ro_on) keep_reads_out(c, c->ro_ready, ticket, job->ro_supported, job->ro);   // for kslam_collect_reads_out
  if (job->tr_on) keep_reads_out(c, c->tr_ready, ticket, job->tr_supported, job->tr);   // for kslam_collect_taxon_reads
  return KSLAM_OK;
}

kslam_status kslam_wait_batch(kslam_ctx *c, uint64_t ticket, kslam_overlap **out, uint64_t *n_out, uint32_t **cigar_pool,
                              uint64_t *n_cigar) {
  if (!c || !out || !n_out || !cigar_pool || !n_cigar) return KSLAM_ERR_ARG;
  *out = nullptr; *cigar_pool = nullptr; *n_out = 0; *n_cigar = 0;
  kslam_batch_result r;
  const kslam_status st = kslam_collect_batch(c, ticket, &r);
  if (st != KSLAM_OK) return st;
  *out = r.overlaps; *n_out = r.n_overlaps; *cigar_pool = r.cigar_pool; *n_cigar = r.n_cigar;
  r.overlaps = nullptr; r.cigar_pool = nullptr;   // the caller's now (kslam_free_batch); everything else goes back
  kslam_release_batch(c, &r);
  return KSLAM_OK;
}

}  // extern "C"
