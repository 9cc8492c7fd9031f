// api_coverage.hip -- the C ABI, part 8: the per-entry coverage table (include/kslam_coverage.h; kernels: coverage.hip).  The
// state lives on the context the switch was set on; its lanes call coverage_mark_resident on the batch they have just finished,
// kslam_coverage_add takes a batch's arrays from the host, kslam_coverage_take counts the bitmap and hands the rows over.
#include "context.h"

namespace kslam_api {

namespace {

CoverageTable table_of(const kslam_ctx *owner, const GenomeIndex &ix) {
  const kslam_ctx::Coverage &v = owner->cov;
  return CoverageTable{v.bitmap.as<unsigned long long>(), v.rows.as<unsigned long long>(), v.skipped.as<unsigned long long>(),
                       v.word_off.as<uint64_t>(), ix.g_off.as<uint64_t>(), v.n_entries, v.n_words};
}

const char *const REPORT_IS = "the coverage table is";
const char *const SWITCHED_OFF = "coverage is switched off: call kslam_set_coverage first";

void zero_state(kslam_ctx *c) {
  kslam_ctx::Coverage &v = c->cov;
  HIPCHK(hipMemsetAsync(v.bitmap.p, 0, (v.n_words + 1) * sizeof(uint64_t), c->stream));
  HIPCHK(hipMemsetAsync(v.rows.p, 0, (v.n_entries + 1) * 4 * sizeof(uint64_t), c->stream));
  HIPCHK(hipMemsetAsync(v.skipped.p, 0, sizeof(uint64_t), c->stream));
  HIPCHK(stream_wait(c->stream));
}

}  // namespace

void coverage_release(kslam_ctx *c) {
  kslam_ctx::Coverage &v = c->cov;
  std::lock_guard<std::mutex> lk(v.mu);
  v.on.store(false, std::memory_order_release);
  for (DevBuf *b : {&v.bitmap, &v.rows, &v.skipped, &v.word_off}) b->release();
  v.up.release_all();
  v.n_entries = v.n_words = 0;
}

void coverage_mark_resident(kslam_ctx *owner, kslam_ctx *lane) {
  const GenomeIndex &ix = lane->need_index();
  kslam_ctx::Coverage &v = owner->cov;
  CoverageTable table;
  {   // the pass runs without the lock (the work buffers are the lane's own, the marks are atomics): the lanes do not wait for each
      // other; the switch is set between batches and waits for the lanes' streams before it frees anything
    std::lock_guard<std::mutex> lk(v.mu);
    if (!v.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the coverage table was switched off while a batch was in flight"};
    if (ix.n_entries != v.n_entries) throw StatusError{KSLAM_ERR_STATE, "the coverage table was laid out for another index"};
    table = table_of(owner, ix);
  }
  const VariantInputs in = resident_inputs(lane, ix, false);
  coverage_mark_device(in.ov, in.n_ov, in.groups, in.n_groups, in.pairs, in.n_pairs, table, lane->covw, lane->stream);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_coverage(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (refused_in_multi(c, REPORT_IS)) throw StatusError{KSLAM_ERR_UNSUPPORTED, c->err};
    if (!on) {
      if (c->cov.on.load(std::memory_order_acquire)) wait_for_lanes(c);
      coverage_release(c);
      return;
    }
    const GenomeIndex &ix = c->need_index();
    if (!c->pairing.stages) throw StatusError{KSLAM_ERR_STATE, "kslam_set_coverage needs the device pairing: call kslam_set_pairing first"};
    kslam_ctx::Coverage &v = c->cov;
    std::lock_guard<std::mutex> lk(v.mu);
    if (v.on.load(std::memory_order_acquire)) return;
    // every entry starts on a word of its own: the word offsets from the index's entry offsets
    std::vector<uint64_t> woff(ix.n_entries + 1, 0);
    for (uint64_t e = 0; e < ix.n_entries; e++) woff[e + 1] = woff[e] + (ix.h_goff[e + 1] - ix.h_goff[e] + 63) / 64;
    v.n_entries = ix.n_entries;
    v.n_words = woff[ix.n_entries];
    try {
      v.bitmap.ensure((v.n_words + 1) * sizeof(uint64_t));
      v.rows.ensure((v.n_entries + 1) * 4 * sizeof(uint64_t));
      v.skipped.ensure(sizeof(uint64_t));
      v.word_off.ensure((v.n_entries + 1) * sizeof(uint64_t));
      HIPCHK(hipMemcpyAsync(v.word_off.p, woff.data(), (v.n_entries + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
      zero_state(c);   // (waits: woff may go)
      if (!v.ev_count[0])
        for (auto &e : v.ev_count) HIPCHK(hipEventCreate(&e));
    } catch (...) {
      for (DevBuf *b : {&v.bitmap, &v.rows, &v.skipped, &v.word_off}) b->release();
      throw;
    }
    v.count_ms = 0;
    v.on.store(true, std::memory_order_release);
  });
}

kslam_status kslam_get_coverage(kslam_ctx *c, int *on) { return get_switch(c, &kslam_ctx::cov, on); }

kslam_status kslam_coverage_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->cov.mu);
    need_on(c->cov.on, SWITCHED_OFF);
    wait_for_lanes(c);
    zero_state(c);
  });
}

kslam_status kslam_coverage_add(kslam_ctx *c, const kslam_overlap *overlaps, uint64_t n_overlaps, const kslam_read_pair *read_pairs,
                                uint64_t n_read_pairs, const kslam_paired_overlap *pairs, uint64_t n_pairs) {
  return guarded(c, [&] {
    if ((n_overlaps && !overlaps) || (n_read_pairs && !read_pairs) || (n_pairs && !pairs)) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::Coverage &v = c->cov;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->cov.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    // nothing is launched for arrays that do not hold together
    const kslam_batch::Arrays batch{overlaps, n_overlaps, 0, nullptr, 0, read_pairs, n_read_pairs, pairs, n_pairs};
    const std::string fault = kslam_batch::check(batch, kslam_batch::Level::pairs);
    if (!fault.empty()) throw StatusError{KSLAM_ERR_ARG, fault};
    hipStream_t s = c->stream;
    const VariantInputs in = v.up.upload(batch, kslam_batch::Level::pairs, nullptr, BatchUpload::no_columns, nullptr, nullptr, &ix, s);
    coverage_mark_device(in.ov, in.n_ov, in.groups, in.n_groups, in.pairs, in.n_pairs, table_of(c, ix), c->covw, s);
  });
}

kslam_status kslam_coverage_take(kslam_ctx *c, kslam_entry_coverage **rows, uint64_t *n_entries, uint64_t *n_skipped) {
  return take_rows(c, rows, n_entries, n_skipped, [&](kslam_entry_coverage *&h) {
    kslam_ctx::Coverage &v = c->cov;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->cov.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    wait_for_lanes(c);
    hipStream_t s = c->stream;
    coverage_count_device(table_of(c, ix), v.ev_count, s);
    h = (kslam_entry_coverage *)pinned_get(c, (v.n_entries + 1) * sizeof(kslam_entry_coverage));
    if (v.n_entries) HIPCHK(hipMemcpyAsync(h, v.rows.p, v.n_entries * sizeof(kslam_entry_coverage), hipMemcpyDeviceToHost, s));
    read_back(n_skipped, v.skipped.p, sizeof(uint64_t), s);   // (waits for the stream)
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, v.ev_count[0], v.ev_count[1]));
    v.count_ms = ms;
    *n_entries = v.n_entries;
  });
}

kslam_status kslam_coverage_bitmap(kslam_ctx *c, uint64_t entry, uint64_t *words, uint64_t n_words) {
  return guarded(c, [&] {
    kslam_ctx::Coverage &v = c->cov;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->cov.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    if (entry >= v.n_entries) throw StatusError{KSLAM_ERR_ARG, "no such entry"};
    const uint64_t len = ix.h_goff[entry + 1] - ix.h_goff[entry], want = (len + 63) / 64;
    if (n_words != want || (want && !words)) throw StatusError{KSLAM_ERR_ARG, "entry " + std::to_string(entry) + " has " + std::to_string(want) + " words"};
    wait_for_lanes(c);
    if (!want) return;
    uint64_t first = 0;   // the entry's first word: the sum of the words before it
    for (uint64_t e = 0; e < entry; e++) first += (ix.h_goff[e + 1] - ix.h_goff[e] + 63) / 64;
    HIPCHK(hipMemcpyAsync(words, v.bitmap.as<uint64_t>() + first, want * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(stream_wait(c->stream));
  });
}

kslam_status kslam_coverage_kernel_ms(kslam_ctx *c, double *mark_ms, double *count_ms) {
  if (!c || !mark_ms || !count_ms) return KSLAM_ERR_ARG;
  *mark_ms = c->covw.ms;
  *count_ms = c->cov.count_ms;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_coverage(kslam_ctx *c, int fd) {
  if (!c) return KSLAM_ERR_ARG;
  if (refused_in_multi(c, REPORT_IS)) return KSLAM_ERR_UNSUPPORTED;
  c->cov.stream_fd = fd >= 0 ? fd : -1;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_coverage(kslam_ctx *c, int *fd) {
  if (!c || !fd) return KSLAM_ERR_ARG;
  *fd = c->cov.stream_fd;
  return KSLAM_OK;
}

}  // extern "C"
