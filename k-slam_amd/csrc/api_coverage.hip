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

void need_on(const kslam_ctx *c) {
  if (!c->cov.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "coverage is switched off: call kslam_set_coverage first"};
}

void zero_state(kslam_ctx *c) {
  kslam_ctx::Coverage &v = c->cov;
  HIPCHK(hipMemsetAsync(v.bitmap.p, 0, (v.n_words + 1) * sizeof(uint64_t), c->stream));
  HIPCHK(hipMemsetAsync(v.rows.p, 0, (v.n_entries + 1) * 4 * sizeof(uint64_t), c->stream));
  HIPCHK(hipMemsetAsync(v.skipped.p, 0, sizeof(uint64_t), c->stream));
  HIPCHK(stream_wait(c->stream));
}

// every lane's marks are in memory before anybody reads or zeroes the table
void wait_for_lanes(kslam_ctx *c) {
  for (auto *l : c->lanes) HIPCHK(hipStreamSynchronize(l->c->stream));
}

}  // namespace

void coverage_release(kslam_ctx *c) {
  kslam_ctx::Coverage &v = c->cov;
  std::lock_guard<std::mutex> lk(v.mu);
  v.on.store(false, std::memory_order_release);
  for (DevBuf *b : {&v.bitmap, &v.rows, &v.skipped, &v.word_off, &v.up_ov, &v.up_groups, &v.up_pairs}) b->release();
  v.n_entries = v.n_words = 0;
}

void coverage_mark_resident(kslam_ctx *owner, kslam_ctx *lane) {
  const GenomeIndex &ix = lane->need_index();
  if (ix.n_entries != owner->cov.n_entries) throw StatusError{KSLAM_ERR_STATE, "the coverage table was laid out for another index"};
  coverage_mark_device(lane->res_ov.as<kslam_overlap>(), lane->n_res, lane->pres.d_groups, lane->pres.n_read_pairs, lane->pres.d_pairs,
                       lane->pres.n_pairs, table_of(owner, ix), lane->covw, lane->stream);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_coverage(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (c->in_multi) throw StatusError{KSLAM_ERR_UNSUPPORTED, "the coverage table is not available on the contexts of a kslam_multi"};
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

kslam_status kslam_get_coverage(kslam_ctx *c, int *on) {
  if (!c || !on) return KSLAM_ERR_ARG;
  *on = c->cov.on.load(std::memory_order_acquire) ? 1 : 0;
  return KSLAM_OK;
}

kslam_status kslam_coverage_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->cov.mu);
    need_on(c);
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
    need_on(c);
    const GenomeIndex &ix = c->need_index();
    // nothing is launched for arrays that do not hold together
    if (n_overlaps >= (1ull << 32)) throw StatusError{KSLAM_ERR_ARG, "2^32 or more overlap records"};
    uint64_t next = 0;
    for (uint64_t g = 0; g < n_read_pairs; g++) {
      const kslam_read_pair &rp = read_pairs[g];
      if (rp.first > n_pairs || rp.count > n_pairs - rp.first)
        throw StatusError{KSLAM_ERR_ARG, "read pair " + std::to_string(g) + ": first + count lies outside the pairs array"};
      if (rp.first < next) throw StatusError{KSLAM_ERR_ARG, "read pair " + std::to_string(g) + ": the groups' slices must ascend and not overlap"};
      next = rp.first + rp.count;
      for (uint64_t k = rp.first; k < rp.first + rp.count; k++)
        for (uint32_t idx : {pairs[k].r1, pairs[k].r2})
          if (idx != KSLAM_NO_OVERLAP && idx >= n_overlaps)
            throw StatusError{KSLAM_ERR_ARG, "alignment pair " + std::to_string(k) + " refers to overlap record " + std::to_string(idx) + " of " + std::to_string(n_overlaps)};
    }
    hipStream_t s = c->stream;
    v.up_ov.ensure((n_overlaps + 1) * sizeof(kslam_overlap));
    v.up_groups.ensure((n_read_pairs + 1) * sizeof(kslam_read_pair));
    v.up_pairs.ensure((n_pairs + 1) * sizeof(kslam_paired_overlap));
    if (n_overlaps) HIPCHK(hipMemcpyAsync(v.up_ov.p, overlaps, n_overlaps * sizeof(kslam_overlap), hipMemcpyHostToDevice, s));
    if (n_read_pairs) HIPCHK(hipMemcpyAsync(v.up_groups.p, read_pairs, n_read_pairs * sizeof(kslam_read_pair), hipMemcpyHostToDevice, s));
    if (n_pairs) HIPCHK(hipMemcpyAsync(v.up_pairs.p, pairs, n_pairs * sizeof(kslam_paired_overlap), hipMemcpyHostToDevice, s));
    HIPCHK(stream_wait(s));   // (pageable sources: the caller's arrays are free again)
    coverage_mark_device(v.up_ov.as<kslam_overlap>(), n_overlaps, v.up_groups.as<kslam_read_pair>(), n_read_pairs,
                         v.up_pairs.as<kslam_paired_overlap>(), n_pairs, table_of(c, ix), c->covw, s);
  });
}

kslam_status kslam_coverage_take(kslam_ctx *c, kslam_entry_coverage **rows, uint64_t *n_entries, uint64_t *n_skipped) {
  if (rows) *rows = nullptr;
  if (n_entries) *n_entries = 0;
  if (n_skipped) *n_skipped = 0;
  kslam_entry_coverage *h = nullptr;
  const kslam_status st = guarded(c, [&] {
    if (!rows || !n_entries || !n_skipped) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::Coverage &v = c->cov;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c);
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
  if (st != KSLAM_OK) {
    if (h) pinned_put(c, h);
    if (n_skipped) *n_skipped = 0;
    return st;
  }
  *rows = h;
  return KSLAM_OK;
}

kslam_status kslam_coverage_bitmap(kslam_ctx *c, uint64_t entry, uint64_t *words, uint64_t n_words) {
  return guarded(c, [&] {
    kslam_ctx::Coverage &v = c->cov;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c);
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
  if (c->in_multi) { c->err = "the coverage table is not available on the contexts of a kslam_multi"; return KSLAM_ERR_UNSUPPORTED; }
  c->cov.stream_fd = fd >= 0 ? fd : -1;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_coverage(kslam_ctx *c, int *fd) {
  if (!c || !fd) return KSLAM_ERR_ARG;
  *fd = c->cov.stream_fd;
  return KSLAM_OK;
}

}  // extern "C"
