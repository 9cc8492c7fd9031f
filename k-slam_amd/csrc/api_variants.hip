// api_variants.hip -- the C ABI, part 9: the SNV table (include/kslam_variants.h; kernels: variants.hip).  The state lives on the
// context the switch was set on; its lanes call variants_emit_resident on the batch they have just finished, kslam_variants_add
// takes a batch's arrays from the host, kslam_variants_take sorts the keys and hands the rows over.
#include "context.h"

namespace kslam_api {

namespace {

constexpr uint64_t VAR_MAX_KEYS = 0xFFFFFFFFull;   // the radix sort's limit

const char *const REPORT_IS = "the variants are";
const char *const SWITCHED_OFF = "the variants are switched off: call kslam_set_variants first";

void empty_state(kslam_ctx::Variants &v) {
  v.n_ev = v.n_iv = v.n_records = v.n_skipped = 0;
  v.sorted = false;
}

// One batch into owner's state: counted on W / s without the lock (the work buffers are the caller's own), appended under it.
// The write pass has finished when the lock is let go, so that whoever grows the arrays next copies complete keys.
void emit(kslam_ctx *owner, const VariantInputs &in, EmitWork &W, hipStream_t s, bool locked) {
  variants_count_device(in, W, s);
  kslam_ctx::Variants &v = owner->var;
  std::unique_lock<std::mutex> lk(v.mu, std::defer_lock);
  if (!locked) lk.lock();
  if (!v.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the variants were switched off while a batch was in flight"};
  if (W.n[VAR_EV] > VAR_MAX_KEYS - v.n_ev || W.n[VAR_IV] > VAR_MAX_KEYS - v.n_iv)
    throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^32 - 1 stored events or intervals (the radix sort's limit): the batch was not added"};
  ensure_keep(v.events, (v.n_ev + W.n[VAR_EV] + 1) * sizeof(uint64_t), v.n_ev * sizeof(uint64_t), s);
  ensure_keep(v.begins, (v.n_iv + W.n[VAR_IV] + 1) * sizeof(uint64_t), v.n_iv * sizeof(uint64_t), s);
  ensure_keep(v.ends, (v.n_iv + W.n[VAR_IV] + 1) * sizeof(uint64_t), v.n_iv * sizeof(uint64_t), s);
  variants_write_device(in, W, v.events.as<uint64_t>() + v.n_ev, v.begins.as<uint64_t>() + v.n_iv, v.ends.as<uint64_t>() + v.n_iv, s);
  v.n_ev += W.n[VAR_EV];
  v.n_iv += W.n[VAR_IV];
  v.n_records += W.n_list;
  v.n_skipped += W.n_skipped;
  if (W.n[VAR_EV] || W.n[VAR_IV]) v.sorted = false;
}

}  // namespace

void variants_release(kslam_ctx *c) {
  kslam_ctx::Variants &v = c->var;
  std::lock_guard<std::mutex> lk(v.mu);
  v.on.store(false, std::memory_order_release);
  VariantTakeWork &T = v.tw;
  for (DevBuf *b : {&v.events, &v.begins, &v.ends, &T.alt, &T.head, &T.run, &T.starts, &T.fwd, &T.rev, &T.depth, &T.keep, &T.out_at, &T.rows, &T.scan_tmp,
                    &T.totals, &T.sortws.hist, &T.sortws.status, &T.sortws.tickets, &T.sortws.digits})
    b->release();
  v.up.release_all();
  empty_state(v);
  v.n_entries = v.total_bases = 0;
}

void variants_emit_resident(kslam_ctx *owner, kslam_ctx *lane) {
  const GenomeIndex &ix = lane->need_index();
  if (ix.n_entries != owner->var.n_entries) throw StatusError{KSLAM_ERR_STATE, "the variants were laid out for another index"};
  emit(owner, resident_inputs(lane, ix, true), lane->varw, lane->stream, false);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_variants(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (refused_in_multi(c, REPORT_IS)) throw StatusError{KSLAM_ERR_UNSUPPORTED, c->err};
    if (!on) {
      if (c->var.on.load(std::memory_order_acquire)) wait_for_lanes(c);
      variants_release(c);
      return;
    }
    const GenomeIndex &ix = c->need_index();
    if (!c->pairing.stages) throw StatusError{KSLAM_ERR_STATE, "kslam_set_variants needs the device pairing: call kslam_set_pairing first"};
    if (!c->prm.report_cigar) throw StatusError{KSLAM_ERR_STATE, "kslam_set_variants needs the CIGARs: create the context with report_cigar != 0"};
    kslam_ctx::Variants &v = c->var;
    std::lock_guard<std::mutex> lk(v.mu);
    if (v.on.load(std::memory_order_acquire)) return;
    if (ix.h_goff[ix.n_entries] >= (1ull << 60)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^60 or more bases in the index"};
    v.n_entries = ix.n_entries;
    v.total_bases = ix.h_goff[ix.n_entries];
    empty_state(v);
    if (!v.ev_take[0])
      for (auto &e : v.ev_take) HIPCHK(hipEventCreate(&e));
    v.take_ms = 0;
    v.on.store(true, std::memory_order_release);
  });
}

kslam_status kslam_get_variants(kslam_ctx *c, int *on) { return get_switch(c, &kslam_ctx::var, on); }

kslam_status kslam_variants_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->var.mu);
    need_on(c->var.on, SWITCHED_OFF);
    wait_for_lanes(c);
    empty_state(c->var);
  });
}

kslam_status kslam_variants_add(kslam_ctx *c, const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                                const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads, const kslam_read_pair *read_pairs,
                                uint64_t n_read_pairs, const kslam_paired_overlap *pairs, uint64_t n_pairs) {
  return guarded(c, [&] {
    if ((n_overlaps && !overlaps) || (n_cigar && !cigar_pool) || (n_reads && !read_offsets) || (n_read_pairs && !read_pairs) || (n_pairs && !pairs))
      throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::Variants &v = c->var;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->var.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    const uint64_t n_rbytes = n_reads ? read_offsets[n_reads] : 0;
    if (n_rbytes && !read_bases) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    // nothing is launched for arrays that do not hold together
    const kslam_batch::Arrays batch{overlaps, n_overlaps, n_cigar, read_offsets, n_reads, read_pairs, n_read_pairs, pairs, n_pairs};
    const std::string fault = kslam_batch::check(batch, kslam_batch::Level::records);
    if (!fault.empty()) throw StatusError{KSLAM_ERR_ARG, fault};
    hipStream_t s = c->stream;
    const VariantInputs in = v.up.upload(batch, kslam_batch::Level::records, cigar_pool, BatchUpload::bases, read_bases, nullptr, &ix, s);
    emit(c, in, c->varw, s, true);
  });
}

kslam_status kslam_variants_take(kslam_ctx *c, uint32_t min_alt, uint32_t min_depth, kslam_variant_row **rows, uint64_t *n_rows,
                                 kslam_variant_stats *stats) {
  return take_rows(c, rows, n_rows, stats, [&](kslam_variant_row *&h) {
    kslam_ctx::Variants &v = c->var;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->var.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    wait_for_lanes(c);
    hipStream_t s = c->stream;
    uint64_t n_sites = 0, n = 0;
    HIPCHK(hipEventRecord(v.ev_take[0], s));
    variants_take_device(v.tw, v.events, v.n_ev, v.begins, v.ends, v.n_iv, v.sorted, ix.g_off.as<uint64_t>(), ix.g_bases.as<uint8_t>(), ix.n_entries,
                         v.total_bases, min_alt, min_depth, &n_sites, &n, s);
    v.sorted = true;
    HIPCHK(hipEventRecord(v.ev_take[1], s));
    h = (kslam_variant_row *)pinned_get(c, (n + 1) * sizeof(kslam_variant_row));
    if (n) HIPCHK(hipMemcpyAsync(h, v.tw.rows.p, n * sizeof(kslam_variant_row), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, v.ev_take[0], v.ev_take[1]));
    v.take_ms = ms;
    *n_rows = n;
    stats->n_records = v.n_records;
    stats->n_skipped = v.n_skipped;
    stats->n_intervals = v.n_iv;
    stats->n_events = v.n_ev;
    stats->n_sites = n_sites;
  });
}

kslam_status kslam_variants_kernel_ms(kslam_ctx *c, double *emit_ms, double *take_ms) {
  if (!c || !emit_ms || !take_ms) return KSLAM_ERR_ARG;
  *emit_ms = c->varw.ms;
  *take_ms = c->var.take_ms;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_variants(kslam_ctx *c, int fd, uint32_t min_alt, uint32_t min_depth) {
  if (!c) return KSLAM_ERR_ARG;
  if (refused_in_multi(c, REPORT_IS)) return KSLAM_ERR_UNSUPPORTED;
  c->var.stream_fd = fd >= 0 ? fd : -1;
  c->var.stream_min_alt = min_alt;
  c->var.stream_min_depth = min_depth;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_variants(kslam_ctx *c, int *fd, uint32_t *min_alt, uint32_t *min_depth) {
  if (!c || !fd || !min_alt || !min_depth) return KSLAM_ERR_ARG;
  *fd = c->var.stream_fd;
  *min_alt = c->var.stream_min_alt;
  *min_depth = c->var.stream_min_depth;
  return KSLAM_OK;
}

}  // extern "C"
