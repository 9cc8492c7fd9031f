// api_depth.hip -- the C ABI, part 12: the depth track (include/kslam_depth.h; kernels: depth.hip).  The state lives on the
// context the switch was set on; its lanes call depth_emit_resident on the batch they have just finished, kslam_depth_add takes a
// batch's arrays from the host, an add that leaves more pending keys than the threshold compacts them, kslam_depth_take compacts
// what is pending and hands the rows over.
#include "context.h"

namespace kslam_api {

namespace {

constexpr uint64_t DEP_MAX_KEYS = 0xFFFFFFFFull;        // the radix sort's limit
constexpr uint64_t DEP_COMPACT_AT = 1ull << 27;         // pending keys: 1 GiB of them plus as much sort scratch

const char *const REPORT_IS = "the depth track is";
const char *const SWITCHED_OFF = "the depth track is switched off: call kslam_set_depth first";

void empty_state(kslam_ctx::Depth &d) {
  d.n_pend = d.n_keys = d.n_records = d.n_skipped = d.n_iv = 0;
  d.compact_ms = d.take_ms = 0;
}

// the pending keys into the compacted list, on s; the caller holds the lock.  Every write pass has finished by then: a lane lets
// the lock go only after its own (depth_write_device waits), and kslam_depth_take waits for the lanes' streams besides.
void compact(kslam_ctx::Depth &d, hipStream_t s) {
  if (!d.n_pend) return;
  HIPCHK(hipEventRecord(d.ev[0], s));
  depth_compact_device(d.tw, d.pending, d.n_pend, d.ckey, d.cnet, &d.n_keys, d.max_key, s);
  d.n_pend = 0;
  HIPCHK(hipEventRecord(d.ev[1], s));
  HIPCHK(stream_wait(s));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, d.ev[0], d.ev[1]));
  d.compact_ms = ms;
}

// One batch into owner's state: counted on W / s without the lock (the work buffers are the caller's own), appended under it.
void emit(kslam_ctx *owner, const VariantInputs &in, EmitWork &W, hipStream_t s, bool locked) {
  depth_count_device(in, W, s);
  kslam_ctx::Depth &d = owner->dep;
  std::unique_lock<std::mutex> lk(d.mu, std::defer_lock);
  if (!locked) lk.lock();
  if (!d.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the depth track was switched off while a batch was in flight"};
  const uint64_t n_new = 2 * W.n[0];
  if (n_new > DEP_MAX_KEYS) throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^32 - 1 depth keys in one batch (the radix sort's limit): the batch was not added"};
  if (n_new > DEP_MAX_KEYS - d.n_pend) compact(d, s);   // (a threshold set beyond the sort's limit)
  ensure_keep(d.pending, (d.n_pend + n_new + 1) * sizeof(uint64_t), d.n_pend * sizeof(uint64_t), s);
  depth_write_device(in, W, d.pending.as<uint64_t>() + d.n_pend, s);
  d.n_pend += n_new;
  d.n_iv += W.n[0];
  d.n_records += W.n_list;
  d.n_skipped += W.n_skipped;
  if (d.n_pend > (d.compact_at ? d.compact_at : DEP_COMPACT_AT)) {
    try {
      compact(d, s);
    } catch (const StatusError &e) {   // the batch IS added; a merge past the limit is the next take's to report
      if (e.st != KSLAM_ERR_UNSUPPORTED) throw;
    }
  }
}

}  // namespace

void depth_release(kslam_ctx *c) {
  kslam_ctx::Depth &d = c->dep;
  std::lock_guard<std::mutex> lk(d.mu);
  d.on.store(false, std::memory_order_release);
  DepthWork &T = d.tw;
  for (DevBuf *b : {&d.pending, &d.ckey, &d.cnet, &T.alt, &T.head, &T.run, &T.starts, &T.pkey, &T.pnet, &T.mkey, &T.mnet, &T.keep, &T.at, &T.nkey, &T.nnet,
                    &T.tile_sum, &T.depth, &T.rows, &T.scan_tmp, &T.totals, &T.sortws.hist, &T.sortws.status, &T.sortws.tickets, &T.sortws.digits})
    b->release();
  d.up.release_all();
  empty_state(d);
  d.n_entries = d.max_key = 0;
}

void depth_emit_resident(kslam_ctx *owner, kslam_ctx *lane) {
  const GenomeIndex &ix = lane->need_index();
  if (ix.n_entries != owner->dep.n_entries) throw StatusError{KSLAM_ERR_STATE, "the depth track was laid out for another index"};
  emit(owner, resident_inputs(lane, ix, false), lane->depw, lane->stream, false);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_depth(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (refused_in_multi(c, REPORT_IS)) throw StatusError{KSLAM_ERR_UNSUPPORTED, c->err};
    if (!on) {
      if (c->dep.on.load(std::memory_order_acquire)) wait_for_lanes(c);
      depth_release(c);
      return;
    }
    const GenomeIndex &ix = c->need_index();
    if (!c->pairing.stages) throw StatusError{KSLAM_ERR_STATE, "kslam_set_depth needs the device pairing: call kslam_set_pairing first"};
    if (!c->prm.report_cigar) throw StatusError{KSLAM_ERR_STATE, "kslam_set_depth needs the CIGARs: create the context with report_cigar != 0"};
    kslam_ctx::Depth &d = c->dep;
    std::lock_guard<std::mutex> lk(d.mu);
    if (d.on.load(std::memory_order_acquire)) return;
    if (ix.h_goff[ix.n_entries] >= (1ull << 60)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^60 or more bases in the index"};
    d.n_entries = ix.n_entries;
    d.max_key = ix.h_goff[ix.n_entries] + ix.n_entries;
    empty_state(d);
    if (!d.ev[0])
      for (auto &e : d.ev) HIPCHK(hipEventCreate(&e));
    d.on.store(true, std::memory_order_release);
  });
}

kslam_status kslam_get_depth(kslam_ctx *c, int *on) { return get_switch(c, &kslam_ctx::dep, on); }

kslam_status kslam_depth_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->dep.mu);
    need_on(c->dep.on, SWITCHED_OFF);
    wait_for_lanes(c);
    empty_state(c->dep);
  });
}

kslam_status kslam_depth_set_compact_at(kslam_ctx *c, uint64_t n_keys) {
  if (!c) return KSLAM_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->dep.mu);
  c->dep.compact_at = n_keys;
  return KSLAM_OK;
}

kslam_status kslam_depth_add(kslam_ctx *c, const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                             const uint64_t *read_offsets, uint64_t n_reads, const kslam_read_pair *read_pairs, uint64_t n_read_pairs,
                             const kslam_paired_overlap *pairs, uint64_t n_pairs) {
  return guarded(c, [&] {
    if ((n_overlaps && !overlaps) || (n_cigar && !cigar_pool) || (n_reads && !read_offsets) || (n_read_pairs && !read_pairs) || (n_pairs && !pairs))
      throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::Depth &d = c->dep;
    std::lock_guard<std::mutex> lk(d.mu);
    need_on(c->dep.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    // nothing is launched for arrays that do not hold together
    const kslam_batch::Arrays batch{overlaps, n_overlaps, n_cigar, read_offsets, n_reads, read_pairs, n_read_pairs, pairs, n_pairs};
    const std::string fault = kslam_batch::check(batch, kslam_batch::Level::records);
    if (!fault.empty()) throw StatusError{KSLAM_ERR_ARG, fault};
    hipStream_t s = c->stream;
    const VariantInputs in = d.up.upload(batch, kslam_batch::Level::records, cigar_pool, BatchUpload::no_columns, nullptr, nullptr, &ix, s);
    emit(c, in, c->depw, s, true);
  });
}

kslam_status kslam_depth_take(kslam_ctx *c, uint32_t min_depth, kslam_depth_row **rows, uint64_t *n_rows, kslam_depth_stats *stats) {
  return take_rows(c, rows, n_rows, stats, [&](kslam_depth_row *&h) {
    kslam_ctx::Depth &d = c->dep;
    std::lock_guard<std::mutex> lk(d.mu);
    need_on(c->dep.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    wait_for_lanes(c);
    hipStream_t s = c->stream;
    compact(d, s);   // (nothing pending: neither the sort nor the merge runs again)
    uint64_t out[4] = {0, 0, 0, 0};
    HIPCHK(hipEventRecord(d.ev[2], s));
    depth_take_device(d.tw, d.ckey.as<uint64_t>(), d.cnet.as<int64_t>(), d.n_keys, ix.g_off.as<uint64_t>(), ix.n_entries, min_depth, out, s);
    HIPCHK(hipEventRecord(d.ev[3], s));
    const uint64_t n = out[3];
    if (n > out[0] || out[0] > d.n_keys)
      throw StatusError{KSLAM_ERR_INTERNAL, "the depth take counted " + std::to_string(n) + " of " + std::to_string(out[0]) + " rows over " + std::to_string(d.n_keys) + " boundaries"};
    h = (kslam_depth_row *)pinned_get(c, (n + 1) * sizeof(kslam_depth_row));
    if (n) HIPCHK(hipMemcpyAsync(h, d.tw.rows.p, n * sizeof(kslam_depth_row), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, d.ev[2], d.ev[3]));
    d.take_ms = ms;
    *n_rows = n;
    stats->n_records = d.n_records;
    stats->n_skipped = d.n_skipped;
    stats->n_intervals = d.n_iv;
    stats->n_keys = d.n_keys;
    stats->n_rows = out[0];
    stats->covered_bases = out[1];
    stats->max_depth = out[2];
  });
}

kslam_status kslam_depth_kernel_ms(kslam_ctx *c, double *emit_ms, double *compact_ms, double *take_ms) {
  if (!c || !emit_ms || !compact_ms || !take_ms) return KSLAM_ERR_ARG;
  *emit_ms = c->depw.ms;
  *compact_ms = c->dep.compact_ms;
  *take_ms = c->dep.take_ms;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_depth(kslam_ctx *c, int fd, uint32_t min_depth) {
  if (!c) return KSLAM_ERR_ARG;
  if (refused_in_multi(c, REPORT_IS)) return KSLAM_ERR_UNSUPPORTED;
  c->dep.stream_fd = fd >= 0 ? fd : -1;
  c->dep.stream_min_depth = min_depth;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_depth(kslam_ctx *c, int *fd, uint32_t *min_depth) {
  if (!c || !fd || !min_depth) return KSLAM_ERR_ARG;
  *fd = c->dep.stream_fd;
  *min_depth = c->dep.stream_min_depth;
  return KSLAM_OK;
}

}  // extern "C"
