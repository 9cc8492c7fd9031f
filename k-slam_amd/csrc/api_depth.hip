// api_depth.hip -- the C ABI, part 12: the depth track (include/kslam_depth.h; kernels: depth.hip).  The state lives on the
// context the switch was set on; its lanes call depth_emit_resident on the batch they have just finished, kslam_depth_add takes a
// batch's arrays from the host, an add that leaves more pending keys than the threshold compacts them, kslam_depth_take compacts
// what is pending and hands the rows over.
#include "context.h"

namespace kslam_api {

namespace {

constexpr uint64_t DEP_MAX_KEYS = 0xFFFFFFFFull;        // the radix sort's limit
constexpr uint64_t DEP_COMPACT_AT = 1ull << 27;         // pending keys: 1 GiB of them plus as much sort scratch

void need_on(const kslam_ctx *c) {
  if (!c->dep.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the depth track is switched off: call kslam_set_depth first"};
}

// every lane's appends are in memory before anybody sorts or empties the arrays
void wait_for_lanes(kslam_ctx *c) {
  for (auto *l : c->lanes) HIPCHK(hipStreamSynchronize(l->c->stream));
}

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
void emit(kslam_ctx *owner, const VariantInputs &in, DepthEmitWork &W, hipStream_t s, bool locked) {
  depth_count_device(in, W, s);
  kslam_ctx::Depth &d = owner->dep;
  std::unique_lock<std::mutex> lk(d.mu, std::defer_lock);
  if (!locked) lk.lock();
  if (!d.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the depth track was switched off while a batch was in flight"};
  const uint64_t n_new = 2 * W.n_iv;
  if (n_new > DEP_MAX_KEYS) throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^32 - 1 depth keys in one batch (the radix sort's limit): the batch was not added"};
  if (n_new > DEP_MAX_KEYS - d.n_pend) compact(d, s);   // (a threshold set beyond the sort's limit)
  ensure_keep(d.pending, (d.n_pend + n_new + 1) * sizeof(uint64_t), d.n_pend * sizeof(uint64_t), s);
  depth_write_device(in, W, d.pending.as<uint64_t>() + d.n_pend, s);
  d.n_pend += n_new;
  d.n_iv += W.n_iv;
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
  for (DevBuf *b : {&d.pending, &d.ckey, &d.cnet, &d.up_ov, &d.up_groups, &d.up_pairs, &d.up_pool, &d.up_roff, &T.alt, &T.head, &T.run, &T.starts, &T.pkey,
                    &T.pnet, &T.mkey, &T.mnet, &T.keep, &T.at, &T.nkey, &T.nnet, &T.tile_sum, &T.depth, &T.rows, &T.scan_tmp, &T.totals, &T.sortws.hist,
                    &T.sortws.status, &T.sortws.tickets, &T.sortws.digits})
    b->release();
  empty_state(d);
  d.n_entries = d.max_key = 0;
}

void depth_emit_resident(kslam_ctx *owner, kslam_ctx *lane) {
  const GenomeIndex &ix = lane->need_index();
  if (ix.n_entries != owner->dep.n_entries) throw StatusError{KSLAM_ERR_STATE, "the depth track was laid out for another index"};
  const VariantInputs in{lane->res_ov.as<kslam_overlap>(), lane->n_res, lane->pres.d_groups, lane->pres.n_read_pairs, lane->pres.d_pairs,
                         lane->pres.n_pairs, lane->res_cig.as<uint32_t>(), lane->n_cig, nullptr, lane->r_off.as<uint64_t>(),
                         lane->n_reads, nullptr, ix.g_off.as<uint64_t>(), ix.n_entries};
  emit(owner, in, lane->depw, lane->stream, false);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_depth(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (c->in_multi) throw StatusError{KSLAM_ERR_UNSUPPORTED, "the depth track is not available on the contexts of a kslam_multi"};
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

kslam_status kslam_get_depth(kslam_ctx *c, int *on) {
  if (!c || !on) return KSLAM_ERR_ARG;
  *on = c->dep.on.load(std::memory_order_acquire) ? 1 : 0;
  return KSLAM_OK;
}

kslam_status kslam_depth_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->dep.mu);
    need_on(c);
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
    need_on(c);
    const GenomeIndex &ix = c->need_index();
    // nothing is launched for arrays that do not hold together
    if (n_overlaps >= (1ull << 32)) throw StatusError{KSLAM_ERR_ARG, "2^32 or more overlap records"};
    for (uint64_t i = 0; i < n_reads; i++)
      if (read_offsets[i + 1] < read_offsets[i]) throw StatusError{KSLAM_ERR_ARG, "the read offsets must ascend"};
    uint64_t next = 0;
    for (uint64_t g = 0; g < n_read_pairs; g++) {
      const kslam_read_pair &rp = read_pairs[g];
      if (rp.first > n_pairs || rp.count > n_pairs - rp.first)
        throw StatusError{KSLAM_ERR_ARG, "read pair " + std::to_string(g) + ": first + count lies outside the pairs array"};
      if (rp.first < next) throw StatusError{KSLAM_ERR_ARG, "read pair " + std::to_string(g) + ": the groups' slices must ascend and not overlap"};
      next = rp.first + rp.count;
      for (uint64_t k = rp.first; k < rp.first + rp.count; k++)
        for (uint32_t idx : {pairs[k].r1, pairs[k].r2}) {
          if (idx == KSLAM_NO_OVERLAP) continue;
          if (idx >= n_overlaps)
            throw StatusError{KSLAM_ERR_ARG, "alignment pair " + std::to_string(k) + " refers to overlap record " + std::to_string(idx) + " of " + std::to_string(n_overlaps)};
          const kslam_overlap &o = overlaps[idx];
          if (o.cigar_off > n_cigar || o.cigar_len > n_cigar - o.cigar_off)
            throw StatusError{KSLAM_ERR_ARG, "overlap record " + std::to_string(idx) + ": its CIGAR slice lies outside the pool"};
          if (o.read >= n_reads)
            throw StatusError{KSLAM_ERR_ARG, "overlap record " + std::to_string(idx) + " refers to read " + std::to_string(o.read) + " of " + std::to_string(n_reads)};
        }
    }
    hipStream_t s = c->stream;
    d.up_ov.ensure((n_overlaps + 1) * sizeof(kslam_overlap));
    d.up_groups.ensure((n_read_pairs + 1) * sizeof(kslam_read_pair));
    d.up_pairs.ensure((n_pairs + 1) * sizeof(kslam_paired_overlap));
    d.up_pool.ensure((n_cigar + 1) * sizeof(uint32_t));
    d.up_roff.ensure((n_reads + 1) * sizeof(uint64_t));
    if (n_overlaps) HIPCHK(hipMemcpyAsync(d.up_ov.p, overlaps, n_overlaps * sizeof(kslam_overlap), hipMemcpyHostToDevice, s));
    if (n_read_pairs) HIPCHK(hipMemcpyAsync(d.up_groups.p, read_pairs, n_read_pairs * sizeof(kslam_read_pair), hipMemcpyHostToDevice, s));
    if (n_pairs) HIPCHK(hipMemcpyAsync(d.up_pairs.p, pairs, n_pairs * sizeof(kslam_paired_overlap), hipMemcpyHostToDevice, s));
    if (n_cigar) HIPCHK(hipMemcpyAsync(d.up_pool.p, cigar_pool, n_cigar * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (n_reads) HIPCHK(hipMemcpyAsync(d.up_roff.p, read_offsets, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(stream_wait(s));   // (pageable sources: the caller's arrays are free again)
    const VariantInputs in{d.up_ov.as<kslam_overlap>(), n_overlaps, d.up_groups.as<kslam_read_pair>(), n_read_pairs,
                           d.up_pairs.as<kslam_paired_overlap>(), n_pairs, d.up_pool.as<uint32_t>(), n_cigar, nullptr,
                           d.up_roff.as<uint64_t>(), n_reads, nullptr, ix.g_off.as<uint64_t>(), ix.n_entries};
    emit(c, in, c->depw, s, true);
  });
}

kslam_status kslam_depth_take(kslam_ctx *c, uint32_t min_depth, kslam_depth_row **rows, uint64_t *n_rows, kslam_depth_stats *stats) {
  if (rows) *rows = nullptr;
  if (n_rows) *n_rows = 0;
  if (stats) memset(stats, 0, sizeof *stats);
  kslam_depth_row *h = nullptr;
  const kslam_status st = guarded(c, [&] {
    if (!rows || !n_rows || !stats) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::Depth &d = c->dep;
    std::lock_guard<std::mutex> lk(d.mu);
    need_on(c);
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
  if (st != KSLAM_OK) {
    if (h) pinned_put(c, h);
    if (n_rows) *n_rows = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    return st;
  }
  *rows = h;
  return KSLAM_OK;
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
  if (c->in_multi) { c->err = "the depth track is not available on the contexts of a kslam_multi"; return KSLAM_ERR_UNSUPPORTED; }
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
