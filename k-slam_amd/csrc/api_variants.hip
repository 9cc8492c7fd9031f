// api_variants.hip -- the C ABI, part 9: the SNV table (include/kslam_variants.h; kernels: variants.hip).  The state lives on the
// context the switch was set on; its lanes call variants_emit_resident on the batch they have just finished, kslam_variants_add
// takes a batch's arrays from the host, kslam_variants_take sorts the keys and hands the rows over.
#include "context.h"

namespace kslam_api {

namespace {

constexpr uint64_t VAR_MAX_KEYS = 0xFFFFFFFFull;   // the radix sort's limit

void need_on(const kslam_ctx *c) {
  if (!c->var.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the variants are switched off: call kslam_set_variants first"};
}

// every lane's appends are in memory before anybody sorts or empties the arrays
void wait_for_lanes(kslam_ctx *c) {
  for (auto *l : c->lanes) HIPCHK(hipStreamSynchronize(l->c->stream));
}

void empty_state(kslam_ctx::Variants &v) {
  v.n_ev = v.n_iv = v.n_records = v.n_skipped = 0;
  v.sorted = false;
}

// One batch into owner's state: counted on W / s without the lock (the work buffers are the caller's own), appended under it.
// The write pass has finished when the lock is let go, so that whoever grows the arrays next copies complete keys.
void emit(kslam_ctx *owner, const VariantInputs &in, VariantEmitWork &W, hipStream_t s, bool locked) {
  variants_count_device(in, W, s);
  kslam_ctx::Variants &v = owner->var;
  std::unique_lock<std::mutex> lk(v.mu, std::defer_lock);
  if (!locked) lk.lock();
  if (!v.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the variants were switched off while a batch was in flight"};
  if (W.n_ev > VAR_MAX_KEYS - v.n_ev || W.n_iv > VAR_MAX_KEYS - v.n_iv)
    throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^32 - 1 stored events or intervals (the radix sort's limit): the batch was not added"};
  ensure_keep(v.events, (v.n_ev + W.n_ev + 1) * sizeof(uint64_t), v.n_ev * sizeof(uint64_t), s);
  ensure_keep(v.begins, (v.n_iv + W.n_iv + 1) * sizeof(uint64_t), v.n_iv * sizeof(uint64_t), s);
  ensure_keep(v.ends, (v.n_iv + W.n_iv + 1) * sizeof(uint64_t), v.n_iv * sizeof(uint64_t), s);
  variants_write_device(in, W, v.events.as<uint64_t>() + v.n_ev, v.begins.as<uint64_t>() + v.n_iv, v.ends.as<uint64_t>() + v.n_iv, s);
  v.n_ev += W.n_ev;
  v.n_iv += W.n_iv;
  v.n_records += W.n_list;
  v.n_skipped += W.n_skipped;
  if (W.n_ev || W.n_iv) v.sorted = false;
}

}  // namespace

void variants_release(kslam_ctx *c) {
  kslam_ctx::Variants &v = c->var;
  std::lock_guard<std::mutex> lk(v.mu);
  v.on.store(false, std::memory_order_release);
  VariantTakeWork &T = v.tw;
  for (DevBuf *b : {&v.events, &v.begins, &v.ends, &v.up_ov, &v.up_groups, &v.up_pairs, &v.up_pool, &v.up_rbases, &v.up_roff, &T.alt, &T.head, &T.run,
                    &T.starts, &T.fwd, &T.rev, &T.depth, &T.keep, &T.out_at, &T.rows, &T.scan_tmp, &T.totals, &T.sortws.hist, &T.sortws.status,
                    &T.sortws.tickets, &T.sortws.digits})
    b->release();
  empty_state(v);
  v.n_entries = v.total_bases = 0;
}

void variants_emit_resident(kslam_ctx *owner, kslam_ctx *lane) {
  const GenomeIndex &ix = lane->need_index();
  if (ix.n_entries != owner->var.n_entries) throw StatusError{KSLAM_ERR_STATE, "the variants were laid out for another index"};
  const VariantInputs in{lane->res_ov.as<kslam_overlap>(), lane->n_res, lane->pres.d_groups, lane->pres.n_read_pairs, lane->pres.d_pairs,
                         lane->pres.n_pairs, lane->res_cig.as<uint32_t>(), lane->n_cig, lane->r_bases.as<uint8_t>(), lane->r_off.as<uint64_t>(),
                         lane->n_reads, ix.g_bases.as<uint8_t>(), ix.g_off.as<uint64_t>(), ix.n_entries};
  emit(owner, in, lane->varw, lane->stream, false);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_variants(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (c->in_multi) throw StatusError{KSLAM_ERR_UNSUPPORTED, "the variants are not available on the contexts of a kslam_multi"};
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

kslam_status kslam_get_variants(kslam_ctx *c, int *on) {
  if (!c || !on) return KSLAM_ERR_ARG;
  *on = c->var.on.load(std::memory_order_acquire) ? 1 : 0;
  return KSLAM_OK;
}

kslam_status kslam_variants_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->var.mu);
    need_on(c);
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
    need_on(c);
    const GenomeIndex &ix = c->need_index();
    // nothing is launched for arrays that do not hold together
    if (n_overlaps >= (1ull << 32)) throw StatusError{KSLAM_ERR_ARG, "2^32 or more overlap records"};
    for (uint64_t i = 0; i < n_reads; i++)
      if (read_offsets[i + 1] < read_offsets[i]) throw StatusError{KSLAM_ERR_ARG, "the read offsets must ascend"};
    const uint64_t n_rbytes = n_reads ? read_offsets[n_reads] : 0;
    if (n_rbytes && !read_bases) throw StatusError{KSLAM_ERR_ARG, "null argument"};
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
    v.up_ov.ensure((n_overlaps + 1) * sizeof(kslam_overlap));
    v.up_groups.ensure((n_read_pairs + 1) * sizeof(kslam_read_pair));
    v.up_pairs.ensure((n_pairs + 1) * sizeof(kslam_paired_overlap));
    v.up_pool.ensure((n_cigar + 1) * sizeof(uint32_t));
    v.up_rbases.ensure(n_rbytes + 64);
    v.up_roff.ensure((n_reads + 1) * sizeof(uint64_t));
    if (n_overlaps) HIPCHK(hipMemcpyAsync(v.up_ov.p, overlaps, n_overlaps * sizeof(kslam_overlap), hipMemcpyHostToDevice, s));
    if (n_read_pairs) HIPCHK(hipMemcpyAsync(v.up_groups.p, read_pairs, n_read_pairs * sizeof(kslam_read_pair), hipMemcpyHostToDevice, s));
    if (n_pairs) HIPCHK(hipMemcpyAsync(v.up_pairs.p, pairs, n_pairs * sizeof(kslam_paired_overlap), hipMemcpyHostToDevice, s));
    if (n_cigar) HIPCHK(hipMemcpyAsync(v.up_pool.p, cigar_pool, n_cigar * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (n_rbytes) HIPCHK(hipMemcpyAsync(v.up_rbases.p, read_bases, n_rbytes, hipMemcpyHostToDevice, s));
    if (n_reads) HIPCHK(hipMemcpyAsync(v.up_roff.p, read_offsets, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(stream_wait(s));   // (pageable sources: the caller's arrays are free again)
    const VariantInputs in{v.up_ov.as<kslam_overlap>(), n_overlaps, v.up_groups.as<kslam_read_pair>(), n_read_pairs,
                           v.up_pairs.as<kslam_paired_overlap>(), n_pairs, v.up_pool.as<uint32_t>(), n_cigar, v.up_rbases.as<uint8_t>(),
                           v.up_roff.as<uint64_t>(), n_reads, ix.g_bases.as<uint8_t>(), ix.g_off.as<uint64_t>(), ix.n_entries};
    emit(c, in, c->varw, s, true);
  });
}

kslam_status kslam_variants_take(kslam_ctx *c, uint32_t min_alt, uint32_t min_depth, kslam_variant_row **rows, uint64_t *n_rows,
                                 kslam_variant_stats *stats) {
  if (rows) *rows = nullptr;
  if (n_rows) *n_rows = 0;
  if (stats) memset(stats, 0, sizeof *stats);
  kslam_variant_row *h = nullptr;
  const kslam_status st = guarded(c, [&] {
    if (!rows || !n_rows || !stats) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::Variants &v = c->var;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c);
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
  if (st != KSLAM_OK) {
    if (h) pinned_put(c, h);
    if (n_rows) *n_rows = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    return st;
  }
  *rows = h;
  return KSLAM_OK;
}

kslam_status kslam_variants_kernel_ms(kslam_ctx *c, double *emit_ms, double *take_ms) {
  if (!c || !emit_ms || !take_ms) return KSLAM_ERR_ARG;
  *emit_ms = c->varw.ms;
  *take_ms = c->var.take_ms;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_variants(kslam_ctx *c, int fd, uint32_t min_alt, uint32_t min_depth) {
  if (!c) return KSLAM_ERR_ARG;
  if (c->in_multi) { c->err = "the variants are not available on the contexts of a kslam_multi"; return KSLAM_ERR_UNSUPPORTED; }
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
