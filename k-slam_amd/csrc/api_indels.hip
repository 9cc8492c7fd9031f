// api_indels.hip -- the C ABI, part 9b: the indel table (include/kslam_indels.h; kernels: indels.hip).  The state lives on the
// context the switch was set on; its lanes call indels_emit_resident on the batch they have just finished, kslam_indels_add takes
// a batch's arrays from the host, kslam_indels_take sorts the keys, takes the filtered rows of each kind and merges them.
#include "context.h"

namespace kslam_api {

namespace {

constexpr uint64_t INDEL_MAX_KEYS = 0xFFFFFFFFull;   // the radix sort's limit

const char *const REPORT_IS = "the indels are";
const char *const SWITCHED_OFF = "the indels are switched off: call kslam_set_indels first";

void empty_state(kslam_ctx::Indels &v) {
  for (auto &n : v.n) n = 0;
  v.n_records = v.n_skipped = v.n_unanchored = v.n_unrepresentable = 0;
  v.sorted = false;
}

// One batch into owner's state: counted on W / s without the lock (the work buffers are the caller's own), appended under it.
// The write pass has finished when the lock is let go, so that whoever grows the arrays next copies complete keys.
void emit(kslam_ctx *owner, const VariantInputs &in, EmitWork &W, hipStream_t s, bool locked) {
  indels_count_device(in, W, s);
  kslam_ctx::Indels &v = owner->ind;
  std::unique_lock<std::mutex> lk(v.mu, std::defer_lock);
  if (!locked) lk.lock();
  if (!v.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the indels were switched off while a batch was in flight"};
  for (int kind : {INDEL_IV, INDEL_DEL, INDEL_INS})
    if (W.n[kind] > INDEL_MAX_KEYS - v.n[kind])
      throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^32 - 1 stored intervals, deletions or insertions (the radix sort's limit): the batch was not added"};
  ensure_keep(v.begins, (v.n[INDEL_IV] + W.n[INDEL_IV] + 1) * sizeof(uint64_t), v.n[INDEL_IV] * sizeof(uint64_t), s);
  ensure_keep(v.ends, (v.n[INDEL_IV] + W.n[INDEL_IV] + 1) * sizeof(uint64_t), v.n[INDEL_IV] * sizeof(uint64_t), s);
  ensure_keep(v.dels, (v.n[INDEL_DEL] + W.n[INDEL_DEL] + 1) * sizeof(uint64_t), v.n[INDEL_DEL] * sizeof(uint64_t), s);
  ensure_keep(v.ins, 2 * (v.n[INDEL_INS] + W.n[INDEL_INS] + 1) * sizeof(uint64_t), 2 * v.n[INDEL_INS] * sizeof(uint64_t), s);
  indels_write_device(in, W,
                      IndelKeys{v.begins.as<uint64_t>() + v.n[INDEL_IV], v.ends.as<uint64_t>() + v.n[INDEL_IV], v.dels.as<uint64_t>() + v.n[INDEL_DEL],
                                v.ins.as<uint64_t>() + 2 * v.n[INDEL_INS]},
                      s);
  for (int kind = 0; kind < INDEL_KINDS; kind++) v.n[kind] += W.n[kind];
  v.n_records += W.n_list;
  v.n_skipped += W.n_skipped;
  v.n_unanchored += W.n_unanchored;
  v.n_unrepresentable += W.n_unrepresentable;
  if (W.n[INDEL_IV] || W.n[INDEL_DEL] || W.n[INDEL_INS]) v.sorted = false;
}

// ascending as the rows do: entry, pos, kind, len, bases
bool row_before(const kslam_indel_row &a, const kslam_indel_row &b) {
  if (a.entry != b.entry) return a.entry < b.entry;
  if (a.pos != b.pos) return a.pos < b.pos;
  if (a.kind != b.kind) return a.kind < b.kind;
  if (a.len != b.len) return a.len < b.len;
  return a.bases < b.bases;
}

}  // namespace

void indels_release(kslam_ctx *c) {
  kslam_ctx::Indels &v = c->ind;
  std::lock_guard<std::mutex> lk(v.mu);
  v.on.store(false, std::memory_order_release);
  VariantTakeWork &T = v.tw;
  for (DevBuf *b : {&v.begins, &v.ends, &v.dels, &v.ins, &T.alt, &T.head, &T.run, &T.starts, &T.fwd, &T.rev, &T.depth, &T.keep, &T.out_at, &T.rows,
                    &T.scan_tmp, &T.totals, &T.sortws.hist, &T.sortws.status, &T.sortws.tickets, &T.sortws.digits})
    b->release();
  v.up.release_all();
  empty_state(v);
  v.n_entries = v.total_bases = 0;
}

void indels_emit_resident(kslam_ctx *owner, kslam_ctx *lane) {
  const GenomeIndex &ix = lane->need_index();
  if (ix.n_entries != owner->ind.n_entries) throw StatusError{KSLAM_ERR_STATE, "the indels were laid out for another index"};
  emit(owner, resident_inputs(lane, ix, true), lane->indw, lane->stream, false);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_indels(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (refused_in_multi(c, REPORT_IS)) throw StatusError{KSLAM_ERR_UNSUPPORTED, c->err};
    if (!on) {
      if (c->ind.on.load(std::memory_order_acquire)) wait_for_lanes(c);
      indels_release(c);
      return;
    }
    const GenomeIndex &ix = c->need_index();
    if (!c->pairing.stages) throw StatusError{KSLAM_ERR_STATE, "kslam_set_indels needs the device pairing: call kslam_set_pairing first"};
    if (!c->prm.report_cigar) throw StatusError{KSLAM_ERR_STATE, "kslam_set_indels needs the CIGARs: create the context with report_cigar != 0"};
    kslam_ctx::Indels &v = c->ind;
    std::lock_guard<std::mutex> lk(v.mu);
    if (v.on.load(std::memory_order_acquire)) return;
    if (ix.h_goff[ix.n_entries] >= (1ull << 47)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^47 or more bases in the index"};
    v.n_entries = ix.n_entries;
    v.total_bases = ix.h_goff[ix.n_entries];
    empty_state(v);
    if (!v.ev_take[0])
      for (auto &e : v.ev_take) HIPCHK(hipEventCreate(&e));
    v.take_ms = 0;
    v.on.store(true, std::memory_order_release);
  });
}

kslam_status kslam_get_indels(kslam_ctx *c, int *on) { return get_switch(c, &kslam_ctx::ind, on); }

kslam_status kslam_indels_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->ind.mu);
    need_on(c->ind.on, SWITCHED_OFF);
    wait_for_lanes(c);
    empty_state(c->ind);
  });
}

kslam_status kslam_indels_add(kslam_ctx *c, const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                              const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads, const kslam_read_pair *read_pairs,
                              uint64_t n_read_pairs, const kslam_paired_overlap *pairs, uint64_t n_pairs) {
  return guarded(c, [&] {
    if ((n_overlaps && !overlaps) || (n_cigar && !cigar_pool) || (n_reads && !read_offsets) || (n_read_pairs && !read_pairs) || (n_pairs && !pairs))
      throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::Indels &v = c->ind;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->ind.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    const uint64_t n_rbytes = n_reads ? read_offsets[n_reads] : 0;
    if (n_rbytes && !read_bases) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    // nothing is launched for arrays that do not hold together
    const kslam_batch::Arrays batch{overlaps, n_overlaps, n_cigar, read_offsets, n_reads, read_pairs, n_read_pairs, pairs, n_pairs};
    const std::string fault = kslam_batch::check(batch, kslam_batch::Level::records);
    if (!fault.empty()) throw StatusError{KSLAM_ERR_ARG, fault};
    hipStream_t s = c->stream;
    const VariantInputs in = v.up.upload(batch, kslam_batch::Level::records, cigar_pool, BatchUpload::bases, read_bases, nullptr, &ix, s);
    emit(c, in, c->indw, s, true);
  });
}

kslam_status kslam_indels_take(kslam_ctx *c, uint32_t min_alt, uint32_t min_depth, kslam_indel_row **rows, uint64_t *n_rows, kslam_indel_stats *stats) {
  return take_rows(c, rows, n_rows, stats, [&](kslam_indel_row *&h) {
    kslam_ctx::Indels &v = c->ind;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->ind.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    wait_for_lanes(c);
    hipStream_t s = c->stream;
    HIPCHK(hipEventRecord(v.ev_take[0], s));
    if (!v.sorted) indels_sort_device(v.tw, v.begins, v.ends, v.n[INDEL_IV], v.dels, v.n[INDEL_DEL], v.ins, v.n[INDEL_INS], v.total_bases, s);
    v.sorted = true;
    // the filtered rows of each kind, in their order; merged here into the one order (only these rows travel)
    std::vector<kslam_indel_row> by_kind[2];
    uint64_t n_sites = 0;
    for (int kind : {KSLAM_INDEL_DEL, KSLAM_INDEL_INS}) {
      uint64_t sites = 0, n = 0;
      indels_take_device(v.tw, kind, kind == KSLAM_INDEL_DEL ? v.dels.as<uint64_t>() : v.ins.as<uint64_t>(),
                         v.n[kind == KSLAM_INDEL_DEL ? INDEL_DEL : INDEL_INS], v.begins.as<uint64_t>(), v.ends.as<uint64_t>(), v.n[INDEL_IV],
                         ix.g_off.as<uint64_t>(), ix.n_entries, min_alt, min_depth, &sites, &n, s);
      n_sites += sites;
      by_kind[kind].resize(n);
      if (n) HIPCHK(hipMemcpyAsync(by_kind[kind].data(), v.tw.rows.p, n * sizeof(kslam_indel_row), hipMemcpyDeviceToHost, s));
      HIPCHK(stream_wait(s));   // (the next kind reuses the work buffers)
    }
    HIPCHK(hipEventRecord(v.ev_take[1], s));
    HIPCHK(stream_wait(s));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, v.ev_take[0], v.ev_take[1]));
    v.take_ms = ms;
    const uint64_t n = by_kind[0].size() + by_kind[1].size();
    h = (kslam_indel_row *)pinned_get(c, (n + 1) * sizeof(kslam_indel_row));
    std::merge(by_kind[0].begin(), by_kind[0].end(), by_kind[1].begin(), by_kind[1].end(), h, row_before);
    *n_rows = n;
    stats->n_records = v.n_records;
    stats->n_skipped = v.n_skipped;
    stats->n_intervals = v.n[INDEL_IV];
    stats->n_deletions = v.n[INDEL_DEL];
    stats->n_insertions = v.n[INDEL_INS];
    stats->n_unanchored = v.n_unanchored;
    stats->n_long_del = v.n[INDEL_LONG];
    stats->n_unrepresentable = v.n_unrepresentable;
    stats->n_sites = n_sites;
  });
}

kslam_status kslam_indels_kernel_ms(kslam_ctx *c, double *emit_ms, double *take_ms) {
  if (!c || !emit_ms || !take_ms) return KSLAM_ERR_ARG;
  *emit_ms = c->indw.ms;
  *take_ms = c->ind.take_ms;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_indels(kslam_ctx *c, int fd, uint32_t min_alt, uint32_t min_depth) {
  if (!c) return KSLAM_ERR_ARG;
  if (refused_in_multi(c, REPORT_IS)) return KSLAM_ERR_UNSUPPORTED;
  c->ind.stream_fd = fd >= 0 ? fd : -1;
  c->ind.stream_min_alt = min_alt;
  c->ind.stream_min_depth = min_depth;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_indels(kslam_ctx *c, int *fd, uint32_t *min_alt, uint32_t *min_depth) {
  if (!c || !fd || !min_alt || !min_depth) return KSLAM_ERR_ARG;
  *fd = c->ind.stream_fd;
  *min_alt = c->ind.stream_min_alt;
  *min_depth = c->ind.stream_min_depth;
  return KSLAM_OK;
}

}  // extern "C"
