// api_consensus.hip -- the C ABI, part 16: the consensus caller (include/kslam_consensus.h; kernels: consensus.hip).  The state
// lives on the context the switch was set on; its lanes call consensus_emit_resident on the batch they have just finished,
// kslam_consensus_add takes a batch's arrays from the host, kslam_consensus_take sorts the keys, calls the touched entries slice by
// slice and hands the reported entries' rows and sequences over.
#include "context.h"

namespace kslam_api {

namespace {

constexpr uint64_t CNS_MAX_KEYS = 0xFFFFFFFFull;   // the radix sort's limit
constexpr uint64_t CNS_MAX_SLICE = 1ull << 32;     // what one launch of the call pass covers

const char *const REPORT_IS = "the consensus is";
const char *const SWITCHED_OFF = "the consensus is switched off: call kslam_set_consensus first";

void empty_state(kslam_ctx::Consensus &v) {
  for (auto &n : v.n) n = 0;
  v.n_records = v.n_skipped = v.n_unanchored = v.n_unrepresentable = 0;
  v.sorted = false;
}

void check_params(const kslam_consensus_params &p) {
  if (p.min_depth < 1) throw StatusError{KSLAM_ERR_ARG, "consensus: min_depth must be at least 1"};
  if (p.call_permille < 500 || p.call_permille > 999) throw StatusError{KSLAM_ERR_ARG, "consensus: call_permille must lie in 500 .. 999"};
  if (p.fill != KSLAM_CONSENSUS_FILL_N && p.fill != KSLAM_CONSENSUS_FILL_REF) throw StatusError{KSLAM_ERR_ARG, "consensus: fill must be N (0) or REF (1)"};
}

// One batch into owner's state: counted on W / s without the lock (the work buffers are the caller's own), appended under it.
// The write pass has finished when the lock is let go, so that whoever grows the arrays next copies complete keys.
void emit(kslam_ctx *owner, const VariantInputs &in, EmitWork &W, hipStream_t s, bool locked) {
  consensus_count_device(in, W, s);
  kslam_ctx::Consensus &v = owner->cns;
  std::unique_lock<std::mutex> lk(v.mu, std::defer_lock);
  if (!locked) lk.lock();
  if (!v.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the consensus was switched off while a batch was in flight"};
  for (int kind = 0; kind < CNS_KINDS; kind++)
    if (W.n[kind] > CNS_MAX_KEYS - v.n[kind])
      throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^32 - 1 stored events, intervals or insertions (the radix sort's limit): the batch was not added"};
  auto room = [&](DevBuf &b, int kind, size_t bytes) { ensure_keep(b, (v.n[kind] + W.n[kind] + 1) * bytes, v.n[kind] * bytes, s); };
  room(v.ev, CNS_EV, 8);
  room(v.mb, CNS_M, 8);
  room(v.me, CNS_M, 8);
  room(v.db, CNS_D, 8);
  room(v.de, CNS_D, 8);
  room(v.ins, CNS_INS, 16);
  const ConsensusKeys at{v.ev.as<uint64_t>() + v.n[CNS_EV], v.mb.as<uint64_t>() + v.n[CNS_M], v.me.as<uint64_t>() + v.n[CNS_M],
                         v.db.as<uint64_t>() + v.n[CNS_D], v.de.as<uint64_t>() + v.n[CNS_D], v.ins.as<uint64_t>() + 2 * v.n[CNS_INS]};
  consensus_write_device(in, W, at, s);
  bool any = false;
  for (int kind = 0; kind < CNS_KINDS; kind++) {
    v.n[kind] += W.n[kind];
    any = any || W.n[kind];
  }
  v.n_records += W.n_list;
  v.n_skipped += W.n_skipped;
  v.n_unanchored += W.n_unanchored;
  v.n_unrepresentable += W.n_unrepresentable;
  if (any) v.sorted = false;
}

}  // namespace

void consensus_release(kslam_ctx *c) {
  kslam_ctx::Consensus &v = c->cns;
  std::lock_guard<std::mutex> lk(v.mu);
  v.on.store(false, std::memory_order_release);
  ConsensusTakeWork &T = v.tw;
  for (DevBuf *b : {&v.ev, &v.mb, &v.me, &v.db, &v.de, &v.ins, &T.alt, &T.tflag, &T.tpos, &T.tlist, &T.tstart, &T.obase, &T.len, &T.off, &T.call, &T.insidx,
                    &T.counters, &T.seq, &T.scan_tmp, &T.totals, &T.sortws.hist, &T.sortws.status, &T.sortws.tickets, &T.sortws.digits})
    b->release();
  v.up.release_all();
  empty_state(v);
  v.n_entries = v.total_bases = 0;
  v.slice = KSLAM_CONSENSUS_DEFAULT_SLICE;
}

void consensus_emit_resident(kslam_ctx *owner, kslam_ctx *lane) {
  const GenomeIndex &ix = lane->need_index();
  if (ix.n_entries != owner->cns.n_entries) throw StatusError{KSLAM_ERR_STATE, "the consensus was laid out for another index"};
  emit(owner, resident_inputs(lane, ix, true), lane->cnsw, lane->stream, false);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_consensus(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (refused_in_multi(c, REPORT_IS)) throw StatusError{KSLAM_ERR_UNSUPPORTED, c->err};
    if (!on) {
      if (c->cns.on.load(std::memory_order_acquire)) wait_for_lanes(c);
      consensus_release(c);
      return;
    }
    const GenomeIndex &ix = c->need_index();
    if (!c->pairing.stages) throw StatusError{KSLAM_ERR_STATE, "kslam_set_consensus needs the device pairing: call kslam_set_pairing first"};
    if (!c->prm.report_cigar) throw StatusError{KSLAM_ERR_STATE, "kslam_set_consensus needs the CIGARs: create the context with report_cigar != 0"};
    kslam_ctx::Consensus &v = c->cns;
    std::lock_guard<std::mutex> lk(v.mu);
    if (v.on.load(std::memory_order_acquire)) return;
    if (ix.h_goff[ix.n_entries] >= (1ull << 57)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^57 or more bases in the index"};
    v.n_entries = ix.n_entries;
    v.total_bases = ix.h_goff[ix.n_entries];
    empty_state(v);
    if (!v.ev_take[0])
      for (auto &e : v.ev_take) HIPCHK(hipEventCreate(&e));
    v.take_ms = 0;
    v.on.store(true, std::memory_order_release);
  });
}

kslam_status kslam_get_consensus(kslam_ctx *c, int *on) { return get_switch(c, &kslam_ctx::cns, on); }

kslam_status kslam_consensus_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->cns.mu);
    need_on(c->cns.on, SWITCHED_OFF);
    wait_for_lanes(c);
    empty_state(c->cns);
  });
}

kslam_status kslam_consensus_set_slice(kslam_ctx *c, uint64_t slice) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->cns.mu);
    need_on(c->cns.on, SWITCHED_OFF);
    c->cns.slice = !slice ? KSLAM_CONSENSUS_DEFAULT_SLICE : std::min(slice, CNS_MAX_SLICE);
  });
}

kslam_status kslam_consensus_add(kslam_ctx *c, const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                                 const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads, const kslam_read_pair *read_pairs,
                                 uint64_t n_read_pairs, const kslam_paired_overlap *pairs, uint64_t n_pairs) {
  return guarded(c, [&] {
    if ((n_overlaps && !overlaps) || (n_cigar && !cigar_pool) || (n_reads && !read_offsets) || (n_read_pairs && !read_pairs) || (n_pairs && !pairs))
      throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::Consensus &v = c->cns;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->cns.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    const uint64_t n_rbytes = n_reads ? read_offsets[n_reads] : 0;
    if (n_rbytes && !read_bases) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    // nothing is launched for arrays that do not hold together
    const kslam_batch::Arrays batch{overlaps, n_overlaps, n_cigar, read_offsets, n_reads, read_pairs, n_read_pairs, pairs, n_pairs};
    const std::string fault = kslam_batch::check(batch, kslam_batch::Level::records);
    if (!fault.empty()) throw StatusError{KSLAM_ERR_ARG, fault};
    hipStream_t s = c->stream;
    const VariantInputs in = v.up.upload(batch, kslam_batch::Level::records, cigar_pool, BatchUpload::bases, read_bases, nullptr, &ix, s);
    emit(c, in, c->cnsw, s, true);
  });
}

kslam_status kslam_consensus_take(kslam_ctx *c, const kslam_consensus_params *params, kslam_consensus_row **rows, uint64_t *n_rows, char **seq,
                                  kslam_consensus_stats *stats) {
  if (seq) *seq = nullptr;
  char *h_seq = nullptr;
  const kslam_status st = take_rows(c, rows, n_rows, stats, [&](kslam_consensus_row *&h) {
    if (!params || !seq) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    check_params(*params);
    kslam_ctx::Consensus &v = c->cns;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->cns.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    wait_for_lanes(c);
    hipStream_t s = c->stream;
    HIPCHK(hipEventRecord(v.ev_take[0], s));
    if (!v.sorted) consensus_sort_device(v.tw, v.ev, v.mb, v.me, v.db, v.de, v.ins, v.n, v.total_bases, s);
    v.sorted = true;
    const ConsensusKeys K{v.ev.as<uint64_t>(), v.mb.as<uint64_t>(), v.me.as<uint64_t>(), v.db.as<uint64_t>(), v.de.as<uint64_t>(), v.ins.as<uint64_t>()};
    ConsensusCall call;
    consensus_take_device(v.tw, K, v.n, ix.g_off.as<uint64_t>(), ix.g_bases.as<uint8_t>(), ix.h_goff, ix.n_entries, *params, v.slice, call, s);
    HIPCHK(hipEventRecord(v.ev_take[1], s));
    const uint64_t n = call.rows.size();
    h = (kslam_consensus_row *)pinned_get(c, (n + 1) * sizeof(kslam_consensus_row));
    h_seq = (char *)pinned_get(c, call.seq_bytes + 1);
    if (n) memcpy(h, call.rows.data(), n * sizeof(kslam_consensus_row));
    if (call.seq_bytes) HIPCHK(hipMemcpyAsync(h_seq, v.tw.seq.p, call.seq_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, v.ev_take[0], v.ev_take[1]));
    v.take_ms = ms;
    *n_rows = n;
    stats->n_records = v.n_records;
    stats->n_skipped = v.n_skipped;
    stats->n_intervals = v.n[CNS_M];
    stats->n_del_intervals = v.n[CNS_D];
    stats->n_events = v.n[CNS_EV];
    stats->n_insertions = v.n[CNS_INS];
    stats->n_ins_unanchored = v.n_unanchored;
    stats->n_ins_unrepresentable = v.n_unrepresentable;
    stats->n_entries_touched = call.n_touched;
    stats->n_entries_reported = n;
  });
  if (st != KSLAM_OK) {
    if (h_seq) pinned_put(c, h_seq);
    return st;
  }
  *seq = h_seq;
  return KSLAM_OK;
}

kslam_status kslam_consensus_kernel_ms(kslam_ctx *c, double *emit_ms, double *take_ms) {
  if (!c || !emit_ms || !take_ms) return KSLAM_ERR_ARG;
  *emit_ms = c->cnsw.ms;
  *take_ms = c->cns.take_ms;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_consensus(kslam_ctx *c, int fd, const kslam_consensus_params *params) {
  if (!c) return KSLAM_ERR_ARG;
  if (refused_in_multi(c, REPORT_IS)) return KSLAM_ERR_UNSUPPORTED;
  const kslam_consensus_params p = params ? *params : kslam_consensus_params{1, 500, KSLAM_CONSENSUS_FILL_N, 1};
  const kslam_status st = guarded(c, [&] { check_params(p); });
  if (st != KSLAM_OK) return st;
  c->cns.stream_fd = fd >= 0 ? fd : -1;
  c->cns.stream_params = p;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_consensus(kslam_ctx *c, int *fd, kslam_consensus_params *params) {
  if (!c || !fd || !params) return KSLAM_ERR_ARG;
  *fd = c->cns.stream_fd;
  *params = c->cns.stream_params;
  return KSLAM_OK;
}

}  // extern "C"
