// api_kreport.hip -- the C ABI, part 10: the Kraken-style report's counts (include/kslam_kreport.h; kernels: kreport.hip).  The
// state lives on the context the switch was set on; its lanes call kreport_count_resident on the taxonomy ids they have just
// computed, kslam_kreport_add takes ids from the host, kslam_kreport_take sums the clades and hands the rows over.
#include "context.h"

namespace kslam_api {

namespace {

constexpr uint64_t KR_MAX_ITEMS = 0xFFFFFFFFull;   // the radix sort's limit

KreportTable table_of(const kslam_ctx *owner) {
  const kslam_ctx::Kreport &v = owner->kr;
  return KreportTable{v.direct.as<unsigned long long>(), v.keys.as<uint32_t>(), v.nodes.as<uint32_t>(), v.n_nodes};
}

const char *const REPORT_IS = "the Kraken-style report is";
const char *const SWITCHED_OFF = "the report is switched off: call kslam_set_kreport first";

void zero_state(kslam_ctx *c) {
  kslam_ctx::Kreport &v = c->kr;
  HIPCHK(hipMemsetAsync(v.direct.p, 0, (v.n_nodes + 1) * sizeof(uint64_t), c->stream));
  HIPCHK(stream_wait(c->stream));
  v.n_items = 0;
}

// n device ids into owner's state with W on stream s; under owner->kr.mu.  The refusal comes before anything is written.
void count_locked(kslam_ctx *owner, const uint32_t *d_ids, uint64_t n, KreportCountWork &W, hipStream_t s) {
  kslam_ctx::Kreport &v = owner->kr;
  const KreportTable T = table_of(owner);
  if (n > KR_MAX_ITEMS - v.n_items) {   // the list could overflow: count the call's items first
    kreport_count_device(d_ids, n, T, W, true, s);
    if (W.n_new > KR_MAX_ITEMS - v.n_items)
      throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^32 - 1 items for ids the tree does not know (the radix sort's limit): the batch was not counted"};
  }
  kreport_count_device(d_ids, n, T, W, false, s);
  if (!W.n_new) return;
  ensure_keep(v.items, (v.n_items + W.n_new + 1) * sizeof(uint64_t), v.n_items * sizeof(uint64_t), s);
  HIPCHK(hipMemcpyAsync(v.items.as<uint64_t>() + v.n_items, W.items.p, W.n_new * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  HIPCHK(stream_wait(s));
  v.n_items += W.n_new;
}

}  // namespace

// the id -> node table of c's device tree: the tree's ids sorted ascending with their nodes (once per switch-on, on the host);
// for the report's count pass and for the reads of chosen taxa (api_taxreads.hip), each into buffers of its own
void id_node_table(kslam_ctx *c, DevBuf &d_keys, DevBuf &d_nodes) {
  const uint64_t N = c->annot.n_nodes;
  if (N >= (1ull << 32)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^32 or more taxonomy nodes"};
  std::vector<uint32_t> tax(N + 1), order(N + 1), keys(N + 1);
  if (N) HIPCHK(hipMemcpyAsync(tax.data(), c->annot.node_tax, N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(stream_wait(c->stream));
  for (uint64_t n = 0; n < N; n++) order[n] = (uint32_t)n;
  std::sort(order.begin(), order.begin() + N, [&](uint32_t a, uint32_t b) { return tax[a] != tax[b] ? tax[a] < tax[b] : a < b; });
  for (uint64_t n = 0; n < N; n++) keys[n] = tax[order[n]];
  d_keys.ensure((N + 1) * sizeof(uint32_t));
  d_nodes.ensure((N + 1) * sizeof(uint32_t));
  if (N) HIPCHK(hipMemcpyAsync(d_keys.p, keys.data(), N * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  if (N) HIPCHK(hipMemcpyAsync(d_nodes.p, order.data(), N * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(stream_wait(c->stream));   // (the vectors may go)
}

void kreport_release(kslam_ctx *c) {
  kslam_ctx::Kreport &v = c->kr;
  std::lock_guard<std::mutex> lk(v.mu);
  v.on.store(false, std::memory_order_release);
  for (DevBuf *b : {&v.direct, &v.keys, &v.nodes, &v.items, &v.up_ids, &v.tw.clade, &v.tw.flag, &v.tw.pos, &v.tw.keys_a, &v.tw.keys_b, &v.tw.head,
                    &v.tw.run, &v.tw.rows})
    b->release();
  v.n_nodes = v.n_items = 0;
}

void kreport_count_resident(kslam_ctx *owner, kslam_ctx *lane, uint64_t n) {
  kslam_ctx::Kreport &v = owner->kr;
  std::lock_guard<std::mutex> lk(v.mu);
  if (!v.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the report was switched off while a batch was in flight"};
  if (owner->annot.n_nodes != v.n_nodes) throw StatusError{KSLAM_ERR_STATE, "the report's state was laid out for another taxonomy tree"};
  count_locked(owner, lane->samw.tax_ids.as<uint32_t>(), n, lane->krw, lane->stream);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_kreport(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (refused_in_multi(c, REPORT_IS)) throw StatusError{KSLAM_ERR_UNSUPPORTED, c->err};
    if (!on) {
      if (c->kr.on.load(std::memory_order_acquire)) wait_for_lanes(c);
      kreport_release(c);
      return;
    }
    if (!c->have_annot || !c->annot.up)
      throw StatusError{KSLAM_ERR_STATE, "kslam_set_kreport needs a taxonomy tree on the device: call kslam_set_sam_annotations with a taxdb first"};
    kslam_ctx::Kreport &v = c->kr;
    std::lock_guard<std::mutex> lk(v.mu);
    if (v.on.load(std::memory_order_acquire)) return;
    const uint64_t N = c->annot.n_nodes;
    if (N >= (1ull << 32)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^32 or more taxonomy nodes"};
    v.n_nodes = N;
    try {
      v.direct.ensure((N + 1) * sizeof(uint64_t));
      id_node_table(c, v.keys, v.nodes);
      zero_state(c);
      if (!v.ev_take[0])
        for (auto &e : v.ev_take) HIPCHK(hipEventCreate(&e));
    } catch (...) {
      for (DevBuf *b : {&v.direct, &v.keys, &v.nodes}) b->release();
      v.n_nodes = 0;
      throw;
    }
    v.take_ms = 0;
    v.on.store(true, std::memory_order_release);
  });
}

kslam_status kslam_get_kreport(kslam_ctx *c, int *on) { return get_switch(c, &kslam_ctx::kr, on); }

kslam_status kslam_kreport_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->kr.mu);
    need_on(c->kr.on, SWITCHED_OFF);
    wait_for_lanes(c);
    zero_state(c);
  });
}

kslam_status kslam_kreport_add(kslam_ctx *c, const uint32_t *tax_ids, uint64_t n) {
  return guarded(c, [&] {
    if (n && !tax_ids) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::Kreport &v = c->kr;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->kr.on, SWITCHED_OFF);
    if (!n) {
      c->krw.ms = 0;
      return;
    }
    hipStream_t s = c->stream;
    v.up_ids.ensure((n + 1) * sizeof(uint32_t));
    HIPCHK(hipMemcpyAsync(v.up_ids.p, tax_ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIPCHK(stream_wait(s));   // (a pageable source: the caller's array is free again)
    count_locked(c, v.up_ids.as<uint32_t>(), n, c->krw, s);
  });
}

kslam_status kslam_kreport_take(kslam_ctx *c, kslam_kreport_row **rows, uint64_t *n_rows, kslam_kreport_stats *stats) {
  return take_rows(c, rows, n_rows, stats, [&](kslam_kreport_row *&h) {
    kslam_ctx::Kreport &v = c->kr;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->kr.on, SWITCHED_OFF);
    if (!c->annot.up || c->annot.n_nodes != v.n_nodes) throw StatusError{KSLAM_ERR_STATE, "the report's state was laid out for another taxonomy tree"};
    wait_for_lanes(c);
    hipStream_t s = c->stream;
    uint64_t n_known = 0, n_unknown = 0;
    kreport_take_device(table_of(c), c->annot.up, c->annot.depth, c->annot.node_tax, v.items.as<uint64_t>(), v.n_items, v.tw, &n_known, &n_unknown,
                        v.ev_take, s);
    const uint64_t n = n_known + n_unknown;
    h = (kslam_kreport_row *)pinned_get(c, (n + 1) * sizeof(kslam_kreport_row));
    if (n) HIPCHK(hipMemcpyAsync(h, v.tw.rows.p, n * sizeof(kslam_kreport_row), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, v.ev_take[0], v.ev_take[1]));
    v.take_ms = ms;
    uint64_t n_ids = 0;   // every id counted sits in some row's direct count
    for (uint64_t i = 0; i < n; i++) n_ids += h[i].direct;
    stats->n_ids = n_ids;
    stats->n_unknown_ids = n_unknown;
    stats->n_rows = n;
    *n_rows = n;
  });
}

kslam_status kslam_kreport_kernel_ms(kslam_ctx *c, double *add_ms, double *take_ms) {
  if (!c || !add_ms || !take_ms) return KSLAM_ERR_ARG;
  *add_ms = c->krw.ms;
  *take_ms = c->kr.take_ms;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_kreport(kslam_ctx *c, int fd) {
  if (!c) return KSLAM_ERR_ARG;
  if (refused_in_multi(c, REPORT_IS)) return KSLAM_ERR_UNSUPPORTED;
  c->kr.stream_fd = fd >= 0 ? fd : -1;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_kreport(kslam_ctx *c, int *fd) {
  if (!c || !fd) return KSLAM_ERR_ARG;
  *fd = c->kr.stream_fd;
  return KSLAM_OK;
}

}  // extern "C"
