// api_taxreads.hip -- the C ABI, part 11: the reads of chosen taxa (include/kslam_taxreads.h; kernels: taxreads.hip and, for the
// lengths, scans and copy, readsplit.hip).  kslam_set_taxon_reads builds the set S on the device; the lanes call
// taxreads_resident on the batch they have just finished; kslam_collect_taxon_reads hands the blocks over, by ticket.
#include "context.h"

namespace kslam_api {

namespace {

TaxReadsSel sel_of(const kslam_ctx *owner) {
  const kslam_ctx::TaxReads &v = owner->tr;
  return TaxReadsSel{v.keys.as<uint32_t>(), v.nodes.as<uint32_t>(), v.n_nodes, v.mask.as<uint8_t>(), v.unknown.as<uint32_t>(), v.n_unknown, v.all_nonzero};
}

void need_on(const kslam_ctx *c) {
  if (!c->tr.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "no taxa are chosen: call kslam_set_taxon_reads first"};
}

}  // namespace

void taxreads_release(kslam_ctx *c) {
  kslam_ctx::TaxReads &v = c->tr;
  std::lock_guard<std::mutex> lk(v.mu);
  v.on.store(false, std::memory_order_release);
  for (DevBuf *b : {&v.keys, &v.nodes, &v.mask, &v.unknown, &v.up_groups, &v.up_ids, &v.mw.ids, &v.mw.seed, &v.mw.items_a, &v.mw.items_b, &v.mw.head,
                    &v.mw.run, &v.mw.cursor, &v.mw.scan_tmp, &v.mw.totals})
    b->release();
  v.ids.clear();
  v.ids.shrink_to_fit();
  v.mode = 0;
  v.n_nodes = v.n_unknown = 0;
  v.all_nonzero = 0;
}

void taxreads_resident(kslam_ctx *owner, kslam_ctx *c, bool single, const kslam_read_pair *d_groups, const uint32_t *d_ids, uint64_t n_groups,
                       bool bgzf, int deflate, kslam_reads_out *out) {
  memset(out, 0, sizeof *out);
  const kslam_ctx::TaxReads &v = owner->tr;
  if (!v.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the selection was switched off while a batch was in flight"};
  if (owner->annot.n_nodes != v.n_nodes) throw StatusError{KSLAM_ERR_STATE, "the selection was laid out for another taxonomy tree"};
  const bool exclude = (v.mode & KSLAM_TAXREADS_EXCLUDE) != 0;
  const uint32_t which = exclude ? KSLAM_READS_OUT_UNCLASSIFIED : KSLAM_READS_OUT_CLASSIFIED;
  ReadSplitWork &W = c->tr_rsw;
  hipStream_t s = c->stream;
  // the flag pass is this feature's own; the lengths, the scans and the copy are the split's
  const uint64_t n = read_split_prepare(c->fqw.st, single, W, s);
  taxreads_flag_device(d_groups, d_ids, n_groups, single ? 0 : 1, n, sel_of(owner), W.flag.as<uint8_t>(), c->trw, s);
  HIPCHK(hipEventRecord(W.ev[0], s));
  uint64_t bytes[4], n_rec[2];
  read_split_flagged(c->fqw.st, single, which, W, bytes, n_rec, s);   // (waits for the stream)
  taxreads_flag_finish(c->trw, s);
  bool counted = true;
#ifdef KSLAM_ABLATE
  counted = getenv("KSLAM_TAXREADS_ABLATE") == nullptr;   // (measurement only: a pass without its count or without its marks)
#endif
  if (counted && c->trw.n_matched != n_rec[0]) throw StatusError{KSLAM_ERR_INTERNAL, "matched read pairs and flagged records differ: two read pairs name one record"};
  out->n_records[0] = exclude ? n_rec[1] : n_rec[0];
  out->n_records[1] = exclude ? n_rec[0] : n_rec[1];
  out->flags = bgzf ? KSLAM_READS_OUT_BGZF : 0u;
  const int from = exclude ? 2 : 0;
  try {
    for (int k = 0; k < (single ? 1 : 2); k++) {
      const void *d_src = W.out[from + k].p;
      uint64_t len = bytes[from + k];
      if (bgzf) {   // the stream's members; the copy below is waited for before the next stream reuses bgzf_out
        bgzf_compress_device(W.out[from + k].as<char>(), bytes[from + k], deflate, c->bgzfw, c->bgzf_out, &len, s);
        d_src = c->bgzf_out.p;
      }
      out->data[k] = (char *)pinned_get(c, len + 1);
      out->len[k] = len;
      if (len) HIPCHK(hipMemcpyAsync(out->data[k], d_src, len, hipMemcpyDeviceToHost, s));
      if (bgzf) HIPCHK(stream_wait(s));
    }
    HIPCHK(stream_wait(s));
  } catch (...) {
    (void)stream_wait(s);
    free_reads_out(c, out);
    throw;
  }
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_taxon_reads(kslam_ctx *c, const uint32_t *ids, uint64_t n, uint32_t mode) {
  return guarded(c, [&] {
    if (c->in_multi) throw StatusError{KSLAM_ERR_UNSUPPORTED, "the reads of chosen taxa are not available on the contexts of a kslam_multi"};
    if (!n) {
      if (c->tr.on.load(std::memory_order_acquire))
        for (auto *l : c->lanes) HIPCHK(hipStreamSynchronize(l->c->stream));
      taxreads_release(c);
      return;
    }
    if (!ids) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    if (mode > 7u) throw StatusError{KSLAM_ERR_ARG, "unknown bits in the taxon-reads mode"};
    for (uint64_t i = 0; i < n; i++)
      if (!ids[i]) throw StatusError{KSLAM_ERR_ARG, "taxonomy id 0 cannot be chosen: the reads without a taxon are what kslam_set_reads_out gives"};
    if (!c->have_annot || !c->annot.up)
      throw StatusError{KSLAM_ERR_STATE, "kslam_set_taxon_reads needs a taxonomy tree on the device: call kslam_set_sam_annotations with a taxdb first"};
    if (!c->pairing.stages) throw StatusError{KSLAM_ERR_STATE, "kslam_set_taxon_reads needs the device pairing: call kslam_set_pairing first"};
    if (c->tr.on.load(std::memory_order_acquire))
      for (auto *l : c->lanes) HIPCHK(hipStreamSynchronize(l->c->stream));
    taxreads_release(c);
    kslam_ctx::TaxReads &v = c->tr;
    std::lock_guard<std::mutex> lk(v.mu);
    const uint64_t N = c->annot.n_nodes;
    try {
      id_node_table(c, v.keys, v.nodes);
      v.mask.ensure(N + 16);
      if (!v.ev_mask[0])
        for (auto &e : v.ev_mask) HIPCHK(hipEventCreate(&e));
      taxreads_mask_device(ids, n, mode, v.keys.as<uint32_t>(), v.nodes.as<uint32_t>(), N, c->annot.up, c->annot.depth, v.mw, v.mask.as<uint8_t>(),
                           v.unknown, &v.n_unknown, &v.all_nonzero, v.ev_mask, c->stream);
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, v.ev_mask[0], v.ev_mask[1]));
      v.mask_ms = ms;
    } catch (...) {
      for (DevBuf *b : {&v.keys, &v.nodes, &v.mask, &v.unknown}) b->release();
      v.n_unknown = 0;
      v.all_nonzero = 0;
      throw;
    }
    v.ids.assign(ids, ids + n);
    v.mode = mode;
    v.n_nodes = N;
    v.on.store(true, std::memory_order_release);
  });
}

kslam_status kslam_get_taxon_reads(kslam_ctx *c, uint32_t **ids, uint64_t *n, uint32_t *mode) {
  if (!c || !ids || !n || !mode) return KSLAM_ERR_ARG;
  *ids = nullptr;
  *n = 0;
  *mode = 0;
  std::lock_guard<std::mutex> lk(c->tr.mu);
  if (!c->tr.on.load(std::memory_order_acquire)) return KSLAM_OK;
  uint32_t *p = (uint32_t *)malloc(c->tr.ids.size() * sizeof(uint32_t));
  if (!p) { c->err = "host allocation failed"; return KSLAM_ERR_OOM; }
  memcpy(p, c->tr.ids.data(), c->tr.ids.size() * sizeof(uint32_t));
  *ids = p;
  *n = c->tr.ids.size();
  *mode = c->tr.mode;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_taxon_reads(kslam_ctx *c, const int fds[2]) {
  if (!c) return KSLAM_ERR_ARG;
  if (c->in_multi) { c->err = "the reads of chosen taxa are not available on the contexts of a kslam_multi"; return KSLAM_ERR_UNSUPPORTED; }
  for (int k = 0; k < 2; k++) c->tr.fds[k] = fds && fds[k] >= 0 ? fds[k] : -1;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_taxon_reads(kslam_ctx *c, int fds[2]) {
  if (!c || !fds) return KSLAM_ERR_ARG;
  for (int k = 0; k < 2; k++) fds[k] = c->tr.fds[k];
  return KSLAM_OK;
}

kslam_status kslam_collect_taxon_reads(kslam_ctx *c, uint64_t ticket, kslam_reads_out *out) {
  if (!c || !out) return KSLAM_ERR_ARG;
  memset(out, 0, sizeof *out);
  std::lock_guard<std::mutex> lk(c->as_mu);
  auto it = c->tr_ready.find(ticket);
  if (it == c->tr_ready.end()) {
    c->err = "no selected reads for this ticket: not collected yet, collected with kslam_set_taxon_reads off, or taken already";
    return KSLAM_ERR_STATE;
  }
  const kslam_ctx::ReadsOutEntry e = it->second;
  c->tr_ready.erase(it);
  if (!e.supported) {
    c->err = "the reads of chosen taxa need a batch submitted with kslam_submit_batch_fastq_text (the text and its index on the device) and the device pairing";
    return KSLAM_ERR_UNSUPPORTED;
  }
  *out = e.out;
  return KSLAM_OK;
}

kslam_status kslam_taxon_reads_mask(kslam_ctx *c, uint8_t **mask, uint64_t *n_nodes, uint32_t **unknown_ids, uint64_t *n_unknown, int *all_nonzero) {
  if (mask) *mask = nullptr;
  if (unknown_ids) *unknown_ids = nullptr;
  uint8_t *hm = nullptr;
  uint32_t *hu = nullptr;
  const kslam_status st = guarded(c, [&] {
    if (!mask || !n_nodes || !unknown_ids || !n_unknown || !all_nonzero) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::TaxReads &v = c->tr;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c);
    hm = (uint8_t *)malloc(v.n_nodes + 1);
    hu = (uint32_t *)malloc((v.n_unknown + 1) * sizeof(uint32_t));
    if (!hm || !hu) throw StatusError{KSLAM_ERR_OOM, "host allocation failed"};
    if (v.n_nodes) HIPCHK(hipMemcpyAsync(hm, v.mask.p, v.n_nodes, hipMemcpyDeviceToHost, c->stream));
    if (v.n_unknown) HIPCHK(hipMemcpyAsync(hu, v.unknown.p, v.n_unknown * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(stream_wait(c->stream));
    *n_nodes = v.n_nodes;
    *n_unknown = v.n_unknown;
    *all_nonzero = v.all_nonzero;
  });
  if (st != KSLAM_OK) {
    if (c) (void)hipStreamSynchronize(c->stream);
    free(hm);
    free(hu);
    return st;
  }
  *mask = hm;
  *unknown_ids = hu;
  return KSLAM_OK;
}

kslam_status kslam_taxon_reads_kernel_ms(kslam_ctx *c, double *mask_ms, double *flag_ms, double *copy_ms, uint64_t *bytes_moved) {
  if (!c || !mask_ms || !flag_ms || !copy_ms || !bytes_moved) return KSLAM_ERR_ARG;
  *mask_ms = c->tr.mask_ms;
  *flag_ms = c->tr.flag_ms;
  *copy_ms = c->tr.copy_ms;
  *bytes_moved = c->tr.bytes_moved;
  return KSLAM_OK;
}

kslam_status kslam_taxon_reads_text(kslam_ctx *c, const char *r1, uint64_t len1, const char *r2, uint64_t len2, uint64_t max_pairs, int at_eof,
                                    const kslam_read_pair *read_pairs, const uint32_t *pair_tax_ids, uint64_t n_read_pairs, kslam_reads_out *out) {
  if (out) memset(out, 0, sizeof *out);
  return guarded(c, [&] {
    if (!out || (len1 && !r1) || (len2 && !r2) || (n_read_pairs && (!read_pairs || !pair_tax_ids))) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    need_on(c);
    const bool single = r2 == nullptr && len2 == 0;
    hipStream_t s = c->stream;
    c->have_reads = false;   // the resident batch's text is replaced
    c->fq_text.ensure(len1 + len2 + 64);
    if (len1) HIPCHK(hipMemcpyAsync(c->fq_text.p, r1, len1, hipMemcpyHostToDevice, s));
    if (len2) HIPCHK(hipMemcpyAsync(c->fq_text.as<uint8_t>() + len1, r2, len2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(c->fq_text.as<uint8_t>() + len1 + len2, 0, 64, s));
    FastqIndexResult ix;
    fastq_index_device(c->fq_text.as<uint8_t>(), len1, len2, len1 ? (const uint8_t *)r1 + len1 - 1 : nullptr,
                       len2 ? (const uint8_t *)r2 + len2 - 1 : nullptr, max_pairs, at_eof != 0, c->fqw, &ix, s, single);
    kslam_ctx::TaxReads &v = c->tr;
    v.up_groups.ensure((n_read_pairs + 1) * sizeof(kslam_read_pair));
    v.up_ids.ensure((n_read_pairs + 1) * sizeof(uint32_t));
    if (n_read_pairs) {
      HIPCHK(hipMemcpyAsync(v.up_groups.p, read_pairs, n_read_pairs * sizeof(kslam_read_pair), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(v.up_ids.p, pair_tax_ids, n_read_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, s));
      HIPCHK(stream_wait(s));   // (pageable sources: the caller's arrays are free again)
    }
    taxreads_resident(c, c, single, v.up_groups.as<kslam_read_pair>(), v.up_ids.as<uint32_t>(), n_read_pairs, c->reads_out.bgzf, c->samtext.deflate, out);
    v.flag_ms = c->trw.ms;
    v.copy_ms = c->tr_rsw.kernel_ms;
    v.bytes_moved = c->tr_rsw.bytes_moved;
  });
}

}  // extern "C"
