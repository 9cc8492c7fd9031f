// api_readsplit.hip -- the C ABI, part 7: the reads split by outcome (include/kslam_readsplit.h; kernels: readsplit.hip).  The lanes
// call split_resident on the batch they have just finished; kslam_collect_reads_out hands the blocks over, by ticket.
#include "context.h"

namespace kslam_api {

void free_reads_out(kslam_ctx *c, kslam_reads_out *out) {
  for (int k = 0; k < 4; k++) {
    if (out->data[k]) kslam_free_pinned(c, out->data[k]);
    out->data[k] = nullptr;
    out->len[k] = 0;
  }
}

void split_resident(kslam_ctx *c, bool single, const kslam_read_pair *d_groups, uint64_t n_groups, uint32_t which, bool bgzf, int deflate,
                    kslam_reads_out *out) {
  memset(out, 0, sizeof *out);
  uint64_t bytes[4];
  read_split_device(c->fqw.st, single, d_groups, n_groups, which, c->rsw, bytes, out->n_records, c->stream);
  out->flags = bgzf ? KSLAM_READS_OUT_BGZF : 0u;
  try {
    for (int k = 0; k < 4; k++) {
      const bool wanted = (which & (k < 2 ? KSLAM_READS_OUT_CLASSIFIED : KSLAM_READS_OUT_UNCLASSIFIED)) && !(single && (k & 1));
      if (!wanted) continue;
      const void *d_src = c->rsw.out[k].p;
      uint64_t len = bytes[k];
      if (bgzf) {   // the stream's members; the copy below is waited for before the next stream reuses bgzf_out
        bgzf_compress_device(c->rsw.out[k].as<char>(), bytes[k], deflate, c->bgzfw, c->bgzf_out, &len, c->stream);
        d_src = c->bgzf_out.p;
      }
      out->data[k] = (char *)pinned_get(c, len + 1);
      out->len[k] = len;
      if (len) HIPCHK(hipMemcpyAsync(out->data[k], d_src, len, hipMemcpyDeviceToHost, c->stream));
      if (bgzf) HIPCHK(stream_wait(c->stream));
    }
    HIPCHK(stream_wait(c->stream));
  } catch (...) {
    (void)stream_wait(c->stream);
    free_reads_out(c, out);
    throw;
  }
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_reads_out(kslam_ctx *c, uint32_t which) {
  return guarded(c, [&] {
    if (c->in_multi) throw StatusError{KSLAM_ERR_UNSUPPORTED, "the reads split is not available on the contexts of a kslam_multi"};
    if (which > 3u) throw StatusError{KSLAM_ERR_ARG, "unknown bits in the reads-out mask"};
    if (which && !c->pairing.stages) throw StatusError{KSLAM_ERR_STATE, "kslam_set_reads_out needs the device pairing: call kslam_set_pairing first"};
    c->reads_out.which = which;
  });
}

kslam_status kslam_get_reads_out(kslam_ctx *c, uint32_t *which) {
  if (!c || !which) return KSLAM_ERR_ARG;
  *which = c->reads_out.which;
  return KSLAM_OK;
}

kslam_status kslam_set_reads_out_bgzf(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (c->in_multi) throw StatusError{KSLAM_ERR_UNSUPPORTED, "the reads split is not available on the contexts of a kslam_multi"};
    c->reads_out.bgzf = on != 0;
  });
}

kslam_status kslam_get_reads_out_bgzf(kslam_ctx *c, int *on) {
  if (!c || !on) return KSLAM_ERR_ARG;
  *on = c->reads_out.bgzf ? 1 : 0;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_reads_out(kslam_ctx *c, const int fds[4]) {
  if (!c) return KSLAM_ERR_ARG;
  if (c->in_multi) { c->err = "the reads split is not available on the contexts of a kslam_multi"; return KSLAM_ERR_UNSUPPORTED; }
  for (int k = 0; k < 4; k++) c->reads_out.fds[k] = fds && fds[k] >= 0 ? fds[k] : -1;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_reads_out(kslam_ctx *c, int fds[4]) {
  if (!c || !fds) return KSLAM_ERR_ARG;
  for (int k = 0; k < 4; k++) fds[k] = c->reads_out.fds[k];
  return KSLAM_OK;
}

kslam_status kslam_collect_reads_out(kslam_ctx *c, uint64_t ticket, kslam_reads_out *out) {
  if (!c || !out) return KSLAM_ERR_ARG;
  memset(out, 0, sizeof *out);
  std::lock_guard<std::mutex> lk(c->as_mu);
  auto it = c->ro_ready.find(ticket);
  if (it == c->ro_ready.end()) {
    c->err = "no streams for this ticket: not collected yet, collected with kslam_set_reads_out off, or taken already";
    return KSLAM_ERR_STATE;
  }
  const kslam_ctx::ReadsOutEntry e = it->second;
  c->ro_ready.erase(it);
  if (!e.supported) {
    c->err = "the reads split needs a batch submitted with kslam_submit_batch_fastq_text (the text and its index on the device) and the device pairing";
    return KSLAM_ERR_UNSUPPORTED;
  }
  *out = e.out;
  return KSLAM_OK;
}

kslam_status kslam_reads_out_kernel_ms(kslam_ctx *c, double *ms, uint64_t *bytes_moved) {
  if (!c || !ms || !bytes_moved) return KSLAM_ERR_ARG;
  *ms = c->rsw.kernel_ms;
  *bytes_moved = c->rsw.bytes_moved;
  return KSLAM_OK;
}

kslam_status kslam_split_reads_text(kslam_ctx *c, const char *r1, uint64_t len1, const char *r2, uint64_t len2, uint64_t max_pairs,
                                    int at_eof, const kslam_read_pair *read_pairs, uint64_t n_read_pairs, uint32_t which,
                                    kslam_reads_out *out) {
  if (out) memset(out, 0, sizeof *out);
  return guarded(c, [&] {
    if (!out || (len1 && !r1) || (len2 && !r2) || (n_read_pairs && !read_pairs)) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    if (which == 0 || which > 3u) throw StatusError{KSLAM_ERR_ARG, "the reads-out mask must be 1, 2 or 3"};
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
    DevBuf groups;
    groups.ensure((n_read_pairs + 1) * sizeof(kslam_read_pair));
    if (n_read_pairs) HIPCHK(hipMemcpyAsync(groups.p, read_pairs, n_read_pairs * sizeof(kslam_read_pair), hipMemcpyHostToDevice, s));
    split_resident(c, single, groups.as<kslam_read_pair>(), n_read_pairs, which, c->reads_out.bgzf, c->samtext.deflate, out);
  });
}

}  // extern "C"
