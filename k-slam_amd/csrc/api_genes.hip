// api_genes.hip -- the C ABI, part 13: the per-gene abundance table (include/kslam_genes.h; kernels: genes.hip).  The state
// lives on the context the switch was set on; its lanes call genes_count_resident on the batch they have just finished,
// kslam_genes_add takes a batch's arrays from the host, kslam_genes_take compacts the counted rows and hands them over.
#include "context.h"

namespace kslam_api {

namespace {

GeneTable table_of(const kslam_ctx *owner) {
  const kslam_ctx::Genes &v = owner->gen;
  const SamAnnot &A = owner->annot;
  return GeneTable{v.n_entries, v.n_genes, A.gene_first, A.gene_start, A.gene_stop, v.order.as<uint32_t>(), v.sstart.as<int32_t>(),
                   v.sstop.as<int32_t>(), v.runmax.as<int32_t>(), v.rows.as<unsigned long long>(), v.stats.as<unsigned long long>()};
}

const char *const REPORT_IS = "the gene table is";
const char *const SWITCHED_OFF = "the gene table is switched off: call kslam_set_genes first";

// the annotations the state was laid out for are still the context's
void need_same_annotations(const kslam_ctx *c) {
  if (!c->have_annot || c->annot.n_entries != c->gen.n_entries || c->annot.n_genes != c->gen.n_genes)
    throw StatusError{KSLAM_ERR_STATE, "the gene table was laid out for other annotations"};
}

void zero_state(kslam_ctx *c) {
  kslam_ctx::Genes &v = c->gen;
  HIPCHK(hipMemsetAsync(v.rows.p, 0, (v.n_genes + 1) * 4 * sizeof(uint64_t), c->stream));
  HIPCHK(hipMemsetAsync(v.stats.p, 0, 4 * sizeof(uint64_t), c->stream));
  HIPCHK(stream_wait(c->stream));
}

// measurement and cross-check: KSLAM_GENES_LOOKUP=linear makes the count pass walk all genes of the entry (the same rows)
bool linear_lookup() {
  const char *e = getenv("KSLAM_GENES_LOOKUP");
  return e && strcmp(e, "linear") == 0;
}

void release_buffers(kslam_ctx::Genes &v) {
  for (DevBuf *b : {&v.order, &v.sstart, &v.sstop, &v.runmax, &v.rows, &v.stats, &v.lk_in, &v.lk_out, &v.tw.flag, &v.tw.pos,
                    &v.tw.rows, &v.tw.scan_tmp, &v.tw.totals})
    b->release();
  v.up.release_all();
  v.n_entries = v.n_genes = 0;
}

}  // namespace

void genes_release(kslam_ctx *c) {
  kslam_ctx::Genes &v = c->gen;
  std::lock_guard<std::mutex> lk(v.mu);
  v.on.store(false, std::memory_order_release);
  release_buffers(v);
}

void genes_count_resident(kslam_ctx *owner, kslam_ctx *lane) {
  const GenomeIndex &ix = lane->need_index();
  kslam_ctx::Genes &v = owner->gen;
  GeneTable table;
  {   // the pass runs without the lock (the work buffers are the lane's own, the counts are atomics): the lanes do not wait for each
      // other; the switch is set between batches and waits for the lanes' streams before it frees anything
    std::lock_guard<std::mutex> lk(v.mu);
    if (!v.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the gene table was switched off while a batch was in flight"};
    need_same_annotations(owner);
    if (ix.n_entries != v.n_entries) throw StatusError{KSLAM_ERR_STATE, "the gene table was laid out for another index"};
    table = table_of(owner);
  }
  const VariantInputs in = resident_inputs(lane, ix, false);
  genes_count_device(in.groups, in.n_groups, in.pairs, in.n_pairs, table, lane->genw, linear_lookup(), lane->stream);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_genes(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (refused_in_multi(c, REPORT_IS)) throw StatusError{KSLAM_ERR_UNSUPPORTED, c->err};
    if (!on) {
      if (c->gen.on.load(std::memory_order_acquire)) wait_for_lanes(c);
      genes_release(c);
      return;
    }
    const GenomeIndex &ix = c->need_index();
    if (!c->pairing.stages) throw StatusError{KSLAM_ERR_STATE, "kslam_set_genes needs the device pairing: call kslam_set_pairing first"};
    if (!c->have_annot) throw StatusError{KSLAM_ERR_STATE, "kslam_set_genes needs the gene columns on the device: call kslam_set_sam_annotations first"};
    kslam_ctx::Genes &v = c->gen;
    std::lock_guard<std::mutex> lk(v.mu);
    if (v.on.load(std::memory_order_acquire)) return;
    const SamAnnot &A = c->annot;
    const uint64_t E = A.n_entries, G = A.n_genes;
    if (E != ix.n_entries) throw StatusError{KSLAM_ERR_STATE, "the annotations belong to another index"};
    if (G >= 0xFFFFFFFEull) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^32 - 2 or more genes"};
    hipStream_t s = c->stream;
    if (G) {   // every kernel takes an entry's genes from gene_first: it must ascend from 0 to n_genes
      std::vector<uint64_t> first(E + 1);
      HIPCHK(hipMemcpyAsync(first.data(), A.gene_first, (E + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
      HIPCHK(stream_wait(s));
      bool ok = E > 0 && first[0] == 0 && first[E] == G;
      for (uint64_t e = 0; ok && e < E; e++) ok = first[e] <= first[e + 1];
      if (!ok) throw StatusError{KSLAM_ERR_ARG, "the annotations' gene_first does not ascend from 0 to n_genes"};
    }
    v.n_entries = E;
    v.n_genes = G;
    try {
      v.order.ensure((G + 1) * sizeof(uint32_t));
      v.sstart.ensure((G + 1) * sizeof(int32_t));
      v.sstop.ensure((G + 1) * sizeof(int32_t));
      v.runmax.ensure((G + 1) * sizeof(int32_t));
      v.rows.ensure((G + 1) * 4 * sizeof(uint64_t));
      v.stats.ensure(4 * sizeof(uint64_t));
      float ms = 0;
      genes_build_device(E, G, A.gene_first, A.gene_start, A.gene_stop, v.order.as<uint32_t>(), v.sstart.as<int32_t>(), v.sstop.as<int32_t>(),
                         v.runmax.as<int32_t>(), &ms, s);
      v.build_ms = ms;
      zero_state(c);
      if (!v.ev_take[0])
        for (auto &e : v.ev_take) HIPCHK(hipEventCreate(&e));
    } catch (...) {
      release_buffers(v);
      throw;
    }
    v.take_ms = 0;
    v.on.store(true, std::memory_order_release);
  });
}

kslam_status kslam_get_genes(kslam_ctx *c, int *on) { return get_switch(c, &kslam_ctx::gen, on); }

kslam_status kslam_genes_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->gen.mu);
    need_on(c->gen.on, SWITCHED_OFF);
    wait_for_lanes(c);
    zero_state(c);
  });
}

kslam_status kslam_genes_add(kslam_ctx *c, const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                             uint64_t n_pairs) {
  return guarded(c, [&] {
    if ((n_read_pairs && !read_pairs) || (n_pairs && !pairs)) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::Genes &v = c->gen;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->gen.on, SWITCHED_OFF);
    need_same_annotations(c);
    // nothing is launched for arrays that do not hold together
    const kslam_batch::Arrays batch{nullptr, 0, 0, nullptr, 0, read_pairs, n_read_pairs, pairs, n_pairs};
    const std::string fault = kslam_batch::check(batch, kslam_batch::Level::groups);
    if (!fault.empty()) throw StatusError{KSLAM_ERR_ARG, fault};
    hipStream_t s = c->stream;
    const VariantInputs in = v.up.upload(batch, kslam_batch::Level::groups, nullptr, BatchUpload::no_columns, nullptr, nullptr, nullptr, s);
    genes_count_device(in.groups, in.n_groups, in.pairs, in.n_pairs, table_of(c), c->genw, linear_lookup(), s);
  });
}

kslam_status kslam_genes_take(kslam_ctx *c, kslam_gene_row **rows, uint64_t *n_rows, kslam_gene_stats *stats) {
  return take_rows(c, rows, n_rows, stats, [&](kslam_gene_row *&h) {
    kslam_ctx::Genes &v = c->gen;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->gen.on, SWITCHED_OFF);
    need_same_annotations(c);
    wait_for_lanes(c);
    hipStream_t s = c->stream;
    uint64_t n = 0;
    genes_take_device(table_of(c), v.tw, &n, v.ev_take, s);
    h = (kslam_gene_row *)pinned_get(c, (n + 1) * sizeof(kslam_gene_row));
    if (n) HIPCHK(hipMemcpyAsync(h, v.tw.rows.p, n * sizeof(kslam_gene_row), hipMemcpyDeviceToHost, s));
    uint64_t counters[4] = {0, 0, 0, 0};
    read_back(counters, v.stats.p, sizeof counters, s);   // (waits for the stream)
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, v.ev_take[0], v.ev_take[1]));
    v.take_ms = ms;
    stats->n_alignments = counters[0];
    stats->n_in_gene = counters[1];
    stats->n_no_gene = counters[2];
    stats->n_skipped = counters[3];
    stats->n_rows = n;
    *n_rows = n;
  });
}

kslam_status kslam_genes_lookup(kslam_ctx *c, const uint32_t *entries, const int32_t *starts, const int32_t *stops, uint64_t n, int64_t *genes_out,
                                int64_t *shared_out, int linear) {
  return guarded(c, [&] {
    if (n && (!entries || !starts || !stops || !genes_out)) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    if (n >= (1ull << 32)) throw StatusError{KSLAM_ERR_ARG, "2^32 triples or more"};
    kslam_ctx::Genes &v = c->gen;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->gen.on, SWITCHED_OFF);
    need_same_annotations(c);
    if (!n) return;
    hipStream_t s = c->stream;
    v.lk_in.ensure(3 * n * sizeof(uint32_t));
    v.lk_out.ensure(2 * n * sizeof(int64_t));
    uint32_t *d_in = v.lk_in.as<uint32_t>();
    int64_t *d_out = v.lk_out.as<int64_t>();
    HIPCHK(hipMemcpyAsync(d_in, entries, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_in + n, starts, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_in + 2 * n, stops, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    genes_lookup_device(d_in, reinterpret_cast<const int32_t *>(d_in + n), reinterpret_cast<const int32_t *>(d_in + 2 * n), n, table_of(c), linear != 0,
                        d_out, d_out + n, s);
    HIPCHK(hipMemcpyAsync(genes_out, d_out, n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (shared_out) HIPCHK(hipMemcpyAsync(shared_out, d_out + n, n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
  });
}

kslam_status kslam_genes_kernel_ms(kslam_ctx *c, double *build_ms, double *count_ms, double *take_ms) {
  if (!c || !build_ms || !count_ms || !take_ms) return KSLAM_ERR_ARG;
  *build_ms = c->gen.build_ms;
  *count_ms = c->genw.ms;
  *take_ms = c->gen.take_ms;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_genes(kslam_ctx *c, int fd) {
  if (!c) return KSLAM_ERR_ARG;
  if (refused_in_multi(c, REPORT_IS)) return KSLAM_ERR_UNSUPPORTED;
  c->gen.stream_fd = fd >= 0 ? fd : -1;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_genes(kslam_ctx *c, int *fd) {
  if (!c || !fd) return KSLAM_ERR_ARG;
  *fd = c->gen.stream_fd;
  return KSLAM_OK;
}

}  // extern "C"
