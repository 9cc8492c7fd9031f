// api_alignqc.hip -- the C ABI, part 15: the alignment QC report's tables (include/kslam_alignqc.h; kernels: alignqc.hip).  The
// state lives on the context the switch was set on; its lanes call alignqc_count_resident on the batch they have just finished,
// kslam_align_qc_add takes a batch's arrays from the host, kslam_align_qc_take copies the tables out.
#include "context.h"

namespace kslam_api {

namespace {

AlignQcTable table_of(const kslam_ctx *owner) { return AlignQcTable{owner->aq.words.as<unsigned long long>(), owner->aq.C}; }

const char *const REPORT_IS = "the alignment QC report is";
const char *const SWITCHED_OFF = "the alignment QC report is switched off: call kslam_set_align_qc first";

void zero_state(kslam_ctx *c) {
  alignqc_zero_device(table_of(c), c->stream);
  HIPCHK(stream_wait(c->stream));
  c->aq.paired = false;
}

uint32_t resolve_cycles(uint32_t max_cycles) {
  if (max_cycles > KSLAM_ALIGN_QC_MAX_CYCLES) throw StatusError{KSLAM_ERR_ARG, "max_cycles must be 0 (= 512) or 1 .. 65536"};
  return max_cycles ? max_cycles : KSLAM_ALIGN_QC_DEFAULT_CYCLES;
}

// measurement and cross-check: KSLAM_ALIGNQC_WALK=thread makes the count pass take one thread per record (the same tables)
bool thread_per_record() {
  const char *e = getenv("KSLAM_ALIGNQC_WALK");
  return e && strcmp(e, "thread") == 0;
}

}  // namespace

void alignqc_release(kslam_ctx *c) {
  kslam_ctx::AlignQc &v = c->aq;
  std::lock_guard<std::mutex> lk(v.mu);
  v.on.store(false, std::memory_order_release);
  v.words.release();
  v.up.release_all();
  v.C = 0;
  v.n_entries = 0;
  v.paired = false;
}

void alignqc_count_resident(kslam_ctx *owner, kslam_ctx *lane, bool single) {
  const GenomeIndex &ix = lane->need_index();
  kslam_ctx::AlignQc &v = owner->aq;
  AlignQcTable table;
  {   // the passes run without the lock (the work buffers are the lane's own, the adds are atomics): the lanes do not wait for
      // each other; the switch is set between batches and waits for the lanes' streams before it frees anything
    std::lock_guard<std::mutex> lk(v.mu);
    if (!v.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the alignment QC report was switched off while a batch was in flight"};
    if (ix.n_entries != v.n_entries) throw StatusError{KSLAM_ERR_STATE, "the alignment QC report was switched on for another index"};
    if (!single && (lane->n_reads & 1)) throw StatusError{KSLAM_ERR_INTERNAL, "a paired batch with an odd number of reads"};
    if (!single) v.paired = true;
    table = table_of(owner);
  }
  alignqc_count_device(resident_inputs(lane, ix, true), lane->have_qual ? lane->r_qual.as<uint8_t>() : nullptr, !single, lane->max_read_len, table, lane->aqw, false,
                       thread_per_record(), lane->stream);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_align_qc(kslam_ctx *c, int on, uint32_t max_cycles) {
  return guarded(c, [&] {
    if (refused_in_multi(c, REPORT_IS)) throw StatusError{KSLAM_ERR_UNSUPPORTED, c->err};
    if (!on) {
      if (c->aq.on.load(std::memory_order_acquire)) wait_for_lanes(c);
      alignqc_release(c);
      return;
    }
    const uint32_t C = resolve_cycles(max_cycles);
    const GenomeIndex &ix = c->need_index();
    if (!c->pairing.stages) throw StatusError{KSLAM_ERR_STATE, "kslam_set_align_qc needs the device pairing: call kslam_set_pairing first"};
    if (!c->prm.report_cigar) throw StatusError{KSLAM_ERR_STATE, "kslam_set_align_qc needs the CIGARs: create the context with report_cigar != 0"};
    kslam_ctx::AlignQc &v = c->aq;
    std::lock_guard<std::mutex> lk(v.mu);
    if (v.on.load(std::memory_order_acquire)) {
      if (v.C != C)
        throw StatusError{KSLAM_ERR_STATE, "the alignment QC report is on with max_cycles " + std::to_string(v.C) + ": switch it off before choosing " + std::to_string(C)};
      return;
    }
    v.C = C;
    v.n_entries = ix.n_entries;
    try {
      v.words.ensure(KSLAM_ALIGN_QC_WORDS(C) * sizeof(uint64_t));
      zero_state(c);
    } catch (...) {
      v.words.release();
      v.C = 0;
      v.n_entries = 0;
      throw;
    }
    c->aqw.ms = 0;
    v.on.store(true, std::memory_order_release);
  });
}

kslam_status kslam_get_align_qc(kslam_ctx *c, int *on, uint32_t *max_cycles) { return get_switch(c, &kslam_ctx::aq, on, max_cycles); }

kslam_status kslam_align_qc_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->aq.mu);
    need_on(c->aq.on, SWITCHED_OFF);
    wait_for_lanes(c);
    zero_state(c);
  });
}

kslam_status kslam_align_qc_add(kslam_ctx *c, const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                                const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads, const kslam_read_pair *read_pairs,
                                uint64_t n_read_pairs, const kslam_paired_overlap *pairs, uint64_t n_pairs, const char *read_quality, int paired) {
  return guarded(c, [&] {
    if ((n_overlaps && !overlaps) || (n_cigar && !cigar_pool) || (n_reads && !read_offsets) || (n_read_pairs && !read_pairs) || (n_pairs && !pairs))
      throw StatusError{KSLAM_ERR_ARG, "null argument"};
    if (paired && (n_reads & 1)) throw StatusError{KSLAM_ERR_ARG, "a paired batch holds an even number of reads"};
    kslam_ctx::AlignQc &v = c->aq;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->aq.on, SWITCHED_OFF);
    const GenomeIndex &ix = c->need_index();
    if (ix.n_entries != v.n_entries) throw StatusError{KSLAM_ERR_STATE, "the alignment QC report was switched on for another index"};
    const uint64_t n_rbytes = n_reads ? read_offsets[n_reads] : 0;
    if (n_rbytes && !read_bases) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    // nothing is launched for arrays that do not hold together
    const kslam_batch::Arrays batch{overlaps, n_overlaps, n_cigar, read_offsets, n_reads, read_pairs, n_read_pairs, pairs, n_pairs};
    uint64_t max_len = 0;
    const std::string fault = kslam_batch::check(batch, kslam_batch::Level::records, &max_len);
    if (!fault.empty()) throw StatusError{KSLAM_ERR_ARG, fault};
    if (paired) v.paired = true;
    c->aqw.ms = 0;
    hipStream_t s = c->stream;
    const VariantInputs in = v.up.upload(batch, kslam_batch::Level::records, cigar_pool, BatchUpload::bases_and_quality, read_bases, read_quality, &ix, s);
    alignqc_count_device(in, read_quality ? v.up.rqual.as<uint8_t>() : nullptr, paired != 0, max_len, table_of(c), c->aqw, true, thread_per_record(), s);
  });
}

kslam_status kslam_align_qc_take(kslam_ctx *c, kslam_align_qc_tables *tables) {
  if (tables) memset(tables, 0, sizeof *tables);
  uint64_t *h = nullptr;
  const kslam_status st = guarded(c, [&] {
    if (!tables) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::AlignQc &v = c->aq;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->aq.on, SWITCHED_OFF);
    wait_for_lanes(c);
    hipStream_t s = c->stream;
    const uint32_t C = v.C;
    const uint64_t nw = KSLAM_ALIGN_QC_WORDS(C);
    h = (uint64_t *)pinned_get(c, nw * sizeof(uint64_t));
    HIPCHK(hipMemcpyAsync(h, v.words.p, nw * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
    tables->max_cycles = C;
    tables->paired = v.paired ? 1 : 0;
    tables->n_words = nw;
    tables->block = h;
    tables->n_read_pairs = h[0];
    tables->pairs_both = h[1];
    tables->pairs_r1_only = h[2];
    tables->pairs_r2_only = h[3];
    tables->insert_sum = h[4];
    tables->insert = h + 6;
    for (int z = 0; z < 2; z++) {
      const uint64_t *w = h + KSLAM_ALIGN_QC_REPORT_WORDS + (uint64_t)z * KSLAM_ALIGN_QC_STREAM_WORDS(C);
      kslam_align_qc_stream &S = tables->stream[z];
      S.n_records = w[0];
      S.n_reverse = w[1];
      S.n_skipped = w[2];
      S.n_without_quality = w[3];
      S.m_columns = w[4];
      S.compared = w[5];
      S.mismatches = w[6];
      S.ins_events = w[7];
      S.ins_bases = w[8];
      S.del_events = w[9];
      S.del_bases = w[10];
      S.unaligned_bases = w[11];
      S.subst = w + KSLAM_ALIGN_QC_SCALARS;
      S.ins_len = S.subst + 16;
      S.del_len = S.ins_len + KSLAM_ALIGN_QC_LEN_BINS;
      S.nm = S.del_len + KSLAM_ALIGN_QC_LEN_BINS;
      S.identity = S.nm + KSLAM_ALIGN_QC_NM_BINS;
      S.cycle = S.identity + KSLAM_ALIGN_QC_IDENTITY_BINS;
      S.cq_compared = S.cycle + ((uint64_t)C + 1) * KSLAM_ALIGN_QC_CYCLE_COLS;
      S.cq_mismatch = S.cq_compared + ((uint64_t)C + 1) * KSLAM_ALIGN_QC_QUAL_COLS;
    }
  });
  if (st != KSLAM_OK) {
    if (h) pinned_put(c, h);
    if (tables) memset(tables, 0, sizeof *tables);
  }
  return st;
}

void kslam_align_qc_release(kslam_ctx *c, kslam_align_qc_tables *tables) {
  if (!c || !tables) return;
  if (tables->block) pinned_put(c, tables->block);
  memset(tables, 0, sizeof *tables);
}

kslam_status kslam_align_qc_kernel_ms(kslam_ctx *c, double *count_ms) {
  if (!c || !count_ms) return KSLAM_ERR_ARG;
  *count_ms = c->aqw.ms;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_align_qc(kslam_ctx *c, int fd, uint32_t max_cycles) {
  if (!c) return KSLAM_ERR_ARG;
  if (refused_in_multi(c, REPORT_IS)) return KSLAM_ERR_UNSUPPORTED;
  if (max_cycles > KSLAM_ALIGN_QC_MAX_CYCLES) { c->err = "max_cycles must be 0 (= 512) or 1 .. 65536"; return KSLAM_ERR_ARG; }
  c->aq.stream_fd = fd >= 0 ? fd : -1;
  c->aq.stream_cycles = max_cycles;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_align_qc(kslam_ctx *c, int *fd, uint32_t *max_cycles) {
  if (!c || !fd || !max_cycles) return KSLAM_ERR_ARG;
  *fd = c->aq.stream_fd;
  *max_cycles = c->aq.stream_cycles;
  return KSLAM_OK;
}

}  // extern "C"
