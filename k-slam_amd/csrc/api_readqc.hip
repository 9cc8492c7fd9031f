// api_readqc.hip -- the C ABI, part 14: the read QC report's tables (include/kslam_readqc.h; kernels: readqc.hip).  The state
// lives on the context the switch was set on; its lanes call readqc_count_resident on the columns they have just cut out of
// their text, kslam_read_qc_add takes columns from the host, kslam_read_qc_take copies the tables out.
#include "context.h"

namespace kslam_api {

namespace {

ReadQcTable table_of(const kslam_ctx *owner) {
  const kslam_ctx::ReadQc &v = owner->rq;
  return ReadQcTable{v.words.as<unsigned long long>(), v.n_words, v.C};
}

const char *const REPORT_IS = "the read QC report is";
const char *const SWITCHED_OFF = "the read QC report is switched off: call kslam_set_read_qc first";

void zero_state(kslam_ctx *c) {
  readqc_zero_device(table_of(c), c->stream);
  HIPCHK(stream_wait(c->stream));
  c->rq.paired = false;
}

uint32_t resolve_cycles(uint32_t max_cycles) {
  if (max_cycles > KSLAM_READ_QC_MAX_CYCLES) throw StatusError{KSLAM_ERR_ARG, "max_cycles must be 0 (= 512) or 1 .. 65536"};
  return max_cycles ? max_cycles : KSLAM_READ_QC_DEFAULT_CYCLES;
}

}  // namespace

void readqc_release(kslam_ctx *c) {
  kslam_ctx::ReadQc &v = c->rq;
  std::lock_guard<std::mutex> lk(v.mu);
  v.on.store(false, std::memory_order_release);
  for (DevBuf *b : {&v.words, &v.up_bases, &v.up_qual, &v.up_off}) b->release();
  v.C = 0;
  v.n_words = 0;
  v.paired = false;
}

void readqc_count_resident(kslam_ctx *owner, kslam_ctx *lane, bool single) {
  kslam_ctx::ReadQc &v = owner->rq;
  std::lock_guard<std::mutex> lk(v.mu);
  if (!v.on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, "the read QC report was switched off while a batch was in flight"};
  const uint64_t n = lane->n_reads;
  if (!single && (n & 1)) throw StatusError{KSLAM_ERR_INTERNAL, "a paired batch with an odd number of reads"};
  if (!single) v.paired = true;
  if (!n) return;
  readqc_count_device(lane->r_bases.as<uint8_t>(), lane->r_qual.as<uint8_t>(), lane->r_off.as<uint64_t>(), n, !single, lane->max_read_len, table_of(owner),
                      lane->rqw, false, lane->stream);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_read_qc(kslam_ctx *c, int on, uint32_t max_cycles) {
  return guarded(c, [&] {
    if (refused_in_multi(c, REPORT_IS)) throw StatusError{KSLAM_ERR_UNSUPPORTED, c->err};
    if (!on) {
      if (c->rq.on.load(std::memory_order_acquire)) wait_for_lanes(c);
      readqc_release(c);
      return;
    }
    const uint32_t C = resolve_cycles(max_cycles);
    kslam_ctx::ReadQc &v = c->rq;
    std::lock_guard<std::mutex> lk(v.mu);
    if (v.on.load(std::memory_order_acquire)) {
      if (v.C != C)
        throw StatusError{KSLAM_ERR_STATE, "the read QC report is on with max_cycles " + std::to_string(v.C) + ": switch it off before choosing " + std::to_string(C)};
      return;
    }
    v.C = C;
    v.n_words = KSLAM_READ_QC_WORDS(C);
    try {
      v.words.ensure(2 * v.n_words * sizeof(uint64_t));
      zero_state(c);
    } catch (...) {
      v.words.release();
      v.C = 0;
      v.n_words = 0;
      throw;
    }
    c->rqw.ms = 0;
    c->rqw.bytes = 0;
    v.on.store(true, std::memory_order_release);
  });
}

kslam_status kslam_get_read_qc(kslam_ctx *c, int *on, uint32_t *max_cycles) { return get_switch(c, &kslam_ctx::rq, on, max_cycles); }

kslam_status kslam_read_qc_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    std::lock_guard<std::mutex> lk(c->rq.mu);
    need_on(c->rq.on, SWITCHED_OFF);
    wait_for_lanes(c);
    zero_state(c);
  });
}

kslam_status kslam_read_qc_add(kslam_ctx *c, const char *bases, const uint64_t *bases_off, const char *quality, uint64_t n_reads, int paired) {
  return guarded(c, [&] {
    if (n_reads && (!bases_off || !bases || !quality)) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    if (paired && (n_reads & 1)) throw StatusError{KSLAM_ERR_ARG, "a paired batch holds an even number of reads"};
    kslam_ctx::ReadQc &v = c->rq;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->rq.on, SWITCHED_OFF);
    // nothing is launched for offsets that do not hold together
    uint64_t max_len = 0;
    for (uint64_t i = 0; i < n_reads; i++) {
      if (bases_off[i + 1] < bases_off[i]) throw StatusError{KSLAM_ERR_ARG, "the read offsets must ascend"};
      max_len = std::max(max_len, bases_off[i + 1] - bases_off[i]);
    }
    if (paired) v.paired = true;
    c->rqw.ms = 0;
    c->rqw.bytes = 0;
    if (!n_reads) return;
    hipStream_t s = c->stream;
    const uint64_t o0 = bases_off[0], total = bases_off[n_reads] - o0;
    std::vector<uint64_t> rel(n_reads + 1);
    for (uint64_t i = 0; i <= n_reads; i++) rel[i] = bases_off[i] - o0;
    v.up_bases.ensure(total + 64);
    v.up_qual.ensure(total + 64);
    v.up_off.ensure((n_reads + 1) * sizeof(uint64_t));
    if (total) HIPCHK(hipMemcpyAsync(v.up_bases.p, bases + o0, total, hipMemcpyHostToDevice, s));
    if (total) HIPCHK(hipMemcpyAsync(v.up_qual.p, quality + o0, total, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(v.up_off.p, rel.data(), (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(stream_wait(s));   // (pageable sources: the caller's arrays and `rel` are free again)
    readqc_count_device(v.up_bases.as<uint8_t>(), v.up_qual.as<uint8_t>(), v.up_off.as<uint64_t>(), n_reads, paired != 0, max_len, table_of(c), c->rqw, true, s);
    c->rqw.bytes = 2 * total;
  });
}

kslam_status kslam_read_qc_take(kslam_ctx *c, kslam_read_qc_tables *tables) {
  if (tables) memset(tables, 0, sizeof *tables);
  uint64_t *h = nullptr;
  const kslam_status st = guarded(c, [&] {
    if (!tables) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    kslam_ctx::ReadQc &v = c->rq;
    std::lock_guard<std::mutex> lk(v.mu);
    need_on(c->rq.on, SWITCHED_OFF);
    wait_for_lanes(c);
    hipStream_t s = c->stream;
    const uint64_t nw = v.n_words;
    h = (uint64_t *)pinned_get(c, 2 * nw * sizeof(uint64_t));
    HIPCHK(hipMemcpyAsync(h, v.words.p, 2 * nw * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
    const uint32_t C = v.C;
    tables->max_cycles = C;
    tables->paired = v.paired ? 1 : 0;
    tables->words_per_stream = nw;
    tables->block = h;
    for (int z = 0; z < 2; z++) {
      uint64_t *w = h + z * nw;
      if (!w[0]) w[2] = 0;   // (no read: the minimum's start value)
      kslam_read_qc_stream &S = tables->stream[z];
      S.n_reads = w[0];
      S.n_bases = w[1];
      S.min_len = w[2];
      S.max_len = w[3];
      S.len_hist = w + 4;
      S.base = S.len_hist + ((uint64_t)C + 2);
      S.qual = S.base + ((uint64_t)C + 1) * KSLAM_READ_QC_BASE_COLS;
      S.mean_q = S.qual + ((uint64_t)C + 1) * KSLAM_READ_QC_QUAL_COLS;
      S.gc = S.mean_q + KSLAM_READ_QC_MEAN_BINS;
    }
  });
  if (st != KSLAM_OK) {
    if (h) pinned_put(c, h);
    if (tables) memset(tables, 0, sizeof *tables);
  }
  return st;
}

void kslam_read_qc_release(kslam_ctx *c, kslam_read_qc_tables *tables) {
  if (!c || !tables) return;
  if (tables->block) pinned_put(c, tables->block);
  memset(tables, 0, sizeof *tables);
}

kslam_status kslam_read_qc_kernel_ms(kslam_ctx *c, double *count_ms, uint64_t *bytes) {
  if (!c || !count_ms || !bytes) return KSLAM_ERR_ARG;
  *count_ms = c->rqw.ms;
  *bytes = c->rqw.bytes;
  return KSLAM_OK;
}

kslam_status kslam_stream_set_read_qc(kslam_ctx *c, int fd, uint32_t max_cycles) {
  if (!c) return KSLAM_ERR_ARG;
  if (refused_in_multi(c, REPORT_IS)) return KSLAM_ERR_UNSUPPORTED;
  if (max_cycles > KSLAM_READ_QC_MAX_CYCLES) { c->err = "max_cycles must be 0 (= 512) or 1 .. 65536"; return KSLAM_ERR_ARG; }
  c->rq.stream_fd = fd >= 0 ? fd : -1;
  c->rq.stream_cycles = max_cycles;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_read_qc(kslam_ctx *c, int *fd, uint32_t *max_cycles) {
  if (!c || !fd || !max_cycles) return KSLAM_ERR_ARG;
  *fd = c->rq.stream_fd;
  *max_cycles = c->rq.stream_cycles;
  return KSLAM_OK;
}

}  // extern "C"
