// api_bamsort.hip -- the C ABI, part 17: the coordinate-sorted BAM and its BAI index (include/kslam_bamsort.h; kernels:
// bamsort.hip).  The store lives on the context the switch was set on: slabs of device memory that hold, per batch, its record
// bytes and behind them its record index; nothing in a slab ever moves, so a lane fills the region it reserved on its own stream
// without the lock.  kslam_bam_sort_add takes a batch's bytes from the host; kslam_bam_sort_take sorts once, gathers and
// compresses slice by slice, and builds the index from the members' sizes.
#include "context.h"
#include "bamsort.h"
#include "../host/bamsort.hpp"

namespace kslam_api {

namespace {

namespace hb = kslam_bamsort;

constexpr uint64_t BS_MAX_RECORDS = 0xFFFFFFFFull;   // the radix sort's limit, and the sort record's ordinal

const char *const REPORT_IS = "the sorted BAM is";
const char *const SWITCHED_OFF = "the sort is switched off: call kslam_set_bam_sort first";

BamSortState &state_of(kslam_ctx *c) {
  if (!c->bsort || !c->bsort_on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, SWITCHED_OFF};
  return *c->bsort;
}

uint64_t up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// Room for a batch of len bytes and n records in the store (under S.mu): the region is [at, at + region_bytes) of a slab
struct Region {
  size_t slab;
  uint64_t at;
  BamSortCols cols;
  uint8_t *bytes;
};
uint64_t region_bytes(uint64_t len, uint64_t n) { return up(up(len, 16) + 24 * n, 256) + 256; }

Region reserve(BamSortState &S, uint64_t len, uint64_t n) {
  const uint64_t need = region_bytes(len, n);
  size_t k = S.slabs.size();
  for (size_t j = 0; j < S.slabs.size(); j++)
    if (S.slabs[j].cap - S.slabs[j].used >= need) { k = j; break; }
  if (k == S.slabs.size()) {
    BamSortSlab slab;
    slab.cap = std::max(need, BAMSORT_SLAB);
    if (hipMalloc(&slab.p, slab.cap) != hipSuccess) {
      (void)hipGetLastError();
      throw StatusError{KSLAM_ERR_OOM, "the sort's store holds " + std::to_string(S.bytes_held()) + " bytes of device memory and " +
                                           std::to_string(slab.cap) + " more were asked for and could not be had: the batch was not added"};
    }
    S.slabs.push_back(slab);
  }
  BamSortSlab &slab = S.slabs[k];
  Region r;
  r.slab = k;
  r.at = slab.used;
  slab.used += need;
  r.bytes = (uint8_t *)slab.p + r.at;
  uint8_t *cols = r.bytes + up(len, 16);
  r.cols.off = (uint64_t *)cols;
  r.cols.len = (uint32_t *)(cols + 8 * n);
  r.cols.ref = r.cols.len + n;
  r.cols.pos1 = r.cols.ref + n;
  r.cols.meta = r.cols.pos1 + n;
  return r;
}

void make_events(BamSortWork &W) {
  if (!W.ev[0])
    for (auto &e : W.ev) HIPCHK(hipEventCreate(&e));
}

void size_work(BamSortWork &W, uint64_t n_seg) {
  W.cnt.ensure((n_seg + 1) * sizeof(uint32_t));
  W.first.ensure((n_seg + 1) * sizeof(uint32_t));
  W.scan_tmp.ensure(scan_tmp_bytes(n_seg + 1));
  W.totals.ensure(2 * sizeof(uint64_t));
}

void publish(BamSortState &S, uint64_t seq, const Region &r, uint64_t len, uint64_t n, double ms) {
  BamSortBatch b;
  b.seq = seq;
  b.slab = r.slab;
  b.at = r.at;
  b.len = len;
  b.n = n;
  b.cols = r.cols;
  S.batches.push_back(b);
  S.ms[0] = ms;
}

void free_store(BamSortState &S) {
  for (auto &slab : S.slabs)
    if (slab.p) (void)hipFree(slab.p);
  S.slabs.clear();
  S.batches.clear();
}

struct Sink {   // the members of one file on their way to the caller
  kslam_write_fn write;
  void *user;
  const char *what;
  void put(const char *p, uint64_t n) {
    if (n && write(user, p, n)) throw StatusError{KSLAM_ERR_ARG, std::string("the write callback of the ") + what + " reported a failure"};
  }
};

}  // namespace

void bamsort_release(kslam_ctx *c) {
  c->bsort_on.store(false, std::memory_order_release);
  if (!c->bsort) return;
  BamSortState &S = *c->bsort;
  std::lock_guard<std::mutex> lk(S.mu);
  free_store(S);
  for (DevBuf *b : {&S.keys_a, &S.keys_b, &S.src, &S.len, &S.meta, &S.s_src, &S.s_len, &S.dst_off, &S.slice_buf, &S.out, &S.hdr_in, &S.member_off, &S.win_off,
                    &S.win, &S.refc, &S.head, &S.run_at, &S.runs, &S.range, &S.scan_tmp, &S.totals, &S.sortws.hist, &S.sortws.status, &S.sortws.tickets,
                    &S.sortws.digits, &S.bgzfw.cand, &S.bgzfw.slots, &S.bgzfw.sizes, &S.bgzfw.offs, &S.bgzfw.scan_tmp, &S.bgzfw.totals, &S.addw.seg,
                    &S.addw.cnt, &S.addw.first, &S.addw.scan_tmp, &S.addw.totals})
    b->release();
  S.slice = BAMSORT_DEFAULT_SLICE;
  S.segment = BAMSORT_DEFAULT_SEGMENT;
  S.gather = 0;
  S.n_ref = 0;
  S.ref_len.clear();
}

void bamsort_destroy(kslam_ctx *c) {
  if (c->bsort) {
    free_store(*c->bsort);
    for (auto &e : c->bsort->ev)
      if (e) (void)hipEventDestroy(e);
    delete c->bsort;
    c->bsort = nullptr;
  }
  delete c->bsort_w;
  c->bsort_w = nullptr;
}

void bamsort_append_resident(kslam_ctx *owner, kslam_ctx *lane, uint64_t ticket, uint64_t n_groups, uint64_t mapped_bytes, uint64_t n_unmapped_rows,
                             uint64_t total_bytes) {
  BamSortState &S = state_of(owner);
  if (!lane->bsort_w) lane->bsort_w = new BamSortWork();
  BamSortWork &W = *lane->bsort_w;
  make_events(W);
  hipStream_t s = lane->stream;
  const uint8_t *text = lane->samw.text.as<uint8_t>();
  // the record starts this lane already knows: text_off per read pair, and the rows of the reads without alignment behind them
  const uint64_t n_seg = n_groups + n_unmapped_rows;
  size_work(W, n_seg);
  HIPCHK(hipEventRecord(W.ev[0], s));
  uint64_t n = 0;
  if (n_seg && total_bytes) {
    bamsort_count_device(text, lane->samw.text_off.as<uint64_t>(), n_groups, 0, mapped_bytes, W.cnt.as<uint32_t>(), s);
    bamsort_count_device(text, lane->sumw.off.as<uint64_t>(), n_unmapped_rows, mapped_bytes, total_bytes, W.cnt.as<uint32_t>() + n_groups, s);
    exclusive_scan_u32(W.cnt.as<uint32_t>(), W.first.as<uint32_t>(), n_seg, W.totals.as<uint64_t>(), W.scan_tmp.p, s);
    read_back(&n, W.totals.p, sizeof n, s);
  }
  Region r;
  uint64_t seq;
  {
    std::lock_guard<std::mutex> lk(S.mu);
    need_on(owner->bsort_on, "the sort was switched off while a batch was in flight");
    if (ticket < S.base_ticket) throw StatusError{KSLAM_ERR_STATE, "a batch submitted before the sort was switched on or reset reached it"};
    seq = ticket - S.base_ticket;
    for (const auto &b : S.batches)
      if (b.seq == seq) throw StatusError{KSLAM_ERR_STATE, "batch ordinal " + std::to_string(seq) + " is already held"};
    r = reserve(S, total_bytes, n);
  }
  if (total_bytes) HIPCHK(hipMemcpyAsync(r.bytes, text, total_bytes, hipMemcpyDeviceToDevice, s));
  if (n) {
    bamsort_write_device(text, lane->samw.text_off.as<uint64_t>(), n_groups, 0, mapped_bytes, W.first.as<uint32_t>(), S.n_ref, r.cols, s);
    bamsort_write_device(text, lane->sumw.off.as<uint64_t>(), n_unmapped_rows, mapped_bytes, total_bytes, W.first.as<uint32_t>() + n_groups, S.n_ref,
                         r.cols, s);
  }
  HIPCHK(hipEventRecord(W.ev[1], s));
  HIPCHK(stream_wait(s));   // the batch is whole before anybody can see it
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
  W.ms = ms;
  std::lock_guard<std::mutex> lk(S.mu);
  need_on(owner->bsort_on, "the sort was switched off while a batch was in flight");
  publish(S, seq, r, total_bytes, n, ms);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_set_bam_sort(kslam_ctx *c, int on) {
  return guarded(c, [&] {
    if (refused_in_multi(c, REPORT_IS)) throw StatusError{KSLAM_ERR_UNSUPPORTED, c->err};
    if (!on) {
      if (c->bsort_on.load(std::memory_order_acquire)) wait_for_lanes(c);
      bamsort_release(c);
      return;
    }
    const GenomeIndex &ix = c->need_index();
    if (c->bsort_on.load(std::memory_order_acquire)) return;
    for (uint64_t e = 0; e < ix.n_entries; e++)
      if (ix.h_goff[e + 1] - ix.h_goff[e] > hb::MAX_REF_LEN)
        throw StatusError{KSLAM_ERR_UNSUPPORTED, "index entry " + std::to_string(e) + " has " + std::to_string(ix.h_goff[e + 1] - ix.h_goff[e]) +
                                                     " bases, more than 2^29: a BAI index cannot address it"};
    if (ix.n_entries >= 0x7FFFFFFFull) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^31 - 1 or more index entries: BAM cannot number them"};
    if (!c->bsort) c->bsort = new BamSortState();
    BamSortState &S = *c->bsort;
    std::lock_guard<std::mutex> lk(S.mu);
    if (!S.ev[0])
      for (auto &e : S.ev) HIPCHK(hipEventCreate(&e));
    make_events(S.addw);
    S.n_ref = (uint32_t)ix.n_entries;
    S.ref_len.assign(ix.n_entries, 0);
    std::vector<uint64_t> win_off(ix.n_entries + 1, 0);
    for (uint64_t e = 0; e < ix.n_entries; e++) {
      S.ref_len[e] = ix.h_goff[e + 1] - ix.h_goff[e];
      win_off[e + 1] = win_off[e] + ((std::max<uint64_t>(S.ref_len[e], 1) - 1) >> 14) + 1;
    }
    S.win_off.ensure(win_off.size() * sizeof(uint64_t));
    HIPCHK(hipMemcpyAsync(S.win_off.p, win_off.data(), win_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(stream_wait(c->stream));
    S.batches.clear();
    for (auto &slab : S.slabs) slab.used = 0;
    for (auto &m : S.ms) m = 0;
    {
      std::lock_guard<std::mutex> as(c->as_mu);
      S.base_ticket = c->next_ticket;
    }
    c->bsort_on.store(true, std::memory_order_release);
  });
}

kslam_status kslam_get_bam_sort(kslam_ctx *c, int *on) {
  if (!c || !on) return KSLAM_ERR_ARG;
  *on = c->bsort_on.load(std::memory_order_acquire) ? 1 : 0;
  return KSLAM_OK;
}

kslam_status kslam_bam_sort_reset(kslam_ctx *c) {
  return guarded(c, [&] {
    BamSortState &S = state_of(c);
    std::lock_guard<std::mutex> lk(S.mu);
    wait_for_lanes(c);
    S.batches.clear();
    for (auto &slab : S.slabs) slab.used = 0;
    std::lock_guard<std::mutex> as(c->as_mu);
    S.base_ticket = c->next_ticket;
  });
}

kslam_status kslam_bam_sort_set_slice(kslam_ctx *c, uint64_t bytes) {
  return guarded(c, [&] {
    BamSortState &S = state_of(c);
    std::lock_guard<std::mutex> lk(S.mu);
    S.slice = !bytes ? BAMSORT_DEFAULT_SLICE : std::max<uint64_t>(bytes / BGZF_MEMBER_IN, 1) * BGZF_MEMBER_IN;
  });
}

kslam_status kslam_bam_sort_set_segment(kslam_ctx *c, uint32_t records) {
  return guarded(c, [&] {
    BamSortState &S = state_of(c);
    std::lock_guard<std::mutex> lk(S.mu);
    S.segment = records ? records : BAMSORT_DEFAULT_SEGMENT;
  });
}

kslam_status kslam_bam_sort_set_gather(kslam_ctx *c, uint32_t lanes) {
  return guarded(c, [&] {
    if (lanes != 0 && lanes != 1 && lanes != 16 && lanes != 64) throw StatusError{KSLAM_ERR_ARG, "the gather moves a record with 1, 16 or 64 lanes (0: the default)"};
    BamSortState &S = state_of(c);
    std::lock_guard<std::mutex> lk(S.mu);
    S.gather = lanes;
  });
}

kslam_status kslam_bam_sort_kernel_ms(kslam_ctx *c, double ms[5]) {
  if (!c || !ms) return KSLAM_ERR_ARG;
  return guarded(c, [&] {
    BamSortState &S = state_of(c);
    std::lock_guard<std::mutex> lk(S.mu);
    for (int k = 0; k < 5; k++) ms[k] = S.ms[k];
  });
}

kslam_status kslam_bam_sort_add(kslam_ctx *c, uint64_t seq, const void *records, uint64_t len) {
  return guarded(c, [&] {
    if (len && !records) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    BamSortState &S = state_of(c);
    std::lock_guard<std::mutex> lk(S.mu);
    need_on(c->bsort_on, SWITCHED_OFF);
    // nothing is launched for bytes that do not hold together: the walk the device repeats, segment by segment
    const uint8_t *data = (const uint8_t *)records;
    std::vector<uint64_t> seg;
    uint64_t n = 0;
    for (uint64_t off = 0; off < len;) {
      hb::Rec r;
      const std::string fault = hb::parse_record(data, len, off, &r);
      if (!fault.empty()) throw StatusError{KSLAM_ERR_ARG, fault};
      if (r.ref >= 0 && (uint32_t)r.ref >= S.n_ref)
        throw StatusError{KSLAM_ERR_ARG, "refID " + std::to_string(r.ref) + " is not below the index's " + std::to_string(S.n_ref) + " entries (record at byte " +
                                             std::to_string(off) + ")"};
      if (r.ref >= 0 && r.pos >= 0 && (uint64_t)r.pos + r.span > S.ref_len[r.ref])
        throw StatusError{KSLAM_ERR_ARG, "a record reaches past the end of its entry (record at byte " + std::to_string(off) + ")"};
      if (n % S.segment == 0) seg.push_back(off);
      n++;
      off += r.len;
    }
    for (const auto &b : S.batches)
      if (b.seq == seq) throw StatusError{KSLAM_ERR_ARG, "batch ordinal " + std::to_string(seq) + " is already held"};
    hipStream_t s = c->stream;
    BamSortWork &W = S.addw;
    const uint64_t n_seg = seg.size();
    size_work(W, n_seg);
    W.seg.ensure((n_seg + 1) * sizeof(uint64_t));
    const Region r = reserve(S, len, n);
    HIPCHK(hipEventRecord(W.ev[0], s));
    if (len) HIPCHK(hipMemcpyAsync(r.bytes, data, len, hipMemcpyHostToDevice, s));
    if (n_seg) {
      HIPCHK(hipMemcpyAsync(W.seg.p, seg.data(), n_seg * sizeof(uint64_t), hipMemcpyHostToDevice, s));
      bamsort_count_device(r.bytes, W.seg.as<uint64_t>(), n_seg, 0, len, W.cnt.as<uint32_t>(), s);
      exclusive_scan_u32(W.cnt.as<uint32_t>(), W.first.as<uint32_t>(), n_seg, W.totals.as<uint64_t>(), W.scan_tmp.p, s);
      bamsort_write_device(r.bytes, W.seg.as<uint64_t>(), n_seg, 0, len, W.first.as<uint32_t>(), S.n_ref, r.cols, s);
    }
    HIPCHK(hipEventRecord(W.ev[1], s));
    uint64_t counted = 0;
    if (n_seg) read_back(&counted, W.totals.p, sizeof counted, s);
    HIPCHK(stream_wait(s));   // (pageable sources)
    if (counted != n) throw StatusError{KSLAM_ERR_INTERNAL, "the device counted " + std::to_string(counted) + " records where the host counted " + std::to_string(n)};
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
    publish(S, seq, r, len, n, ms);
  });
}

kslam_status kslam_bam_sort_take(kslam_ctx *c, const char *sam_header, uint64_t len, kslam_write_fn write_bam, void *user_bam, kslam_write_fn write_bai,
                                 void *user_bai, kslam_bam_sort_stats *stats) {
  if (stats) memset(stats, 0, sizeof *stats);
  char *h_out = nullptr;
  const kslam_status st = guarded(c, [&] {
    if (!write_bam || !stats || (len && !sam_header)) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    BamSortState &S = state_of(c);
    std::lock_guard<std::mutex> lk(S.mu);
    need_on(c->bsort_on, SWITCHED_OFF);
    wait_for_lanes(c);
    hipStream_t s = c->stream;
    const int deflate = c->samtext.deflate;
    // the batches in submission order
    std::vector<const BamSortBatch *> order;
    for (const auto &b : S.batches) order.push_back(&b);
    std::sort(order.begin(), order.end(), [](const BamSortBatch *a, const BamSortBatch *b) { return a->seq < b->seq; });
    uint64_t n = 0, total = 0;
    for (size_t k = 0; k < order.size(); k++) {
      if (order[k]->seq != k) throw StatusError{KSLAM_ERR_STATE, "batch ordinal " + std::to_string(k) + " is missing: " + std::to_string(order.size()) +
                                                                    " batches are held, the highest ordinal is " + std::to_string(order.back()->seq)};
      n += order[k]->n;
      total += order[k]->len;
    }
    if (n > BS_MAX_RECORDS) throw StatusError{KSLAM_ERR_UNSUPPORTED, std::to_string(n) + " records, more than 2^32 - 1 in one sort"};
    // the header
    std::string herr;
    std::vector<uint64_t> ref_len;
    const std::string header = hb::bam_header_of(hb::coordinate_header(sam_header, len), &ref_len, &herr);
    if (!herr.empty()) throw StatusError{KSLAM_ERR_ARG, herr};
    if (ref_len != S.ref_len) throw StatusError{KSLAM_ERR_ARG, "the header's @SQ lines are not the index's entries with their lengths, in entry order"};
    Sink bam{write_bam, user_bam, "BAM file"};
    uint64_t header_clen = 0;
    S.hdr_in.ensure(header.size() + 64);
    HIPCHK(hipMemcpyAsync(S.hdr_in.p, header.data(), header.size(), hipMemcpyHostToDevice, s));
    bgzf_compress_device(S.hdr_in.as<char>(), header.size(), deflate, S.bgzfw, S.out, &header_clen, s);
    h_out = (char *)pinned_get(c, header_clen + 64);
    HIPCHK(hipMemcpyAsync(h_out, S.out.p, header_clen, hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
    bam.put(h_out, header_clen);
    pinned_put(c, h_out);
    h_out = nullptr;
    for (int k = 1; k < 5; k++) S.ms[k] = 0;
    auto lap = [&](int k, hipEvent_t a, hipEvent_t b) {   // after the stream has been waited for
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, a, b));
      S.ms[k] += ms;
    };
    // the sort: one 4-word record per record in submission order; the radix sort is stable, so ties keep that order
    const uint4 *keys = nullptr;
    if (n) {
      S.keys_a.ensure(n * sizeof(uint4));
      S.keys_b.ensure(n * sizeof(uint4));
      S.src.ensure(n * sizeof(uint64_t));
      S.len.ensure(n * sizeof(uint32_t));
      S.meta.ensure(n * sizeof(uint32_t));
      S.s_src.ensure(n * sizeof(uint64_t));
      S.s_len.ensure(n * sizeof(uint32_t));
      S.dst_off.ensure((n + 1) * sizeof(uint64_t));
      S.scan_tmp.ensure(scan_tmp_bytes(n + 1));
      S.totals.ensure(2 * sizeof(uint64_t));
      S.range.ensure(2 * sizeof(uint64_t));
      HIPCHK(hipEventRecord(S.ev[0], s));
      uint64_t at = 0;
      for (const BamSortBatch *b : order) {
        bamsort_keys_device(b->cols, (const uint8_t *)S.slabs[b->slab].p + b->at, b->n, at, S.keys_a.as<uint4>(), S.src.as<uint64_t>(), S.len.as<uint32_t>(),
                            S.meta.as<uint32_t>(), s);
        at += b->n;
      }
      keys = S.keys_a.as<uint4>();
      if (n > 1) {
        SortPass passes[8];
        int n_passes = 0;
        for (int p = 0; p < 4; p++) passes[n_passes++] = SortPass{0u, (uint32_t)(8 * p), 0u};
        for (uint32_t p = 0; p < (bits_for(S.n_ref) + 7) / 8; p++) passes[n_passes++] = SortPass{1u, 8 * p, 0u};
        keys = (const uint4 *)radix_sort(S.keys_a.p, S.keys_b.p, n, 4, passes, n_passes, S.sortws, s, nullptr, nullptr, nullptr);
      }
      bamsort_order_device(keys, S.src.as<uint64_t>(), S.len.as<uint32_t>(), n, S.s_src.as<uint64_t>(), S.s_len.as<uint32_t>(), s);
      exclusive_scan_u32_to_u64(S.s_len.as<uint32_t>(), S.dst_off.as<uint64_t>(), n, S.totals.as<uint64_t>(), S.scan_tmp.p, s);
      HIPCHK(hipMemcpyAsync(S.dst_off.as<uint64_t>() + n, S.totals.p, sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
      HIPCHK(hipEventRecord(S.ev[1], s));
      uint64_t scanned = 0;
      read_back(&scanned, S.totals.p, sizeof scanned, s);
      if (scanned != total) throw StatusError{KSLAM_ERR_INTERNAL, "the records' lengths sum to " + std::to_string(scanned) + ", the batches hold " + std::to_string(total)};
      lap(1, S.ev[0], S.ev[1]);
    }
    // slice by slice: gather, compress, hand over
    std::vector<uint64_t> member_off{0};
    if (total) S.slice_buf.ensure(std::min(S.slice, total) + 64);
    const uint32_t lanes = S.gather ? S.gather : (n && total / n >= 1024 ? 64u : 16u);
    for (uint64_t a = 0; a < total; a += S.slice) {
      const uint64_t b = std::min(a + S.slice, total);
      uint64_t range[2];
      bamsort_range_device(S.dst_off.as<uint64_t>(), n, a, b, S.range.as<uint64_t>(), s);
      read_back(range, S.range.p, sizeof range, s);
      if (range[0] > range[1] || range[1] > n) throw StatusError{KSLAM_ERR_INTERNAL, "the slice's record range is out of order"};
      HIPCHK(hipEventRecord(S.ev[2], s));
      bamsort_gather_device(S.s_src.as<uint64_t>(), S.dst_off.as<uint64_t>(), range[0], range[1], a, b, S.slice_buf.as<uint8_t>(), lanes, s);
      HIPCHK(hipEventRecord(S.ev[3], s));
      uint64_t clen = 0;
      bgzf_compress_device(S.slice_buf.as<char>(), b - a, deflate, S.bgzfw, S.out, &clen, s);
      HIPCHK(hipEventRecord(S.ev[4], s));
      h_out = (char *)pinned_get(c, clen + 64);
      HIPCHK(hipMemcpyAsync(h_out, S.out.p, clen, hipMemcpyDeviceToHost, s));
      HIPCHK(stream_wait(s));
      lap(2, S.ev[2], S.ev[3]);
      lap(3, S.ev[3], S.ev[4]);
      uint64_t members = 0;
      for (uint64_t p = 0; p < clen; members++) {
        if (clen - p < 18) throw StatusError{KSLAM_ERR_INTERNAL, "a truncated member came out of the compressor"};
        const uint64_t bsize = (uint64_t)hb::le16((const uint8_t *)h_out + p + 16) + 1;
        member_off.push_back(member_off.back() + bsize);
        p += bsize;
      }
      if (members != (b - a + BGZF_MEMBER_IN - 1) / BGZF_MEMBER_IN) throw StatusError{KSLAM_ERR_INTERNAL, "the compressor's members are not those of the slice"};
      bam.put(h_out, clen);
      pinned_put(c, h_out);
      h_out = nullptr;
    }
    bam.put(KSLAM_BGZF_EOF, KSLAM_BGZF_EOF_LEN);
    const uint64_t n_members = member_off.size() - 1;
    stats->n_records = n;
    stats->record_bytes = total;
    stats->compressed_bytes = member_off.back();
    stats->n_members = n_members;
    stats->bytes_held = S.bytes_held();
    // the index
    std::vector<hb::RefCount> refs(S.n_ref);
    std::vector<hb::Run> runs;
    std::vector<uint64_t> win_off(S.n_ref + 1, 0), win;
    for (uint32_t e = 0; e < S.n_ref; e++) win_off[e + 1] = win_off[e] + ((std::max<uint64_t>(S.ref_len[e], 1) - 1) >> 14) + 1;
    win.assign(win_off[S.n_ref], ~0ull);
    uint64_t first_no_coor = n;
    const hb::Voff V{member_off.data(), n_members, header_clen, total};
    if (n) {
      const uint64_t R = S.n_ref;
      S.member_off.ensure(member_off.size() * sizeof(uint64_t));
      S.win.ensure((win.size() + 1) * sizeof(uint64_t));
      S.refc.ensure((5 * R + 1) * sizeof(uint64_t));
      S.head.ensure(n * sizeof(uint32_t));
      S.run_at.ensure(n * sizeof(uint32_t));
      HIPCHK(hipMemcpyAsync(S.member_off.p, member_off.data(), member_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
      HIPCHK(hipEventRecord(S.ev[5], s));
      HIPCHK(hipMemsetAsync(S.win.p, 0xFF, (win.size() + 1) * sizeof(uint64_t), s));
      HIPCHK(hipMemsetAsync(S.refc.p, 0, (5 * R + 1) * sizeof(uint64_t), s));
      if (R) HIPCHK(hipMemsetAsync(S.refc.p, 0xFF, R * sizeof(uint64_t), s));
      uint64_t *rc = S.refc.as<uint64_t>();
      HIPCHK(hipMemcpyAsync(rc + 5 * R, &n, sizeof n, hipMemcpyHostToDevice, s));
      const BamSortIndexIn in{keys, S.meta.as<uint32_t>(), S.dst_off.as<uint64_t>(), n, S.n_ref, S.member_off.as<uint64_t>(), n_members, header_clen, total,
                              S.win_off.as<uint64_t>()};
      const BamSortIndexOut out{S.win.as<uint64_t>(), rc, rc + R, rc + 2 * R, rc + 3 * R, rc + 4 * R, rc + 5 * R, S.head.as<uint32_t>()};
      bamsort_index_device(in, out, s);
      exclusive_scan_u32(S.head.as<uint32_t>(), S.run_at.as<uint32_t>(), n, S.totals.as<uint64_t>(), S.scan_tmp.p, s);
      uint64_t n_runs = 0;
      read_back(&n_runs, S.totals.p, sizeof n_runs, s);
      if (!n_runs || n_runs > n) throw StatusError{KSLAM_ERR_INTERNAL, "the run heads do not add up"};
      S.runs.ensure(n_runs * sizeof(BamSortRun));
      bamsort_runs_device(in, S.head.as<uint32_t>(), S.run_at.as<uint32_t>(), S.runs.as<BamSortRun>(), s);
      HIPCHK(hipEventRecord(S.ev[6], s));
      // only the compacted runs, the windows and the per-reference counters travel
      std::vector<BamSortRun> d_runs(n_runs);
      std::vector<uint64_t> counters(5 * R + 1);
      HIPCHK(hipMemcpyAsync(d_runs.data(), S.runs.p, n_runs * sizeof(BamSortRun), hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(counters.data(), S.refc.p, counters.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
      if (!win.empty()) HIPCHK(hipMemcpyAsync(win.data(), S.win.p, win.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
      HIPCHK(stream_wait(s));
      lap(4, S.ev[5], S.ev[6]);
      for (const BamSortRun &r : d_runs) runs.push_back(hb::Run{r.ref, r.bin, r.beg, 0});
      for (uint64_t e = 0; e < R; e++) refs[e] = hb::RefCount{counters[e], counters[R + e], counters[2 * R + e], counters[3 * R + e], counters[4 * R + e]};
      first_no_coor = counters[5 * R];
    }
    stats->n_no_coor = n - first_no_coor;
    uint64_t n_chunks = 0;
    const std::string bai = hb::assemble_bai(S.n_ref, runs, refs, win, win_off, V.at(total), n - first_no_coor, &n_chunks);
    stats->n_chunks = n_chunks;
    if (write_bai) {
      Sink sink{write_bai, user_bai, "BAI index"};
      sink.put(bai.data(), bai.size());
    }
  });
  if (st != KSLAM_OK) {
    if (h_out) pinned_put(c, h_out);
    if (stats) memset(stats, 0, sizeof *stats);
  }
  return st;
}

kslam_status kslam_stream_set_bam_sort(kslam_ctx *c, int on, int bai_fd) {
  if (!c) return KSLAM_ERR_ARG;
  if (on && refused_in_multi(c, REPORT_IS)) return KSLAM_ERR_UNSUPPORTED;
  c->bsort_stream.on = on ? 1 : 0;
  c->bsort_stream.bai_fd = on && bai_fd >= 0 ? bai_fd : -1;
  return KSLAM_OK;
}

kslam_status kslam_stream_get_bam_sort(kslam_ctx *c, int *on, int *bai_fd) {
  if (!c || !on || !bai_fd) return KSLAM_ERR_ARG;
  *on = c->bsort_stream.on;
  *bai_fd = c->bsort_stream.bai_fd;
  return KSLAM_OK;
}

}  // extern "C"
