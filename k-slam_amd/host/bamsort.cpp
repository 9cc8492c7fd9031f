// bamsort.cpp -- include/kslam_bamsort.h, the host twins: the sorted record stream of a run's batches and the BAI index of the
// sorted file, the same bytes csrc/bamsort.hip and api_bamsort.hip make on the device.  The first thing the device is compared
// with.  Plain C++, no device code.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kslam_bamsort.h"
#include "bamsort.hpp"
#include "workers.hpp"

namespace {
using namespace kslam_host;
using namespace kslam_bamsort;

void hand_over(const std::string &s, char **out, uint64_t *out_len) {
  char *buf = (char *)malloc(s.size() + 1);
  if (!buf) fail(KSLAM_ERR_OOM, "out of host memory");
  memcpy(buf, s.data(), s.size());
  buf[s.size()] = 0;
  *out = buf;
  *out_len = s.size();
}

std::vector<Rec> records_of(const uint8_t *data, uint64_t len) {
  std::vector<Rec> recs;
  for (uint64_t off = 0; off < len;) {
    Rec r;
    const std::string fault = parse_record(data, len, off, &r);
    if (!fault.empty()) fail(KSLAM_ERR_ARG, fault);
    recs.push_back(r);
    off += r.len;
  }
  return recs;
}

}  // namespace

extern "C" {

kslam_status kslam_tail_bam_sort_header(const char *sam_header, uint64_t len, char **out, uint64_t *out_len) {
  return guarded([&] {
    if (!out || !out_len || (len && !sam_header)) fail(KSLAM_ERR_ARG, "null argument");
    std::string err;
    const std::string h = bam_header_of(coordinate_header(sam_header, len), nullptr, &err);
    if (!err.empty()) fail(KSLAM_ERR_ARG, err);
    hand_over(h, out, out_len);
  });
}

kslam_status kslam_tail_bam_sort(const char *const *batches, const uint64_t *lens, uint64_t n_batches, char **out, uint64_t *out_len) {
  return guarded([&] {
    if (!out || !out_len || (n_batches && (!batches || !lens))) fail(KSLAM_ERR_ARG, "null argument");
    struct Item {
      uint64_t key;
      const uint8_t *p;
      uint32_t len;
    };
    std::vector<Item> items;
    uint64_t total = 0;
    for (uint64_t b = 0; b < n_batches; b++) {
      if (lens[b] && !batches[b]) fail(KSLAM_ERR_ARG, "null argument");
      const uint8_t *data = (const uint8_t *)batches[b];
      for (const Rec &r : records_of(data, lens[b])) items.push_back(Item{sort_key(r), data + r.off, r.len});
      total += lens[b];
    }
    if (items.size() > 0xFFFFFFFFull) fail(KSLAM_ERR_UNSUPPORTED, "more than 2^32 - 1 records in one sort");
    std::stable_sort(items.begin(), items.end(), [](const Item &a, const Item &b) { return a.key < b.key; });
    std::string o;
    o.reserve(total);
    for (const Item &it : items) o.append((const char *)it.p, it.len);
    hand_over(o, out, out_len);
  });
}

kslam_status kslam_tail_bai(const char *stream, uint64_t len, uint32_t n_ref, const uint32_t *member_sizes, uint64_t n_members,
                            uint64_t header_compressed_len, char **out, uint64_t *out_len) {
  return guarded([&] {
    if (!out || !out_len || (len && !stream) || (n_members && !member_sizes)) fail(KSLAM_ERR_ARG, "null argument");
    if (n_members != (len + MEMBER_IN - 1) / MEMBER_IN) fail(KSLAM_ERR_ARG, "the member sizes are not those of the stream's members of 65 280 bytes");
    if (n_ref > INT32_MAX) fail(KSLAM_ERR_ARG, "the reference list is too long for BAM");
    std::vector<uint64_t> moff(n_members + 1, 0);
    for (uint64_t m = 0; m < n_members; m++) moff[m + 1] = moff[m] + member_sizes[m];
    const Voff V{moff.data(), n_members, header_compressed_len, len};
    const uint8_t *data = (const uint8_t *)stream;
    const std::vector<Rec> recs = records_of(data, len);
    std::vector<RefCount> refs(n_ref);
    std::vector<Run> runs;
    uint64_t n_no_coor = 0, prev_key = 0;
    for (size_t i = 0; i < recs.size(); i++) {
      const Rec &r = recs[i];
      if (r.ref >= 0 && (uint32_t)r.ref >= n_ref) fail(KSLAM_ERR_ARG, "a record's refID is not below n_ref");
      if (i && sort_key(r) < sort_key(recs[i - 1])) fail(KSLAM_ERR_ARG, "the record stream is not sorted");
      if (r.ref >= 0 && r.pos >= 0 && (uint64_t)r.pos + r.span > MAX_REF_LEN) fail(KSLAM_ERR_ARG, "a record ends beyond 2^29: BAI cannot address it");
      const uint64_t sv = V.at(r.off), ev = V.at(r.off + r.len);
      const bool indexed = r.ref >= 0 && r.pos >= 0;
      const uint32_t ref = r.ref >= 0 ? (uint32_t)r.ref : n_ref;
      const uint32_t bin = indexed ? reg2bin((uint64_t)r.pos, (uint64_t)r.pos + r.span) : NO_BIN;
      const uint64_t key = (uint64_t)ref << 32 | bin;
      if (!i || key != prev_key) runs.push_back(Run{ref, bin, sv, 0});
      prev_key = key;
      if (r.ref < 0) {
        n_no_coor++;
        continue;
      }
      RefCount &rc = refs[ref];
      rc.first = std::min(rc.first, sv);
      rc.last = std::max(rc.last, ev);
      (r.unmapped ? rc.n_unmapped : rc.n_mapped)++;
      if (indexed) rc.max_end = std::max(rc.max_end, (uint64_t)r.pos + r.span);
    }
    std::vector<uint64_t> win_off(n_ref + 1, 0);
    for (uint32_t r = 0; r < n_ref; r++) win_off[r + 1] = win_off[r] + (refs[r].max_end ? 1 + ((refs[r].max_end - 1) >> 14) : 0);
    std::vector<uint64_t> win(win_off[n_ref], ~0ull);
    for (const Rec &r : recs) {
      if (r.ref < 0 || r.pos < 0) continue;
      const uint64_t sv = V.at(r.off), end = (uint64_t)r.pos + r.span;
      for (uint64_t w = (uint64_t)r.pos >> 14; w <= (end - 1) >> 14; w++) win[win_off[r.ref] + w] = std::min(win[win_off[r.ref] + w], sv);
    }
    uint64_t n_chunks = 0;
    hand_over(assemble_bai(n_ref, runs, refs, win, win_off, V.at(len), n_no_coor, &n_chunks), out, out_len);
  });
}

}  // extern "C"
