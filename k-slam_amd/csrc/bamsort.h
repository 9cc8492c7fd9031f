// bamsort.h -- interface of bamsort.hip (the coordinate-sorted BAM and its index, include/kslam_bamsort.h) and the state behind
// kslam_ctx::bsort / bsort_w (api_bamsort.hip)
#pragma once
#include <mutex>
#include <vector>

#include "common.h"
#include "bgzf.h"

namespace kslam {

constexpr uint64_t BAMSORT_SLAB = 256ull << 20;              // a slab of the store; a larger batch gets a slab of its own
constexpr uint64_t BAMSORT_DEFAULT_SLICE = 16448ull * BGZF_MEMBER_IN;   // about 1 GiB of the sorted stream
constexpr uint32_t BAMSORT_DEFAULT_SEGMENT = 64;
constexpr uint32_t BAMSORT_NO_BIN = 0xFFFFFFFFu;
constexpr uint32_t BAMSORT_UNMAPPED = 1u << 31;              // in BamSortCols::meta, above max(1, reflen)

struct BamSortCols {   // a batch's record index inside its slab, n entries each
  uint64_t *off;       // of the record inside the batch's bytes
  uint32_t *len;       // block_size + 4
  uint32_t *ref;       // refID, n_ref for a refID outside 0 .. n_ref - 1
  uint32_t *pos1;      // pos + 1
  uint32_t *meta;      // max(1, reflen), clamped to 2^29, | BAMSORT_UNMAPPED
};

struct BamSortWork {   // the record-index passes of one appender: a lane, or the owner's kslam_bam_sort_add
  DevBuf seg, cnt, first, scan_tmp, totals;
  hipEvent_t ev[2]{};
  double ms = 0;
  BamSortWork() = default;
  BamSortWork(const BamSortWork &) = delete;
  BamSortWork &operator=(const BamSortWork &) = delete;
  ~BamSortWork() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// Segment i of the chain is data[base + seg_off[i] .. base + seg_off[i + 1]) and the last one ends at `end`; every segment is a
// whole number of records.  Counts the records of each into cnt[i] (u32).
void bamsort_count_device(const uint8_t *data, const uint64_t *seg_off, uint64_t n_seg, uint64_t base, uint64_t end, uint32_t *cnt, hipStream_t s);
// ... and writes the columns of segment i's records from entry first[i] on
void bamsort_write_device(const uint8_t *data, const uint64_t *seg_off, uint64_t n_seg, uint64_t base, uint64_t end, const uint32_t *first,
                          uint32_t n_ref, BamSortCols cols, hipStream_t s);

// One batch's n records as sort records keys[at .. at + n) = {pos + 1, ref, at + i, 0} with their place in the store (src) and
// their columns for the index
void bamsort_keys_device(BamSortCols cols, const uint8_t *bytes, uint64_t n, uint64_t at, uint4 *keys, uint64_t *src, uint32_t *len, uint32_t *meta,
                         hipStream_t s);
// the sorted order's sources and lengths: s_src[i] = src[keys[i].z], s_len[i] = len[keys[i].z]
void bamsort_order_device(const uint4 *keys, const uint64_t *src, const uint32_t *len, uint64_t n, uint64_t *s_src, uint32_t *s_len, hipStream_t s);
// range[0] = the first record that ends behind a, range[1] = the first that starts at or behind b (dst_off: n + 1 ascending offsets)
void bamsort_range_device(const uint64_t *dst_off, uint64_t n, uint64_t a, uint64_t b, uint64_t *range, hipStream_t s);
// The gather: records i0 .. i1 of the sorted order, clipped to the stream's bytes [a, b), into out[0 .. b - a).  lanes: 16 or 64
// lanes per record, or 1: the baseline, one thread per record running the same copy.
void bamsort_gather_device(const uint64_t *s_src, const uint64_t *dst_off, uint64_t i0, uint64_t i1, uint64_t a, uint64_t b, uint8_t *out, uint32_t lanes,
                           hipStream_t s);

struct BamSortIndexIn {
  const uint4 *keys;          // sorted
  const uint32_t *meta;       // by keys[i].z
  const uint64_t *dst_off;    // n + 1
  uint64_t n;
  uint32_t n_ref;
  const uint64_t *member_off; // n_members + 1: compressed bytes of the record members before each
  uint64_t n_members, header_clen, total;
  const uint64_t *win_off;    // n_ref + 1
};
struct BamSortRun {           // as kslam_bamsort::Run without its end
  uint32_t ref, bin;
  uint64_t beg;
};
struct BamSortIndexOut {
  uint64_t *win;              // win_off[n_ref] windows, preset to ~0
  uint64_t *ref_first, *ref_last, *ref_mapped, *ref_unmapped, *ref_max_end;   // n_ref each; first preset to ~0, the others to 0
  uint64_t *first_no_coor;    // preset to n
  uint32_t *head;             // n
};
// pass 1: per record its windows, its reference's counters and whether it starts a run of equal (ref, bin)
void bamsort_index_device(const BamSortIndexIn &in, const BamSortIndexOut &out, hipStream_t s);
// pass 2, after an exclusive scan of head into run_at: the run heads compacted
void bamsort_runs_device(const BamSortIndexIn &in, const uint32_t *head, const uint32_t *run_at, BamSortRun *runs, hipStream_t s);

struct BamSortBatch {
  uint64_t seq = 0;
  size_t slab = 0;
  uint64_t at = 0, len = 0, n = 0;   // where in the slab the bytes lie, how many, the records
  BamSortCols cols{};
};

struct BamSortSlab {
  void *p = nullptr;
  uint64_t cap = 0, used = 0;
};

struct BamSortState {
  std::mutex mu;                      // add / the lanes' reservations / take / reset / the switch: one at a time
  uint32_t n_ref = 0;
  std::vector<uint64_t> ref_len;
  std::vector<BamSortSlab> slabs;
  std::vector<BamSortBatch> batches;  // in arrival order
  uint64_t base_ticket = 0;           // the ticket that is ordinal 0
  uint64_t slice = BAMSORT_DEFAULT_SLICE;
  uint32_t segment = BAMSORT_DEFAULT_SEGMENT, gather = 0;
  BamSortWork addw;                   // kslam_bam_sort_add's
  // take
  DevBuf keys_a, keys_b, src, len, meta, s_src, s_len, dst_off, slice_buf, out, hdr_in, member_off, win_off, win, refc, head, run_at, runs, range,
      scan_tmp, totals;
  SortWorkspace sortws;
  BgzfWork bgzfw;
  hipEvent_t ev[8]{};
  double ms[5] = {0, 0, 0, 0, 0};
  uint64_t bytes_held() const {
    uint64_t b = 0;
    for (const auto &s : slabs) b += s.cap;
    return b;
  }
};

}  // namespace kslam
