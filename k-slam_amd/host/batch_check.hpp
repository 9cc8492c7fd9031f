// batch_check.hpp -- do a batch's arrays hold together?  The one check in front of everything that indexes with a batch's numbers:
// the device entries that take a batch from the host (csrc/api_*.hip: kslam_*_add) and their host twins (host/*.cpp:
// kslam_tail_*).  Plain C++17, header only, no GPU: it needs include/kslam.h and nothing else of the library.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/kslam.h"

namespace kslam_batch {

// how far the check goes; each level includes the ones before it
enum class Level {
  groups,    // the groups' slices lie inside the pairs array, ascend and do not overlap
  pairs,     // + fewer than 2^32 overlap records, and every live alignment pair's r1 / r2 names one of them
  records,   // + the read offsets ascend, every named record's CIGAR slice lies inside the pool and its read exists
};

struct Arrays {
  const kslam_overlap *overlaps;       // not read below Level::records
  uint64_t n_overlaps;
  uint64_t n_cigar;                    // words in the CIGAR pool (the pool itself is not read)
  const uint64_t *read_offsets;        // [n_reads + 1]
  uint64_t n_reads;
  const kslam_read_pair *read_pairs;   // the groups
  uint64_t n_read_pairs;
  const kslam_paired_overlap *pairs;
  uint64_t n_pairs;
};

struct Ignore {
  void operator()(uint32_t) const {}
};

// "" when the arrays hold together, otherwise what is wrong with them (a KSLAM_ERR_ARG for every caller).  From Level::pairs on,
// `named` is called with the index of every overlap record a live alignment pair names, once per naming and after the record
// passed; at Level::records *longest_read receives the longest read's length.  No sum is formed that could wrap around.
template <typename Named = Ignore>
std::string check(const Arrays &a, Level level, uint64_t *longest_read = nullptr, Named &&named = Named{}) {
  using std::to_string;
  if (longest_read) *longest_read = 0;
  if (level >= Level::pairs && a.n_overlaps >= (1ull << 32)) return "2^32 or more overlap records";
  if (level >= Level::records) {
    uint64_t longest = 0;
    for (uint64_t i = 0; i < a.n_reads; i++) {
      if (a.read_offsets[i + 1] < a.read_offsets[i]) return "the read offsets must ascend";
      longest = std::max(longest, a.read_offsets[i + 1] - a.read_offsets[i]);
    }
    if (longest_read) *longest_read = longest;
  }
  uint64_t next = 0;
  for (uint64_t g = 0; g < a.n_read_pairs; g++) {
    const kslam_read_pair &rp = a.read_pairs[g];
    if (rp.first > a.n_pairs || rp.count > a.n_pairs - rp.first) return "read pair " + to_string(g) + ": first + count lies outside the pairs array";
    if (rp.first < next) return "read pair " + to_string(g) + ": the groups' slices must ascend and not overlap";
    next = rp.first + rp.count;
    if (level < Level::pairs) continue;
    for (uint64_t k = rp.first; k < next; k++)
      for (uint32_t idx : {a.pairs[k].r1, a.pairs[k].r2}) {
        if (idx == KSLAM_NO_OVERLAP) continue;
        if (idx >= a.n_overlaps) return "alignment pair " + to_string(k) + " refers to overlap record " + to_string(idx) + " of " + to_string(a.n_overlaps);
        if (level >= Level::records) {
          const kslam_overlap &o = a.overlaps[idx];
          if (o.cigar_off > a.n_cigar || o.cigar_len > a.n_cigar - o.cigar_off)
            return "overlap record " + to_string(idx) + ": its CIGAR slice lies outside the pool";
          if (o.read >= a.n_reads) return "overlap record " + to_string(idx) + " refers to read " + to_string(o.read) + " of " + to_string(a.n_reads);
        }
        named(idx);
      }
  }
  return std::string();
}

}  // namespace kslam_batch
