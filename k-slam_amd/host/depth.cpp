// depth.cpp -- include/kslam_depth.h, the host side: the twin of csrc/depth.hip (the same rows from host arrays, one serial walk,
// one std::map of boundaries where the device sorts, reduces and merges keys) and the bedGraph writer.  Plain C++, no GPU.
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <unistd.h>
#include <vector>

#include "../../include/kslam_depth.h"
#include "pileup_walk.hpp"
#include "workers.hpp"

namespace {
using namespace kslam_host;
using namespace kslam_pileup;
}  // namespace

extern "C" kslam_status kslam_tail_depth(const uint64_t *entry_offsets, uint64_t n_entries, const kslam_overlap *overlaps, uint64_t n_overlaps,
                                         const uint32_t *cigar_pool, uint64_t n_cigar, const uint64_t *read_offsets, uint64_t n_reads,
                                         const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                                         uint64_t n_pairs, uint32_t min_depth, kslam_depth_row **rows_out, uint64_t *n_rows,
                                         kslam_depth_stats *stats) {
  if (rows_out) *rows_out = nullptr;
  if (n_rows) *n_rows = 0;
  return guarded([&] {
    if (!rows_out || !n_rows || !stats || (n_entries && !entry_offsets) || (n_overlaps && !overlaps) || (n_cigar && !cigar_pool) ||
        (n_reads && !read_offsets) || (n_read_pairs && !read_pairs) || (n_pairs && !pairs))
      fail(KSLAM_ERR_ARG, "null argument");
    memset(stats, 0, sizeof *stats);
    // ---- the walk of the contributing set: per entry, the change of depth at each position (position `length` closes what
    // reaches the last base) ----
    std::vector<std::map<uint64_t, int64_t>> change(n_entries);
    const std::string fault = for_each_contributing_record({overlaps, n_overlaps, n_cigar, read_offsets, n_reads, read_pairs, n_read_pairs, pairs, n_pairs},
                                                           cigar_pool, entry_offsets, n_entries, stats->n_records, stats->n_skipped,
                                                           [&](const kslam_overlap &o, int64_t, int64_t) {
      uint64_t rp = (uint64_t)o.ref_begin;
      for (uint32_t k = 0; k < o.cigar_len; k++) {
        const uint32_t c = cigar_pool[o.cigar_off + k], op = c & 15u, len = c >> 4;
        if (op == 0) {
          if (len) {
            change[o.entry][rp]++;
            change[o.entry][rp + len]--;
            stats->n_intervals++;
          }
          rp += len;
        } else if (op == 2) {
          rp += len;
        }
      }
    });
    if (!fault.empty()) fail(KSLAM_ERR_ARG, fault);
    const uint64_t floor = min_depth ? min_depth : 1;
    std::vector<kslam_depth_row> out;
    for (uint64_t e = 0; e < n_entries; e++) {
      int64_t depth = 0;
      uint64_t from = 0;
      for (const auto &kv : change[e]) {
        if (kv.second == 0) continue;   // begins and ends cancel: no boundary
        stats->n_keys++;
        if (depth > 0) {
          stats->n_rows++;
          stats->covered_bases += kv.first - from;
          stats->max_depth = std::max<uint64_t>(stats->max_depth, (uint64_t)depth);
          if ((uint64_t)depth >= floor) out.push_back(kslam_depth_row{(uint32_t)e, (uint32_t)from, (uint32_t)kv.first, (uint32_t)std::min<int64_t>(depth, 0xFFFFFFFFll)});
        }
        depth += kv.second;
        from = kv.first;
      }
    }
    kslam_depth_row *p = (kslam_depth_row *)malloc(sizeof(kslam_depth_row) * (out.size() + 1));
    if (!p) fail(KSLAM_ERR_OOM, "out of host memory");
    if (!out.empty()) memcpy(p, out.data(), sizeof(kslam_depth_row) * out.size());
    *rows_out = p;
    *n_rows = out.size();
  });
}

extern "C" kslam_status kslam_depth_write(const kslam_index_view *index, const kslam_depth_row *rows, uint64_t n_rows, int fd) {
  return guarded([&] {
    if (!index || !index->locus_tag_off || (n_rows && !rows)) fail(KSLAM_ERR_ARG, "null argument");
    // nothing is written for rows that cannot become lines
    for (uint64_t i = 0; i < n_rows; i++) {
      if (rows[i].entry >= index->n_entries) fail(KSLAM_ERR_ARG, "row " + std::to_string(i) + ": entry " + std::to_string(rows[i].entry) + " is not of this index");
      if (index->locus_tag_off[rows[i].entry + 1] == index->locus_tag_off[rows[i].entry])
        fail(KSLAM_ERR_ARG, "entry " + std::to_string(rows[i].entry) + " has an empty locus: a bedGraph line needs a chromosome");
    }
    std::string text;
    char num[96];
    for (uint64_t i = 0; i < n_rows; i++) {
      const kslam_depth_row &r = rows[i];
      text.append(index->locus_tag + index->locus_tag_off[r.entry], index->locus_tag_off[r.entry + 1] - index->locus_tag_off[r.entry]);
      snprintf(num, sizeof num, "\t%u\t%u\t%u\n", r.start, r.end, r.depth);
      text += num;
    }
    const char *p = text.data();
    size_t n = text.size();
    while (n) {
      const ssize_t w = ::write(fd, p, n);
      if (w < 0) {
        if (errno == EINTR) continue;
        fail(KSLAM_ERR_ARG, std::string("writing the depth file failed: ") + strerror(errno));
      }
      p += w;
      n -= (size_t)w;
    }
  });
}
