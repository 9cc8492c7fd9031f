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
#include "batch_check.hpp"
#include "workers.hpp"

namespace {
using namespace kslam_host;

// does the record's CIGAR stay inside its read and its entry?  (the whole CIGAR, before anything is emitted)
bool fits(const kslam_overlap &o, const uint32_t *pool, int64_t read_len, int64_t ref_len) {
  int64_t rp = o.ref_begin, qp = o.query_begin > 0 ? o.query_begin : 0;
  for (uint32_t k = 0; k < o.cigar_len; k++) {
    const uint32_t c = pool[o.cigar_off + k], op = c & 15u;
    const int64_t len = c >> 4;
    if (op == 0) {
      if (rp + len > ref_len || qp + len > read_len) return false;
      rp += len;
      qp += len;
    } else if (op == 1) {
      if (qp + len > read_len) return false;
      qp += len;
    } else if (op == 2) {
      if (rp + len > ref_len) return false;
      rp += len;
    }
  }
  return true;
}

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
    // ---- the contributing set: every overlap record a live alignment pair names, once ----
    std::vector<uint8_t> named(n_overlaps < (1ull << 32) ? n_overlaps : 0, 0);   // (2^32 or more: refused before anything is named)
    const std::string fault = kslam_batch::check({overlaps, n_overlaps, n_cigar, read_offsets, n_reads, read_pairs, n_read_pairs, pairs, n_pairs},
                                                 kslam_batch::Level::records, nullptr, [&](uint32_t idx) { named[idx] = 1; });
    if (!fault.empty()) fail(KSLAM_ERR_ARG, fault);
    // ---- the walk: per entry, the change of depth at each position (position `length` closes what reaches the last base) ----
    std::vector<std::map<uint64_t, int64_t>> change(n_entries);
    for (uint64_t i = 0; i < n_overlaps; i++) {
      if (!named[i]) continue;
      stats->n_records++;
      const kslam_overlap &o = overlaps[i];
      if (o.entry >= n_entries || o.cigar_len == 0 || o.ref_begin < 0) { stats->n_skipped++; continue; }
      const int64_t ref_len = (int64_t)(entry_offsets[o.entry + 1] - entry_offsets[o.entry]);
      const int64_t L = (int64_t)(read_offsets[o.read + 1] - read_offsets[o.read]);
      if (!fits(o, cigar_pool, L, ref_len)) { stats->n_skipped++; continue; }
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
    }
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
