// coverage.cpp -- include/kslam_coverage.h, the host side: the twin of csrc/coverage.hip (the same rows from host arrays, one
// serial pass, a byte per base where the device keeps a bit) and the report writer.  Plain C++, no GPU.
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#include "../../include/kslam_coverage.h"
#include "batch_check.hpp"
#include "workers.hpp"

namespace {
using namespace kslam_host;
}  // namespace

extern "C" kslam_status kslam_tail_coverage(const uint64_t *entry_lengths, uint64_t n_entries, const kslam_overlap *overlaps, uint64_t n_overlaps,
                                            const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                                            uint64_t n_pairs, kslam_entry_coverage *rows, uint64_t *n_skipped) {
  return guarded([&] {
    if ((n_entries && (!entry_lengths || !rows)) || !n_skipped || (n_overlaps && !overlaps) || (n_read_pairs && !read_pairs) || (n_pairs && !pairs))
      fail(KSLAM_ERR_ARG, "null argument");
    const std::string fault = kslam_batch::check({overlaps, n_overlaps, 0, nullptr, 0, read_pairs, n_read_pairs, pairs, n_pairs}, kslam_batch::Level::pairs);
    if (!fault.empty()) fail(KSLAM_ERR_ARG, fault);
    *n_skipped = 0;
    if (n_entries) memset(rows, 0, sizeof(kslam_entry_coverage) * n_entries);
    std::vector<uint64_t> base(n_entries + 1, 0);
    for (uint64_t e = 0; e < n_entries; e++) base[e + 1] = base[e] + entry_lengths[e];
    std::vector<uint8_t> seen(base[n_entries] + 1, 0);
    for (uint64_t g = 0; g < n_read_pairs; g++) {
      const kslam_read_pair &rp = read_pairs[g];
      bool one_entry = true;
      for (uint64_t k = rp.first; k < rp.first + rp.count; k++) {
        const kslam_paired_overlap &p = pairs[k];
        if (p.entry != pairs[rp.first].entry) one_entry = false;
        if (p.entry < n_entries) rows[p.entry].alignments++;
        for (uint32_t idx : {p.r1, p.r2}) {
          if (idx == KSLAM_NO_OVERLAP) continue;
          const kslam_overlap &o = overlaps[idx];
          if (o.entry >= n_entries || o.ref_begin < 0 || o.ref_end < o.ref_begin || (uint64_t)o.ref_end >= entry_lengths[o.entry]) {
            ++*n_skipped;
            continue;
          }
          rows[o.entry].aligned_bases += (uint64_t)(o.ref_end - o.ref_begin) + 1;
          uint8_t *s = seen.data() + base[o.entry];
          for (int64_t at = o.ref_begin; at <= o.ref_end; at++)
            if (!s[at]) {
              s[at] = 1;
              rows[o.entry].covered_bases++;
            }
        }
      }
      if (rp.count && one_entry && pairs[rp.first].entry < n_entries) rows[pairs[rp.first].entry].unique_read_pairs++;
    }
  });
}

extern "C" kslam_status kslam_coverage_write(const kslam_index_view *index, const kslam_entry_coverage *rows, uint64_t n_entries, int fd) {
  return guarded([&] {
    if (!index || !index->bases_off || !index->locus_tag_off || !index->taxonomy_id || (n_entries && !rows)) fail(KSLAM_ERR_ARG, "null argument");
    if (n_entries != index->n_entries) fail(KSLAM_ERR_ARG, "the rows are not of this index");
    std::string text = "#entry\tlocus\ttaxid\tlength\talignments\tunique_read_pairs\taligned_bases\tcovered_bases\tbreadth\tmean_depth\n";
    char num[256];
    for (uint64_t e = 0; e < n_entries; e++) {
      const kslam_entry_coverage &r = rows[e];
      if (!r.alignments) continue;
      const uint64_t len = index->bases_off[e + 1] - index->bases_off[e];
      text += std::to_string(e);
      text += '\t';
      text.append(index->locus_tag + index->locus_tag_off[e], index->locus_tag_off[e + 1] - index->locus_tag_off[e]);
      snprintf(num, sizeof num, "\t%u\t%llu\t%llu\t%llu\t%llu\t%llu\t%.6f\t%.4f\n", index->taxonomy_id[e], (unsigned long long)len,
               (unsigned long long)r.alignments, (unsigned long long)r.unique_read_pairs, (unsigned long long)r.aligned_bases,
               (unsigned long long)r.covered_bases, len ? (double)r.covered_bases / (double)len : 0.0,
               len ? (double)r.aligned_bases / (double)len : 0.0);
      text += num;
    }
    const char *p = text.data();
    size_t n = text.size();
    while (n) {
      const ssize_t w = ::write(fd, p, n);
      if (w < 0) {
        if (errno == EINTR) continue;
        fail(KSLAM_ERR_ARG, std::string("writing the coverage report failed: ") + strerror(errno));
      }
      p += w;
      n -= (size_t)w;
    }
  });
}
