// variants.cpp -- include/kslam_variants.h, the host side: the twin of csrc/variants.hip (the same rows from host arrays, one
// serial walk, one std::map per site where the device sorts keys) and the VCF writer.  Plain C++, no GPU.
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <unistd.h>
#include <vector>

#include "../../include/kslam_variants.h"
#include "pileup_walk.hpp"
#include "workers.hpp"

namespace {
using namespace kslam_host;
using namespace kslam_pileup;

struct Counts { uint32_t fwd = 0, rev = 0; };

}  // namespace

extern "C" kslam_status kslam_tail_variants(const char *entry_bases, const uint64_t *entry_offsets, uint64_t n_entries,
                                            const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                                            const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads,
                                            const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                                            uint64_t n_pairs, uint32_t min_alt, uint32_t min_depth, kslam_variant_row **rows_out,
                                            uint64_t *n_rows, kslam_variant_stats *stats) {
  if (rows_out) *rows_out = nullptr;
  if (n_rows) *n_rows = 0;
  return guarded([&] {
    if (!rows_out || !n_rows || !stats || (n_entries && !entry_offsets) || (n_overlaps && !overlaps) || (n_cigar && !cigar_pool) ||
        (n_reads && !read_offsets) || (n_read_pairs && !read_pairs) || (n_pairs && !pairs))
      fail(KSLAM_ERR_ARG, "null argument");
    memset(stats, 0, sizeof *stats);
    if (n_reads && read_offsets[n_reads] && !read_bases) fail(KSLAM_ERR_ARG, "null argument");
    if (n_entries && entry_offsets[n_entries] && !entry_bases) fail(KSLAM_ERR_ARG, "null argument");
    // ---- the walk of the contributing set ----
    std::map<std::tuple<uint32_t, uint32_t, uint8_t>, Counts> sites;          // (entry, pos, alt): ascending as the rows do
    std::vector<std::vector<uint32_t>> begins(n_entries), ends(n_entries);     // per entry: the closed M intervals
    std::string query;
    const std::string fault = for_each_contributing_record({overlaps, n_overlaps, n_cigar, read_offsets, n_reads, read_pairs, n_read_pairs, pairs, n_pairs},
                                                           cigar_pool, entry_offsets, n_entries, stats->n_records, stats->n_skipped,
                                                           [&](const kslam_overlap &o, int64_t L, int64_t) {
      const uint8_t *ref = (const uint8_t *)entry_bases + entry_offsets[o.entry];
      oriented_query(query, (const uint8_t *)read_bases + read_offsets[o.read], L, o.revcomp != 0);
      int64_t rp = o.ref_begin, qp = o.query_begin > 0 ? o.query_begin : 0;
      for (uint32_t k = 0; k < o.cigar_len; k++) {
        const uint32_t c = cigar_pool[o.cigar_off + k], op = c & 15u;
        const int64_t len = c >> 4;
        if (op == 0) {
          if (len) {
            begins[o.entry].push_back((uint32_t)rp);
            ends[o.entry].push_back((uint32_t)(rp + len - 1));
            stats->n_intervals++;
          }
          for (int64_t j = 0; j < len; j++) {
            const uint8_t r = ref[rp + j], q = (uint8_t)query[(size_t)(qp + j)];
            if (acgt(r) < 4 && acgt(q) < 4 && r != q) {
              Counts &s = sites[std::make_tuple(o.entry, (uint32_t)(rp + j), q)];
              (o.revcomp ? s.rev : s.fwd)++;
              stats->n_events++;
            }
          }
          rp += len;
          qp += len;
        } else if (op == 1) {
          qp += len;
        } else if (op == 2) {
          rp += len;
        }
      }
    });
    if (!fault.empty()) fail(KSLAM_ERR_ARG, fault);
    stats->n_sites = sites.size();
    for (auto &v : begins) std::sort(v.begin(), v.end());
    for (auto &v : ends) std::sort(v.begin(), v.end());
    std::vector<kslam_variant_row> out;
    for (const auto &kv : sites) {
      const Counts &s = kv.second;
      if ((uint64_t)s.fwd + s.rev < min_alt) continue;
      const uint32_t e = std::get<0>(kv.first), pos = std::get<1>(kv.first);
      // the intervals that began at or before pos less those that ended before it
      const uint32_t depth = (uint32_t)((std::upper_bound(begins[e].begin(), begins[e].end(), pos) - begins[e].begin()) -
                                        (std::lower_bound(ends[e].begin(), ends[e].end(), pos) - ends[e].begin()));
      if (depth < min_depth) continue;
      kslam_variant_row r;
      memset(&r, 0, sizeof r);
      r.entry = e;
      r.pos = pos;
      r.ref = (uint8_t)entry_bases[entry_offsets[e] + pos];
      r.alt = std::get<2>(kv.first);
      r.alt_fwd = s.fwd;
      r.alt_rev = s.rev;
      r.depth = depth;
      out.push_back(r);
    }
    kslam_variant_row *p = (kslam_variant_row *)malloc(sizeof(kslam_variant_row) * (out.size() + 1));
    if (!p) fail(KSLAM_ERR_OOM, "out of host memory");
    if (!out.empty()) memcpy(p, out.data(), sizeof(kslam_variant_row) * out.size());
    *rows_out = p;
    *n_rows = out.size();
  });
}

extern "C" kslam_status kslam_variants_write(const kslam_index_view *index, const kslam_variant_row *rows, uint64_t n_rows,
                                             const kslam_variant_stats *stats, int fd) {
  (void)stats;
  return guarded([&] {
    if (!index || !index->bases_off || !index->locus_tag_off || (n_rows && !rows)) fail(KSLAM_ERR_ARG, "null argument");
    auto locus = [&](uint64_t e) { return std::string(index->locus_tag + index->locus_tag_off[e], index->locus_tag_off[e + 1] - index->locus_tag_off[e]); };
    // nothing is written for rows that cannot become lines
    for (uint64_t i = 0; i < n_rows; i++) {
      if (rows[i].entry >= index->n_entries) fail(KSLAM_ERR_ARG, "row " + std::to_string(i) + ": entry " + std::to_string(rows[i].entry) + " is not of this index");
      if (index->locus_tag_off[rows[i].entry + 1] == index->locus_tag_off[rows[i].entry])
        fail(KSLAM_ERR_ARG, "entry " + std::to_string(rows[i].entry) + " has an empty locus: a VCF line needs a CHROM");
      if (i && rows[i].entry < rows[i - 1].entry) fail(KSLAM_ERR_ARG, "the rows must ascend by entry");
    }
    const char *version = kslam_version();
    std::string text = "##fileformat=VCFv4.2\n##source=";
    text.append(version, strcspn(version, " \t\n"));
    text += '\n';
    for (uint64_t i = 0; i < n_rows; i++) {
      if (i && rows[i].entry == rows[i - 1].entry) continue;
      const uint64_t e = rows[i].entry;
      text += "##contig=<ID=" + locus(e) + ",length=" + std::to_string(index->bases_off[e + 1] - index->bases_off[e]) + ">\n";
    }
    text += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Aligned reads with a match or mismatch column at the site\">\n"
            "##INFO=<ID=AO,Number=A,Type=Integer,Description=\"Alternate allele observations\">\n"
            "##INFO=<ID=SAF,Number=A,Type=Integer,Description=\"Alternate allele observations on the forward strand\">\n"
            "##INFO=<ID=SAR,Number=A,Type=Integer,Description=\"Alternate allele observations on the reverse strand\">\n"
            "##INFO=<ID=AF,Number=A,Type=Float,Description=\"Alternate allele observations over depth\">\n"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    char num[256];
    for (uint64_t i = 0; i < n_rows; i++) {
      const kslam_variant_row &r = rows[i];
      const uint64_t ao = (uint64_t)r.alt_fwd + r.alt_rev;
      text += locus(r.entry);
      snprintf(num, sizeof num, "\t%llu\t.\t%c\t%c\t.\t.\tDP=%u;AO=%llu;SAF=%u;SAR=%u;AF=%.6f\n", (unsigned long long)r.pos + 1, (char)r.ref, (char)r.alt,
               r.depth, (unsigned long long)ao, r.alt_fwd, r.alt_rev, r.depth ? (double)ao / (double)r.depth : 0.0);
      text += num;
    }
    const char *p = text.data();
    size_t n = text.size();
    while (n) {
      const ssize_t w = ::write(fd, p, n);
      if (w < 0) {
        if (errno == EINTR) continue;
        fail(KSLAM_ERR_ARG, std::string("writing the VCF file failed: ") + strerror(errno));
      }
      p += w;
      n -= (size_t)w;
    }
  });
}
