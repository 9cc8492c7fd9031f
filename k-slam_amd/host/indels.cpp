// indels.cpp -- include/kslam_indels.h, the host side: the twin of csrc/indels.hip (the same rows from host arrays, one serial
// walk, the normalisation on the bytes themselves where the device rotates a packed word, std::sort and a run reduction where
// the device sorts keys) and the VCF writer.  Plain C++, no GPU.
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <tuple>
#include <unistd.h>
#include <vector>

#include "../../include/kslam_indels.h"
#include "pileup_walk.hpp"
#include "workers.hpp"

namespace {
using namespace kslam_host;
using namespace kslam_pileup;

// (entry, anchor, kind, len, bases, strand): ascending as the rows do, the forward strand first inside a row
using Event = std::tuple<uint32_t, uint32_t, uint8_t, uint32_t, uint64_t, uint8_t>;

// the leftmost equivalent position of a deletion of ref[p .. p + len)
int64_t normalise_deletion(const uint8_t *ref, int64_t p, int64_t len) {
  while (p >= 2 && ref[p - 1] == ref[p + len - 1] && acgt(ref[p - 1]) < 4) p--;
  return p;
}
// ... of an insertion of s (upper-case ACGT alone) in front of ref[p]; s is rotated on the way
int64_t normalise_insertion(const uint8_t *ref, int64_t p, std::string &s) {
  while (p >= 2 && ref[p - 1] == (uint8_t)s.back()) {
    s.insert(s.begin(), s.back());
    s.pop_back();
    p--;
  }
  return p;
}

const char ACGT[] = "ACGT";

}  // namespace

extern "C" kslam_status kslam_tail_indels(const char *entry_bases, const uint64_t *entry_offsets, uint64_t n_entries,
                                          const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                                          const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads,
                                          const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                                          uint64_t n_pairs, uint32_t min_alt, uint32_t min_depth, kslam_indel_row **rows_out, uint64_t *n_rows,
                                          kslam_indel_stats *stats) {
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
    std::vector<Event> events;
    std::vector<std::vector<uint32_t>> begins(n_entries), ends(n_entries);   // per entry: the closed M intervals
    std::string query, s;
    const std::string fault = for_each_contributing_record({overlaps, n_overlaps, n_cigar, read_offsets, n_reads, read_pairs, n_read_pairs, pairs, n_pairs},
                                                           cigar_pool, entry_offsets, n_entries, stats->n_records, stats->n_skipped,
                                                           [&](const kslam_overlap &o, int64_t L, int64_t) {
      const uint8_t *ref = (const uint8_t *)entry_bases + entry_offsets[o.entry];
      oriented_query(query, (const uint8_t *)read_bases + read_offsets[o.read], L, o.revcomp != 0);
      const uint8_t strand = o.revcomp ? 1 : 0;
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
          rp += len;
          qp += len;
        } else if (op == 1) {
          if (len) {
            uint64_t w = 0;
            if (rp <= o.ref_begin) stats->n_unanchored++;
            else if (len > (int64_t)KSLAM_INDEL_MAX_INS || !insertion_bases(query, qp, len, &w)) stats->n_unrepresentable++;
            else {
              s.assign(query, (size_t)qp, (size_t)len);
              const int64_t p = normalise_insertion(ref, rp, s);
              (void)insertion_bases(s, 0, len, &w);
              events.emplace_back(o.entry, (uint32_t)(p - 1), (uint8_t)KSLAM_INDEL_INS, (uint32_t)len, w, strand);
              stats->n_insertions++;
            }
          }
          qp += len;
        } else if (op == 2) {
          if (len) {
            if (rp <= o.ref_begin) stats->n_unanchored++;
            else if (len > (int64_t)KSLAM_INDEL_MAX_DEL) stats->n_long_del++;
            else {
              const int64_t p = normalise_deletion(ref, rp, len);
              events.emplace_back(o.entry, (uint32_t)(p - 1), (uint8_t)KSLAM_INDEL_DEL, (uint32_t)len, (uint64_t)0, strand);
              stats->n_deletions++;
            }
          }
          rp += len;
        }
      }
    });
    if (!fault.empty()) fail(KSLAM_ERR_ARG, fault);
    std::sort(events.begin(), events.end());
    for (auto &v : begins) std::sort(v.begin(), v.end());
    for (auto &v : ends) std::sort(v.begin(), v.end());
    // ---- one row per run of events that are equal but for their strand ----
    std::vector<kslam_indel_row> out;
    for (size_t i = 0; i < events.size();) {
      size_t j = i;
      uint32_t fwd = 0, rev = 0;
      auto same = [&](const Event &a, const Event &b) {
        return std::get<0>(a) == std::get<0>(b) && std::get<1>(a) == std::get<1>(b) && std::get<2>(a) == std::get<2>(b) &&
               std::get<3>(a) == std::get<3>(b) && std::get<4>(a) == std::get<4>(b);
      };
      for (; j < events.size() && same(events[i], events[j]); j++) (std::get<5>(events[j]) ? rev : fwd)++;
      const Event &ev = events[i];
      i = j;
      stats->n_sites++;
      if ((uint64_t)fwd + rev < min_alt) continue;
      const uint32_t e = std::get<0>(ev), pos = std::get<1>(ev);
      // the intervals that began at or before pos less those that ended before it
      const uint32_t depth = (uint32_t)((std::upper_bound(begins[e].begin(), begins[e].end(), pos) - begins[e].begin()) -
                                        (std::lower_bound(ends[e].begin(), ends[e].end(), pos) - ends[e].begin()));
      if (depth < min_depth) continue;
      kslam_indel_row r;
      memset(&r, 0, sizeof r);
      r.entry = e;
      r.pos = pos;
      r.kind = std::get<2>(ev);
      r.len = std::get<3>(ev);
      r.bases = std::get<4>(ev);
      r.alt_fwd = fwd;
      r.alt_rev = rev;
      r.depth = depth;
      out.push_back(r);
    }
    kslam_indel_row *p = (kslam_indel_row *)malloc(sizeof(kslam_indel_row) * (out.size() + 1));
    if (!p) fail(KSLAM_ERR_OOM, "out of host memory");
    if (!out.empty()) memcpy(p, out.data(), sizeof(kslam_indel_row) * out.size());
    *rows_out = p;
    *n_rows = out.size();
  });
}

extern "C" kslam_status kslam_indels_write(const kslam_index_view *index, const kslam_indel_row *rows, uint64_t n_rows,
                                           const kslam_indel_stats *stats, int fd) {
  (void)stats;
  return guarded([&] {
    if (!index || !index->bases_off || !index->locus_tag_off || (n_rows && !rows)) fail(KSLAM_ERR_ARG, "null argument");
    auto locus = [&](uint64_t e) { return std::string(index->locus_tag + index->locus_tag_off[e], index->locus_tag_off[e + 1] - index->locus_tag_off[e]); };
    // nothing is written for rows that cannot become lines
    for (uint64_t i = 0; i < n_rows; i++) {
      const kslam_indel_row &r = rows[i];
      const std::string row = "row " + std::to_string(i) + ": ";
      if (r.entry >= index->n_entries) fail(KSLAM_ERR_ARG, row + "entry " + std::to_string(r.entry) + " is not of this index");
      if (index->locus_tag_off[r.entry + 1] == index->locus_tag_off[r.entry])
        fail(KSLAM_ERR_ARG, "entry " + std::to_string(r.entry) + " has an empty locus: a VCF line needs a CHROM");
      if (i && r.entry < rows[i - 1].entry) fail(KSLAM_ERR_ARG, "the rows must ascend by entry");
      const uint64_t entry_len = index->bases_off[r.entry + 1] - index->bases_off[r.entry];
      if (r.pos >= entry_len) fail(KSLAM_ERR_ARG, row + "pos " + std::to_string(r.pos) + " lies outside the entry");
      if (r.kind != KSLAM_INDEL_DEL && r.kind != KSLAM_INDEL_INS) fail(KSLAM_ERR_ARG, row + "kind " + std::to_string(r.kind) + " is none");
      if (r.len == 0 || (r.kind == KSLAM_INDEL_INS && r.len > KSLAM_INDEL_MAX_INS)) fail(KSLAM_ERR_ARG, row + "len " + std::to_string(r.len) + " is none");
      if (r.kind == KSLAM_INDEL_DEL && (uint64_t)r.pos + r.len >= entry_len)
        fail(KSLAM_ERR_ARG, row + "the deletion of " + std::to_string(r.len) + " bases behind pos " + std::to_string(r.pos) + " runs past the entry");
    }
    if (n_rows && !index->bases) fail(KSLAM_ERR_ARG, "null argument");
    const char *version = kslam_version();
    std::string text = "##fileformat=VCFv4.2\n##source=";
    text.append(version, strcspn(version, " \t\n"));
    text += '\n';
    for (uint64_t i = 0; i < n_rows; i++) {
      if (i && rows[i].entry == rows[i - 1].entry) continue;
      const uint64_t e = rows[i].entry;
      text += "##contig=<ID=" + locus(e) + ",length=" + std::to_string(index->bases_off[e + 1] - index->bases_off[e]) + ">\n";
    }
    text += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Aligned reads with a match or mismatch column at the anchor\">\n"
            "##INFO=<ID=AO,Number=A,Type=Integer,Description=\"Alternate allele observations\">\n"
            "##INFO=<ID=SAF,Number=A,Type=Integer,Description=\"Alternate allele observations on the forward strand\">\n"
            "##INFO=<ID=SAR,Number=A,Type=Integer,Description=\"Alternate allele observations on the reverse strand\">\n"
            "##INFO=<ID=AF,Number=A,Type=Float,Description=\"Alternate allele observations over depth (not clamped)\">\n"
            "##INFO=<ID=TYPE,Number=A,Type=String,Description=\"del or ins\">\n"
            "##INFO=<ID=LEN,Number=A,Type=Integer,Description=\"Deleted or inserted bases\">\n"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    char num[256];
    for (uint64_t i = 0; i < n_rows; i++) {
      const kslam_indel_row &r = rows[i];
      const uint64_t ao = (uint64_t)r.alt_fwd + r.alt_rev;
      const char *anchor = index->bases + index->bases_off[r.entry] + r.pos;
      text += locus(r.entry);
      text += '\t' + std::to_string((uint64_t)r.pos + 1) + "\t.\t";
      if (r.kind == KSLAM_INDEL_DEL) {
        text.append(anchor, (size_t)r.len + 1);
        text += '\t';
        text += *anchor;
      } else {
        text += *anchor;
        text += '\t';
        text += *anchor;
        for (uint32_t j = 0; j < r.len; j++) text += ACGT[(r.bases >> (2 * (r.len - 1 - j))) & 3u];
      }
      snprintf(num, sizeof num, "\t.\t.\tDP=%u;AO=%llu;SAF=%u;SAR=%u;AF=%.6f;TYPE=%s;LEN=%u\n", r.depth, (unsigned long long)ao, r.alt_fwd, r.alt_rev,
               r.depth ? (double)ao / (double)r.depth : 0.0, r.kind == KSLAM_INDEL_DEL ? "del" : "ins", r.len);
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
