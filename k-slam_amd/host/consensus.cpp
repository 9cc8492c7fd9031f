// consensus.cpp -- include/kslam_consensus.h, the host side: the twin of csrc/consensus.hip (the same rows and sequences from host
// arrays, one serial walk into dense per-position counters of the touched entries and one std::map of insertions, where the
// device sorts keys and searches them) and the FASTA writer.  Plain C++, no GPU.
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <unistd.h>
#include <vector>

#include "../../include/kslam_consensus.h"
#include "pileup_walk.hpp"
#include "workers.hpp"

namespace {
using namespace kslam_host;
using namespace kslam_pileup;

struct Column { uint32_t m = 0, dl = 0, ev[5] = {0, 0, 0, 0, 0}; };

void check_params(const kslam_consensus_params *p) {
  if (!p) fail(KSLAM_ERR_ARG, "null argument");
  if (p->min_depth < 1) fail(KSLAM_ERR_ARG, "consensus: min_depth must be at least 1");
  if (p->call_permille < 500 || p->call_permille > 999) fail(KSLAM_ERR_ARG, "consensus: call_permille must lie in 500 .. 999");
  if (p->fill != KSLAM_CONSENSUS_FILL_N && p->fill != KSLAM_CONSENSUS_FILL_REF) fail(KSLAM_ERR_ARG, "consensus: fill must be N (0) or REF (1)");
}

}  // namespace

extern "C" kslam_status kslam_tail_consensus(const char *entry_bases, const uint64_t *entry_offsets, uint64_t n_entries,
                                             const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                                             const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads,
                                             const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                                             uint64_t n_pairs, const kslam_consensus_params *params, kslam_consensus_row **rows_out,
                                             uint64_t *n_rows, char **seq_out, kslam_consensus_stats *stats) {
  if (rows_out) *rows_out = nullptr;
  if (n_rows) *n_rows = 0;
  if (seq_out) *seq_out = nullptr;
  return guarded([&] {
    if (!rows_out || !n_rows || !seq_out || !stats || (n_entries && !entry_offsets) || (n_overlaps && !overlaps) || (n_cigar && !cigar_pool) ||
        (n_reads && !read_offsets) || (n_read_pairs && !read_pairs) || (n_pairs && !pairs))
      fail(KSLAM_ERR_ARG, "null argument");
    memset(stats, 0, sizeof *stats);
    check_params(params);
    if (n_reads && read_offsets[n_reads] && !read_bases) fail(KSLAM_ERR_ARG, "null argument");
    if (n_entries && entry_offsets[n_entries] && !entry_bases) fail(KSLAM_ERR_ARG, "null argument");
    // ---- the walk of the contributing set: dense counters for the entries it touches ----
    std::vector<std::vector<Column>> cols(n_entries);
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, std::string>, uint64_t> ins;   // (entry, anchor, len, bases): ascending as the device's keys
    std::string query;
    const std::string fault = for_each_contributing_record({overlaps, n_overlaps, n_cigar, read_offsets, n_reads, read_pairs, n_read_pairs, pairs, n_pairs},
                                                           cigar_pool, entry_offsets, n_entries, stats->n_records, stats->n_skipped,
                                                           [&](const kslam_overlap &o, int64_t L, int64_t ref_len) {
      const uint8_t *ref = (const uint8_t *)entry_bases + entry_offsets[o.entry];
      oriented_query(query, (const uint8_t *)read_bases + read_offsets[o.read], L, o.revcomp != 0);
      std::vector<Column> &col = cols[o.entry];
      int64_t rp = o.ref_begin, qp = o.query_begin > 0 ? o.query_begin : 0;
      for (uint32_t k = 0; k < o.cigar_len; k++) {
        const uint32_t c = cigar_pool[o.cigar_off + k], op = c & 15u;
        const int64_t len = c >> 4;
        if (op == 0) {
          if (len) {
            stats->n_intervals++;
            if (col.empty()) col.resize((size_t)ref_len);
          }
          for (int64_t j = 0; j < len; j++) {
            const uint8_t q = (uint8_t)query[(size_t)(qp + j)];
            Column &at = col[(size_t)(rp + j)];
            at.m++;
            if (ref[rp + j] != q) {
              at.ev[acgt(q)]++;
              stats->n_events++;
            }
          }
          rp += len;
          qp += len;
        } else if (op == 1) {
          if (len) {
            const std::string run = query.substr((size_t)qp, (size_t)len);
            const bool plain = std::all_of(run.begin(), run.end(), [](char b) { return acgt((uint8_t)b) < 4; });
            if (rp <= o.ref_begin) stats->n_ins_unanchored++;
            else if (len > (int64_t)KSLAM_CONSENSUS_MAX_INS || !plain) stats->n_ins_unrepresentable++;
            else {
              ins[std::make_tuple(o.entry, (uint32_t)(rp - 1), (uint32_t)len, run)]++;
              stats->n_insertions++;
            }
          }
          qp += len;
        } else if (op == 2) {
          if (len) {
            stats->n_del_intervals++;
            if (col.empty()) col.resize((size_t)ref_len);
          }
          for (int64_t j = 0; j < len; j++) col[(size_t)(rp + j)].dl++;
          rp += len;
        }
      }
    });
    if (!fault.empty()) fail(KSLAM_ERR_ARG, fault);
    // ---- the call ----
    const uint64_t min_covered = params->min_covered ? params->min_covered : 1;
    std::vector<kslam_consensus_row> out;
    std::string seq, one;
    auto it = ins.begin();
    for (uint64_t e = 0; e < n_entries; e++) {
      const std::vector<Column> &col = cols[e];
      if (col.empty()) continue;   // not touched (an entry of length 0 holds no run)
      stats->n_entries_touched++;
      const uint8_t *ref = (const uint8_t *)entry_bases + entry_offsets[e];
      kslam_consensus_row r;
      memset(&r, 0, sizeof r);
      r.entry = (uint32_t)e;
      r.entry_len = col.size();
      one.clear();
      while (it != ins.end() && std::get<0>(it->first) < e) ++it;
      for (size_t pos = 0; pos < col.size(); pos++) {
        const Column &at = col[pos];
        const uint64_t d = (uint64_t)at.m + at.dl;
        // (the insertions anchored here come next in the map, whether the position is covered or not)
        auto first = it;
        while (it != ins.end() && std::get<0>(it->first) == e && std::get<1>(it->first) == pos) ++it;
        if (d < params->min_depth) {
          one += params->fill == KSLAM_CONSENSUS_FILL_REF ? (char)ref[pos] : 'N';
          continue;
        }
        r.covered++;
        const uint64_t need = d * params->call_permille;
        const uint64_t refc = at.m - ((uint64_t)at.ev[0] + at.ev[1] + at.ev[2] + at.ev[3] + at.ev[4]);
        int won = 5;
        for (int b = 0; b < 4; b++)
          if (((uint64_t)at.ev[b] + (acgt(ref[pos]) == b ? refc : 0)) * 1000 > need) won = b;
        if ((uint64_t)at.dl * 1000 > need) won = 4;
        if (won < 4) {
          one += "ACGT"[won];
          if ((uint8_t)"ACGT"[won] != ref[pos]) r.substitutions++;
        } else if (won == 4) {
          r.deleted++;
        } else {
          one += 'N';
          r.ambiguous++;
        }
        for (auto j = first; j != it; ++j)   // ascending by length, then by the string: the first that passes
          if (j->second * 1000 > need) {
            one += std::get<3>(j->first);
            r.insertions++;
            r.inserted_bases += std::get<2>(j->first);
            break;
          }
      }
      if (r.covered < min_covered) continue;
      r.seq_off = seq.size();
      r.seq_len = one.size();
      seq += one;
      out.push_back(r);
    }
    stats->n_entries_reported = out.size();
    kslam_consensus_row *p = (kslam_consensus_row *)malloc(sizeof(kslam_consensus_row) * (out.size() + 1));
    char *sq = (char *)malloc(seq.size() + 1);
    if (!p || !sq) {
      free(p);
      free(sq);
      fail(KSLAM_ERR_OOM, "out of host memory");
    }
    if (!out.empty()) memcpy(p, out.data(), sizeof(kslam_consensus_row) * out.size());
    memcpy(sq, seq.data(), seq.size());
    sq[seq.size()] = 0;
    *rows_out = p;
    *seq_out = sq;
    *n_rows = out.size();
  });
}

extern "C" kslam_status kslam_consensus_write(const kslam_index_view *index, const kslam_consensus_row *rows, uint64_t n_rows, const char *seq, int fd) {
  return guarded([&] {
    if (!index || !index->locus_tag_off || (n_rows && !rows)) fail(KSLAM_ERR_ARG, "null argument");
    auto locus = [&](uint64_t e) { return std::string(index->locus_tag + index->locus_tag_off[e], index->locus_tag_off[e + 1] - index->locus_tag_off[e]); };
    // nothing is written for rows that cannot become records
    for (uint64_t i = 0; i < n_rows; i++) {
      if (rows[i].entry >= index->n_entries) fail(KSLAM_ERR_ARG, "row " + std::to_string(i) + ": entry " + std::to_string(rows[i].entry) + " is not of this index");
      if (index->locus_tag_off[rows[i].entry + 1] == index->locus_tag_off[rows[i].entry])
        fail(KSLAM_ERR_ARG, "entry " + std::to_string(rows[i].entry) + " has an empty locus: a FASTA record needs a name");
      if (rows[i].seq_len && !seq) fail(KSLAM_ERR_ARG, "null argument");
    }
    std::string text;
    char num[320];
    for (uint64_t i = 0; i < n_rows; i++) {
      const kslam_consensus_row &r = rows[i];
      text += '>';
      text += locus(r.entry);
      snprintf(num, sizeof num, " kslam_consensus entry_length=%llu covered=%llu substitutions=%llu deletions=%llu insertions=%llu ambiguous=%llu\n",
               (unsigned long long)r.entry_len, (unsigned long long)r.covered, (unsigned long long)r.substitutions, (unsigned long long)r.deleted,
               (unsigned long long)r.insertions, (unsigned long long)r.ambiguous);
      text += num;
      for (uint64_t at = 0; at < r.seq_len; at += 60) {
        text.append(seq + r.seq_off + at, (size_t)std::min<uint64_t>(60, r.seq_len - at));
        text += '\n';
      }
    }
    const char *p = text.data();
    size_t n = text.size();
    while (n) {
      const ssize_t w = ::write(fd, p, n);
      if (w < 0) {
        if (errno == EINTR) continue;
        fail(KSLAM_ERR_ARG, std::string("writing the consensus file failed: ") + strerror(errno));
      }
      p += w;
      n -= (size_t)w;
    }
  });
}
