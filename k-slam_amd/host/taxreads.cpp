// taxreads.cpp -- include/kslam_taxreads.h, the host twin: the set S of the chosen taxa from the tree's public accessors
// (kslam_taxdb_dense, kslam_taxdb_node), the matched read pairs in one serial pass, and the record bytes through the reads
// split's own twin (host/readsplit.cpp) -- the same plain bytes csrc/taxreads.hip selects.  Plain C++, no GPU.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/kslam_taxreads.h"
#include "../../include/kslam_tail.h"
#include "workers.hpp"

namespace {
using namespace kslam_host;
constexpr uint32_t NONE = 0xFFFFFFFFu;
}  // namespace

extern "C" kslam_status kslam_tail_taxon_reads(const kslam_taxdb *taxdb, const uint32_t *ids, uint64_t n, uint32_t mode, const char *r1, uint64_t len1,
                                               const char *r2, uint64_t len2, uint64_t max_pairs, int at_eof, const kslam_read_pair *read_pairs,
                                               const uint32_t *pair_tax_ids, uint64_t n_read_pairs, kslam_reads_out *out) {
  if (out) memset(out, 0, sizeof *out);
  std::vector<kslam_read_pair> matched;
  bool exclude = false;
  const kslam_status st = guarded([&] {
    if (!out || !taxdb || !ids || (n_read_pairs && (!read_pairs || !pair_tax_ids))) fail(KSLAM_ERR_ARG, "null argument");
    if (!n) fail(KSLAM_ERR_ARG, "no taxonomy id is chosen");
    if (mode > 7u) fail(KSLAM_ERR_ARG, "unknown bits in the taxon-reads mode");
    for (uint64_t i = 0; i < n; i++)
      if (!ids[i]) fail(KSLAM_ERR_ARG, "taxonomy id 0 cannot be chosen");
    uint64_t N = 0;
    const uint32_t *up = nullptr, *depth = nullptr, *tax = nullptr;
    if (kslam_taxdb_dense(taxdb, &N, &up, &depth, &tax) != KSLAM_OK) fail(KSLAM_ERR_ARG, "the taxonomy tree has no dense form");
    exclude = (mode & KSLAM_TAXREADS_EXCLUDE) != 0;
    // S: a byte per node, the unknown chosen ids, and "every non-zero id"
    std::vector<uint8_t> seed(N, 0), in_s(N, 0);
    std::unordered_set<uint32_t> unknown;
    bool all_nonzero = false;
    auto node_of = [&](uint32_t id) -> uint32_t {
      const uint32_t v = kslam_taxdb_node(taxdb, id);
      return v == NONE || v >= N ? NONE : v;
    };
    for (uint64_t i = 0; i < n; i++) {
      if (ids[i] == 1u && (mode & KSLAM_TAXREADS_CHILDREN)) all_nonzero = true;
      const uint32_t v = node_of(ids[i]);
      if (v == NONE) { unknown.insert(ids[i]); continue; }
      seed[v] = in_s[v] = 1;
      if (mode & KSLAM_TAXREADS_PARENTS)
        for (uint32_t at = v, steps = 0; at < N && steps <= N; at = up[at], steps++) in_s[at] = 1;
    }
    if (mode & KSLAM_TAXREADS_PARENTS) {   // id 1 by rule: `up` stops below the root
      const uint32_t v = node_of(1u);
      if (v == NONE) unknown.insert(1u);
      else in_s[v] = 1;
    }
    if (mode & KSLAM_TAXREADS_CHILDREN) {
      // 0: not looked at, 1: below a seed (or one), 2: not below one; every path is walked once
      std::vector<uint8_t> below(N, 0);
      std::vector<uint32_t> path;
      for (uint64_t v0 = 0; v0 < N; v0++) {
        path.clear();
        uint8_t verdict = 2;
        for (uint32_t at = (uint32_t)v0; at < N && path.size() <= N; at = up[at]) {
          if (below[at]) { verdict = below[at]; break; }
          if (seed[at]) { below[at] = 1; verdict = 1; break; }
          path.push_back(at);
        }
        for (uint32_t p : path) below[p] = verdict;
      }
      for (uint64_t v = 0; v < N; v++)
        if (below[v] == 1) in_s[v] = 1;
    }
    for (uint64_t g = 0; g < n_read_pairs; g++) {
      const uint32_t id = pair_tax_ids[g];
      if (!id) continue;
      bool m = all_nonzero;
      if (!m) {
        const uint32_t v = node_of(id);
        m = v == NONE ? unknown.count(id) != 0 : in_s[v] != 0;
      }
      if (m) matched.push_back(read_pairs[g]);
    }
  });
  if (st != KSLAM_OK) return st;
  // the matched read pairs are the split's "classified" records; with EXCLUDE the other stream is the selection
  kslam_reads_out ro;
  const kslam_status sp = kslam_tail_split_reads(r1, len1, r2, len2, max_pairs, at_eof, matched.data(), matched.size(),
                                                 exclude ? KSLAM_READS_OUT_UNCLASSIFIED : KSLAM_READS_OUT_CLASSIFIED, &ro);
  if (sp != KSLAM_OK) return sp;
  const int from = exclude ? 2 : 0;
  for (int k = 0; k < 2; k++) {
    out->data[k] = ro.data[from + k];
    out->len[k] = ro.len[from + k];
  }
  out->n_records[0] = ro.n_records[exclude ? 1 : 0];
  out->n_records[1] = ro.n_records[exclude ? 0 : 1];
  out->flags = ro.flags;
  return KSLAM_OK;
}
