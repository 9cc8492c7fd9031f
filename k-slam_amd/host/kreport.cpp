// kreport.cpp -- include/kslam_kreport.h, the host side: the twin of csrc/kreport.hip (the same rows from host ids, one serial
// pass) and the writer of the six-column report.  Plain C++, no GPU; the tree only through the public kslam_taxdb_* accessors.
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <unistd.h>
#include <unordered_map>
#include <vector>

#include "../../include/kslam_kreport.h"
#include "workers.hpp"

namespace {
using namespace kslam_host;
constexpr uint32_t NONE = KSLAM_KREPORT_NO_NODE;

struct Tree {
  uint64_t n = 0;
  const uint32_t *up = nullptr, *depth = nullptr, *tax = nullptr;
};
Tree tree_of(const kslam_taxdb *db) {
  if (!db) fail(KSLAM_ERR_ARG, "null taxonomy tree");
  Tree t;
  if (kslam_taxdb_dense(db, &t.n, &t.up, &t.depth, &t.tax) != KSLAM_OK) fail(KSLAM_ERR_ARG, "the taxonomy tree has no dense form");
  return t;
}

std::string text_of(const kslam_taxdb *db, uint32_t id, int which) {
  char *p = nullptr;
  uint64_t n = 0;
  if (kslam_taxdb_text(db, id, which, &p, &n) != KSLAM_OK) fail(KSLAM_ERR_ARG, "kslam_taxdb_text failed");
  std::string s(p ? p : "", n);
  kslam_free(p);
  return s;
}

// Kraken 2's letters; 0: the rank has none
char rank_letter(const std::string &rank) {
  static const struct { const char *text; char code; } table[] = {{"superkingdom", 'D'}, {"domain", 'D'}, {"kingdom", 'K'},
                                                                  {"phylum", 'P'},       {"class", 'C'},  {"order", 'O'},
                                                                  {"family", 'F'},       {"genus", 'G'},  {"species", 'S'}};
  for (const auto &t : table)
    if (rank == t.text) return t.code;
  return 0;
}

void line(std::string &out, uint64_t clade, uint64_t direct, uint64_t total, char letter, uint64_t number, uint32_t tax_id, uint64_t level,
          const std::string &name) {
  char buf[128];
  snprintf(buf, sizeof buf, "%6.2f\t%llu\t%llu\t%c", 100.0 * (double)clade / (double)total, (unsigned long long)clade, (unsigned long long)direct, letter);
  out += buf;
  if (number) out += std::to_string(number);
  snprintf(buf, sizeof buf, "\t%u\t", tax_id);
  out += buf;
  out.append(2 * level, ' ');
  out += name;
  out += '\n';
}
}  // namespace

extern "C" kslam_status kslam_tail_kreport(const kslam_taxdb *taxdb, const uint32_t *tax_ids, uint64_t n, kslam_kreport_row **rows, uint64_t *n_rows,
                                           kslam_kreport_stats *stats) {
  if (rows) *rows = nullptr;
  if (n_rows) *n_rows = 0;
  return guarded([&] {
    if (!rows || !n_rows || !stats || (n && !tax_ids)) fail(KSLAM_ERR_ARG, "null argument");
    const Tree t = tree_of(taxdb);
    std::vector<uint64_t> direct(t.n, 0), clade(t.n, 0);
    std::map<uint32_t, uint64_t> unknown;   // (ascending ids)
    uint64_t n_ids = 0;
    for (uint64_t i = 0; i < n; i++) {
      const uint32_t id = tax_ids[i];
      if (!id) continue;
      n_ids++;
      const uint32_t node = kslam_taxdb_node(taxdb, id);
      if (node == NONE || node >= t.n) unknown[id]++;
      else direct[node]++;
    }
    for (uint64_t v = 0; v < t.n; v++) {
      if (!direct[v]) continue;
      uint32_t at = (uint32_t)v;
      for (uint64_t steps = t.depth[v]; steps && at < t.n; steps--) {   // depth = the nodes on the path, this one included
        clade[at] += direct[v];
        at = t.up[at];
      }
    }
    uint64_t count = unknown.size();
    for (uint64_t v = 0; v < t.n; v++) count += clade[v] != 0;
    kslam_kreport_row *out = (kslam_kreport_row *)malloc(sizeof(kslam_kreport_row) * (count + 1));
    if (!out) fail(KSLAM_ERR_OOM, "out of host memory");
    uint64_t k = 0;
    for (uint64_t v = 0; v < t.n; v++)
      if (clade[v]) out[k++] = kslam_kreport_row{t.tax[v], (uint32_t)v, direct[v], clade[v]};
    for (const auto &u : unknown) out[k++] = kslam_kreport_row{u.first, NONE, u.second, u.second};
    *rows = out;
    *n_rows = count;
    stats->n_ids = n_ids;
    stats->n_unknown_ids = unknown.size();
    stats->n_rows = count;
  });
}

extern "C" kslam_status kslam_kreport_write(const kslam_taxdb *taxdb, const kslam_kreport_row *rows, uint64_t n_rows, uint64_t total, int fd) {
  return guarded([&] {
    if (n_rows && !rows) fail(KSLAM_ERR_ARG, "null argument");
    const Tree t = tree_of(taxdb);
    uint64_t sum = 0;
    std::unordered_map<uint32_t, uint64_t> row_of;   // node -> row
    for (uint64_t i = 0; i < n_rows; i++) {
      const kslam_kreport_row &r = rows[i];
      if (r.node != NONE && (r.node >= t.n || t.tax[r.node] != r.tax_id || !row_of.emplace(r.node, i).second))
        fail(KSLAM_ERR_ARG, "row " + std::to_string(i) + " is not a row of this tree");
      if (r.direct > r.clade || sum + r.direct < sum) fail(KSLAM_ERR_ARG, "row " + std::to_string(i) + " holds counts that cannot be");
      sum += r.direct;
    }
    if (total < sum) fail(KSLAM_ERR_ARG, "the run has " + std::to_string(total) + " read pairs, the rows count " + std::to_string(sum));
    // the synthetic root: parent of every top-level node and of every unknown id; the tree's own node for id 1 is folded into it
    const uint32_t root_node = kslam_taxdb_node(taxdb, 1);
    const std::string root_name = root_node != NONE ? text_of(taxdb, 1, 0) : std::string("root");
    uint64_t root_direct = 0;
    std::vector<std::vector<uint64_t>> kids(n_rows + 1);   // kids[n_rows]: root's
    for (uint64_t i = 0; i < n_rows; i++) {
      const kslam_kreport_row &r = rows[i];
      if (!r.clade) continue;
      if (r.tax_id == 1) {   // the tree's own node for id 1 -- or id 1 unknown to the tree -- is the root row itself
        root_direct += r.direct;
        continue;
      }
      const uint32_t up = r.node == NONE ? NONE : t.up[r.node];
      if (up == NONE || up == root_node) {
        kids[n_rows].push_back(i);
        continue;
      }
      const auto it = row_of.find(up);
      if (it == row_of.end()) fail(KSLAM_ERR_ARG, "row " + std::to_string(i) + ": the parent node has no row");
      kids[it->second].push_back(i);
    }
    for (auto &k : kids)
      std::sort(k.begin(), k.end(), [&](uint64_t a, uint64_t b) {
        return rows[a].clade != rows[b].clade ? rows[a].clade > rows[b].clade : rows[a].tax_id < rows[b].tax_id;
      });
    std::string text;
    if (total > sum) line(text, total - sum, total - sum, total, 'U', 0, 0, 0, "unclassified");
    if (sum) {
      line(text, sum, root_direct, total, 'R', 0, 1, 0, root_name);
      struct Item { uint64_t row, level; char letter; uint64_t number; };   // letter / number: the PARENT's
      std::vector<Item> stack;
      for (size_t k = kids[n_rows].size(); k-- > 0;) stack.push_back(Item{kids[n_rows][k], 1, 'R', 0});
      while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        const kslam_kreport_row &r = rows[it.row];
        const bool known = r.node != NONE;
        const char own = known ? rank_letter(text_of(taxdb, r.tax_id, 1)) : 0;
        const char letter = own ? own : it.letter;
        const uint64_t number = own ? 0 : it.number + 1;
        line(text, r.clade, r.direct, total, letter, number, r.tax_id, it.level, known ? text_of(taxdb, r.tax_id, 0) : std::string());
        for (size_t k = kids[it.row].size(); k-- > 0;) stack.push_back(Item{kids[it.row][k], it.level + 1, letter, number});
      }
    }
    const char *p = text.data();
    size_t n = text.size();
    while (n) {
      const ssize_t w = ::write(fd, p, n);
      if (w < 0) {
        if (errno == EINTR) continue;
        fail(KSLAM_ERR_ARG, std::string("writing the report failed: ") + strerror(errno));
      }
      p += w;
      n -= (size_t)w;
    }
  });
}
