// kreport_check.cpp -- host-only run of the Kraken-style report's host side (include/kslam_kreport.h: kslam_tail_kreport,
// kslam_kreport_write) on a synthetic tree with repeated records, undefined parents and a deep chain, and synthetic ids with
// zeros and ids the tree does not know; the rows and the file are checked against sums kept while the ids were made.
// tools/sanitize_host.sh builds it with ASan+UBSan.
//   g++ -O2 -std=c++17 -pthread tools/kreport_check.cpp k-slam_amd/host/kreport.cpp k-slam_amd/host/taxonomy.cpp k-slam_amd/host/tail.cpp -o /tmp/kreport_check
//   /tmp/kreport_check [n_ids] [out_dir]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <map>
#include <random>
#include <string>
#include <unistd.h>
#include <vector>

#include "../include/kslam_kreport.h"

void kslam_free(void *p) { free(p); }   // csrc/api_core.hip is not linked

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fputc('\n', stderr);          \
      return 1;                     \
    }                               \
  } while (0)

int main(int argc, char **argv) {
  const uint64_t n_ids = argc > 1 ? strtoull(argv[1], 0, 10) : 20000;
  const std::string dir = argc > 2 ? argv[2] : "/tmp";
  std::mt19937_64 rng(9);
  // ---- the tree: ids 2 .. n_nodes + 1 with parents among the earlier ones (or 1), a chain of 400, two undefined parents, a
  // repeated record ----
  const uint32_t n_nodes = 3000, chain0 = 100000, chain_len = 400;
  static const char *ranks[] = {"no rank", "superkingdom", "phylum", "class", "order", "family", "genus", "species", "strain"};
  std::string text;
  auto record = [&](uint32_t id, uint32_t parent, const std::string &name, const char *rank) {
    text += std::to_string(id) + "\n" + std::to_string(parent) + "\n" + name + "\n" + rank + "\n";
  };
  record(1, 1, "root", "no rank");
  std::vector<uint32_t> ids_known;
  for (uint32_t k = 0; k < n_nodes; k++) {
    const uint32_t id = 2 + k, parent = k < 5 ? 1 : (rng() % 50 == 0 ? 900000 + (uint32_t)(rng() % 2) : 2 + (uint32_t)(rng() % k));
    record(id, parent, "taxon " + std::to_string(id), ranks[rng() % 9]);
    ids_known.push_back(id);
  }
  for (uint32_t k = 0; k < chain_len; k++) {
    record(chain0 + k, k ? chain0 + k - 1 : 1, "link " + std::to_string(k), k % 100 == 0 ? "genus" : "no rank");
    ids_known.push_back(chain0 + k);
  }
  record(7, 3, "seven again", "species");   // (the first record of id 7 is kept)
  ids_known.push_back(900000);              // the undefined parents are nodes too
  ids_known.push_back(900001);
  kslam_taxdb *db = nullptr;
  CHECK(kslam_taxdb_parse(text.data(), text.size(), &db) == KSLAM_OK, "kslam_taxdb_parse failed: %s", kslam_tail_last_error());
  // ---- the ids, and what they must add up to ----
  std::vector<uint32_t> ids(n_ids);
  std::map<uint32_t, uint64_t> want_direct;
  uint64_t want_nonzero = 0;
  std::map<uint32_t, uint64_t> want_unknown;
  for (uint64_t i = 0; i < n_ids; i++) {
    const uint64_t r = rng() % 100;
    uint32_t id;
    if (r < 10) id = 0;
    else if (r < 14) id = 5000000 + (uint32_t)(rng() % 7);            // unknown
    else if (r < 15) id = 0xFFFFFFFFu;
    else if (r < 60) id = ids_known[rng() % 20];                       // a few taxa take most reads
    else id = ids_known[rng() % ids_known.size()];
    ids[i] = id;
    if (!id) continue;
    want_nonzero++;
    want_direct[id]++;
    if (kslam_taxdb_node(db, id) == KSLAM_KREPORT_NO_NODE) want_unknown[id]++;
  }
  kslam_kreport_row *rows = nullptr;
  uint64_t n_rows = 0;
  kslam_kreport_stats st;
  CHECK(kslam_tail_kreport(db, ids.data(), ids.size(), &rows, &n_rows, &st) == KSLAM_OK, "kslam_tail_kreport failed: %s", kslam_tail_last_error());
  CHECK(st.n_ids == want_nonzero && st.n_unknown_ids == want_unknown.size() && st.n_rows == n_rows, "the statistics differ");
  uint64_t direct = 0, top_clade = 0;
  uint64_t n_nodes_all = 0;
  const uint32_t *up = nullptr, *depth = nullptr, *node_tax = nullptr;
  CHECK(kslam_taxdb_dense(db, &n_nodes_all, &up, &depth, &node_tax) == KSLAM_OK, "no dense tree");
  for (uint64_t i = 0; i < n_rows; i++) {
    const kslam_kreport_row &r = rows[i];
    direct += r.direct;
    CHECK(r.clade >= r.direct && r.clade > 0, "row %llu: a row that cannot be", (unsigned long long)i);
    const auto it = want_direct.find(r.tax_id);
    CHECK(r.direct == (it == want_direct.end() ? 0 : it->second), "row %llu: direct count of id %u", (unsigned long long)i, r.tax_id);
    if (r.node == KSLAM_KREPORT_NO_NODE) CHECK(want_unknown.count(r.tax_id) && r.clade == r.direct, "row %llu: not an unknown id", (unsigned long long)i);
    else CHECK(r.node < n_nodes_all && node_tax[r.node] == r.tax_id, "row %llu: not this node", (unsigned long long)i);
    if (r.node == KSLAM_KREPORT_NO_NODE || up[r.node] == 0xFFFFFFFFu) top_clade += r.clade;
    if (i) CHECK((rows[i - 1].node != KSLAM_KREPORT_NO_NODE && (r.node == KSLAM_KREPORT_NO_NODE || rows[i - 1].node < r.node)) ||
                 (rows[i - 1].node == KSLAM_KREPORT_NO_NODE && r.node == KSLAM_KREPORT_NO_NODE && rows[i - 1].tax_id < r.tax_id),
                 "row %llu: out of order", (unsigned long long)i);
  }
  CHECK(direct == want_nonzero && top_clade == want_nonzero, "sums differ: %llu direct, %llu under the root, %llu ids", (unsigned long long)direct,
        (unsigned long long)top_clade, (unsigned long long)want_nonzero);
  // ---- the file ----
  const std::string name = dir + "/kreport_check.txt";
  int fd = open(name.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
  CHECK(fd >= 0, "cannot open %s", name.c_str());
  CHECK(kslam_kreport_write(db, rows, n_rows, want_nonzero - 1, fd) == KSLAM_ERR_ARG && lseek(fd, 0, SEEK_END) == 0, "a total below the ids was not refused");
  CHECK(kslam_kreport_write(db, rows, n_rows, n_ids, fd) == KSLAM_OK, "kslam_kreport_write failed: %s", kslam_tail_last_error());
  const off_t size = lseek(fd, 0, SEEK_END);
  std::string file((size_t)size, 0);
  CHECK(pread(fd, &file[0], file.size(), 0) == (ssize_t)file.size(), "reading the file back failed");
  close(fd);
  unlink(name.c_str());
  uint64_t lines = 0, direct_in_file = 0, level0 = 0;
  for (size_t at = 0; at < file.size();) {
    const size_t end = file.find('\n', at);
    CHECK(end != std::string::npos, "a line without its end");
    unsigned long long clade = 0, own = 0;
    double pct = 0;
    char code[32];
    unsigned tax = 0;
    int used = 0;
    CHECK(sscanf(file.c_str() + at, "%lf\t%llu\t%llu\t%31[A-Z0-9]\t%u%n", &pct, &clade, &own, code, &tax, &used) == 5 && used > 0 &&
              file[at + used] == '\t', "line %llu does not parse", (unsigned long long)lines);   // (a blank in a format skips the indent too: stop before it)
    CHECK(clade > 0 && own <= clade, "line %llu: counts", (unsigned long long)lines);
    direct_in_file += own;
    if (file[at + used + 1] != ' ') level0++;
    lines++;
    at = end + 1;
  }
  CHECK(direct_in_file == n_ids && level0 == 2, "the file's direct counts add up to %llu of %llu; %llu lines without indent", (unsigned long long)direct_in_file,
        (unsigned long long)n_ids, (unsigned long long)level0);
  CHECK(lines == n_rows + 2 - (want_direct.count(1) ? 1 : 0), "the file has %llu lines for %llu rows", (unsigned long long)lines, (unsigned long long)n_rows);
  // ---- nothing counted ----
  kslam_kreport_row *none = nullptr;
  uint64_t n_none = 1;
  CHECK(kslam_tail_kreport(db, nullptr, 0, &none, &n_none, &st) == KSLAM_OK && n_none == 0 && st.n_ids == 0, "the empty set");
  kslam_free(none);
  kslam_free(rows);
  kslam_taxdb_free(db);
  printf("%llu ids, %llu counted, %llu rows, %llu unknown ids, %llu lines\n", (unsigned long long)n_ids, (unsigned long long)want_nonzero,
         (unsigned long long)n_rows, (unsigned long long)want_unknown.size(), (unsigned long long)lines);
  return 0;
}
