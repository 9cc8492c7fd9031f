// taxreads_check.cpp -- host-only run of the host twin of the reads of chosen taxa (include/kslam_taxreads.h:
// kslam_tail_taxon_reads) on the header's worked example and on random trees with undefined parents, a deep chain and a
// repeated record; chosen ids known and unknown, duplicates, id 1; all eight modes; paired and single-end texts.  Every result
// is held against a selection made here from nothing but the tree's dense arrays (a walk up per read pair and per chosen id),
// and the EXCLUDE stream against the complement.  tools/sanitize_host.sh builds it with ASan+UBSan.
//   g++ -O2 -std=c++17 -pthread tools/taxreads_check.cpp k-slam_amd/host/taxreads.cpp k-slam_amd/host/readsplit.cpp k-slam_amd/host/taxonomy.cpp k-slam_amd/host/tail.cpp -o /tmp/taxreads_check
//   /tmp/taxreads_check [n_pairs]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../include/kslam_taxreads.h"

void kslam_free(void *p) { free(p); }                   // csrc/api_core.hip is not linked
void kslam_free_pinned(kslam_ctx *, void *p) { free(p); }

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fputc('\n', stderr);          \
      return 1;                     \
    }                               \
  } while (0)

namespace {
constexpr uint32_t NONE = 0xFFFFFFFFu;

struct Dense {
  uint64_t n = 0;
  const uint32_t *up = nullptr, *depth = nullptr, *tax = nullptr;
};

// is `id` in S?  From the definition: the chosen ids; CHILDREN: a chosen id on id's way up; PARENTS: id on a chosen id's way up, or 1.
bool in_set(const kslam_taxdb *db, const Dense &t, const std::vector<uint32_t> &chosen, uint32_t mode, uint32_t id) {
  if (!id) return false;
  for (uint32_t c : chosen)
    if (c == id) return true;
  const uint32_t v = kslam_taxdb_node(db, id);
  if (mode & KSLAM_TAXREADS_CHILDREN) {
    for (uint32_t c : chosen)
      if (c == 1u) return true;
    if (v != NONE)
      for (uint32_t at = t.up[v]; at < t.n; at = t.up[at])
        for (uint32_t c : chosen)
          if (t.tax[at] == c) return true;
  }
  if (mode & KSLAM_TAXREADS_PARENTS) {
    if (id == 1u) return true;
    if (v != NONE)
      for (uint32_t c : chosen) {
        const uint32_t w = kslam_taxdb_node(db, c);
        if (w == NONE) continue;
        for (uint32_t at = t.up[w]; at < t.n; at = t.up[at])
          if (at == v) return true;
      }
  }
  return false;
}

std::string record(uint64_t k, int mate, std::mt19937_64 &rng) {
  const size_t len = 5 + rng() % 40;
  std::string bases(len, 'A'), qual(len, 'I');
  for (auto &b : bases) b = "ACGT"[rng() % 4];
  return "@p" + std::to_string(k) + "/" + std::to_string(mate) + "\n" + bases + "\n+\n" + qual + "\n";
}
}  // namespace

int main(int argc, char **argv) {
  const uint64_t n_pairs = argc > 1 ? strtoull(argv[1], 0, 10) : 20000;
  std::mt19937_64 rng(12);
  // ---- the worked example ----
  {
    const std::string text =
        "1\n1\nroot\nno rank\n131567\n1\ncellular organisms\nno rank\n2\n131567\nBacteria\nsuperkingdom\n1224\n2\nProteobacteria\nphylum\n"
        "562\n1224\nEscherichia coli\nspecies\n83333\n562\nEscherichia coli K-12\nstrain\n10239\n1\nViruses\nsuperkingdom\n"
        "10760\n10239\nEscherichia phage T7\nspecies\n";
    kslam_taxdb *db = nullptr;
    CHECK(kslam_taxdb_parse(text.data(), text.size(), &db) == KSLAM_OK, "kslam_taxdb_parse failed: %s", kslam_tail_last_error());
    const uint32_t pair_ids[10] = {562, 562, 562, 83333, 83333, 2, 10760, 999999, 0, 0};
    std::string r1, r2;
    std::vector<kslam_read_pair> rp(10);
    for (uint32_t k = 0; k < 10; k++) {
      r1 += record(k, 1, rng);
      r2 += record(k, 2, rng);
      rp[k].r1_read = k;
      rp[k].r2_read = k + 10;
      rp[k].first = k;
      rp[k].count = 1;
    }
    const struct { uint32_t id, mode; uint64_t want; } rows[] = {{562, 0, 3}, {562, 1, 5}, {562, 2, 4}, {562, 3, 6}, {2, 1, 6}, {10239, 1, 1}, {999999, 1, 1},
                                                                   {1, 1, 8}, {562, 5, 5}};
    for (const auto &row : rows) {
      kslam_reads_out out;
      CHECK(kslam_tail_taxon_reads(db, &row.id, 1, row.mode, r1.data(), r1.size(), r2.data(), r2.size(), 0, 1, rp.data(), pair_ids, 10, &out) == KSLAM_OK,
            "the example failed: %s", kslam_tail_last_error());
      CHECK(out.n_records[0] == row.want && out.n_records[1] == 10 - row.want, "example id %u mode %u: %llu selected, %llu wanted", row.id, row.mode,
            (unsigned long long)out.n_records[0], (unsigned long long)row.want);
      kslam_release_reads_out(nullptr, &out);
    }
    kslam_reads_out out;
    const uint32_t zero = 0, one = 1;
    CHECK(kslam_tail_taxon_reads(db, &zero, 1, 0, r1.data(), r1.size(), nullptr, 0, 0, 1, rp.data(), pair_ids, 10, &out) == KSLAM_ERR_ARG, "id 0 was not refused");
    CHECK(kslam_tail_taxon_reads(db, &one, 1, 8, r1.data(), r1.size(), nullptr, 0, 0, 1, rp.data(), pair_ids, 10, &out) == KSLAM_ERR_ARG, "mode 8 was not refused");
    CHECK(kslam_tail_taxon_reads(db, &one, 0, 0, r1.data(), r1.size(), nullptr, 0, 0, 1, rp.data(), pair_ids, 10, &out) == KSLAM_ERR_ARG, "n == 0 was not refused");
    kslam_taxdb_free(db);
  }
  // ---- random trees ----
  uint64_t n_cases = 0, n_selected = 0;
  for (int round = 0; round < 4; round++) {
    const uint32_t n_nodes = 200 + 300 * round, chain0 = 100000, chain_len = 300;
    std::string text;
    auto node = [&](uint32_t id, uint32_t parent) { text += std::to_string(id) + "\n" + std::to_string(parent) + "\nname\nno rank\n"; };
    std::vector<uint32_t> known;
    if (round & 1) node(1, 1), known.push_back(1);   // with and without a node for id 1
    for (uint32_t k = 0; k < n_nodes; k++) {
      node(2 + k, k < 4 ? 1 : (rng() % 40 == 0 ? 900000 + (uint32_t)(rng() % 2) : 2 + (uint32_t)(rng() % k)));
      known.push_back(2 + k);
    }
    for (uint32_t k = 0; k < chain_len; k++) {
      node(chain0 + k, k ? chain0 + k - 1 : 1);
      known.push_back(chain0 + k);
    }
    node(9, 3);   // (the first record of id 9 is kept)
    kslam_taxdb *db = nullptr;
    CHECK(kslam_taxdb_parse(text.data(), text.size(), &db) == KSLAM_OK, "kslam_taxdb_parse failed: %s", kslam_tail_last_error());
    Dense t;
    CHECK(kslam_taxdb_dense(db, &t.n, &t.up, &t.depth, &t.tax) == KSLAM_OK, "no dense tree");
    if (kslam_taxdb_node(db, 900000) != NONE) known.push_back(900000);
    // the batch: records, the read pairs of three records in four (out of order), their ids
    const bool single = round == 2;
    std::vector<std::string> rec1(n_pairs), rec2(n_pairs);
    std::string r1, r2;
    for (uint64_t k = 0; k < n_pairs; k++) {
      rec1[k] = record(k, 1, rng);
      rec2[k] = record(k, 2, rng);
      r1 += rec1[k];
      r2 += rec2[k];
    }
    std::vector<kslam_read_pair> rp;
    std::vector<uint32_t> pair_ids;
    for (uint64_t k = n_pairs; k-- > 0;) {
      if (k % 4 == 3) continue;
      kslam_read_pair p;
      memset(&p, 0, sizeof p);
      p.r1_read = (uint32_t)k;
      p.r2_read = single ? 0u : (uint32_t)(k + n_pairs);
      p.count = 1;
      rp.push_back(p);
      const uint64_t r = rng() % 100;
      pair_ids.push_back(r < 10 ? 0u : r < 14 ? 5000000u + (uint32_t)(rng() % 5) : r < 15 ? 1u : r < 50 ? known[rng() % 12] : known[rng() % known.size()]);
    }
    const std::vector<std::vector<uint32_t>> lists = {{known[3]}, {known[3], known[3], 5000001u}, {1u}, {chain0 + 7, chain0 + 250}, {chain0 + chain_len - 1},
                                                      {900000u}, {5000002u, 77u + 1000000u}, {known[rng() % known.size()], known[rng() % known.size()], known[5]}};
    for (const auto &chosen : lists)
      for (uint32_t mode = 0; mode < 8; mode++) {
        std::vector<uint8_t> hit(n_pairs, 0);
        for (size_t g = 0; g < rp.size(); g++)
          if (in_set(db, t, chosen, mode, pair_ids[g])) hit[rp[g].r1_read] = 1;
        std::string want1, want2;
        uint64_t want_n = 0;
        for (uint64_t k = 0; k < n_pairs; k++)
          if ((hit[k] != 0) != ((mode & KSLAM_TAXREADS_EXCLUDE) != 0)) {
            want1 += rec1[k];
            want2 += rec2[k];
            want_n++;
          }
        kslam_reads_out out;
        CHECK(kslam_tail_taxon_reads(db, chosen.data(), chosen.size(), mode, r1.data(), r1.size(), single ? nullptr : r2.data(), single ? 0 : r2.size(), 0, 1,
                                     rp.data(), pair_ids.data(), rp.size(), &out) == KSLAM_OK,
              "kslam_tail_taxon_reads failed: %s", kslam_tail_last_error());
        CHECK(out.n_records[0] == want_n && out.n_records[1] == n_pairs - want_n, "round %d mode %u: %llu records selected, %llu wanted", round, mode,
              (unsigned long long)out.n_records[0], (unsigned long long)want_n);
        CHECK(out.len[0] == want1.size() && (want1.empty() || memcmp(out.data[0], want1.data(), want1.size()) == 0), "round %d mode %u: the R1 stream differs", round, mode);
        if (single) CHECK(out.data[1] == nullptr && out.len[1] == 0, "a second stream for single-end reads");
        else CHECK(out.len[1] == want2.size() && (want2.empty() || memcmp(out.data[1], want2.data(), want2.size()) == 0), "round %d mode %u: the R2 stream differs", round, mode);
        CHECK(out.data[2] == nullptr && out.data[3] == nullptr && (out.flags & KSLAM_READS_OUT_HOST_MEMORY), "the other streams are not empty");
        kslam_release_reads_out(nullptr, &out);
        n_cases++;
        n_selected += want_n;
      }
    kslam_taxdb_free(db);
  }
  printf("%llu pairs per batch, %llu cases, %llu records selected in all\n", (unsigned long long)n_pairs, (unsigned long long)n_cases, (unsigned long long)n_selected);
  return 0;
}
