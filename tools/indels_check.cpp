// indels_check.cpp -- host-only run of the indel table's host side (include/kslam_indels.h: kslam_tail_indels,
// kslam_indels_write) on the shapes the tests hold it to: indels at every phase of homopolymers and tandem repeats, repeats at an
// entry's start and behind an entry that ends in the same base, N and lower case inside a repeat, I runs of 1 / 32 / 33 and D runs
// of 65 536 / 65 537 bases, unanchored runs, a shift of 5 000 steps, both strands with the batch's first read reversed, records
// that are skipped, and the writer's refusals.  The rows are checked against what the shapes were made to give.
// tools/sanitize_host.sh builds it with ASan+UBSan.
//   g++ -O2 -std=c++17 -pthread tools/indels_check.cpp k-slam_amd/host/indels.cpp -o /tmp/indels_check
//   /tmp/indels_check [out_dir]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <random>
#include <string>
#include <unistd.h>
#include <vector>

#include "../include/kslam_indels.h"

const char *kslam_tail_last_error(void) { return "(see the status)"; }   // host/tail.cpp is not linked
const char *kslam_version(void) { return "indels_check 0"; }             // csrc/api_core.hip is not linked
void kslam_free(void *p) { free(p); }

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      fprintf(stderr, "indels_check: " __VA_ARGS__); \
      fprintf(stderr, "\n");                      \
      return 1;                                   \
    }                                             \
  } while (0)

namespace {

struct Op { uint32_t len; char op; };

std::string revcomp(const std::string &s) {
  std::string r(s.rbegin(), s.rend());
  for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
  return r;
}

struct World {
  std::vector<std::string> entries;
  std::string rbases;
  std::vector<uint64_t> roff{0};
  std::vector<uint32_t> pool;
  std::vector<kslam_overlap> ov;
  std::vector<kslam_read_pair> rp;
  std::vector<kslam_paired_overlap> pr;

  // an alignment of `ops` at ref_begin whose I runs read `fill`, as a read, a CIGAR, a record and a group of its own
  void al(uint32_t entry, int32_t ref_begin, const std::vector<Op> &ops, bool rc = false, const std::string &fill = "A", bool live = true) {
    const std::string &ref = entries[entry];
    std::string q;
    size_t at = (size_t)ref_begin;
    kslam_overlap o;
    memset(&o, 0, sizeof o);
    o.cigar_off = pool.size();
    for (const Op &x : ops) {
      pool.push_back((x.len << 4) | (x.op == 'M' ? 0u : x.op == 'I' ? 1u : 2u));
      if (x.op == 'M') q += at + x.len <= ref.size() ? ref.substr(at, x.len) : std::string(x.len, 'A');
      if (x.op == 'I') for (uint32_t j = 0; j < x.len; j++) q += fill[j % fill.size()];
      if (x.op != 'I') at += x.len;
    }
    o.read = (uint32_t)(roff.size() - 1);
    o.entry = entry;
    o.ref_begin = ref_begin;
    o.revcomp = rc ? 1 : 0;
    o.cigar_len = (uint32_t)ops.size();
    rbases += rc ? revcomp(q) : q;
    roff.push_back(rbases.size());
    ov.push_back(o);
    kslam_paired_overlap p;
    memset(&p, 0, sizeof p);
    p.entry = entry;
    p.r1 = (uint32_t)(ov.size() - 1);
    p.r2 = KSLAM_NO_OVERLAP;
    rp.push_back(kslam_read_pair{(uint32_t)rp.size(), 0, pr.size(), live ? 1ull : 0ull});
    pr.push_back(p);
  }
  void gap(uint32_t entry, uint32_t at, char op, uint32_t n, bool rc = false, const std::string &fill = "A") {
    const uint32_t total = (uint32_t)entries[entry].size();
    al(entry, 0, {{at, 'M'}, {n, op}, {total - at - (op == 'D' ? n : 0), 'M'}}, rc, fill);
  }
};

const kslam_indel_row *find(const kslam_indel_row *rows, uint64_t n, uint32_t entry, uint32_t pos, int kind, uint32_t len) {
  for (uint64_t i = 0; i < n; i++)
    if (rows[i].entry == entry && rows[i].pos == pos && rows[i].kind == kind && rows[i].len == len) return rows + i;
  return nullptr;
}

}  // namespace

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::string left = "GTCAGTCTGACTGCATGCTC", right = "GTCGATCGTAGCTAGCTTGCAGT";
  std::mt19937_64 rng(7);
  auto random_bases = [&](size_t n) { std::string s(n, 'A'); for (char &c : s) c = "ACGT"[rng() % 4]; return s; };
  World w;
  w.entries = {left + std::string(8, 'A') + right,                 // 0: a homopolymer
               left + "CACACACACACA" + right,                      // 1: a tandem repeat
               std::string(8, 'A') + right,                        // 2: the repeat at the entry's start, behind an entry ...
               left + "AAAA",                                      // 3: ... (this one is in front of 4) that ends in the same base
               std::string(8, 'A') + right,                        // 4
               left + "AAAANAAAA" + "C" + "TTTTtTTTT" + right,     // 5: the alphabet
               random_bases(70000),                                // 6: the limits
               left + std::string(5000, 'A') + right,              // 7: a long shift
               ""};                                                // 8: an entry without bases
  const uint32_t a = (uint32_t)left.size();
  w.al(0, 0, {{30, 'M'}}, true);                                   // the batch's first read is reverse-complemented
  for (uint32_t j = 0; j < 8; j++) w.gap(0, a + j, 'D', 1, j & 1);
  for (uint32_t j = 0; j <= 8; j++) w.gap(0, a + j, 'I', 1, j & 1, "A");
  for (uint32_t j = 0; j <= 10; j++) w.gap(1, a + j, 'D', 2, j % 3 == 1);
  for (uint32_t j = 0; j <= 12; j++) w.gap(1, a + j, 'I', 2, j % 3 == 1, j & 1 ? "AC" : "CA");
  for (uint32_t e : {2u, 4u})
    for (uint32_t j = 1; j < 8; j++) {
      w.gap(e, j, 'D', 1, j & 1);
      w.gap(e, j, 'I', 1, j & 1, "A");
    }
  for (uint32_t p : {a + 5, a + 8, a + 3, a + 4, a + 15, a + 17, a + 14}) {
    w.gap(5, p, 'D', 1, p & 1);
    w.gap(5, p, 'I', 1, p & 1, p < a + 10 ? "A" : "T");
  }
  w.gap(5, 30, 'I', 1, false, "N");
  w.gap(5, 30, 'I', 3, true, "ANA");
  w.gap(5, 30, 'I', 1, false, "a");
  for (uint32_t n : {1u, 32u, 33u}) w.al(6, 20, {{30, 'M'}, {n, 'I'}, {30, 'M'}}, n & 1, random_bases(n));
  for (uint32_t n : {65536u, 65537u}) w.al(6, 100, {{100, 'M'}, {n, 'D'}, {100, 'M'}});
  w.al(6, 5, {{3, 'I'}, {40, 'M'}});
  w.al(6, 5, {{3, 'D'}, {40, 'M'}});
  w.al(6, 50, {{5, 'M'}, {2, 'I'}, {3, 'D'}, {5, 'M'}}, false, "GT");
  const uint32_t end = a + 5000;
  w.al(7, (int32_t)end - 12, {{11, 'M'}, {1, 'D'}, {15, 'M'}});
  w.al(7, (int32_t)end - 12, {{12, 'M'}, {1, 'I'}, {15, 'M'}}, true, "A");
  // skipped: past the entry, past the read (the read is built from what there is), no CIGAR, an entry outside, ref_begin < 0
  w.al(0, 40, {{5, 'M'}, {2, 'D'}, {30, 'M'}});
  w.al(0, 0, {{10, 'M'}, {2, 'I'}, {10, 'M'}});
  w.pool.back() = (11u << 4) | 0u;
  w.al(0, 0, {{10, 'M'}});
  w.ov.back().cigar_len = 0;
  w.al(0, 0, {{10, 'M'}});
  w.ov.back().entry = 99;
  w.al(0, 0, {{10, 'M'}});
  w.ov.back().ref_begin = -1;
  w.al(8, 0, {{1, 'M'}});                                          // nothing fits an entry without bases
  w.al(1, 0, {{20, 'M'}, {1, 'D'}, {5, 'M'}}, false, "A", false);  // a dead record: not named

  std::string gbases;
  std::vector<uint64_t> goff{0}, tag_off{0};
  std::string tags;
  std::vector<uint32_t> tax;
  for (size_t e = 0; e < w.entries.size(); e++) {
    gbases += w.entries[e];
    goff.push_back(gbases.size());
    tags += "LOC" + std::to_string(e);
    tag_off.push_back(tags.size());
    tax.push_back(100 + (uint32_t)e);
  }
  kslam_indel_row *rows = nullptr;
  uint64_t n_rows = 0;
  kslam_indel_stats st;
  auto tail = [&](uint32_t min_alt, uint32_t min_depth) {
    if (rows) kslam_free(rows);
    rows = nullptr;
    return kslam_tail_indels(gbases.data(), goff.data(), w.entries.size(), w.ov.data(), w.ov.size(), w.pool.data(), w.pool.size(), w.rbases.data(),
                             w.roff.data(), w.roff.size() - 1, w.rp.data(), w.rp.size(), w.pr.data(), w.pr.size(), min_alt, min_depth, &rows, &n_rows, &st);
  };
  CHECK(tail(1, 0) == KSLAM_OK, "kslam_tail_indels failed");
  CHECK(st.n_records == w.ov.size() - 1 && st.n_skipped == 6, "records %llu skipped %llu", (unsigned long long)st.n_records, (unsigned long long)st.n_skipped);
  CHECK(st.n_long_del == 1 && st.n_unrepresentable == 4 && st.n_unanchored == 2, "tallies %llu %llu %llu", (unsigned long long)st.n_long_del,
        (unsigned long long)st.n_unrepresentable, (unsigned long long)st.n_unanchored);
  CHECK(st.n_sites == n_rows, "sites");
  const uint64_t n_sites = st.n_sites;
  const kslam_indel_row *r;
  CHECK((r = find(rows, n_rows, 0, a - 1, KSLAM_INDEL_DEL, 1)) && r->alt_fwd == 4 && r->alt_rev == 4, "the homopolymer's deletion");
  CHECK((r = find(rows, n_rows, 0, a - 1, KSLAM_INDEL_INS, 1)) && r->alt_fwd + r->alt_rev == 9 && r->bases == 0, "the homopolymer's insertion");
  CHECK((r = find(rows, n_rows, 1, a - 1, KSLAM_INDEL_DEL, 2)) && r->alt_fwd + r->alt_rev == 11, "the tandem repeat's deletion");
  CHECK((r = find(rows, n_rows, 1, a - 1, KSLAM_INDEL_INS, 2)) && r->alt_fwd + r->alt_rev == 13 && r->bases == 0x4, "the tandem repeat's insertion (CA)");
  for (uint32_t e : {2u, 4u}) {
    CHECK((r = find(rows, n_rows, e, 0, KSLAM_INDEL_DEL, 1)) && r->alt_fwd + r->alt_rev == 7, "the deletion at the start of entry %u", e);
    CHECK((r = find(rows, n_rows, e, 0, KSLAM_INDEL_INS, 1)) && r->alt_fwd + r->alt_rev == 7, "the insertion at the start of entry %u", e);
  }
  CHECK(!find(rows, n_rows, 3, a + 3, KSLAM_INDEL_DEL, 1) && !find(rows, n_rows, 3, a + 3, KSLAM_INDEL_INS, 1), "an event stepped into entry 3");
  CHECK((r = find(rows, n_rows, 5, a + 4, KSLAM_INDEL_DEL, 1)) && r->alt_fwd + r->alt_rev == 2, "the deletions right of the N stop at it");
  CHECK((r = find(rows, n_rows, 5, a - 1, KSLAM_INDEL_DEL, 1)) && r->alt_fwd + r->alt_rev == 1, "the deletion left of the N");
  CHECK(find(rows, n_rows, 5, a + 14, KSLAM_INDEL_DEL, 1) && find(rows, n_rows, 5, a + 13, KSLAM_INDEL_DEL, 1), "lower case stops the shift");
  CHECK(find(rows, n_rows, 7, a - 1, KSLAM_INDEL_DEL, 1) && find(rows, n_rows, 7, a - 1, KSLAM_INDEL_INS, 1), "the shift of 5 000 steps");
  uint64_t n32 = 0, n33 = 0, n65536 = 0;
  for (uint64_t i = 0; i < n_rows; i++) {
    n32 += rows[i].kind == KSLAM_INDEL_INS && rows[i].len == 32;
    n33 += rows[i].len == 33 || rows[i].len == 65537;
    n65536 += rows[i].kind == KSLAM_INDEL_DEL && rows[i].len == 65536;
    CHECK(i == 0 || std::make_tuple(rows[i - 1].entry, rows[i - 1].pos, rows[i - 1].kind, rows[i - 1].len, rows[i - 1].bases) <
                        std::make_tuple(rows[i].entry, rows[i].pos, rows[i].kind, rows[i].len, rows[i].bases), "row %llu is out of order", (unsigned long long)i);
  }
  CHECK(n32 == 1 && n33 == 0 && n65536 == 1, "the limits: %llu %llu %llu", (unsigned long long)n32, (unsigned long long)n33, (unsigned long long)n65536);

  // ---- the writer ----
  kslam_index_view view;
  memset(&view, 0, sizeof view);
  view.n_entries = w.entries.size();
  view.bases = gbases.data();
  view.bases_off = goff.data();
  view.locus_tag = tags.data();
  view.locus_tag_off = tag_off.data();
  view.taxonomy_id = tax.data();
  const std::string path = dir + "/indels_check.vcf";
  int fd = open(path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
  CHECK(fd >= 0, "unable to open %s", path.c_str());
  CHECK(kslam_indels_write(&view, rows, n_rows, &st, fd) == KSLAM_OK, "kslam_indels_write failed");
  const off_t size = lseek(fd, 0, SEEK_END);
  std::string text((size_t)size, '\0');
  CHECK(pread(fd, &text[0], text.size(), 0) == (ssize_t)size, "reading the file back");
  uint64_t lines = 0;
  for (char c : text) lines += c == '\n';
  CHECK(lines > n_rows + 10 && text.find("TYPE=del;LEN=65536\n") != std::string::npos && text.find("\tCA\tC\t") != std::string::npos, "the file's lines");
  CHECK(ftruncate(fd, 0) == 0, "ftruncate");
  std::vector<kslam_indel_row> bad(rows, rows + n_rows);
  r = find(rows, n_rows, 0, a - 1, KSLAM_INDEL_DEL, 1);
  const size_t k = (size_t)(r - rows);
  bad[k].len = (uint32_t)(w.entries[0].size() - a + 1);            // one past the entry's last base
  CHECK(kslam_indels_write(&view, bad.data(), n_rows, nullptr, fd) == KSLAM_ERR_ARG, "a deletion past the entry was written");
  bad[k].len -= 1;
  CHECK(kslam_indels_write(&view, bad.data(), n_rows, nullptr, fd) == KSLAM_OK && lseek(fd, 0, SEEK_END) > 0, "a deletion up to the entry's end");
  CHECK(ftruncate(fd, 0) == 0, "ftruncate");
  bad = std::vector<kslam_indel_row>(rows, rows + n_rows);
  bad.back().entry = (uint32_t)w.entries.size();
  CHECK(kslam_indels_write(&view, bad.data(), n_rows, nullptr, fd) == KSLAM_ERR_ARG, "an entry outside the view was written");
  tag_off[1] = 0;                                                   // entry 0 without a locus
  CHECK(kslam_indels_write(&view, rows, n_rows, nullptr, fd) == KSLAM_ERR_ARG && lseek(fd, 0, SEEK_END) == 0, "an empty locus was written");
  close(fd);
  unlink(path.c_str());
  // the filters, and arrays that do not hold together
  CHECK(tail(8, 1) == KSLAM_OK && n_rows >= 4, "the filter kept %llu rows", (unsigned long long)n_rows);
  w.pr[2].r1 = (uint32_t)w.ov.size();
  CHECK(tail(1, 0) == KSLAM_ERR_ARG && rows == nullptr, "a record outside the array was taken");
  printf("indels_check: %zu records, %llu sites, clean\n", w.ov.size(), (unsigned long long)n_sites);
  return 0;
}
