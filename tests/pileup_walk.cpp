// pileup_walk.cpp -- k-slam_amd/host/pileup_walk.hpp alone, at the edges of its rules: one entry of 8 bases, reads of 4 to 8
// bases, CIGARs whose M, I and D runs end exactly at the read's or the entry's end and one further, the skip preamble, the
// contributing set and the oriented query.  Stand-alone: tests/test_pileup_walk.py builds it with the address and
// undefined-behaviour sanitizers, so that a read outside an array (every array here is a heap block of exactly its size) fails
// the run.  Prints "ok".
#include <cstdio>
#include <string>
#include <vector>

#include "../k-slam_amd/host/pileup_walk.hpp"

namespace {
constexpr uint32_t NO = KSLAM_NO_OVERLAP;
constexpr int64_t ENTRY_LEN = 8;

int failures = 0;

uint32_t M(uint32_t len) { return len << 4 | 0u; }
uint32_t I(uint32_t len) { return len << 4 | 1u; }
uint32_t D(uint32_t len) { return len << 4 | 2u; }

struct Batch {
  std::vector<kslam_overlap> ov;
  std::vector<uint32_t> pool;
  std::vector<uint64_t> roff{0};
  std::vector<kslam_read_pair> groups;
  std::vector<kslam_paired_overlap> pairs;
  std::vector<uint64_t> goff{0, (uint64_t)ENTRY_LEN};

  uint32_t read(uint64_t len) {
    roff.push_back(roff.back() + len);
    return (uint32_t)roff.size() - 2;
  }
  // a record of `read` on entry 0 with these CIGAR words; returns its index
  uint32_t record(uint32_t read, int32_t ref_begin, int32_t query_begin, const std::vector<uint32_t> &cigar) {
    kslam_overlap o{};
    o.read = read;
    o.ref_begin = ref_begin;
    o.query_begin = query_begin;
    o.cigar_off = pool.size();
    o.cigar_len = (uint32_t)cigar.size();
    pool.insert(pool.end(), cigar.begin(), cigar.end());
    ov.push_back(o);
    return (uint32_t)ov.size() - 1;
  }
  // an alignment pair (r1, r2) in a group of its own (live), or behind every group (dead)
  void pair(uint32_t r1, uint32_t r2, bool live = true) {
    kslam_paired_overlap p{};
    p.r1 = r1;
    p.r2 = r2;
    if (live) groups.push_back(kslam_read_pair{0, 1, pairs.size(), 1});
    pairs.push_back(p);
  }
  // every array as a heap block of exactly its size (a vector that grew may own more)
  void shrink() {
    ov.shrink_to_fit();
    pool.shrink_to_fit();
    roff.shrink_to_fit();
    groups.shrink_to_fit();
    pairs.shrink_to_fit();
  }
};

struct Seen {
  std::string fault;
  std::vector<uint32_t> held;   // the records handed to fn, in order
  std::vector<int64_t> L, ref_len;
  uint64_t n_records = 0, n_skipped = 0;
};

Seen walk(Batch &b, uint64_t n_entries = 1) {
  b.shrink();
  // exact copies: the pool and the offsets as blocks of their own
  const std::vector<uint32_t> pool(b.pool.begin(), b.pool.end());
  const std::vector<uint64_t> goff(b.goff.begin(), b.goff.begin() + (long)n_entries + 1);
  const kslam_batch::Arrays arrays{b.ov.empty() ? nullptr : b.ov.data(), b.ov.size(), pool.size(), b.roff.data(), b.roff.size() - 1,
                                   b.groups.empty() ? nullptr : b.groups.data(), b.groups.size(), b.pairs.empty() ? nullptr : b.pairs.data(), b.pairs.size()};
  Seen s;
  s.fault = kslam_pileup::for_each_contributing_record(arrays, pool.empty() ? nullptr : pool.data(), goff.data(), n_entries, s.n_records, s.n_skipped,
                                                       [&](const kslam_overlap &o, int64_t L, int64_t ref_len) {
                                                         s.held.push_back((uint32_t)(&o - b.ov.data()));
                                                         s.L.push_back(L);
                                                         s.ref_len.push_back(ref_len);
                                                       });
  return s;
}

void expect(const char *what, const Seen &s, const std::vector<uint32_t> &held, uint64_t n_records, uint64_t n_skipped) {
  if (!s.fault.empty() || s.held != held || s.n_records != n_records || s.n_skipped != n_skipped) {
    failures++;
    printf("FAILED %s: fault \"%s\", %zu records held, %llu records, %llu skipped\n", what, s.fault.c_str(), s.held.size(),
           (unsigned long long)s.n_records, (unsigned long long)s.n_skipped);
  }
}

// ONE record of a read of read_len bases, named by one live pair: does it hold?
void edge(const char *what, uint64_t read_len, int32_t ref_begin, int32_t query_begin, const std::vector<uint32_t> &cigar, bool holds) {
  Batch b;
  const uint32_t r = b.record(b.read(read_len), ref_begin, query_begin, cigar);
  b.pair(r, NO);
  const Seen s = walk(b);
  expect(what, s, holds ? std::vector<uint32_t>{r} : std::vector<uint32_t>{}, 1, holds ? 0 : 1);
  if (holds && s.held.size() == 1 && (s.L[0] != (int64_t)read_len || s.ref_len[0] != ENTRY_LEN)) {
    failures++;
    printf("FAILED %s: lengths %lld and %lld\n", what, (long long)s.L[0], (long long)s.ref_len[0]);
  }
}

void expect_text(const char *what, const std::string &got, const std::string &want) {
  if (got != want) {
    failures++;
    printf("FAILED %s: got \"%s\", expected \"%s\"\n", what, got.c_str(), want.c_str());
  }
}

}  // namespace

int main() {
  // ---- the fit check: each run exactly at its end, and one further ----
  edge("an M run to the entry's last base", 8, 4, 0, {M(4)}, true);
  edge("an M run one column past the entry", 8, 4, 0, {M(5)}, false);
  edge("an M run over the whole entry and read", 8, 0, 0, {M(8)}, true);
  edge("an M run to the read's last base", 4, 0, 0, {M(4)}, true);
  edge("an M run one column past the read", 4, 0, 0, {M(5)}, false);
  edge("an M run past the read from query_begin on", 4, 0, 1, {M(4)}, false);
  edge("an M run to the read's last base from query_begin on", 4, 0, 1, {M(3)}, true);
  edge("an I run to the read's last base", 6, 0, 0, {M(4), I(2)}, true);
  edge("an I run one base past the read", 6, 0, 0, {M(4), I(3)}, false);
  edge("a D run to the entry's last base", 4, 2, 0, {M(4), D(2)}, true);
  edge("a D run one base past the entry", 4, 2, 0, {M(4), D(3)}, false);
  edge("an M run behind a D run at the entry's end", 5, 2, 0, {M(4), D(2), M(1)}, false);
  edge("an M run behind an I run at the read's end", 6, 0, 0, {M(4), I(2), M(1)}, false);
  // ---- query_begin below 0 counts as 0 (unclamped, -1 + 5 would fit a read of 4) ----
  edge("query_begin -1, four columns", 4, 0, -1, {M(4)}, true);
  edge("query_begin -1, five columns", 4, 0, -1, {M(5)}, false);
  // ---- runs of length 0 skip nothing, wherever they stand; other operations are passed over ----
  edge("runs of length 0 at the ends of the read and the entry", 4, 4, 0, {M(4), M(0), I(0), D(0)}, true);
  edge("runs of length 0 in front", 4, 4, 0, {D(0), I(0), M(0), M(4)}, true);
  edge("a soft clip of any length", 4, 4, 0, {100u << 4 | 4u, M(4)}, true);

  {   // ---- the skip preamble ----
    Batch b;
    const uint32_t rd = b.read(4);
    const uint32_t sound = b.record(rd, 0, 0, {M(4)});
    const uint32_t empty = b.record(rd, 0, 0, {});
    const uint32_t before = b.record(rd, -1, 0, {M(4)});
    const uint32_t other = b.record(rd, 0, 0, {M(4)});
    b.ov[other].entry = 1;   // == n_entries
    for (uint32_t r : {sound, empty, before, other}) b.pair(r, NO);
    expect("cigar_len == 0, ref_begin < 0 and entry == n_entries", walk(b), {sound}, 4, 3);
    // with two entries the last record's entry exists, with 0 bases: its M run does not fit
    b.goff = {0, (uint64_t)ENTRY_LEN, (uint64_t)ENTRY_LEN};
    expect("an entry of length 0", walk(b, 2), {sound}, 4, 3);
    b.ov[other].cigar_len = 1;
    b.pool[b.ov[other].cigar_off] = M(0);
    expect("an entry of length 0 under a run of length 0", walk(b, 2), {sound, other}, 4, 2);
  }
  {   // ---- the contributing set ----
    Batch b;
    const uint32_t rd = b.read(4), rd2 = b.read(5);
    const uint32_t thrice = b.record(rd, 0, 0, {M(4)});
    const uint32_t dead = b.record(rd, 0, 0, {M(4)});
    const uint32_t unnamed = b.record(rd2, 0, 0, {M(5)});
    const uint32_t second = b.record(rd2, 3, 0, {M(5)});
    (void)unnamed;
    b.pair(thrice, NO);
    b.pair(NO, thrice);
    b.pair(second, thrice);
    b.pair(dead, dead, false);
    b.pair(dead, NO, false);
    const Seen s = walk(b);
    expect("named three times, named by dead pairs alone, not named", s, {thrice, second}, 2, 0);
    if (s.L != std::vector<int64_t>{4, 5}) {
      failures++;
      printf("FAILED the reads' lengths\n");
    }
  }
  {   // ---- arrays that do not hold together: the check's own words, and nothing is visited ----
    Batch b;
    const uint32_t r = b.record(b.read(4), 0, 0, {M(4)});
    b.pair(r, 7);
    const Seen s = walk(b);
    expect_text("the fault", s.fault, "alignment pair 0 refers to overlap record 7 of 1");
    if (!s.held.empty() || s.n_records || s.n_skipped) {
      failures++;
      printf("FAILED a record was visited although the arrays do not hold together\n");
    }
    expect("no arrays at all", [] { Batch e; return walk(e, 0); }(), {}, 0, 0);
  }
  {   // ---- the alphabet and the oriented query ----
    const std::string text = "ACGTNacg";
    const std::vector<uint8_t> read(text.begin(), text.end());
    std::string q = "left over";
    kslam_pileup::oriented_query(q, read.data(), (int64_t)read.size(), false);
    expect_text("the forward query", q, "ACGTNacg");
    kslam_pileup::oriented_query(q, read.data(), (int64_t)read.size(), true);
    expect_text("the reverse query", q, "gcaNACGT");
    kslam_pileup::oriented_query(q, read.data(), 0, true);
    expect_text("the query of an empty read", q, "");
    std::string codes;
    for (uint8_t c : read) codes += (char)('0' + kslam_pileup::acgt(c));
    expect_text("the codes", codes, "01234444");
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
