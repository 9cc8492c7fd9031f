// batch_check.cpp -- k-slam_amd/host/batch_check.hpp alone, at the smallest shapes at which each of its rules can go wrong (at most
// 2 groups, 2 alignment pairs, 2 overlap records, 2 reads, 2 CIGAR words), at every level, message by message.  Stand-alone:
// tests/test_batch_check.py builds it with the address and undefined-behaviour sanitizers, so that a read outside an array (every
// array here is a heap block of exactly its size) or a sum that wraps around fails the run.  Prints "ok".
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../k-slam_amd/host/batch_check.hpp"

namespace {
using kslam_batch::Level;
const Level LEVELS[3] = {Level::groups, Level::pairs, Level::records};
const char *const LEVEL_NAME[3] = {"groups", "pairs", "records"};
constexpr uint32_t NO = KSLAM_NO_OVERLAP;
constexpr uint64_t U64_MAX = ~0ull;

int failures = 0;

struct Batch {
  std::vector<kslam_overlap> ov;
  uint64_t n_cigar = 0;
  std::vector<uint64_t> roff;   // n_reads + 1 of them, or none
  std::vector<kslam_read_pair> groups;
  std::vector<kslam_paired_overlap> pairs;
  uint64_t claimed_overlaps = U64_MAX;   // (a count that is not the array's)

  kslam_batch::Arrays arrays() const {
    return kslam_batch::Arrays{ov.empty() ? nullptr : ov.data(),
                               claimed_overlaps != U64_MAX ? claimed_overlaps : ov.size(),
                               n_cigar,
                               roff.empty() ? nullptr : roff.data(),
                               roff.empty() ? 0 : roff.size() - 1,
                               groups.empty() ? nullptr : groups.data(),
                               groups.size(),
                               pairs.empty() ? nullptr : pairs.data(),
                               pairs.size()};
  }
};

kslam_overlap record(uint32_t read, uint64_t cigar_off, uint32_t cigar_len) {
  kslam_overlap o{};
  o.read = read;
  o.cigar_off = cigar_off;
  o.cigar_len = cigar_len;
  return o;
}
kslam_paired_overlap pair_of(uint32_t r1, uint32_t r2) {
  kslam_paired_overlap p{};
  p.r1 = r1;
  p.r2 = r2;
  return p;
}
kslam_read_pair group(uint64_t first, uint64_t count) { return kslam_read_pair{0, 1, first, count}; }

// two reads of 3 and 2 bases, a record of each with one CIGAR word, two alignment pairs (both mates; the second mate alone), a
// group of each
Batch sound() {
  Batch b;
  b.ov = {record(0, 0, 1), record(1, 1, 1)};
  b.n_cigar = 2;
  b.roff = {0, 3, 5};
  b.pairs = {pair_of(0, 1), pair_of(1, NO)};
  b.groups = {group(0, 1), group(1, 1)};
  return b;
}

// the check of b at every level: `from` is the first level that refuses it, with `message`; the levels before it accept it
void expect(const char *what, const Batch &b, int from, const std::string &message) {
  for (int l = 0; l < 3; l++) {
    const std::string want = l >= from ? message : std::string();
    const std::string got = kslam_batch::check(b.arrays(), LEVELS[l]);
    if (got != want) {
      failures++;
      printf("FAILED %s at level %s: got \"%s\", expected \"%s\"\n", what, LEVEL_NAME[l], got.c_str(), want.c_str());
    }
  }
}
void accept(const char *what, const Batch &b) { expect(what, b, 3, ""); }
// ... at one level: a batch with two faults, of which each level names its own first
void expect_at(const char *what, const Batch &b, int l, const std::string &message) {
  const std::string got = kslam_batch::check(b.arrays(), LEVELS[l]);
  if (got != message) {
    failures++;
    printf("FAILED %s at level %s: got \"%s\", expected \"%s\"\n", what, LEVEL_NAME[l], got.c_str(), message.c_str());
  }
}

// the records the callable sees and the longest read, at every level
void expect_outputs(const char *what, const Batch &b, const std::multiset<uint32_t> &named, uint64_t longest) {
  for (int l = 0; l < 3; l++) {
    std::multiset<uint32_t> seen;
    uint64_t got_longest = 77;
    const std::string got = kslam_batch::check(b.arrays(), LEVELS[l], &got_longest, [&](uint32_t idx) { seen.insert(idx); });
    const std::multiset<uint32_t> want_seen = l >= 1 ? named : std::multiset<uint32_t>();
    const uint64_t want_longest = l >= 2 ? longest : 0;
    if (!got.empty() || seen != want_seen || got_longest != want_longest) {
      failures++;
      printf("FAILED %s at level %s: \"%s\", %zu records named, longest read %llu\n", what, LEVEL_NAME[l], got.c_str(), seen.size(),
             (unsigned long long)got_longest);
    }
  }
}

}  // namespace

int main() {
  const std::string outside0 = "read pair 0: first + count lies outside the pairs array";
  const std::string overlap1 = "read pair 1: the groups' slices must ascend and not overlap";

  accept("everything empty, null pointers", Batch());
  accept("the sound batch", sound());

  {   // first + count against the end of the pairs array
    Batch b = sound();
    b.groups = {group(0, 2)};
    accept("first + count == n_pairs", b);
    b.groups = {group(0, 3)};
    expect("count one too many", b, 0, outside0);
    b.groups = {group(1, 2)};
    expect("first + count one too many", b, 0, outside0);
    b.groups = {group(2, 0)};
    accept("an empty group at the end", b);
    b.groups = {group(3, 0)};
    expect("an empty group behind the end", b, 0, outside0);
    b.groups = {group(U64_MAX, 2)};
    expect("first = 2^64 - 1, count = 2: no wrap-around", b, 0, outside0);
    b.groups = {group(1, U64_MAX)};
    expect("count = 2^64 - 1: no wrap-around", b, 0, outside0);
    b.groups = {group(0, 1), group(1, 2)};
    expect("the second group's count one too many", b, 0, "read pair 1: first + count lies outside the pairs array");
  }
  {   // two groups against each other
    Batch b = sound();
    accept("two groups that touch", b);
    b.groups = {group(0, 2), group(1, 1)};
    expect("two groups that overlap by one", b, 0, overlap1);
    b.groups = {group(1, 1), group(0, 1)};
    expect("two groups that descend", b, 0, overlap1);
    b.groups = {group(0, 1), group(0, 0)};
    expect("an empty group inside the one before", b, 0, overlap1);
  }
  {   // alignment pair -> overlap record
    Batch b = sound();
    b.pairs[1] = pair_of(NO, 1);
    accept("r2 = n_overlaps - 1", b);
    b.pairs[1] = pair_of(1, 0);
    accept("r1 = n_overlaps - 1", b);
    b.pairs[1] = pair_of(2, NO);
    expect("r1 = n_overlaps", b, 1, "alignment pair 1 refers to overlap record 2 of 2");
    b.pairs[1] = pair_of(NO, 2);
    expect("r2 = n_overlaps", b, 1, "alignment pair 1 refers to overlap record 2 of 2");
    b.pairs[0] = pair_of(4294967294u, 0);
    expect("r1 = 2^32 - 2", b, 1, "alignment pair 0 refers to overlap record 4294967294 of 2");
    b = sound();
    b.pairs[1] = pair_of(2, NO);
    b.groups = {group(0, 1)};
    accept("a pair no group holds is not looked at", b);
    b = Batch();
    b.pairs = {pair_of(NO, NO), pair_of(NO, NO)};
    b.groups = {group(0, 2)};
    accept("KSLAM_NO_OVERLAP on both sides, no overlap record at all", b);
    expect_outputs("KSLAM_NO_OVERLAP on both sides names nothing", b, {}, 0);
    b.pairs[1] = pair_of(0, NO);
    expect("record 0 of none", b, 1, "alignment pair 1 refers to overlap record 0 of 0");
  }
  {   // group by group: the first group's pair comes before the second group's slice
    Batch b = sound();
    b.pairs[0] = pair_of(2, NO);
    b.groups = {group(0, 1), group(0, 1)};
    expect_at("two faults, the second group's slice", b, 0, overlap1);
    expect_at("two faults, the first group's pair", b, 1, "alignment pair 0 refers to overlap record 2 of 2");
    expect_at("two faults, the first group's pair", b, 2, "alignment pair 0 refers to overlap record 2 of 2");
  }
  {   // 2^32 overlap records: refused before any of them is looked at
    Batch b = sound();
    b.claimed_overlaps = 1ull << 32;
    expect("2^32 overlap records", b, 1, "2^32 or more overlap records");
    b.claimed_overlaps = (1ull << 32) - 1;
    accept("2^32 - 1 overlap records", b);
    b.claimed_overlaps = 1ull << 32;
    b.roff = {0, 3, 2};
    b.groups = {group(0, 3)};
    expect_at("2^32 overlap records come first", b, 0, outside0);
    expect_at("2^32 overlap records come first", b, 1, "2^32 or more overlap records");
    expect_at("2^32 overlap records come first", b, 2, "2^32 or more overlap records");
  }
  {   // a record's CIGAR slice against the pool
    Batch b = sound();
    b.ov[0] = record(0, 2, 0);
    accept("cigar_off == n_cigar, length 0", b);
    b.ov[0] = record(0, 2, 1);
    expect("cigar_off == n_cigar, length 1", b, 2, "overlap record 0: its CIGAR slice lies outside the pool");
    b.ov[0] = record(0, 3, 0);
    expect("cigar_off behind the pool, length 0", b, 2, "overlap record 0: its CIGAR slice lies outside the pool");
    b.ov[0] = record(0, 0, 2);
    accept("the whole pool", b);
    b.ov[0] = record(0, 0, 1);
    b.ov[1] = record(1, 1, 2);
    expect("length one too many", b, 2, "overlap record 1: its CIGAR slice lies outside the pool");
    b.ov[1] = record(1, U64_MAX, 2);
    expect("cigar_off = 2^64 - 1, length 2: no wrap-around", b, 2, "overlap record 1: its CIGAR slice lies outside the pool");
    b = sound();
    b.ov[1] = record(1, 1, 5);
    b.pairs = {pair_of(0, NO), pair_of(0, NO)};
    accept("a record no live pair names is not looked at", b);
  }
  {   // a record's read
    Batch b = sound();
    b.ov[1] = record(2, 1, 1);
    expect("read == n_reads", b, 2, "overlap record 1 refers to read 2 of 2");
    b.roff.clear();
    expect("read 0 of none", b, 2, "overlap record 0 refers to read 0 of 0");
  }
  {   // the read offsets
    Batch b = sound();
    b.roff = {0, 3, 2};
    expect("offsets descending at the last read", b, 2, "the read offsets must ascend");
    b.roff = {4, 3, 5};
    expect("offsets descending at the first read", b, 2, "the read offsets must ascend");
    b.roff = {0, 3, 3};
    accept("an empty last read", b);
    b.roff = {0, 3, 2};
    b.groups = {group(0, 3)};
    expect_at("two faults: the offsets come before the groups", b, 2, "the read offsets must ascend");
    expect_at("two faults: below the offsets' level, the group", b, 1, outside0);
    expect_at("two faults: below the offsets' level, the group", b, 0, outside0);
  }
  {   // what comes back
    Batch b = sound();
    expect_outputs("the sound batch: records 0, 1 and 1 again; reads of 3 and 2", b, {0, 1, 1}, 3);
    b.roff = {0, 1, 5};
    b.pairs = {pair_of(NO, 1), pair_of(NO, NO)};
    expect_outputs("record 1 alone; reads of 1 and 4", b, {1}, 4);
    b.groups = {group(1, 1)};
    expect_outputs("a pair no group holds names nothing", b, {}, 4);
    b = sound();
    b.pairs[1] = pair_of(2, NO);
    std::multiset<uint32_t> seen;   // the records named before the fault, and only they
    const std::string got = kslam_batch::check(b.arrays(), Level::records, nullptr, [&](uint32_t idx) { seen.insert(idx); });
    if (got != "alignment pair 1 refers to overlap record 2 of 2" || seen != std::multiset<uint32_t>{0, 1}) {
      failures++;
      printf("FAILED a fault in the second group: \"%s\", %zu records named\n", got.c_str(), seen.size());
    }
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
