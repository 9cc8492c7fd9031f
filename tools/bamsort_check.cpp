// bamsort_check.cpp -- the host twins of the coordinate-sorted BAM (include/kslam_bamsort.h; k-slam_amd/host/bamsort.cpp) on
// random records, for the sanitizers (tools/sanitize_host.sh, tests/test_bamsort_host.py): every batch and every stream is a heap
// block of exactly its size, so a walk that reads past one is caught.  Checks what can be checked without a second
// implementation: the output is a permutation in key order with ties in submission order, the index has the size its counts
// give, and broken chains are refused.   usage: bamsort_check N_RECORDS
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/kslam_bamsort.h"
#include "../k-slam_amd/host/workers.hpp"

namespace {

void put32(std::string &o, uint32_t v) {
  for (int k = 0; k < 4; k++) o.push_back((char)(v >> (8 * k)));
}
void put16(std::string &o, uint32_t v) {
  o.push_back((char)v);
  o.push_back((char)(v >> 8));
}

std::string record(int32_t ref, int32_t pos, uint32_t serial, uint32_t span, bool unmapped, uint32_t seq_len) {
  std::string name = "r" + std::to_string(serial), b;
  put32(b, (uint32_t)ref);
  put32(b, (uint32_t)pos);
  b.push_back((char)(name.size() + 1));
  b.push_back(0);
  put16(b, 4680);
  put16(b, unmapped ? 0 : 2);
  put16(b, unmapped ? 4 : 0);
  put32(b, seq_len);
  put32(b, 0xFFFFFFFFu);
  put32(b, 0xFFFFFFFFu);
  put32(b, 0);
  b += name;
  b.push_back('\0');
  if (!unmapped) {
    put32(b, 3u << 4 | 4u);
    put32(b, span << 4 | 0u);
  }
  b.append((seq_len + 1) / 2 + seq_len, '\x11');
  std::string out;
  put32(out, (uint32_t)b.size());
  return out + b;
}

#define NEED(cond)                                                                                 \
  do {                                                                                             \
    if (!(cond)) {                                                                                 \
      fprintf(stderr, "bamsort_check: %s failed at line %d (%s)\n", #cond, __LINE__, kslam_host::g_err.c_str()); \
      return 1;                                                                                    \
    }                                                                                              \
  } while (0)

uint32_t le32(const char *p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
}

}  // namespace

int main(int argc, char **argv) {
  const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 3000;
  const uint32_t n_ref = 5;
  const uint32_t ref_len[5] = {300000, 10, 70000, 1u << 29, 5000};
  std::mt19937_64 rng(17);
  const uint64_t n_batches = 7;
  std::vector<char *> blocks(n_batches, nullptr);
  std::vector<uint64_t> lens(n_batches, 0);
  uint32_t serial = 0;
  for (uint64_t b = 0; b < n_batches; b++) {
    std::string bytes;
    const uint64_t k = b == 3 ? 0 : n / (n_batches - 1);
    for (uint64_t i = 0; i < k; i++) {
      const uint32_t pick = (uint32_t)(rng() % 7);
      if (pick == 6) bytes += record(-1, -1, serial++, 1, true, (uint32_t)(rng() % 120));
      else {
        const uint32_t ref = pick % n_ref == 1 ? 0 : pick % n_ref, span = 1 + (uint32_t)(rng() % 400);
        const bool loose = rng() % 50 == 0;   // a mate without position of its own
        const int32_t pos = loose ? -1 : (int32_t)(rng() % (ref_len[ref] - span));
        bytes += record((int32_t)ref, pos, serial++, span, loose || rng() % 20 == 0, (uint32_t)(rng() % 300));
      }
    }
    lens[b] = bytes.size();
    blocks[b] = (char *)malloc(bytes.size() ? bytes.size() : 1);   // exactly its size
    memcpy(blocks[b], bytes.data(), bytes.size());
  }
  char *stream = nullptr;
  uint64_t len = 0, total = 0;
  NEED(kslam_tail_bam_sort(blocks.data(), lens.data(), n_batches, &stream, &len) == KSLAM_OK);
  for (uint64_t l : lens) total += l;
  NEED(len == total);
  char *exact = (char *)malloc(len ? len : 1);
  memcpy(exact, stream, len);
  free(stream);
  // key order, ties by serial (= submission order)
  uint64_t prev_key = 0, n_rec = 0, n_no_coor = 0;
  long prev_serial = -1;
  for (uint64_t p = 0; p < len;) {
    const uint64_t key = (uint64_t)le32(exact + p + 4) << 32 | (uint32_t)(le32(exact + p + 8) + 1u);
    const long s = strtol(exact + p + 37, nullptr, 10);
    NEED(key >= prev_key && (key > prev_key || s > prev_serial));
    prev_key = key;
    prev_serial = s;
    n_no_coor += (int32_t)le32(exact + p + 4) < 0;
    p += 4 + le32(exact + p);
    n_rec++;
  }
  NEED(n_rec == serial);
  const uint64_t n_members = (len + 65279) / 65280;
  std::vector<uint32_t> sizes(n_members, 20000);
  char *bai = nullptr;
  uint64_t bai_len = 0;
  NEED(kslam_tail_bai(exact, len, n_ref, sizes.data(), n_members, 1234, &bai, &bai_len) == KSLAM_OK);
  NEED(bai_len >= 8 + 8 * n_ref + 8 && memcmp(bai, "BAI\1", 4) == 0);
  uint64_t tail_count;
  memcpy(&tail_count, bai + bai_len - 8, 8);
  NEED(tail_count == n_no_coor);
  free(bai);
  // refusals: a chain cut short, an unsorted stream, a refID outside the list
  if (len > 40) {
    char *cut = (char *)malloc(len - 1);
    memcpy(cut, exact, len - 1);
    NEED(kslam_tail_bai(cut, len - 1, n_ref, sizes.data(), (len - 1 + 65279) / 65280, 0, &bai, &bai_len) == KSLAM_ERR_ARG);
    const char *one[1] = {cut};
    const uint64_t one_len[1] = {len - 1};
    NEED(kslam_tail_bam_sort(one, one_len, 1, &stream, &len) == KSLAM_ERR_ARG);
    free(cut);
  }
  NEED(kslam_tail_bai(exact, total, 3, sizes.data(), n_members, 0, &bai, &bai_len) == KSLAM_ERR_ARG);
  char *header = nullptr;
  uint64_t header_len = 0;
  const char text[] = "@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:a\tLN:300000\n@SQ\tSN:b\tLN:10\n";
  NEED(kslam_tail_bam_sort_header(text, sizeof text - 1, &header, &header_len) == KSLAM_OK);
  NEED(header_len == 12 + (sizeof text - 1) + 2 + 2 * 10 && memcmp(header + 8, "@HD\tVN:1.0\tSO:coordinate\n", 25) == 0);
  free(header);
  free(exact);
  for (char *b : blocks) free(b);
  printf("bamsort_check ok: %llu records, %llu without coordinate\n", (unsigned long long)n_rec, (unsigned long long)n_no_coor);
  puts("bamsort_check ok");
  return 0;
}
