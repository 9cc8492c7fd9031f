// readqc_check.cpp -- host-only run of the read QC report's host side (include/kslam_readqc.h: kslam_tail_read_qc,
// kslam_read_qc_write) on synthetic reads of every length around the pooled row, with every byte value in both columns, paired
// and single-end, and through the argument errors; checks the totals against sums made here and the file's first and last
// bytes.  For tools/sanitize_host.sh (ASan + UBSan); needs no GPU.
//   g++ -O2 -std=c++17 -pthread tools/readqc_check.cpp k-slam_amd/host/readqc.cpp k-slam_amd/host/tail.cpp -o /tmp/readqc_check
//   /tmp/readqc_check [n_reads] [out_dir]
#include <cstdio>
#include <cstdlib>
#include <fcntl.h>
#include <string>
#include <unistd.h>
#include <vector>

#include "../include/kslam_readqc.h"
#include "../include/kslam_tail.h"

#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      fprintf(stderr, "readqc_check: "); \
      fprintf(stderr, __VA_ARGS__);     \
      fprintf(stderr, "\n");            \
      return 1;                         \
    }                                   \
  } while (0)

int main(int argc, char **argv) {
  const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) & ~1ull : 20000;
  const std::string dir = argc > 2 ? argv[2] : "/tmp";
  uint64_t x = 88172645463325252ull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (uint32_t C : {0u, 1u, 7u, 300u, 65536u}) {
    const uint64_t rows = C ? C : 512;
    std::vector<uint64_t> off(n + 1, 0);
    std::string bases, quality;
    uint64_t valid = 0, acgtn_other[6] = {0, 0, 0, 0, 0, 0};
    for (uint64_t i = 0; i < n; i++) {
      const uint64_t len = i % 97 == 0 ? 0 : rnd() % (2 * rows < 700 ? 2 * rows + 3 : 700);
      for (uint64_t c = 0; c < len; c++) {
        const uint8_t b = rnd() % 8 ? "ACGTNacgtn"[rnd() % 10] : (uint8_t)rnd(), q = rnd() % 16 ? 33 + rnd() % 42 : (uint8_t)rnd();
        bases.push_back((char)b);
        quality.push_back((char)q);
        valid += q >= 33 && q <= 126;
        const char u = (char)(b & 0xDF);
        acgtn_other[u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : u == 'N' ? 4 : 5]++;
      }
      off[i + 1] = off[i] + len;
    }
    for (int paired = 0; paired < 2; paired++) {
      kslam_read_qc_tables t;
      CHECK(kslam_tail_read_qc(bases.data(), off.data(), quality.data(), off.data(), n, paired, C, &t) == KSLAM_OK, "kslam_tail_read_qc failed: %s",
            kslam_tail_last_error());
      CHECK(t.max_cycles == rows && t.paired == paired && t.words_per_stream == KSLAM_READ_QC_WORDS(rows), "the tables' head");
      uint64_t reads = 0, total = 0, hist = 0, col[6] = {0, 0, 0, 0, 0, 0}, q_valid = 0, q_all = 0, mean = 0;
      for (int z = 0; z < 2; z++) {
        const kslam_read_qc_stream &S = t.stream[z];
        reads += S.n_reads;
        total += S.n_bases;
        for (uint64_t l = 0; l <= rows + 1; l++) hist += S.len_hist[l];
        for (uint64_t r = 0; r <= rows; r++) {
          for (int k = 0; k < 6; k++) col[k] += S.base[r * 6 + k];
          for (int q = 0; q < 95; q++) (q < 94 ? q_valid : q_all) += S.qual[r * 95 + q];
        }
        for (int m = 0; m < 94; m++) mean += S.mean_q[m];
      }
      q_all += q_valid;
      CHECK(reads == n && hist == n && total == off[n] && q_all == total && q_valid == valid && mean <= n, "the totals (C = %u, paired = %d)", C, paired);
      for (int k = 0; k < 6; k++) CHECK(col[k] == acgtn_other[k], "base column %d (C = %u)", k, C);
      CHECK(paired || t.stream[1].n_reads == 0, "stream 1 of a single-end set");
      const std::string name = dir + "/readqc_check.json";
      const int fd = open(name.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0600);
      CHECK(fd >= 0, "cannot create %s", name.c_str());
      CHECK(kslam_read_qc_write(&t, fd) == KSLAM_OK, "kslam_read_qc_write failed: %s", kslam_tail_last_error());
      const off_t size = lseek(fd, 0, SEEK_END);
      char head[2] = {0, 0}, tail[3] = {0, 0, 0};
      CHECK(size > 100 && pread(fd, head, 2, 0) == 2 && pread(fd, tail, 3, size - 3) == 3, "reading the file back");
      CHECK(head[0] == '{' && head[1] == '\n' && tail[0] == '\n' && tail[1] == '}' && tail[2] == '\n', "the file's first and last bytes");
      close(fd);
      unlink(name.c_str());
      kslam_tail_read_qc_free(&t);
      CHECK(t.block == nullptr, "the free call leaves the block behind");
    }
  }
  // the argument errors
  const char b[] = "ACGTAC", q[] = "IIIIII";
  const uint64_t good[] = {0, 3, 6}, shorter[] = {0, 2, 6}, back[] = {0, 4, 3}, three[] = {0, 2, 4, 6};
  kslam_read_qc_tables t;
  CHECK(kslam_tail_read_qc(b, good, q, shorter, 2, 0, 0, &t) == KSLAM_ERR_ARG && !t.block, "two lengths that differ");
  CHECK(kslam_tail_read_qc(b, back, q, back, 2, 0, 0, &t) == KSLAM_ERR_ARG && !t.block, "offsets that do not ascend");
  CHECK(kslam_tail_read_qc(b, three, q, three, 3, 1, 0, &t) == KSLAM_ERR_ARG && !t.block, "paired with an odd number");
  CHECK(kslam_tail_read_qc(b, good, q, good, 2, 0, 65537, &t) == KSLAM_ERR_ARG && !t.block, "too many cycle rows");
  CHECK(kslam_tail_read_qc(nullptr, nullptr, nullptr, nullptr, 0, 0, 0, &t) == KSLAM_OK && t.stream[0].n_reads == 0 && t.stream[0].min_len == 0, "the empty set");
  CHECK(kslam_read_qc_write(&t, -1) == KSLAM_ERR_ARG, "a bad descriptor");
  kslam_tail_read_qc_free(&t);
  CHECK(kslam_read_qc_write(&t, 1) == KSLAM_ERR_ARG, "tables without a block");
  printf("readqc_check: ok (%llu reads per set)\n", (unsigned long long)n);
  return 0;
}
