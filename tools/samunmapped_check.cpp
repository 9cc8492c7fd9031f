// samunmapped_check.cpp -- the host twin of the rows for the reads without alignment (include/kslam_samunmapped.h,
// host/samunmapped.cpp) on a made-up batch, every form (text / BAM, SEQ off / on, with / without qualities, paired / single-end),
// with the sizes checked against a count made here.  Plain C++ with its own main: what tools/sanitize_host.sh builds under
// ASan + UBSan.     usage: samunmapped_check N_RECORDS
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/kslam_samunmapped.h"

int main(int argc, char **argv) {
  const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1000;
  uint64_t state = 88172645463325252ull;
  auto rnd = [&] { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  uint64_t total = 0;
  for (int paired = 0; paired < 2; paired++) {
    const uint64_t n_reads = paired ? 2 * n : n;
    std::string bases, quals, ids;
    std::vector<uint64_t> boff(1, 0), ioff(1, 0);
    for (uint64_t r = 0; r < n_reads; r++) {
      const uint64_t len = rnd() % 40 == 0 ? 0 : rnd() % 152;
      for (uint64_t k = 0; k < len; k++) {
        bases.push_back("ACGTNacgtnRYKM.="[rnd() % 16]);
        quals.push_back((char)(33 + rnd() % 94));
      }
      boff.push_back(bases.size());
      ids += "read" + std::to_string(r % n) + std::string(rnd() % 7 == 0 ? 200 : 0, 'x');
      ioff.push_back(ids.size());
    }
    std::vector<kslam_read_pair> rp;
    std::vector<uint8_t> has_row(n, 0);
    uint64_t first = 0;
    for (uint64_t p = 0; p < n; p++) {
      if (rnd() % 2) continue;
      const uint64_t count = rnd() % 5 == 0 ? 0 : 1 + rnd() % 3;   // a group without alignment pairs counts as absent
      rp.push_back(kslam_read_pair{(uint32_t)p, (uint32_t)(paired ? p + n : 0), first, count});
      first += count;
      has_row[p] = count != 0;
    }
    kslam_tail_params P;
    memset(&P, 0, sizeof P);
    P.paired = paired;
    for (int with_qual = 0; with_qual < 2; with_qual++)
      for (int bam = 0; bam < 2; bam++)
        for (int seq = 0; seq < 2; seq++) {
          kslam_reads_view rv = {n_reads, bases.data(), boff.data(), with_qual ? quals.data() : nullptr, boff.data(), ids.data(), ioff.data()};
          char *out = nullptr;
          uint64_t len = 0;
          if (kslam_tail_sam_unmapped(&P, &rv, rp.data(), rp.size(), n, bam, seq, &out, &len) != KSLAM_OK) {
            fprintf(stderr, "kslam_tail_sam_unmapped: %s\n", kslam_tail_last_error());
            return 1;
          }
          uint64_t want = 0;
          for (uint64_t p = 0; p < n; p++) {
            if (has_row[p]) continue;
            for (int mate = 0; mate < (paired ? 2 : 1); mate++) {
              const uint64_t r = p + (mate ? n : 0), id = ioff[r + 1] - ioff[r], L = seq ? boff[r + 1] - boff[r] : 0;
              if (bam) want += 36 + id + 1 + (L + 1) / 2 + L;
              else want += id + 1 + (paired ? (mate ? 3 : 2) : 1) + 15 + (L ? L + 1 + (with_qual ? L : 1) : 3) + 1;   // id, tab, FLAG, the fixed columns, SEQ QUAL, newline
            }
          }
          if (len != want) {
            fprintf(stderr, "paired %d bam %d seq %d qualities %d: %llu bytes, expected %llu\n", paired, bam, seq, with_qual,
                    (unsigned long long)len, (unsigned long long)want);
            return 1;
          }
          total += len;
          free(out);
        }
  }
  printf("%llu bytes in 16 forms\n", (unsigned long long)total);
  return 0;
}
