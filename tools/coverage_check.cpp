// coverage_check.cpp -- host-only run of the coverage table's host side (include/kslam_coverage.h: kslam_tail_coverage,
// kslam_coverage_write) on synthetic arrays with dead records, missing mates and mates of every invalid kind; the rows are
// checked against sums taken while the arrays were made.  tools/sanitize_host.sh builds it with ASan+UBSan and with TSan.
//   g++ -O2 -std=c++17 -pthread tools/coverage_check.cpp k-slam_amd/host/coverage.cpp -o /tmp/coverage_check
//   /tmp/coverage_check [n_read_pairs] [out_dir]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <random>
#include <string>
#include <unistd.h>
#include <vector>

#include "../include/kslam_coverage.h"

const char *kslam_tail_last_error(void) { return "(see the status)"; }   // host/tail.cpp is not linked

int main(int argc, char **argv) {
  const uint64_t n_groups = argc > 1 ? strtoull(argv[1], 0, 10) : 20000;
  const std::string dir = argc > 2 ? argv[2] : "/tmp";
  const uint64_t n_entries = 37;
  std::mt19937_64 rng(5);
  std::vector<uint64_t> len(n_entries), bases_off(n_entries + 1, 0), tag_off(n_entries + 1, 0);
  std::vector<uint32_t> tax(n_entries);
  std::string tags;
  for (uint64_t e = 0; e < n_entries; e++) {
    len[e] = e == 3 ? 0 : 1 + rng() % 3000;
    bases_off[e + 1] = bases_off[e] + len[e];
    tags += "LOC" + std::to_string(e);
    tag_off[e + 1] = tags.size();
    tax[e] = 100 + (uint32_t)e;
  }
  std::vector<kslam_overlap> ov;
  std::vector<kslam_paired_overlap> pr;
  std::vector<kslam_read_pair> rp;
  uint64_t want_alignments = 0, want_aligned = 0, want_skipped = 0;
  for (uint64_t g = 0; g < n_groups; g++) {
    const uint64_t size = 1 + rng() % 5, live = rng() % 4 ? size : rng() % (size + 1);
    rp.push_back(kslam_read_pair{(uint32_t)g, (uint32_t)(n_groups + g), pr.size(), live});
    for (uint64_t k = 0; k < size; k++) {
      kslam_paired_overlap p;
      memset(&p, 0, sizeof p);
      p.entry = (uint32_t)(rng() % (n_entries + 1));   // (one value outside)
      p.r1 = p.r2 = KSLAM_NO_OVERLAP;
      if (k < live && p.entry < n_entries) want_alignments++;
      for (int m = 0; m < 2; m++) {
        if (rng() % 6 == 0) continue;
        kslam_overlap o;
        memset(&o, 0, sizeof o);
        o.entry = (uint32_t)(rng() % n_entries);
        const int64_t L = (int64_t)len[o.entry];
        o.ref_begin = L ? (int32_t)(rng() % L) : 0;
        o.ref_end = L ? (int32_t)std::min<int64_t>(L - 1, o.ref_begin + (int64_t)(rng() % 400)) : 0;
        switch (rng() % 40) {
          case 0: o.entry = (uint32_t)n_entries + 2; break;
          case 1: o.ref_begin = -3; break;
          case 2: o.ref_end = o.ref_begin - 1; break;
          case 3: o.ref_end = (int32_t)L; break;
          default: break;
        }
        const bool valid = o.entry < n_entries && o.ref_begin >= 0 && o.ref_end >= o.ref_begin && (uint64_t)o.ref_end < len[o.entry];
        if (k < live) {
          if (valid) want_aligned += (uint64_t)(o.ref_end - o.ref_begin) + 1;
          else want_skipped++;
        }
        (m ? p.r2 : p.r1) = (uint32_t)ov.size();
        ov.push_back(o);
      }
      pr.push_back(p);
    }
  }
  std::vector<kslam_entry_coverage> rows(n_entries);
  uint64_t skipped = 0;
  if (kslam_tail_coverage(len.data(), n_entries, ov.data(), ov.size(), rp.data(), rp.size(), pr.data(), pr.size(), rows.data(), &skipped) != KSLAM_OK) {
    fprintf(stderr, "kslam_tail_coverage failed\n");
    return 1;
  }
  uint64_t alignments = 0, aligned = 0, covered = 0;
  for (uint64_t e = 0; e < n_entries; e++) {
    alignments += rows[e].alignments;
    aligned += rows[e].aligned_bases;
    covered += rows[e].covered_bases;
    if (rows[e].covered_bases > len[e] || rows[e].covered_bases > rows[e].aligned_bases || rows[e].unique_read_pairs > rows[e].alignments) {
      fprintf(stderr, "entry %llu: a row that cannot be\n", (unsigned long long)e);
      return 1;
    }
  }
  if (alignments != want_alignments || aligned != want_aligned || skipped != want_skipped) {
    fprintf(stderr, "sums differ: %llu / %llu alignments, %llu / %llu aligned bases, %llu / %llu skipped\n", (unsigned long long)alignments,
            (unsigned long long)want_alignments, (unsigned long long)aligned, (unsigned long long)want_aligned, (unsigned long long)skipped,
            (unsigned long long)want_skipped);
    return 1;
  }
  // refusals: nothing is read outside the arrays
  std::vector<kslam_read_pair> bad = rp;
  bad.back().count = pr.size() + 1;
  if (kslam_tail_coverage(len.data(), n_entries, ov.data(), ov.size(), bad.data(), bad.size(), pr.data(), pr.size(), rows.data(), &skipped) != KSLAM_ERR_ARG) return 1;
  kslam_tail_coverage(len.data(), n_entries, ov.data(), ov.size(), rp.data(), rp.size(), pr.data(), pr.size(), rows.data(), &skipped);
  kslam_index_view view;
  memset(&view, 0, sizeof view);
  view.n_entries = n_entries;
  view.bases_off = bases_off.data();
  view.locus_tag = tags.data();
  view.locus_tag_off = tag_off.data();
  view.taxonomy_id = tax.data();
  const std::string name = dir + "/coverage_check.tsv";
  const int fd = open(name.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0 || kslam_coverage_write(&view, rows.data(), n_entries, fd) != KSLAM_OK || close(fd) != 0) {
    fprintf(stderr, "writing %s failed\n", name.c_str());
    return 1;
  }
  unlink(name.c_str());
  printf("%llu read pairs, %llu alignments, %llu aligned and %llu covered bases, %llu skipped mates\n", (unsigned long long)n_groups,
         (unsigned long long)alignments, (unsigned long long)aligned, (unsigned long long)covered, (unsigned long long)skipped);
  return 0;
}
