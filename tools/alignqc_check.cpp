// alignqc_check.cpp -- host-only run of the alignment QC report's host side (include/kslam_alignqc.h: kslam_tail_align_qc,
// kslam_align_qc_write) on random records -- both strands, insertions and deletions, every skip reason (one byte past the read,
// one past the entry among them, on the last read and the last entry of their arrays), records nobody names, groups with dead
// tails and with count == 0 --; the tables are checked against sums taken while the records were made.
// tools/sanitize_host.sh builds it with ASan+UBSan.
//   g++ -O2 -std=c++17 -pthread tools/alignqc_check.cpp k-slam_amd/host/alignqc.cpp -o /tmp/alignqc_check
//   /tmp/alignqc_check [n_records] [out_dir]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <random>
#include <string>
#include <unistd.h>
#include <vector>

#include "../include/kslam_alignqc.h"

const char *kslam_tail_last_error(void) { return "(see the status)"; }   // host/tail.cpp is not linked

namespace {
char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }
struct Want { uint64_t records = 0, reverse = 0, skipped = 0, m = 0, compared = 0, miss = 0, ins_ev = 0, ins = 0, del_ev = 0, del = 0, unaligned = 0; };
}  // namespace

int main(int argc, char **argv) {
  const uint64_t n_records = argc > 1 ? strtoull(argv[1], 0, 10) : 20000;
  const std::string dir = argc > 2 ? argv[2] : "/tmp";
  const uint32_t C = 64;
  std::mt19937_64 rng(11);
  const char alphabet[] = "ACGTACGTACGTACGTNacgt";   // mostly upper-case ACGT
  const uint64_t n_entries = 17;
  std::string gbases;
  std::vector<uint64_t> goff(1, 0);
  for (uint64_t e = 0; e < n_entries; e++) {
    const uint64_t len = 150 + rng() % 400;
    for (uint64_t i = 0; i < len; i++) gbases += alphabet[rng() % (sizeof alphabet - 1)];
    goff.push_back(gbases.size());
  }
  std::string rbases, rqual;
  std::vector<uint64_t> roff(1, 0);
  std::vector<uint32_t> pool;
  std::vector<kslam_overlap> ov;
  std::vector<bool> is_skip, is_rev;
  std::vector<Want> each;   // what record i adds when it contributes
  for (uint64_t i = 0; i < n_records; i++) {
    const bool last = i + 1 == n_records;   // the last record sits on the last entry and reads one byte past both ends
    const uint32_t e = last ? (uint32_t)n_entries - 1 : (uint32_t)(rng() % n_entries);
    const int64_t ref_len = (int64_t)(goff[e + 1] - goff[e]);
    const bool rc = rng() % 2;
    kslam_overlap o;
    memset(&o, 0, sizeof o);
    o.read = (uint32_t)i;
    o.entry = e;
    o.revcomp = rc;
    o.cigar_off = pool.size();
    // a CIGAR of M runs with I / D runs between them
    const int64_t span = 20 + (int64_t)(rng() % 100);
    int64_t rp = last ? ref_len - span : (int64_t)(rng() % (uint64_t)(ref_len - span - 8)), left = span;
    o.ref_begin = (int32_t)rp;
    std::string query;
    Want w;
    w.records = 1;
    while (left > 0) {
      const int64_t m = std::min<int64_t>(left, 1 + (int64_t)(rng() % 70));
      pool.push_back((uint32_t)(m << 4));
      for (int64_t j = 0; j < m; j++) {
        const char r = gbases[goff[e] + rp + j];
        char q = rng() % 16 == 0 ? alphabet[rng() % (sizeof alphabet - 1)] : r;
        query += q;
        const bool ru = r == 'A' || r == 'C' || r == 'G' || r == 'T', qu = q == 'A' || q == 'C' || q == 'G' || q == 'T';
        w.compared += ru && qu;
        w.miss += ru && qu && r != q;
      }
      w.m += (uint64_t)m;
      rp += m;
      left -= m;
      if (left > 3 && rng() % 3 == 0) {
        const int64_t n = 1 + (int64_t)(rng() % 3);
        if (rng() % 2) {
          pool.push_back((uint32_t)(n << 4 | 1));
          query.append((size_t)n, 'G');
          w.ins_ev++;
          w.ins += (uint64_t)n;
        } else {
          pool.push_back((uint32_t)(n << 4 | 2));
          rp += n;
          left -= n;
          w.del_ev++;
          w.del += (uint64_t)n;
        }
      }
    }
    const uint64_t clip = rng() % 4;   // unaligned bases in front of the alignment
    o.query_begin = (int32_t)clip;
    query.insert(0, clip, 'T');
    w.unaligned = clip;
    w.reverse = rc;
    // a skip reason for one record in eight, and for the last one
    const uint32_t why = last ? 4 : (rng() % 8 == 0 ? 1 + (uint32_t)(rng() % 6) : 0);
    if (why == 1) o.entry = (uint32_t)n_entries + (uint32_t)(rng() % 3);
    if (why == 2) o.ref_begin = -1 - (int32_t)(rng() % 5);
    if (why == 3) pool.back() += 1u << 4, pool.push_back((uint32_t)((ref_len) << 4));   // an M run longer than the entry
    if (why == 4) pool.push_back(1u << 4);                                              // one M column past the read (and, on `last`, past the entry)
    if (why == 5) pool.push_back(1u << 4 | 1);                                          // one inserted base past the read
    if (why == 6) pool.push_back((uint32_t)((ref_len + 1) << 4 | 2));                    // a D run past the entry
    o.cigar_len = why == 1 && rng() % 2 ? 0 : (uint32_t)(pool.size() - o.cigar_off);      // (and cigar_len == 0)
    if (why) {
      w = Want();
      w.records = w.skipped = 1;
    }
    std::string read = query;
    if (rc) {
      std::reverse(read.begin(), read.end());
      for (char &c : read) c = complement(c);
    }
    rbases += read;
    for (size_t j = 0; j < read.size(); j++) rqual += (char)(rng() % 256);
    roff.push_back(rbases.size());
    ov.push_back(o);
    each.push_back(w);
  }
  // groups: live pairs, dead tails, count == 0; about a tenth of the records is named by nobody or by dead pairs alone
  std::vector<kslam_read_pair> rp;
  std::vector<kslam_paired_overlap> pr;
  std::vector<uint8_t> named(n_records, 0);
  uint64_t want_groups = 0, want_both = 0, want_r1 = 0, want_r2 = 0, want_sum = 0;
  std::vector<uint64_t> want_insert(KSLAM_ALIGN_QC_INSERT_BINS, 0);
  for (uint64_t i = 0; i < n_records;) {
    const uint64_t size = 1 + rng() % 4, live = rng() % 10 == 0 ? rng() % size : size;
    rp.push_back(kslam_read_pair{(uint32_t)i, 0, pr.size(), live});
    want_groups += live != 0;
    for (uint64_t k = 0; k < size; k++) {
      kslam_paired_overlap p;
      memset(&p, 0, sizeof p);
      const uint32_t a = (uint32_t)std::min<uint64_t>(i + rng() % 3, n_records - 1), b = (uint32_t)std::min<uint64_t>(i + rng() % 3, n_records - 1);
      const uint32_t kind = (uint32_t)(rng() % 4);
      p.r1 = kind == 2 ? KSLAM_NO_OVERLAP : a;
      p.r2 = kind == 1 ? KSLAM_NO_OVERLAP : b;
      p.insert_size = rng() % 8 == 0 ? 0xFFFFFFFFu - (uint32_t)(rng() % 3) : (uint32_t)(rng() % 1200);
      if (k < live) {
        if (p.r1 != KSLAM_NO_OVERLAP) named[p.r1] = 1;
        if (p.r2 != KSLAM_NO_OVERLAP) named[p.r2] = 1;
        if (p.r1 != KSLAM_NO_OVERLAP && p.r2 != KSLAM_NO_OVERLAP) {
          want_both++;
          want_sum += p.insert_size;
          want_insert[std::min<uint64_t>(p.insert_size, KSLAM_ALIGN_QC_INSERT_BINS - 1)]++;
        } else if (p.r1 != KSLAM_NO_OVERLAP) {
          want_r1++;
        } else {
          want_r2++;
        }
      }
      pr.push_back(p);
    }
    i += 1 + rng() % 3;
  }
  named[n_records - 1] = 1;   // the record that reads past both ends contributes
  rp.push_back(kslam_read_pair{0, 0, pr.size(), 1});
  want_groups++;
  {
    kslam_paired_overlap p;
    memset(&p, 0, sizeof p);
    p.r1 = (uint32_t)(n_records - 1);
    p.r2 = KSLAM_NO_OVERLAP;
    pr.push_back(p);
    want_r1++;
  }
  Want want;
  for (uint64_t i = 0; i < n_records; i++) {
    if (!named[i]) continue;
    const Want &w = each[i];
    want.records += w.records; want.reverse += w.reverse; want.skipped += w.skipped; want.m += w.m; want.compared += w.compared; want.miss += w.miss;
    want.ins_ev += w.ins_ev; want.ins += w.ins; want.del_ev += w.del_ev; want.del += w.del; want.unaligned += w.unaligned;
  }
  // the arrays end where their last byte ends: a read past them is the sanitizer's to find
  std::vector<char> gb(gbases.begin(), gbases.end()), rb(rbases.begin(), rbases.end()), rq(rqual.begin(), rqual.end());
  kslam_align_qc_tables t;
  auto run = [&](const char *quality, kslam_align_qc_tables *out) {
    return kslam_tail_align_qc(gb.data(), goff.data(), n_entries, ov.data(), ov.size(), pool.data(), pool.size(), rb.data(), roff.data(), n_records,
                               rp.data(), rp.size(), pr.data(), pr.size(), quality, 0, C, out);
  };
  if (run(rq.data(), &t) != KSLAM_OK) {
    fprintf(stderr, "kslam_tail_align_qc failed\n");
    return 1;
  }
  const kslam_align_qc_stream &S = t.stream[0];
  const uint64_t got[11] = {S.n_records, S.n_reverse, S.n_skipped, S.m_columns, S.compared, S.mismatches, S.ins_events, S.ins_bases, S.del_events, S.del_bases,
                            S.unaligned_bases};
  const uint64_t exp[11] = {want.records, want.reverse, want.skipped, want.m, want.compared, want.miss, want.ins_ev, want.ins, want.del_ev, want.del,
                            want.unaligned};
  for (int k = 0; k < 11; k++)
    if (got[k] != exp[k]) {
      fprintf(stderr, "scalar %d differs: %llu, the records' sum is %llu\n", k, (unsigned long long)got[k], (unsigned long long)exp[k]);
      return 1;
    }
  uint64_t cyc[4] = {0, 0, 0, 0}, cq = 0, cm = 0, subst = 0, nm = 0, ident = 0;
  for (uint64_t r = 0; r <= C; r++) {
    for (int k = 0; k < 4; k++) cyc[k] += S.cycle[r * 4 + k];
    for (uint64_t q = 0; q < 95; q++) cq += S.cq_compared[r * 95 + q], cm += S.cq_mismatch[r * 95 + q];
  }
  for (int k = 0; k < 16; k++) subst += S.subst[k];
  for (int k = 0; k < 65; k++) nm += S.nm[k];
  for (int k = 0; k < 101; k++) ident += S.identity[k];
  if (cyc[0] != want.compared || cyc[1] != want.miss || cyc[2] != want.ins || cyc[3] != want.del_ev || cq != want.compared || cm != want.miss ||
      subst != want.compared || nm != want.records - want.skipped || ident > nm || S.n_without_quality != 0 || t.stream[1].n_records != 0) {
    fprintf(stderr, "the tables' sums differ from the scalars\n");
    return 1;
  }
  if (t.n_read_pairs != want_groups || t.pairs_both != want_both || t.pairs_r1_only != want_r1 || t.pairs_r2_only != want_r2 || t.insert_sum != want_sum ||
      memcmp(t.insert, want_insert.data(), sizeof(uint64_t) * want_insert.size()) != 0) {
    fprintf(stderr, "the pair counters differ\n");
    return 1;
  }
  // without a quality column: the same scalars, no cell by quality
  kslam_align_qc_tables u;
  if (run(nullptr, &u) != KSLAM_OK || u.stream[0].compared != want.compared || u.stream[0].n_without_quality != want.records) return 1;
  for (uint64_t k = 0; k < (C + 1) * 95; k++)
    if (u.stream[0].cq_compared[k] || u.stream[0].cq_mismatch[k]) return 1;
  kslam_tail_align_qc_free(&u);
  // refusals: nothing is read outside the arrays, nothing is written for tables nobody laid out
  std::vector<kslam_read_pair> bad = rp;
  bad.back().count = pr.size() + 1;
  kslam_align_qc_tables none;
  if (kslam_tail_align_qc(gb.data(), goff.data(), n_entries, ov.data(), ov.size(), pool.data(), pool.size(), rb.data(), roff.data(), n_records, bad.data(),
                          bad.size(), pr.data(), pr.size(), rq.data(), 0, C, &none) != KSLAM_ERR_ARG || none.block)
    return 1;
  const std::string name = dir + "/alignqc_check.json";
  const int fd = open(name.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0 || kslam_align_qc_write(&t, fd) != KSLAM_OK) {
    fprintf(stderr, "writing %s failed\n", name.c_str());
    return 1;
  }
  const off_t written = lseek(fd, 0, SEEK_END);
  kslam_align_qc_tables wrong = t;
  wrong.n_words++;
  if (kslam_align_qc_write(&wrong, fd) != KSLAM_ERR_ARG || lseek(fd, 0, SEEK_END) != written || close(fd) != 0) return 1;
  unlink(name.c_str());
  kslam_tail_align_qc_free(&t);
  printf("%llu records (%llu contribute, %llu skipped), %llu compared columns, %llu mismatches, %llu pairs with both mates, %lld bytes\n",
         (unsigned long long)n_records, (unsigned long long)want.records, (unsigned long long)want.skipped, (unsigned long long)want.compared,
         (unsigned long long)want.miss, (unsigned long long)want_both, (long long)written);
  return 0;
}
