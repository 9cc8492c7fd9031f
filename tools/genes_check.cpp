// genes_check.cpp -- host-only run of the per-gene table's host side (include/kslam_genes.h: kslam_tail_genes, kslam_genes_write)
// on synthetic genes -- file order descending by start, duplicates, short genes nested in long ones, stop < start, entries
// without genes -- and records with dead tails, gene-less intervals and entries outside the index; the rows are checked against
// sums taken while the records were made.  tools/sanitize_host.sh builds it with ASan+UBSan.
//   g++ -O2 -std=c++17 -pthread tools/genes_check.cpp k-slam_amd/host/genes.cpp -o /tmp/genes_check
//   /tmp/genes_check [n_read_pairs] [out_dir]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <random>
#include <string>
#include <unistd.h>
#include <vector>

#include "../include/kslam_genes.h"

const char *kslam_tail_last_error(void) { return "(see the status)"; }   // host/tail.cpp is not linked

int main(int argc, char **argv) {
  const uint64_t n_groups = argc > 1 ? strtoull(argv[1], 0, 10) : 20000;
  const std::string dir = argc > 2 ? argv[2] : "/tmp";
  const uint64_t n_entries = 23;
  std::mt19937_64 rng(7);
  // Entry e has A(e) anchors: anchor k covers [1000 k + 100, 1000 k + 600).  In the file the anchors come in DESCENDING order of
  // start, each followed by its clutter: a duplicate (the tie goes to the anchor, which comes first), a short gene nested in it,
  // a gene whose stop lies before its start, and a gene that only touches it.
  std::vector<uint64_t> gene_first(n_entries + 1, 0), bases_off(n_entries + 1, 0), tag_off(n_entries + 1, 0);
  std::vector<int32_t> start, stop;
  std::vector<uint32_t> tax(n_entries);
  std::vector<std::vector<uint64_t>> anchor(n_entries);   // anchor[e][k]: its gene index
  std::string tags, names, prots, prods;
  std::vector<uint64_t> name_off(1, 0), prot_off(1, 0), prod_off(1, 0);
  auto add_gene = [&](int64_t b, int64_t t) {
    start.push_back((int32_t)b);
    stop.push_back((int32_t)t);
    if (start.size() % 3) names += "g" + std::to_string(start.size());   // (every third name is empty)
    prots += "NP_" + std::to_string(start.size());
    if (start.size() % 2) prods += "product " + std::to_string(start.size());
    name_off.push_back(names.size());
    prot_off.push_back(prots.size());
    prod_off.push_back(prods.size());
  };
  for (uint64_t e = 0; e < n_entries; e++) {
    const uint64_t A = e % 5 == 2 ? 0 : 1 + rng() % 40;
    anchor[e].assign(A, 0);
    for (uint64_t k = A; k-- > 0;) {
      const int64_t base = 1000 * (int64_t)k;
      anchor[e][k] = start.size();
      add_gene(base + 100, base + 600);
      if (rng() % 2) add_gene(base + 100, base + 600);
      if (rng() % 2) add_gene(base + 200, base + 300);
      if (rng() % 3 == 0) add_gene(base + 500, base + 200);
      if (rng() % 3 == 0) add_gene(base + 600, base + 650);
    }
    gene_first[e + 1] = start.size();
    bases_off[e + 1] = bases_off[e] + 1000 * A;
    tags += "LOC" + std::to_string(e);
    tag_off[e + 1] = tags.size();
    tax[e] = 100 + (uint32_t)e;
  }
  const uint64_t n_genes = start.size();
  kslam_index_view view;
  memset(&view, 0, sizeof view);
  view.n_entries = n_entries;
  view.bases_off = bases_off.data();
  view.locus_tag = tags.data();
  view.locus_tag_off = tag_off.data();
  view.taxonomy_id = tax.data();
  view.n_genes = n_genes;
  view.gene_first = gene_first.data();
  view.gene_start = start.data();
  view.gene_stop = stop.data();
  view.gene_name = names.data();
  view.gene_name_off = name_off.data();
  view.protein_id = prots.data();
  view.protein_id_off = prot_off.data();
  view.product = prods.data();
  view.product_off = prod_off.data();

  std::vector<kslam_paired_overlap> pr;
  std::vector<kslam_read_pair> rp;
  std::vector<uint64_t> want_alignments(n_genes, 0), want_unique(n_genes, 0), want_overlap(n_genes, 0);
  uint64_t want_live = 0, want_none = 0, want_skipped = 0;
  for (uint64_t g = 0; g < n_groups; g++) {
    const uint64_t size = 1 + rng() % 5, live = rng() % 4 ? size : rng() % (size + 1);
    rp.push_back(kslam_read_pair{(uint32_t)g, (uint32_t)(n_groups + g), pr.size(), live});
    int64_t only = -1;      // the gene of every live record of the group, -2 once they differ or one has none
    uint64_t home_e = rng() % n_entries, home_k = rng();
    for (uint64_t k = 0; k < size; k++) {
      kslam_paired_overlap p;
      memset(&p, 0, sizeof p);
      p.r1 = p.r2 = KSLAM_NO_OVERLAP;
      const bool stray = rng() % 8 == 0;
      const uint64_t e = stray ? rng() % (n_entries + 2) : home_e;   // (two values outside)
      p.entry = (uint32_t)e;
      int64_t gene = -1, shared = 0;
      if (e >= n_entries) {
        p.ref_start = 0;
        p.ref_end = 100;
        if (k < live) want_skipped++;
      } else if (anchor[e].empty() || rng() % 10 == 0) {   // between two anchors, or in an entry without genes
        p.ref_start = 700 + (int32_t)(rng() % 100);
        p.ref_end = p.ref_start + 1 + (int32_t)(rng() % 99);
        if (k < live) want_none++;
      } else {
        const uint64_t a = (stray ? rng() : home_k) % anchor[e].size();
        const int64_t b = 1000 * (int64_t)a + 50 + (int64_t)(rng() % 100), t = b + 350 + (int64_t)(rng() % 300);   // from before or inside the anchor to inside or behind it
        p.ref_start = (int32_t)b;
        p.ref_end = (int32_t)t;
        gene = (int64_t)anchor[e][a];
        shared = std::min<int64_t>(t, 1000 * (int64_t)a + 600) - std::max<int64_t>(b, 1000 * (int64_t)a + 100);   // > 250: more than any clutter shares
      }
      if (k < live) {
        want_live++;
        if (gene >= 0) {
          want_alignments[gene]++;
          want_overlap[gene] += (uint64_t)shared;
        }
        only = (k == 0 || only == gene) && gene >= 0 ? gene : -2;
      }
      pr.push_back(p);
    }
    if (live && only >= 0) want_unique[only]++;
  }
  kslam_gene_row *rows = nullptr;
  uint64_t n_rows = 0;
  kslam_gene_stats st;
  if (kslam_tail_genes(&view, rp.data(), rp.size(), pr.data(), pr.size(), &rows, &n_rows, &st) != KSLAM_OK) {
    fprintf(stderr, "kslam_tail_genes failed\n");
    return 1;
  }
  uint64_t want_rows = 0, want_in = 0;
  for (uint64_t g = 0; g < n_genes; g++) {
    want_rows += want_alignments[g] != 0;
    want_in += want_alignments[g];
  }
  if (n_rows != want_rows || st.n_rows != n_rows || st.n_alignments != want_live || st.n_in_gene != want_in || st.n_no_gene != want_none ||
      st.n_skipped != want_skipped) {
    fprintf(stderr, "statistics differ: %llu / %llu rows, %llu / %llu alignments, %llu / %llu in a gene, %llu / %llu without, %llu / %llu skipped\n",
            (unsigned long long)n_rows, (unsigned long long)want_rows, (unsigned long long)st.n_alignments, (unsigned long long)want_live,
            (unsigned long long)st.n_in_gene, (unsigned long long)want_in, (unsigned long long)st.n_no_gene, (unsigned long long)want_none,
            (unsigned long long)st.n_skipped, (unsigned long long)want_skipped);
    return 1;
  }
  for (uint64_t i = 0; i < n_rows; i++) {
    const kslam_gene_row &r = rows[i];
    if (r.gene >= n_genes || (i && rows[i - 1].gene >= r.gene) || r.alignments != want_alignments[r.gene] || r.unique_read_pairs != want_unique[r.gene] ||
        r.overlap_bases != want_overlap[r.gene]) {
      fprintf(stderr, "row %llu (gene %llu) differs from the sums\n", (unsigned long long)i, (unsigned long long)r.gene);
      return 1;
    }
  }
  // refusals: nothing is read outside the arrays, nothing is written for a row of another index
  std::vector<kslam_read_pair> bad = rp;
  bad.back().count = pr.size() + 1;
  kslam_gene_row *none = nullptr;
  uint64_t n_none = 0;
  if (kslam_tail_genes(&view, bad.data(), bad.size(), pr.data(), pr.size(), &none, &n_none, &st) != KSLAM_ERR_ARG || none) return 1;
  const std::string name = dir + "/genes_check.tsv";
  const int fd = open(name.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0 || kslam_genes_write(&view, rows, n_rows, fd) != KSLAM_OK) {
    fprintf(stderr, "writing %s failed\n", name.c_str());
    return 1;
  }
  const off_t written = lseek(fd, 0, SEEK_END);
  kslam_gene_row outside = rows[0];
  outside.gene = n_genes;
  if (kslam_genes_write(&view, &outside, 1, fd) != KSLAM_ERR_ARG || lseek(fd, 0, SEEK_END) != written || close(fd) != 0) return 1;
  unlink(name.c_str());
  free(rows);
  printf("%llu read pairs, %llu genes, %llu rows, %llu alignments (%llu in a gene, %llu without, %llu skipped), %lld bytes\n", (unsigned long long)n_groups,
         (unsigned long long)n_genes, (unsigned long long)n_rows, (unsigned long long)want_live, (unsigned long long)want_in,
         (unsigned long long)want_none, (unsigned long long)want_skipped, (long long)written);
  return 0;
}
