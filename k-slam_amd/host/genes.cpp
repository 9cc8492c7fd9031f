// genes.cpp -- include/kslam_genes.h, the host side: the twin of csrc/genes.hip (the same rows from host arrays, one serial pass
// with the linear walk over an entry's genes) and the table writer.  Plain C++, no GPU.
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#include "../../include/kslam_genes.h"
#include "batch_check.hpp"
#include "workers.hpp"

namespace {
using namespace kslam_host;

// GenbankEntry::getGene (src/GenbankTools.h:170-185) in 64 bits: the gene of entry e that shares most with [start, stop), the
// first among equals; -1 when none shares a base
int64_t best_gene(const kslam_index_view &ix, uint32_t e, int32_t start, int32_t stop, int64_t *shared_out) {
  int64_t best = -1, widest = 0;
  if (ix.n_genes)
    for (uint64_t g = ix.gene_first[e]; g < ix.gene_first[e + 1]; g++) {
      const int64_t lo = std::max<int64_t>(start, ix.gene_start[g]), hi = std::min<int64_t>(stop, ix.gene_stop[g]);
      if (hi - lo > widest) {
        best = (int64_t)g;
        widest = hi - lo;
      }
    }
  *shared_out = widest;
  return best;
}

// text[off[i] .. off[i + 1]) behind s (an empty field may come with a null text)
void append_field(std::string &s, const char *text, const uint64_t *off, uint64_t i) {
  if (off[i + 1] > off[i]) s.append(text + off[i], off[i + 1] - off[i]);
}

void need_gene_columns(const kslam_index_view *ix) {
  if (!ix) fail(KSLAM_ERR_ARG, "null index view");
  if (ix->n_genes && (!ix->gene_first || !ix->gene_start || !ix->gene_stop)) fail(KSLAM_ERR_ARG, "index view has n_genes > 0 but no gene columns");
  if (!ix->n_genes) return;
  bool ok = ix->n_entries > 0 && ix->gene_first[0] == 0 && ix->gene_first[ix->n_entries] == ix->n_genes;
  for (uint64_t e = 0; ok && e < ix->n_entries; e++) ok = ix->gene_first[e] <= ix->gene_first[e + 1];
  if (!ok) fail(KSLAM_ERR_ARG, "the index view's gene_first does not ascend from 0 to n_genes");
}
}  // namespace

extern "C" kslam_status kslam_tail_genes(const kslam_index_view *index, const kslam_read_pair *read_pairs, uint64_t n_read_pairs,
                                         const kslam_paired_overlap *pairs, uint64_t n_pairs, kslam_gene_row **rows_out, uint64_t *n_rows,
                                         kslam_gene_stats *stats) {
  if (rows_out) *rows_out = nullptr;
  if (n_rows) *n_rows = 0;
  if (stats) memset(stats, 0, sizeof *stats);
  return guarded([&] {
    if (!rows_out || !n_rows || !stats || (n_read_pairs && !read_pairs) || (n_pairs && !pairs)) fail(KSLAM_ERR_ARG, "null argument");
    need_gene_columns(index);
    const std::string fault = kslam_batch::check({nullptr, 0, 0, nullptr, 0, read_pairs, n_read_pairs, pairs, n_pairs}, kslam_batch::Level::groups);
    if (!fault.empty()) fail(KSLAM_ERR_ARG, fault);
    const uint64_t G = index->n_genes;
    std::vector<kslam_gene_row> table(G);
    for (uint64_t g = 0; g < G; g++) table[g] = kslam_gene_row{g, 0, 0, 0};
    kslam_gene_stats st;
    memset(&st, 0, sizeof st);
    for (uint64_t g = 0; g < n_read_pairs; g++) {
      const kslam_read_pair &rp = read_pairs[g];
      int64_t only = -1;      // the gene of every live record so far
      bool one_gene = true;
      for (uint64_t k = rp.first; k < rp.first + rp.count; k++) {
        const kslam_paired_overlap &p = pairs[k];
        st.n_alignments++;
        int64_t gene = -1, shared = 0;
        if (p.entry >= index->n_entries) st.n_skipped++;
        else gene = best_gene(*index, p.entry, p.ref_start, p.ref_end, &shared);
        if (gene >= 0) {
          st.n_in_gene++;
          table[gene].alignments++;
          table[gene].overlap_bases += (uint64_t)shared;
        } else if (p.entry < index->n_entries) {
          st.n_no_gene++;
        }
        if (gene < 0 || (k != rp.first && gene != only)) one_gene = false;
        only = gene;
      }
      if (rp.count && one_gene) table[only].unique_read_pairs++;
    }
    uint64_t n = 0;
    for (uint64_t g = 0; g < G; g++) n += table[g].alignments != 0;
    kslam_gene_row *out = (kslam_gene_row *)malloc(sizeof(kslam_gene_row) * (n + 1));
    if (!out) fail(KSLAM_ERR_OOM, "host allocation failed");
    uint64_t at = 0;
    for (uint64_t g = 0; g < G; g++)
      if (table[g].alignments) out[at++] = table[g];
    st.n_rows = n;
    *rows_out = out;
    *n_rows = n;
    *stats = st;
  });
}

extern "C" kslam_status kslam_genes_write(const kslam_index_view *index, const kslam_gene_row *rows, uint64_t n_rows, int fd) {
  return guarded([&] {
    if (!index || (n_rows && !rows)) fail(KSLAM_ERR_ARG, "null argument");
    if (n_rows && (!index->locus_tag_off || !index->taxonomy_id || !index->gene_first || !index->gene_start || !index->gene_stop ||
                   !index->gene_name_off || !index->protein_id_off || !index->product_off))
      fail(KSLAM_ERR_ARG, "index view needs locus tags, taxonomy ids and the gene columns");
    if (n_rows) need_gene_columns(index);
    for (uint64_t i = 0; i < n_rows; i++)
      if (rows[i].gene >= index->n_genes) fail(KSLAM_ERR_ARG, "row " + std::to_string(i) + ": gene " + std::to_string(rows[i].gene) + " is not one of the index view's");
    // rpk per row, and their sum in row order
    std::vector<double> rpk(n_rows);
    double sum = 0.0;
    for (uint64_t i = 0; i < n_rows; i++) {
      const int64_t length = (int64_t)index->gene_stop[rows[i].gene] - (int64_t)index->gene_start[rows[i].gene];
      rpk[i] = length > 0 ? (double)rows[i].alignments * 1000.0 / (double)length : 0.0;
      sum += rpk[i];
    }
    std::string text = "#entry\tlocus\ttaxid\tgene\tstart\tstop\tlength\tname\tprotein_id\tproduct\talignments\tunique_read_pairs\toverlap_bases\trpk\ttpm\n";
    char num[256];
    uint64_t e = 0;   // the entry of a gene: the rows mostly ascend, so the search starts where the last one ended
    for (uint64_t i = 0; i < n_rows; i++) {
      const kslam_gene_row &r = rows[i];
      const uint64_t g = r.gene;
      if (index->gene_first[e] > g) e = 0;
      while (index->gene_first[e + 1] <= g) e++;   // (gene_first[n_entries] == n_genes > g)
      const int64_t start = index->gene_start[g], stop = index->gene_stop[g];
      text += std::to_string(e);
      text += '\t';
      append_field(text, index->locus_tag, index->locus_tag_off, e);
      snprintf(num, sizeof num, "\t%u\t%llu\t%lld\t%lld\t%lld\t", index->taxonomy_id[e], (unsigned long long)g, (long long)start, (long long)stop,
               (long long)(stop - start));
      text += num;
      append_field(text, index->gene_name, index->gene_name_off, g);
      text += '\t';
      append_field(text, index->protein_id, index->protein_id_off, g);
      text += '\t';
      append_field(text, index->product, index->product_off, g);
      snprintf(num, sizeof num, "\t%llu\t%llu\t%llu\t%.4f\t%.4f\n", (unsigned long long)r.alignments, (unsigned long long)r.unique_read_pairs,
               (unsigned long long)r.overlap_bases, rpk[i], sum != 0.0 ? rpk[i] * 1e6 / sum : 0.0);
      text += num;
    }
    const char *p = text.data();
    size_t n = text.size();
    while (n) {
      const ssize_t w = ::write(fd, p, n);
      if (w < 0) {
        if (errno == EINTR) continue;
        fail(KSLAM_ERR_ARG, std::string("writing the gene table failed: ") + strerror(errno));
      }
      p += w;
      n -= (size_t)w;
    }
  });
}
