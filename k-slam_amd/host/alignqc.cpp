// alignqc.cpp -- include/kslam_alignqc.h, the host side: the twin of csrc/alignqc.hip (the same tables from host arrays, one
// serial walk, a base at a time) and the writer of the JSON report.  Plain C++, no GPU.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#include "../../include/kslam_alignqc.h"
#include "pileup_walk.hpp"
#include "workers.hpp"

namespace {
using namespace kslam_host;
using namespace kslam_pileup;
constexpr uint64_t NQ = KSLAM_ALIGN_QC_QUAL_COLS, NC = KSLAM_ALIGN_QC_CYCLE_COLS, NL = KSLAM_ALIGN_QC_LEN_BINS, NN = KSLAM_ALIGN_QC_NM_BINS,
                   NI = KSLAM_ALIGN_QC_IDENTITY_BINS, NS = KSLAM_ALIGN_QC_INSERT_BINS, NSC = KSLAM_ALIGN_QC_SCALARS;

uint32_t resolve_cycles(uint32_t max_cycles) {
  if (max_cycles > KSLAM_ALIGN_QC_MAX_CYCLES) fail(KSLAM_ERR_ARG, "max_cycles must be 0 (= 512) or 1 .. 65536");
  return max_cycles ? max_cycles : KSLAM_ALIGN_QC_DEFAULT_CYCLES;
}

// a stream's tables inside the block, writable
struct StreamWords {
  uint64_t *w, *subst, *ins_len, *del_len, *nm, *identity, *cycle, *cq_compared, *cq_mismatch;
  StreamWords(uint64_t *block, uint64_t C, int z) {
    w = block + KSLAM_ALIGN_QC_REPORT_WORDS + (uint64_t)z * KSLAM_ALIGN_QC_STREAM_WORDS(C);
    subst = w + NSC;
    ins_len = subst + 16;
    del_len = ins_len + NL;
    nm = del_len + NL;
    identity = nm + NN;
    cycle = identity + NI;
    cq_compared = cycle + (C + 1) * NC;
    cq_mismatch = cq_compared + (C + 1) * NQ;
  }
};

// the views of a block in the header's layout
void point_into(kslam_align_qc_tables *t) {
  const uint64_t C = t->max_cycles;
  uint64_t *b = t->block;
  t->n_read_pairs = b[0];
  t->pairs_both = b[1];
  t->pairs_r1_only = b[2];
  t->pairs_r2_only = b[3];
  t->insert_sum = b[4];
  t->insert = b + 6;
  for (int z = 0; z < 2; z++) {
    const StreamWords S(b, C, z);
    kslam_align_qc_stream &V = t->stream[z];
    V.n_records = S.w[0];
    V.n_reverse = S.w[1];
    V.n_skipped = S.w[2];
    V.n_without_quality = S.w[3];
    V.m_columns = S.w[4];
    V.compared = S.w[5];
    V.mismatches = S.w[6];
    V.ins_events = S.w[7];
    V.ins_bases = S.w[8];
    V.del_events = S.w[9];
    V.del_bases = S.w[10];
    V.unaligned_bases = S.w[11];
    V.subst = S.subst;
    V.ins_len = S.ins_len;
    V.del_len = S.del_len;
    V.nm = S.nm;
    V.identity = S.identity;
    V.cycle = S.cycle;
    V.cq_compared = S.cq_compared;
    V.cq_mismatch = S.cq_mismatch;
  }
}

inline uint64_t qual_col(uint8_t q) { return q >= 33 && q <= 126 ? (uint64_t)(q - 33) : 94; }

std::string ratio(uint64_t num, uint64_t den) {
  char buf[64];
  snprintf(buf, sizeof buf, "\"%.6f\"", den ? (double)num / (double)den : 0.0);
  return buf;
}
std::string num(uint64_t v) { return std::to_string((unsigned long long)v); }
std::string array_of(const uint64_t *v, uint64_t n) {
  std::string s = "[";
  for (uint64_t i = 0; i < n; i++) {
    if (i) s += ", ";
    s += num(v[i]);
  }
  return s + "]";
}

// the scalar lines shared by the summary and a stream's block; w: the twelve scalars
void scalar_lines(std::string &o, const uint64_t *w) {
  const std::string in = "    ";
  static const char *const names[NSC] = {"records", "reverse", "skipped", "without_quality", "m_columns", "compared", "mismatches", "ins_events",
                                         "ins_bases", "del_events", "del_bases", "unaligned_bases"};
  for (uint64_t k = 0; k < NSC; k++) {
    o += in + "\"" + names[k] + "\": " + num(w[k]) + ",\n";
    if (k == 6) o += in + "\"error_rate\": " + ratio(w[6], w[5]) + ",\n";
  }
  o += in + "\"mean_identity\": " + ratio(w[5] - w[6], w[5] + w[8] + w[10]);
}

// {"key": count, ...} of the bins that hold a count; the last bin under `pool` when it is given
void sparse(std::string &o, const char *key, const uint64_t *v, uint64_t n, const char *pool, int base, const char *end) {
  o += std::string("\"") + key + "\": {";
  bool first = true;
  for (uint64_t i = 0; i < n; i++) {
    if (!v[i]) continue;
    if (!first) o += ", ";
    first = false;
    o += "\"" + (pool && i == n - 1 ? std::string(pool) : num(i + (uint64_t)base)) + "\": " + num(v[i]);
  }
  o += std::string("}") + end;
}

void stream_block(std::string &o, const char *name, const kslam_align_qc_stream &S, const uint64_t *w, uint64_t C) {
  const std::string in = "    ";
  o += "  \"" + std::string(name) + "\": {\n";
  scalar_lines(o, w);
  o += ",\n";
  uint64_t rate_rows = 0;
  for (uint64_t r = 0; r < C; r++)
    if (S.cycle[r * NC]) rate_rows = r + 1;
  o += in + "\"mismatch_rate_by_cycle\": [";
  for (uint64_t r = 0; r < rate_rows; r++) {
    if (r) o += ", ";
    o += ratio(S.cycle[r * NC + 1], S.cycle[r * NC]);
  }
  o += "],\n";
  o += in + "\"mismatch_rate_tail\": " + ratio(S.cycle[C * NC + 1], S.cycle[C * NC]) + ",\n";
  static const char *const cols[NC] = {"compared_by_cycle", "mismatches_by_cycle", "inserted_bases_by_cycle", "deletions_by_cycle"};
  for (uint64_t k = 0; k < NC; k++) {
    uint64_t last = 0;
    for (uint64_t r = 0; r < C; r++)
      if (S.cycle[r * NC + k]) last = r + 1;
    o += in + "\"" + cols[k] + "\": [";
    for (uint64_t r = 0; r < last; r++) {
      if (r) o += ", ";
      o += num(S.cycle[r * NC + k]);
    }
    o += "],\n";
  }
  o += in + "\"tail\": " + array_of(S.cycle + C * NC, NC) + ",\n";
  o += in + "\"substitutions\": {";
  uint64_t matches = 0;
  for (int r = 0; r < 4; r++)
    for (int q = 0; q < 4; q++) {
      if (r == q) {
        matches += S.subst[4 * r + q];
        continue;
      }
      o += std::string("\"") + "ACGT"[r] + ">" + "ACGT"[q] + "\": " + num(S.subst[4 * r + q]) + ", ";
    }
  o += "\"matches\": " + num(matches) + "},\n";
  o += in + "\"by_quality\": {";
  bool first = true;
  for (uint64_t q = 0; q < NQ; q++) {
    uint64_t n = 0, m = 0;
    for (uint64_t r = 0; r <= C; r++) {
      n += S.cq_compared[r * NQ + q];
      m += S.cq_mismatch[r * NQ + q];
    }
    if (!n) continue;
    if (!first) o += ", ";
    first = false;
    char buf[64];
    snprintf(buf, sizeof buf, "\"%.6f\"", n && m ? -10.0 * log10((double)m / (double)n) + 0.0 : 0.0);   // (+ 0.0: a rate of 1 gives -0.0)
    o += "\"" + (q < 94 ? num(q) : std::string("invalid")) + "\": [" + num(n) + ", " + num(m) + ", " + buf + "]";
  }
  o += "},\n";
  o += in;
  sparse(o, "insertion_lengths", S.ins_len, NL, ">64", 1, ",\n");
  o += in;
  sparse(o, "deletion_lengths", S.del_len, NL, ">64", 1, ",\n");
  o += in;
  sparse(o, "edit_distance_counts", S.nm, NN, "64+", 0, ",\n");
  o += in;
  sparse(o, "identity_counts", S.identity, NI, nullptr, 0, "\n");
  o += "  }";
}

}  // namespace

extern "C" kslam_status kslam_tail_align_qc(const char *entry_bases, const uint64_t *entry_offsets, uint64_t n_entries, const kslam_overlap *overlaps,
                                            uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar, const char *read_bases,
                                            const uint64_t *read_offsets, uint64_t n_reads, const kslam_read_pair *read_pairs,
                                            uint64_t n_read_pairs, const kslam_paired_overlap *pairs, uint64_t n_pairs, const char *read_quality,
                                            int paired, uint32_t max_cycles, kslam_align_qc_tables *tables) {
  if (tables) memset(tables, 0, sizeof *tables);
  uint64_t *block = nullptr;
  const kslam_status st = guarded([&] {
    if (!tables || (n_entries && !entry_offsets) || (n_overlaps && !overlaps) || (n_cigar && !cigar_pool) || (n_reads && !read_offsets) ||
        (n_read_pairs && !read_pairs) || (n_pairs && !pairs))
      fail(KSLAM_ERR_ARG, "null argument");
    const uint64_t C = resolve_cycles(max_cycles);
    if (paired && (n_reads & 1)) fail(KSLAM_ERR_ARG, "a paired batch holds an even number of reads");
    if (n_reads && read_offsets[n_reads] && !read_bases) fail(KSLAM_ERR_ARG, "null argument");
    if (n_entries && entry_offsets[n_entries] && !entry_bases) fail(KSLAM_ERR_ARG, "null argument");
    const uint64_t nw = KSLAM_ALIGN_QC_WORDS(C);
    block = (uint64_t *)calloc(nw, sizeof(uint64_t));
    if (!block) fail(KSLAM_ERR_OOM, "out of host memory");
    // ---- the walk of the contributing set ----
    const uint64_t half = n_reads / 2;
    const std::string fault = for_each_named_record({overlaps, n_overlaps, n_cigar, read_offsets, n_reads, read_pairs, n_read_pairs, pairs, n_pairs}, cigar_pool,
                                                    entry_offsets, n_entries, [&](const kslam_overlap &o, int64_t L, int64_t, bool holds) {
      const StreamWords S(block, C, paired && o.read >= half ? 1 : 0);
      S.w[0]++;
      if (!read_quality) S.w[3]++;
      if (!holds) { S.w[2]++; return; }
      const uint8_t *ref = (const uint8_t *)entry_bases + entry_offsets[o.entry];
      const uint8_t *read = (const uint8_t *)read_bases + read_offsets[o.read];
      const uint8_t *qual = read_quality ? (const uint8_t *)read_quality + read_offsets[o.read] : nullptr;
      const bool rc = o.revcomp != 0;
      if (rc) S.w[1]++;
      auto cycle_of = [&](int64_t q) { return rc ? L - 1 - q : q; };
      auto row_of = [&](int64_t cyc) { return (uint64_t)cyc < C ? (uint64_t)cyc : C; };
      uint64_t mcols = 0, compared = 0, miss = 0, ins = 0, del = 0;
      int64_t rp = o.ref_begin, qp = o.query_begin > 0 ? o.query_begin : 0;
      for (uint32_t k = 0; k < o.cigar_len; k++) {
        const uint32_t c = cigar_pool[o.cigar_off + k], op = c & 15u;
        const int64_t len = c >> 4;
        if (op == 0) {
          for (int64_t j = 0; j < len; j++) {
            const int64_t cyc = cycle_of(qp + j);
            const uint8_t r = ref[rp + j], b = read[cyc], q = rc ? complement(b) : b;
            const int rk = acgt(r), qk = acgt(q);
            if (rk > 3 || qk > 3) continue;
            const uint64_t row = row_of(cyc);
            compared++;
            S.cycle[row * NC]++;
            if (qual) S.cq_compared[row * NQ + qual_col(qual[cyc])]++;
            S.subst[rc ? 4 * (3 - rk) + (3 - qk) : 4 * rk + qk]++;
            if (rk != qk) {
              miss++;
              S.cycle[row * NC + 1]++;
              if (qual) S.cq_mismatch[row * NQ + qual_col(qual[cyc])]++;
            }
          }
          mcols += (uint64_t)len;
          rp += len;
          qp += len;
        } else if (op == 1) {
          if (len) {
            S.w[7]++;
            S.ins_len[(len < (int64_t)NL ? len : (int64_t)NL) - 1]++;
            for (int64_t j = 0; j < len; j++) S.cycle[row_of(cycle_of(qp + j)) * NC + 2]++;
          }
          ins += (uint64_t)len;
          qp += len;
        } else if (op == 2) {
          if (len) {
            S.w[9]++;
            S.del_len[(len < (int64_t)NL ? len : (int64_t)NL) - 1]++;
            if (L > 0) S.cycle[row_of(cycle_of(qp < L - 1 ? qp : L - 1)) * NC + 3]++;
          }
          del += (uint64_t)len;
          rp += len;
        }
      }
      S.w[4] += mcols;
      S.w[5] += compared;
      S.w[6] += miss;
      S.w[8] += ins;
      S.w[10] += del;
      S.w[11] += (uint64_t)L - mcols - ins;
      const uint64_t edits = miss + ins + del, den = compared + ins + del;
      S.nm[edits < NN - 1 ? edits : NN - 1]++;
      if (den) S.identity[100 * (compared - miss) / den]++;
    });
    if (!fault.empty()) fail(KSLAM_ERR_ARG, fault);
    // ---- the pairs (the check has passed: every live pair lies inside the arrays) ----
    uint64_t *insert = block + 6;
    for (uint64_t g = 0; g < n_read_pairs; g++) {
      const kslam_read_pair &rp = read_pairs[g];
      if (rp.count) block[0]++;
      for (uint64_t k = rp.first; k < rp.first + rp.count; k++) {
        const bool h1 = pairs[k].r1 != KSLAM_NO_OVERLAP, h2 = pairs[k].r2 != KSLAM_NO_OVERLAP;
        if (h1 && h2) {
          block[1]++;
          block[4] += pairs[k].insert_size;
          insert[pairs[k].insert_size < NS - 1 ? pairs[k].insert_size : NS - 1]++;
        } else if (h1) {
          block[2]++;
        } else if (h2) {
          block[3]++;
        }
      }
    }
    tables->max_cycles = (uint32_t)C;
    tables->paired = paired ? 1 : 0;
    tables->n_words = nw;
    tables->block = block;
    point_into(tables);
  });
  if (st != KSLAM_OK) {
    free(block);
    if (tables) memset(tables, 0, sizeof *tables);
  }
  return st;
}

extern "C" void kslam_tail_align_qc_free(kslam_align_qc_tables *tables) {
  if (!tables) return;
  free(tables->block);
  memset(tables, 0, sizeof *tables);
}

extern "C" kslam_status kslam_align_qc_write(const kslam_align_qc_tables *tables, int fd) {
  return guarded([&] {
    if (!tables || !tables->block) fail(KSLAM_ERR_ARG, "null argument");
    const uint64_t C = tables->max_cycles;
    if (!C || C > KSLAM_ALIGN_QC_MAX_CYCLES || tables->n_words != KSLAM_ALIGN_QC_WORDS(C)) fail(KSLAM_ERR_ARG, "tables that were not laid out by this library");
    // the counters from the block alone: the views are made again here
    kslam_align_qc_tables t = *tables;
    point_into(&t);
    const bool paired = t.paired != 0;
    const uint64_t *w0 = StreamWords(t.block, C, 0).w, *w1 = StreamWords(t.block, C, 1).w;
    uint64_t sum[NSC];
    for (uint64_t k = 0; k < NSC; k++) sum[k] = w0[k] + w1[k];
    std::string o = "{\n";
    o += "  \"kslam_align_qc\": 1,\n";
    o += std::string("  \"paired\": ") + (paired ? "true" : "false") + ",\n";
    o += "  \"max_cycles\": " + num(C) + ",\n";
    o += "  \"summary\": {\n";
    scalar_lines(o, sum);
    o += ",\n";
    o += "    \"read_pairs\": " + num(t.n_read_pairs) + ",\n";
    o += "    \"pairs_both\": " + num(t.pairs_both) + ",\n";
    o += "    \"pairs_r1_only\": " + num(t.pairs_r1_only) + ",\n";
    o += "    \"pairs_r2_only\": " + num(t.pairs_r2_only) + ",\n";
    o += "    \"insert_size_mean\": " + ratio(t.insert_sum, t.pairs_both) + ",\n";
    uint64_t median = 0, seen = 0;
    if (t.pairs_both)
      for (median = 0; median < NS - 1; median++) {
        seen += t.insert[median];
        if (2 * seen >= t.pairs_both) break;
      }
    o += "    \"insert_size_median\": \"" + (median == NS - 1 ? std::string(">1000") : num(median)) + "\"\n";
    o += "  },\n";
    stream_block(o, "read1", t.stream[0], w0, C);
    o += ",\n";
    if (paired) {
      stream_block(o, "read2", t.stream[1], w1, C);
      o += ",\n";
    }
    o += "  ";
    sparse(o, "insert_size_counts", t.insert, NS, ">1000", 0, "\n");
    o += "}\n";
    const char *p = o.data();
    size_t n = o.size();
    while (n) {
      const ssize_t w = ::write(fd, p, n);
      if (w < 0) {
        if (errno == EINTR) continue;
        fail(KSLAM_ERR_ARG, std::string("writing the alignment QC report failed: ") + strerror(errno));
      }
      p += w;
      n -= (size_t)w;
    }
  });
}
