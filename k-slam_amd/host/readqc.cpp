// readqc.cpp -- include/kslam_readqc.h, the host side: the twin of csrc/readqc.hip (the same tables from host columns, one serial
// pass) and the writer of the JSON report.  Plain C++, no GPU.
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <unistd.h>

#include "../../include/kslam_readqc.h"
#include "workers.hpp"

namespace {
using namespace kslam_host;
constexpr uint32_t NB = KSLAM_READ_QC_BASE_COLS, NQ = KSLAM_READ_QC_QUAL_COLS, NM = KSLAM_READ_QC_MEAN_BINS, NG = KSLAM_READ_QC_GC_BINS;

uint32_t resolve_cycles(uint32_t max_cycles) {
  if (max_cycles > KSLAM_READ_QC_MAX_CYCLES) fail(KSLAM_ERR_ARG, "max_cycles must be 0 (= 512) or 1 .. 65536");
  return max_cycles ? max_cycles : KSLAM_READ_QC_DEFAULT_CYCLES;
}

// the stream views of a block in the header's layout
void point_into(kslam_read_qc_tables *t) {
  const uint64_t C = t->max_cycles;
  for (int z = 0; z < 2; z++) {
    uint64_t *w = t->block + (uint64_t)z * t->words_per_stream;
    kslam_read_qc_stream &S = t->stream[z];
    S.n_reads = w[0];
    S.n_bases = w[1];
    S.min_len = w[2];
    S.max_len = w[3];
    S.len_hist = w + 4;
    S.base = S.len_hist + (C + 2);
    S.qual = S.base + (C + 1) * NB;
    S.mean_q = S.qual + (C + 1) * NQ;
    S.gc = S.mean_q + NM;
  }
}

uint32_t base_col(uint8_t b) {
  switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    case 'N': case 'n': return 4;
    default: return 5;
  }
}

std::string ratio(uint64_t num, uint64_t den) {
  char buf[64];
  snprintf(buf, sizeof buf, "\"%.6f\"", den ? (double)num / (double)den : 0.0);
  return buf;
}

std::string num(uint64_t v) { return std::to_string((unsigned long long)v); }

// [a, b, c] of v[0 .. n)
std::string array_of(const uint64_t *v, uint64_t n) {
  std::string s = "[";
  for (uint64_t i = 0; i < n; i++) {
    if (i) s += ", ";
    s += num(v[i]);
  }
  return s + "]";
}

struct Sums {
  uint64_t col[NB] = {0, 0, 0, 0, 0, 0};
  uint64_t q20 = 0, q30 = 0, invalid = 0;
};

Sums sums_of(const kslam_read_qc_stream &S, uint64_t C) {
  Sums u;
  for (uint64_t r = 0; r <= C; r++) {
    for (uint32_t k = 0; k < NB; k++) u.col[k] += S.base[r * NB + k];
    for (uint32_t q = 20; q < 94; q++) u.q20 += S.qual[r * NQ + q];
    for (uint32_t q = 30; q < 94; q++) u.q30 += S.qual[r * NQ + q];
    u.invalid += S.qual[r * NQ + 94];
  }
  return u;
}

std::string row_mean(const uint64_t *row) {
  uint64_t n = 0, sum = 0;
  for (uint32_t q = 0; q < 94; q++) {
    n += row[q];
    sum += (uint64_t)q * row[q];
  }
  return ratio(sum, n);
}

void stream_block(std::string &o, const char *name, const kslam_read_qc_stream &S, uint64_t C) {
  const Sums u = sums_of(S, C);
  const std::string in = "    ";
  o += "  \"" + std::string(name) + "\": {\n";
  o += in + "\"total_reads\": " + num(S.n_reads) + ",\n";
  o += in + "\"total_bases\": " + num(S.n_bases) + ",\n";
  o += in + "\"min_length\": " + num(S.min_len) + ",\n";
  o += in + "\"max_length\": " + num(S.max_len) + ",\n";
  o += in + "\"mean_length\": " + ratio(S.n_bases, S.n_reads) + ",\n";
  o += in + "\"q20_bases\": " + num(u.q20) + ",\n";
  o += in + "\"q30_bases\": " + num(u.q30) + ",\n";
  o += in + "\"gc_content\": " + ratio(u.col[1] + u.col[2], u.col[0] + u.col[1] + u.col[2] + u.col[3]) + ",\n";
  o += in + "\"n_bases\": " + num(u.col[4]) + ",\n";
  o += in + "\"other_bases\": " + num(u.col[5]) + ",\n";
  o += in + "\"invalid_quality_bytes\": " + num(u.invalid) + ",\n";
  // the lengths that occur
  o += in + "\"length_counts\": {";
  bool first = true;
  for (uint64_t l = 0; l <= C + 1; l++) {
    if (!S.len_hist[l]) continue;
    if (!first) o += ", ";
    first = false;
    o += "\"" + (l <= C ? num(l) : ">" + num(C)) + "\": " + num(S.len_hist[l]);
  }
  o += "},\n";
  // base content per cycle
  static const char *const names[NB] = {"A", "C", "G", "T", "N", "other"};
  o += in + "\"content\": {\n";
  std::string col;
  for (uint32_t k = 0; k < NB; k++) {
    uint64_t last = 0;   // rows to write
    for (uint64_t r = 0; r < C; r++)
      if (S.base[r * NB + k]) last = r + 1;
    col = "[";
    for (uint64_t r = 0; r < last; r++) {
      if (r) col += ", ";
      col += num(S.base[r * NB + k]);
    }
    o += in + "  \"" + names[k] + "\": " + col + "],\n";
  }
  o += in + "  \"tail\": " + array_of(S.base + C * NB, NB) + "\n";
  o += in + "},\n";
  // quality per cycle
  uint64_t q_rows = 0;
  for (uint64_t r = 0; r < C; r++)
    for (uint32_t q = 0; q < NQ; q++)
      if (S.qual[r * NQ + q]) q_rows = r + 1;
  o += in + "\"quality_mean\": [";
  for (uint64_t r = 0; r < q_rows; r++) {
    if (r) o += ", ";
    o += row_mean(S.qual + r * NQ);
  }
  o += "],\n";
  o += in + "\"quality_tail_mean\": " + row_mean(S.qual + C * NQ) + ",\n";
  o += in + "\"quality_counts\": {";
  first = true;
  for (uint32_t q = 0; q < NQ; q++) {
    uint64_t last = 0;
    for (uint64_t r = 0; r <= C; r++)
      if (S.qual[r * NQ + q]) last = r + 1;
    if (!last) continue;
    if (!first) o += ", ";
    first = false;
    o += "\"" + (q < 94 ? num(q) : std::string("invalid")) + "\": [";
    for (uint64_t r = 0; r < last; r++) {
      if (r) o += ", ";
      o += num(S.qual[r * NQ + q]);
    }
    o += "]";
  }
  o += "},\n";
  auto bins = [&](const char *key, const uint64_t *v, uint32_t n, const char *end) {
    o += in + "\"" + key + "\": {";
    bool f = true;
    for (uint32_t i = 0; i < n; i++) {
      if (!v[i]) continue;
      if (!f) o += ", ";
      f = false;
      o += "\"" + num(i) + "\": " + num(v[i]);
    }
    o += std::string("}") + end;
  };
  bins("mean_quality_counts", S.mean_q, NM, ",\n");
  bins("gc_counts", S.gc, NG, "\n");
  o += "  }";
}

}  // namespace

extern "C" kslam_status kslam_tail_read_qc(const char *bases, const uint64_t *bases_off, const char *quality, const uint64_t *quality_off,
                                           uint64_t n_reads, int paired, uint32_t max_cycles, kslam_read_qc_tables *tables) {
  if (tables) memset(tables, 0, sizeof *tables);
  uint64_t *block = nullptr;
  const kslam_status st = guarded([&] {
    if (!tables || (n_reads && (!bases || !bases_off || !quality || !quality_off))) fail(KSLAM_ERR_ARG, "null argument");
    const uint64_t C = resolve_cycles(max_cycles);
    if (paired && (n_reads & 1)) fail(KSLAM_ERR_ARG, "a paired batch holds an even number of reads");
    for (uint64_t i = 0; i < n_reads; i++) {
      if (bases_off[i + 1] < bases_off[i] || quality_off[i + 1] < quality_off[i]) fail(KSLAM_ERR_ARG, "the read offsets must ascend");
      if (bases_off[i + 1] - bases_off[i] != quality_off[i + 1] - quality_off[i])
        fail(KSLAM_ERR_ARG, "read " + std::to_string(i) + " has " + std::to_string(bases_off[i + 1] - bases_off[i]) + " bases and " +
                                std::to_string(quality_off[i + 1] - quality_off[i]) + " quality bytes");
    }
    const uint64_t nw = KSLAM_READ_QC_WORDS(C);
    block = (uint64_t *)calloc(2 * nw, sizeof(uint64_t));
    if (!block) fail(KSLAM_ERR_OOM, "out of host memory");
    const uint64_t half = paired ? n_reads / 2 : n_reads;
    for (uint64_t i = 0; i < n_reads; i++) {
      uint64_t *w = block + (i < half ? 0 : nw);
      uint64_t *len_hist = w + 4, *base = len_hist + (C + 2), *qual = base + (C + 1) * NB, *mean_q = qual + (C + 1) * NQ, *gc = mean_q + NM;
      const uint8_t *b = (const uint8_t *)bases + bases_off[i], *q = (const uint8_t *)quality + quality_off[i];
      const uint64_t len = bases_off[i + 1] - bases_off[i];
      if (!w[0] || len < w[2]) w[2] = len;
      if (len > w[3]) w[3] = len;
      w[0]++;
      w[1] += len;
      len_hist[len <= C ? len : C + 1]++;
      uint64_t n_gc = 0, n_acgt = 0, n_q = 0, q_sum = 0;
      for (uint64_t c = 0; c < len; c++) {
        const uint64_t row = c < C ? c : C;
        const uint32_t k = base_col(b[c]);
        base[row * NB + k]++;
        n_gc += k == 1 || k == 2;
        n_acgt += k < 4;
        if (q[c] >= 33 && q[c] <= 126) {
          qual[row * NQ + (q[c] - 33)]++;
          n_q++;
          q_sum += q[c] - 33;
        } else {
          qual[row * NQ + 94]++;
        }
      }
      if (n_q) mean_q[q_sum / n_q]++;
      if (n_acgt) gc[(200 * n_gc + n_acgt) / (2 * n_acgt)]++;
    }
    tables->max_cycles = (uint32_t)C;
    tables->paired = paired ? 1 : 0;
    tables->words_per_stream = nw;
    tables->block = block;
    point_into(tables);
  });
  if (st != KSLAM_OK) {
    free(block);
    if (tables) memset(tables, 0, sizeof *tables);
  }
  return st;
}

extern "C" void kslam_tail_read_qc_free(kslam_read_qc_tables *tables) {
  if (!tables) return;
  free(tables->block);
  memset(tables, 0, sizeof *tables);
}

extern "C" kslam_status kslam_read_qc_write(const kslam_read_qc_tables *tables, int fd) {
  return guarded([&] {
    if (!tables || !tables->block) fail(KSLAM_ERR_ARG, "null argument");
    const uint64_t C = tables->max_cycles;
    if (!C || C > KSLAM_READ_QC_MAX_CYCLES || tables->words_per_stream != KSLAM_READ_QC_WORDS(C)) fail(KSLAM_ERR_ARG, "tables that were not laid out by this library");
    // the counters from the block alone: the views are made again here
    kslam_read_qc_tables t = *tables;
    point_into(&t);
    const bool paired = t.paired != 0;
    const Sums a = sums_of(t.stream[0], C), b = sums_of(t.stream[1], C);
    const uint64_t reads = t.stream[0].n_reads + t.stream[1].n_reads, total = t.stream[0].n_bases + t.stream[1].n_bases;
    uint64_t col[NB];
    for (uint32_t k = 0; k < NB; k++) col[k] = a.col[k] + b.col[k];
    std::string o = "{\n";
    o += "  \"kslam_read_qc\": 1,\n";
    o += std::string("  \"paired\": ") + (paired ? "true" : "false") + ",\n";
    o += "  \"max_cycles\": " + num(C) + ",\n";
    o += "  \"summary\": {\n";
    o += "    \"total_reads\": " + num(reads) + ",\n";
    o += "    \"total_bases\": " + num(total) + ",\n";
    o += "    \"q20_bases\": " + num(a.q20 + b.q20) + ",\n";
    o += "    \"q30_bases\": " + num(a.q30 + b.q30) + ",\n";
    o += "    \"q20_rate\": " + ratio(a.q20 + b.q20, total) + ",\n";
    o += "    \"q30_rate\": " + ratio(a.q30 + b.q30, total) + ",\n";
    o += "    \"gc_content\": " + ratio(col[1] + col[2], col[0] + col[1] + col[2] + col[3]) + ",\n";
    o += "    \"n_bases\": " + num(col[4]) + ",\n";
    o += "    \"other_bases\": " + num(col[5]) + ",\n";
    o += "    \"invalid_quality_bytes\": " + num(a.invalid + b.invalid) + "\n";
    o += "  },\n";
    stream_block(o, "read1", t.stream[0], C);
    if (paired) {
      o += ",\n";
      stream_block(o, "read2", t.stream[1], C);
    }
    o += "\n}\n";
    const char *p = o.data();
    size_t n = o.size();
    while (n) {
      const ssize_t w = ::write(fd, p, n);
      if (w < 0) {
        if (errno == EINTR) continue;
        fail(KSLAM_ERR_ARG, std::string("writing the read QC report failed: ") + strerror(errno));
      }
      p += w;
      n -= (size_t)w;
    }
  });
}
