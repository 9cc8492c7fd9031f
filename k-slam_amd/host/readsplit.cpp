// readsplit.cpp -- include/kslam_readsplit.h, the host twin: the records of a batch split by outcome from host text, the same
// bytes csrc/readsplit.hip writes.  For a batch whose pseudo-assembly the device left to the host (its final read pairs exist
// only after the host stage) and for a host that formats everything itself.  Plain C++, one pass over each text.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kslam_readsplit.h"
#include "../../include/kslam_tail.h"
#include "workers.hpp"

namespace {
using namespace kslam_host;

// one stream's lines by the reader's rule (host/fastq.cpp: index_stream; csrc/fastq_lines.h: line_span)
struct Stream {
  const char *t = nullptr;
  uint64_t len = 0;
  std::vector<uint64_t> ev;   // terminator positions
  uint64_t rest_start = 0, n = 0;

  uint64_t line_after(uint64_t p) const { return (t[p] == '\r' && p + 1 < len && t[p + 1] == '\n') ? p + 2 : p + 1; }
  void index(const char *text, uint64_t length, uint64_t max_pairs, bool at_eof) {
    t = text;
    len = length;
    // without the rest of the stream a trailing "\r" may or may not be half of "\r\n"
    const uint64_t scan_len = (!at_eof && len && t[len - 1] == '\r') ? len - 1 : len;
    for (uint64_t p = 0; p < scan_len; p++)
      if (t[p] == '\r' || (t[p] == '\n' && !(p > 0 && t[p - 1] == '\r'))) ev.push_back(p);
    rest_start = ev.empty() ? 0 : line_after(ev.back());
    const uint64_t rest_lines = at_eof ? (rest_start < len ? 2 : 1) : 0;
    n = (ev.size() + rest_lines) / 4;
    if (max_pairs && n > max_pairs) n = max_pairs;
  }
  void line(uint64_t l, uint64_t *a, uint64_t *b) const {
    if (l < ev.size()) {
      *a = l == 0 ? 0 : line_after(ev[l - 1]);
      *b = ev[l];
    } else if (l == ev.size() && rest_start < len) {
      *a = rest_start; *b = len;     // the unterminated rest
    } else {
      *a = len; *b = len;            // the empty line read at end of stream
    }
  }
};

}  // namespace

extern "C" kslam_status kslam_tail_split_reads(const char *r1, uint64_t len1, const char *r2, uint64_t len2, uint64_t max_pairs, int at_eof,
                                               const kslam_read_pair *read_pairs, uint64_t n_read_pairs, uint32_t which,
                                               kslam_reads_out *out) {
  if (out) memset(out, 0, sizeof *out);
  std::string blocks[4];
  const kslam_status st = guarded([&] {
    if (!out || (len1 && !r1) || (len2 && !r2) || (n_read_pairs && !read_pairs)) fail(KSLAM_ERR_ARG, "null argument");
    if (which == 0 || which > 3u) fail(KSLAM_ERR_ARG, "the reads-out mask must be 1, 2 or 3");
    const bool single = r2 == nullptr && len2 == 0;
    Stream s[2];
    s[0].index(r1, len1, max_pairs, at_eof != 0);
    if (!single) s[1].index(r2, len2, max_pairs, at_eof != 0);
    if (!single && s[0].n != s[1].n) fail(KSLAM_ERR_ARG, "mismatch in R1 and R2 size");
    const uint64_t n = s[0].n;
    std::vector<uint8_t> flag(n + 1, 0);
    for (uint64_t g = 0; g < n_read_pairs; g++) {
      const kslam_read_pair &rp = read_pairs[g];
      if (rp.r1_read >= n || (!single && rp.r2_read != rp.r1_read + n)) fail(KSLAM_ERR_ARG, "read pair refers to a record outside the batch");
      flag[rp.r1_read] = 1;
    }
    for (int k = 0; k < (single ? 1 : 2); k++)
      for (uint64_t r = 0; r < n; r++) {
        const bool f = flag[r] != 0;
        if (k == 0) out->n_records[f ? 0 : 1]++;
        if (!(which & (f ? KSLAM_READS_OUT_CLASSIFIED : KSLAM_READS_OUT_UNCLASSIFIED))) continue;
        std::string &dst = blocks[(f ? 0 : 2) + k];
        for (int l = 0; l < 4; l++) {
          uint64_t a, b;
          s[k].line(4 * r + l, &a, &b);
          dst.append(s[k].t + a, b - a);
          dst.push_back('\n');
        }
      }
    for (int k = 0; k < 4; k++) {
      const bool wanted = (which & (k < 2 ? KSLAM_READS_OUT_CLASSIFIED : KSLAM_READS_OUT_UNCLASSIFIED)) && !(single && (k & 1));
      if (!wanted) continue;
      out->data[k] = (char *)malloc(blocks[k].size() + 1);
      if (!out->data[k]) fail(KSLAM_ERR_OOM, "out of host memory");
      memcpy(out->data[k], blocks[k].data(), blocks[k].size());
      out->len[k] = blocks[k].size();
    }
    out->flags = KSLAM_READS_OUT_HOST_MEMORY;
  });
  if (st != KSLAM_OK && out) {
    for (int k = 0; k < 4; k++) free(out->data[k]);
    memset(out, 0, sizeof *out);
  }
  return st;
}

extern "C" void kslam_release_reads_out(kslam_ctx *ctx, kslam_reads_out *out) {
  if (!out) return;
  for (int k = 0; k < 4; k++) {
    if (!out->data[k]) continue;
    if (out->flags & KSLAM_READS_OUT_HOST_MEMORY) free(out->data[k]);
    else kslam_free_pinned(ctx, out->data[k]);
  }
  memset(out, 0, sizeof *out);
}
