// samunmapped.cpp -- include/kslam_samunmapped.h, the host twin: the rows of a batch's reads without alignment, the same bytes
// csrc/samunmapped.hip appends on the device.  For a batch whose text the device left to the host (kslam_stream_classify), and
// the first thing the device is compared with.  Plain C++, one pass over the batch's records.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kslam_samunmapped.h"
#include "../csrc/seqcodes.h"
#include "workers.hpp"

namespace {
using namespace kslam_host;

void put_le(std::string &o, uint32_t v, int k) {
  for (int i = 0; i < k; i++) o.push_back((char)(v >> (8 * i)));
}

struct Cols {   // one read's id, bases and qualities
  const char *id, *bases, *qual;   // qual nullptr: the batch has no qualities
  size_t id_len, len;
};

Cols cols_of(const kslam_reads_view *rd, uint64_t read, bool seq) {
  Cols c{rd->ids + rd->ids_off[read], nullptr, nullptr, (size_t)(rd->ids_off[read + 1] - rd->ids_off[read]), 0};
  if (!seq) return c;
  c.len = (size_t)(rd->bases_off[read + 1] - rd->bases_off[read]);
  c.bases = rd->bases + rd->bases_off[read];
  c.qual = rd->quality ? rd->quality + rd->quality_off[read] : nullptr;
  if (c.qual && rd->quality_off[read + 1] - rd->quality_off[read] != c.len)
    fail(KSLAM_ERR_ARG, "quality string length differs from the read length");
  return c;
}

// QNAME FLAG * 0 0 * * 0 0 SEQ QUAL
void put_line(std::string &o, const Cols &c, uint32_t flag) {
  o.append(c.id, c.id_len);
  o.push_back('\t');
  o.append(std::to_string(flag));
  o.append("\t*\t0\t0\t*\t*\t0\t0\t");
  if (!c.len) {   // the switch off, or a read without bases
    o.append("*\t*\n");
    return;
  }
  o.append(c.bases, c.len);
  o.push_back('\t');
  if (c.qual) o.append(c.qual, c.len); else o.push_back('*');
  o.push_back('\n');
}

// the unplaced record: refID -1, pos -1, bin reg2bin(-1, 0) = 4680, no CIGAR, no tags
void put_record(std::string &o, const Cols &c, uint32_t flag) {
  const size_t n = c.len;
  put_le(o, (uint32_t)(32 + c.id_len + 1 + (n + 1) / 2 + n), 4);   // block_size
  put_le(o, 0xFFFFFFFFu, 4);                                       // refID
  put_le(o, 0xFFFFFFFFu, 4);                                       // pos
  put_le(o, (uint32_t)c.id_len + 1, 1);                            // l_read_name
  put_le(o, 0, 1);                                                 // mapq
  put_le(o, 4680, 2);                                              // bin
  put_le(o, 0, 2);                                                 // n_cigar_op
  put_le(o, flag, 2);
  put_le(o, (uint32_t)n, 4);                                       // l_seq
  put_le(o, 0xFFFFFFFFu, 4);                                       // next_refID
  put_le(o, 0xFFFFFFFFu, 4);                                       // next_pos
  put_le(o, 0, 4);                                                 // tlen
  o.append(c.id, c.id_len);
  o.push_back('\0');
  for (size_t i = 0; i < n; i += 2)   // the last nibble of an odd length is 0
    o.push_back((char)(kslam_seq::nibble((uint8_t)c.bases[i]) << 4 | (i + 1 < n ? kslam_seq::nibble((uint8_t)c.bases[i + 1]) : 0u)));
  for (size_t i = 0; i < n; i++) o.push_back(c.qual ? (char)((uint8_t)c.qual[i] - 33) : (char)0xFF);
}

}  // namespace

extern "C" kslam_status kslam_tail_sam_unmapped(const kslam_tail_params *params, const kslam_reads_view *reads,
                                                const kslam_read_pair *read_pairs, uint64_t n_read_pairs, uint64_t n_consumed_pairs,
                                                int bam, int seq, char **out, uint64_t *len) {
  if (out) *out = nullptr;
  if (len) *len = 0;
  return guarded([&] {
    if (!params || !reads || !out || !len || (n_read_pairs && !read_pairs)) fail(KSLAM_ERR_ARG, "null argument");
    const bool paired = params->paired != 0;
    if (paired && (reads->n_reads & 1)) fail(KSLAM_ERR_ARG, "paired data needs an even number of reads ([R1 block | R2 block])");
    const uint64_t n = paired ? reads->n_reads / 2 : reads->n_reads;
    if (n_consumed_pairs > n) fail(KSLAM_ERR_ARG, "more consumed records than the batch has");
    if (n_consumed_pairs && (!reads->ids_off || (reads->ids_off[reads->n_reads] && !reads->ids))) fail(KSLAM_ERR_ARG, "the batch has no read identifiers");
    if (n_consumed_pairs && seq && (!reads->bases_off || (reads->bases_off[reads->n_reads] && !reads->bases) || (reads->quality && !reads->quality_off)))
      fail(KSLAM_ERR_ARG, "SEQ and QUAL need the batch's bases");
    std::vector<uint8_t> has_row(n + 1, 0);
    for (uint64_t g = 0; g < n_read_pairs; g++) {
      const kslam_read_pair &rp = read_pairs[g];
      if (rp.r1_read >= n || (paired && rp.r2_read != rp.r1_read + n)) fail(KSLAM_ERR_ARG, "read pair refers to a record outside the batch");
      if (rp.count) has_row[rp.r1_read] = 1;   // (n_rows = min(count, max(--num-alignments, 1)): no row only without alignment pairs)
    }
    if (bam)   // the lowest read whose id a record cannot hold: read numbers ascend through the R1 block, then the R2 block
      for (int mate = 0; mate < (paired ? 2 : 1); mate++)
        for (uint64_t p = 0; p < n_consumed_pairs; p++) {
          const uint64_t r = p + (mate ? n : 0), k = reads->ids_off[r + 1] - reads->ids_off[r];
          if (!has_row[p] && k > 254)
            fail(KSLAM_ERR_ARG, "read id \"" + std::string(reads->ids + reads->ids_off[r], k) + "\" is longer than 254 bytes: a BAM record cannot hold it");
        }
    std::string text;
    for (uint64_t p = 0; p < n_consumed_pairs; p++) {
      if (has_row[p]) continue;
      for (int mate = 0; mate < (paired ? 2 : 1); mate++) {
        const Cols c = cols_of(reads, p + (mate ? n : 0), seq != 0);
        const uint32_t flag = paired ? (mate ? 141u : 77u) : 4u;
        if (!bam) {
          put_line(text, c, flag);
          continue;
        }
        put_record(text, c, flag);
      }
    }
    char *h = (char *)malloc(text.size() + 1);
    if (!h) fail(KSLAM_ERR_OOM, "out of host memory");
    memcpy(h, text.data(), text.size());
    *out = h;
    *len = text.size();
  });
}
