// bamsort.hpp -- what the host twin (bamsort.cpp) and the host side of the device take (csrc/api_bamsort.hip) share of
// include/kslam_bamsort.h: the walk over a block_size chain, the header's sort order, virtual offsets, and the assembly of the BAI
// bytes from chunk runs, windows and per-reference counters.  Plain C++, header only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace kslam_bamsort {

constexpr uint64_t MEMBER_IN = 65280;          // input bytes per BGZF member
constexpr uint32_t PSEUDO_BIN = 37450;
constexpr uint32_t NO_BIN = 0xFFFFFFFFu;       // a record that enters no bin
constexpr uint64_t MAX_REF_LEN = 1ull << 29;   // what BAI addresses

inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// htslib's hts_reg2bin(beg, end, 14, 5)
inline uint32_t reg2bin(uint64_t beg, uint64_t end) {
  end--;
  if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
  return 0;
}

struct Rec {            // one record of a chain, as the sort and the index see it
  uint64_t off = 0;     // of its block_size field
  uint32_t len = 0;     // block_size + 4
  int32_t ref = -1, pos = -1;
  uint32_t span = 1;    // max(1, reflen)
  bool unmapped = false;
};

// The record at data[off ..) of a chain that ends at len.  Empty string: *r is filled; otherwise what is wrong with it.
inline std::string parse_record(const uint8_t *data, uint64_t len, uint64_t off, Rec *r) {
  const std::string at = " (record at byte " + std::to_string(off) + ")";
  if (len - off < 4) return "the block_size chain does not end at the end of the records" + at;
  const uint64_t bs = le32(data + off);
  if (bs < 32) return "a record shorter than its fixed part" + at;
  if (bs > len - off - 4) return "the block_size chain does not end at the end of the records" + at;
  const uint8_t *p = data + off + 4;
  const uint32_t l_name = p[8], n_cig = le16(p + 12), flag = le16(p + 14);
  if (32ull + l_name + 4ull * n_cig > bs) return "a record shorter than its fixed part, read name and CIGAR" + at;
  r->off = off;
  r->len = (uint32_t)(bs + 4);
  r->ref = (int32_t)le32(p);
  r->pos = (int32_t)le32(p + 4);
  r->unmapped = (flag & 4u) != 0;
  uint64_t reflen = 0;
  if (!r->unmapped)
    for (uint32_t k = 0; k < n_cig; k++) {
      const uint32_t c = le32(p + 32 + l_name + 4 * k), op = c & 15u;
      if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += c >> 4;
    }
  r->span = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(reflen, 1), MAX_REF_LEN);
  return std::string();
}

// the sort key: refID as unsigned above pos + 1 as unsigned
inline uint64_t sort_key(const Rec &r) { return (uint64_t)(uint32_t)r.ref << 32 | (uint32_t)(r.pos + 1); }

// The SAM header text with SO:coordinate (include/kslam_bamsort.h, THE FILE)
inline std::string coordinate_header(const char *text, uint64_t len) {
  const std::string h(text ? text : "", text ? (size_t)len : 0);
  if (h.compare(0, 3, "@HD") != 0 || (h.size() > 3 && h[3] != '\t' && h[3] != '\n')) return "@HD\tVN:1.0\tSO:coordinate\n" + h;
  size_t eol = h.find('\n');
  if (eol == std::string::npos) eol = h.size();
  std::string line = h.substr(0, eol);
  const size_t so = line.find("\tSO:");
  if (so == std::string::npos) line += "\tSO:coordinate";
  else {
    size_t end = line.find('\t', so + 1);
    if (end == std::string::npos) end = line.size();
    line = line.substr(0, so) + "\tSO:coordinate" + line.substr(end);
  }
  return line + h.substr(eol);
}

// "BAM\1", l_text, the text, n_ref and the reference list from the text's @SQ lines.  Empty *err: fine.
inline std::string bam_header_of(const std::string &text, std::vector<uint64_t> *ref_len, std::string *err) {
  std::string out("BAM\1", 4), refs;
  auto i32 = [](std::string &o, uint64_t v) {
    for (int k = 0; k < 4; k++) o.push_back((char)(v >> (8 * k)));
  };
  err->clear();
  if (text.size() > INT32_MAX) *err = "the header text is too long for BAM";
  uint64_t n_ref = 0;
  for (size_t a = 0; a < text.size();) {
    size_t b = text.find('\n', a);
    if (b == std::string::npos) b = text.size();
    if (b - a >= 4 && text.compare(a, 4, "@SQ\t") == 0) {
      std::string sn, ln;
      for (size_t f = a + 4; f < b;) {
        size_t g = text.find('\t', f);
        if (g == std::string::npos || g > b) g = b;
        if (g - f >= 3 && text.compare(f, 3, "SN:") == 0) sn = text.substr(f + 3, g - f - 3);
        if (g - f >= 3 && text.compare(f, 3, "LN:") == 0) ln = text.substr(f + 3, g - f - 3);
        f = g + 1;
      }
      if (sn.empty() || ln.empty() || ln.size() > 10 || ln.find_first_not_of("0123456789") != std::string::npos)
        *err = "an @SQ line of the header without SN or LN";
      const uint64_t l = ln.empty() || !err->empty() ? 0 : std::stoull(ln);
      i32(refs, sn.size() + 1);
      refs += sn;
      refs.push_back('\0');
      i32(refs, l);
      if (ref_len) ref_len->push_back(l);
      n_ref++;
    }
    a = b + 1;
  }
  if (n_ref > INT32_MAX) *err = "the reference list is too long for BAM";
  i32(out, text.size());
  out += text;
  i32(out, n_ref);
  return out + refs;
}

// Virtual offsets of stream positions: member_off[m] = the compressed bytes of the record members before m (n_members + 1 of them)
struct Voff {
  const uint64_t *member_off;
  uint64_t n_members, header_clen, total;
  uint64_t at(uint64_t o) const {
    if (o >= total) return (header_clen + member_off[n_members]) << 16;   // the EOF member
    const uint64_t m = o / MEMBER_IN;
    return (header_clen + member_off[m]) << 16 | (o % MEMBER_IN);
  }
};

struct Run {            // file-consecutive records of one (ref, bin): a chunk.  end is filled by assemble_bai
  uint32_t ref, bin;
  uint64_t beg, end;
};
struct RefCount {       // per reference; first = ~0 when it has no record
  uint64_t first = ~0ull, last = 0, n_mapped = 0, n_unmapped = 0, max_end = 0;
};

// The BAI bytes.  runs: every run head in any order, the records that enter no bin as runs of NO_BIN (they end the run in
// front of them), beg = the start virtual offset of the run's first record; eof = the end virtual offset of the last record.
// win: per reference win_off[r + 1] - win_off[r] windows (at least n_intv of them) holding the smallest start, ~0 = none.
inline std::string assemble_bai(uint32_t n_ref, std::vector<Run> &runs, const std::vector<RefCount> &refs, const std::vector<uint64_t> &win,
                                const std::vector<uint64_t> &win_off, uint64_t eof, uint64_t n_no_coor, uint64_t *n_chunks) {
  std::sort(runs.begin(), runs.end(), [](const Run &a, const Run &b) { return a.beg < b.beg; });   // file order
  for (size_t k = 0; k < runs.size(); k++) runs[k].end = k + 1 < runs.size() ? runs[k + 1].beg : eof;
  runs.erase(std::remove_if(runs.begin(), runs.end(), [](const Run &r) { return r.bin == NO_BIN; }), runs.end());
  std::sort(runs.begin(), runs.end(), [](const Run &a, const Run &b) {
    return a.ref != b.ref ? a.ref < b.ref : a.bin != b.bin ? a.bin < b.bin : a.beg < b.beg;
  });
  std::string o("BAI\1", 4);
  auto put = [&](uint64_t v, int bytes) {
    for (int k = 0; k < bytes; k++) o.push_back((char)(v >> (8 * k)));
  };
  put(n_ref, 4);
  size_t k = 0;
  *n_chunks = runs.size();
  for (uint32_t r = 0; r < n_ref; r++) {
    const RefCount &rc = refs[r];
    if (rc.first == ~0ull) {
      put(0, 4);
      put(0, 4);
      continue;
    }
    size_t k1 = k;
    uint32_t n_bin = 1;
    while (k1 < runs.size() && runs[k1].ref == r) {
      if (k1 == k || runs[k1].bin != runs[k1 - 1].bin) n_bin++;
      k1++;
    }
    put(n_bin, 4);
    while (k < k1) {
      size_t e = k;
      while (e < k1 && runs[e].bin == runs[k].bin) e++;
      put(runs[k].bin, 4);
      put(e - k, 4);
      for (; k < e; k++) {
        put(runs[k].beg, 8);
        put(runs[k].end, 8);
      }
    }
    put(PSEUDO_BIN, 4);
    put(2, 4);
    put(rc.first, 8);
    put(rc.last, 8);
    put(rc.n_mapped, 8);
    put(rc.n_unmapped, 8);
    const uint64_t n_intv = rc.max_end ? 1 + ((rc.max_end - 1) >> 14) : 0;
    put(n_intv, 4);
    std::vector<uint64_t> w(win.begin() + win_off[r], win.begin() + win_off[r] + n_intv);
    for (uint64_t i = n_intv; i-- > 0;)
      if (w[i] == ~0ull && i + 1 < n_intv) w[i] = w[i + 1];
    for (uint64_t v : w) put(v, 8);
  }
  put(n_no_coor, 8);
  return o;
}

}  // namespace kslam_bamsort
