// pileup_walk.hpp -- what the host twins of the reports that walk the contributing records share (host/variants.cpp,
// consensus.cpp, depth.cpp, alignqc.cpp): the alphabet, the whole-CIGAR fit check, the oriented query and the loop over the
// records a live alignment pair names.  The rules are csrc/pileup_walk.h's, restated serially.  Plain C++17, header only, no GPU:
// it needs batch_check.hpp and include/kslam.h and nothing else of the library.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "batch_check.hpp"

namespace kslam_pileup {

// A 0, C 1, G 2, T 3 (upper case), anything else 4
inline int acgt(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }
inline uint8_t complement(uint8_t c) {
  switch (c) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    default: return c;   // N, lower case, anything else: as it is
  }
}

// does the record's CIGAR stay inside its read and its entry?  (the whole CIGAR, before anything is emitted)
inline bool fits(const kslam_overlap &o, const uint32_t *pool, int64_t read_len, int64_t ref_len) {
  int64_t rp = o.ref_begin, qp = o.query_begin > 0 ? o.query_begin : 0;
  for (uint32_t k = 0; k < o.cigar_len; k++) {
    const uint32_t c = pool[o.cigar_off + k], op = c & 15u;
    const int64_t len = c >> 4;
    if (op == 0) {
      if (rp + len > ref_len || qp + len > read_len) return false;
      rp += len;
      qp += len;
    } else if (op == 1) {
      if (qp + len > read_len) return false;
      qp += len;
    } else if (op == 2) {
      if (rp + len > ref_len) return false;
      rp += len;
    }
  }
  return true;
}

// the read as the alignment saw it: as it is, or reversed with upper-case ACGT complemented
inline void oriented_query(std::string &query, const uint8_t *read, int64_t L, bool revcomp) {
  query.assign((const char *)read, (size_t)L);
  if (revcomp)
    for (int64_t j = 0; j < L; j++) query[(size_t)j] = (char)complement(read[L - 1 - j]);
}

// the bases query[qp .. qp + len) of an I run at 2 bits each, the first one highest (len <= 32); false: one of them is not
// upper-case ACGT (csrc/pileup_walk.h: insertion_bases)
inline bool insertion_bases(const std::string &query, int64_t qp, int64_t len, uint64_t *bases) {
  uint64_t w = 0;
  bool ok = true;
  for (int64_t j = 0; j < len; j++) {
    const int code = acgt((uint8_t)query[(size_t)(qp + j)]);
    ok = ok && code < 4;
    w = (w << 2) | (uint64_t)(code & 3);
  }
  *bases = w;
  return ok;
}

// Every overlap record a live alignment pair names, once, ascending: fn(o, L, ref_len, holds) with the read's and the entry's
// length.  holds == false: the record is skipped -- its entry is not of the index, its CIGAR is empty, ref_begin < 0, or the CIGAR
// leaves the read or the entry (L and ref_len are 0 for the first three).  Returns kslam_batch::check's fault (Level::records),
// "" when the arrays hold together; nothing is visited otherwise.
template <class Fn>
std::string for_each_named_record(const kslam_batch::Arrays &batch, const uint32_t *pool, const uint64_t *entry_offsets, uint64_t n_entries, Fn &&fn) {
  std::vector<uint8_t> named(batch.n_overlaps < (1ull << 32) ? batch.n_overlaps : 0, 0);   // (2^32 or more: refused before anything is named)
  const std::string fault = kslam_batch::check(batch, kslam_batch::Level::records, nullptr, [&](uint32_t idx) { named[idx] = 1; });
  if (!fault.empty()) return fault;
  for (uint64_t i = 0; i < batch.n_overlaps; i++) {
    if (!named[i]) continue;
    const kslam_overlap &o = batch.overlaps[i];
    if (o.entry >= n_entries || o.cigar_len == 0 || o.ref_begin < 0) {
      fn(o, (int64_t)0, (int64_t)0, false);
      continue;
    }
    const int64_t ref_len = (int64_t)(entry_offsets[o.entry + 1] - entry_offsets[o.entry]);
    const int64_t L = (int64_t)(batch.read_offsets[o.read + 1] - batch.read_offsets[o.read]);
    fn(o, L, ref_len, fits(o, pool, L, ref_len));
  }
  return fault;
}

// the same with the counting every report but the alignment QC does (which counts per stream): fn(o, L, ref_len) for the
// records that hold
template <class Fn>
std::string for_each_contributing_record(const kslam_batch::Arrays &batch, const uint32_t *pool, const uint64_t *entry_offsets, uint64_t n_entries,
                                         uint64_t &n_records, uint64_t &n_skipped, Fn &&fn) {
  return for_each_named_record(batch, pool, entry_offsets, n_entries, [&](const kslam_overlap &o, int64_t L, int64_t ref_len, bool holds) {
    n_records++;
    if (holds) fn(o, L, ref_len);
    else n_skipped++;
  });
}

}  // namespace kslam_pileup
