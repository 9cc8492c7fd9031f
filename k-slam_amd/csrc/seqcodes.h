// seqcodes.h -- the two byte tables of the SEQ / QUAL columns (include/kslam_samseq.h), one definition for the device
// writer (samtext.hip) and its host twin (host/tail.cpp): the IUPAC complement and BAM's 4-bit base code.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define KSLAM_SEQ_HD __host__ __device__
#else
#define KSLAM_SEQ_HD
#endif

namespace kslam_seq {

// A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D; W, S, N and every other byte unchanged; the case is kept
KSLAM_SEQ_HD inline uint8_t complement(uint8_t c) {
  const uint8_t lower = c & 0x20u;
  uint8_t r;
  switch (c & 0xDFu) {
    case 'A': r = 'T'; break;
    case 'T': r = 'A'; break;
    case 'C': r = 'G'; break;
    case 'G': r = 'C'; break;
    case 'M': r = 'K'; break;
    case 'K': r = 'M'; break;
    case 'R': r = 'Y'; break;
    case 'Y': r = 'R'; break;
    case 'V': r = 'B'; break;
    case 'B': r = 'V'; break;
    case 'H': r = 'D'; break;
    case 'D': r = 'H'; break;
    default: return c;
  }
  return (uint8_t)(r | lower);   // (c & 0xDF is a letter only when c is that letter in either case)
}

// the index of c in "=ACMGRSVTWYHKDBN", either case; every other byte 15 (htslib's seq_nt16_table without its digits)
KSLAM_SEQ_HD inline uint8_t nibble(uint8_t c) {
  if (c == '=') return 0;
  switch (c & 0xDFu) {
    case 'A': return 1;
    case 'C': return 2;
    case 'M': return 3;
    case 'G': return 4;
    case 'R': return 5;
    case 'S': return 6;
    case 'V': return 7;
    case 'T': return 8;
    case 'W': return 9;
    case 'Y': return 10;
    case 'H': return 11;
    case 'K': return 12;
    case 'D': return 13;
    case 'B': return 14;
    default: return 15;
  }
}

}  // namespace kslam_seq
