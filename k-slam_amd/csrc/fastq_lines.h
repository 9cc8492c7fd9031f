// fastq_lines.h -- the reader's line rule on the device, for the kernels that walk an indexed FASTQ stream (fastq_index.hip,
// readsplit.hip): a line ends at "\n", "\r\n" or a lone "\r"; at the true end of the stream the unterminated rest (if any)
// and then one more, empty, line are read (src/sequenceTools.h:45-73; host/fastq.cpp: index_stream).
#pragma once
#include "common.h"

namespace kslam {

__device__ inline uint64_t line_after(const uint8_t *t, uint64_t len, uint64_t p) {
  return (t[p] == '\r' && p + 1 < len && t[p + 1] == '\n') ? p + 2 : p + 1;
}

// line `l` of the stream: [start, end) and where the next line starts (host/fastq.cpp: index_stream)
__device__ inline void line_span(const FqStream &s, uint64_t l, uint64_t *start, uint64_t *end, uint64_t *next) {
  if (l < s.terminated) {
    *start = l == 0 ? 0 : line_after(s.text, s.len, s.ev[l - 1]);
    *end = s.ev[l];
    *next = line_after(s.text, s.len, s.ev[l]);
  } else if (l == s.terminated && s.rest_start < s.len) {
    *start = s.rest_start; *end = s.len; *next = s.len;     // the unterminated rest
  } else {
    *start = s.len; *end = s.len; *next = s.len;            // the empty line read at end of stream
  }
}

}  // namespace kslam
