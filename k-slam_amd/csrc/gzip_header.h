// gzip_header.h -- the walk over one RFC 1952 member header, for the host (host/gunzip.cpp: the first member, and
// kslam_gunzip_header) and for the device (gunzip.hip: a wave that decodes across a member's end walks the next member's
// header itself).  Plain C++ with no library calls, so that both compile it.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define KSLAM_GZ_HD __host__ __device__
#else
#define KSLAM_GZ_HD
#endif

namespace kslam {

enum GzipHeaderError : uint32_t { GZH_OK = 0, GZH_NOT_MEMBER = 1, GZH_HEADER = 2 };

// The member header at d[at .. end): *deflate_at = the first byte of its deflate data.  GZH_NOT_MEMBER: fewer than two bytes,
// or not the magic 1f 8b.  GZH_HEADER: the header ends before it is complete (a name or comment without its NUL included), the
// method is not 8 (deflate), or a reserved FLG bit (5, 6, 7) is set.  The FHCRC field is skipped, not checked (as zlib and
// Python's gzip do).
KSLAM_GZ_HD inline uint32_t gzip_header_walk(const uint8_t *d, uint64_t at, uint64_t end, uint64_t *deflate_at) {
  if (end < at || end - at < 2 || d[at] != 0x1f || d[at + 1] != 0x8b) return GZH_NOT_MEMBER;
  if (end - at < 10 || d[at + 2] != 8) return GZH_HEADER;
  const uint32_t flg = d[at + 3];
  if (flg & 0xe0u) return GZH_HEADER;
  uint64_t p = at + 10;
  if (flg & 4u) {   // FEXTRA: XLEN and that many bytes
    if (end - p < 2) return GZH_HEADER;
    const uint64_t xlen = (uint64_t)d[p] | ((uint64_t)d[p + 1] << 8);
    p += 2;
    if (end - p < xlen) return GZH_HEADER;
    p += xlen;
  }
  for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) {   // FNAME, FCOMMENT: zero-terminated
    if (!(flg & bit)) continue;
    while (p < end && d[p] != 0) p++;
    if (p == end) return GZH_HEADER;
    p++;
  }
  if (flg & 2u) {   // FHCRC
    if (end - p < 2) return GZH_HEADER;
    p += 2;
  }
  *deflate_at = p;
  return GZH_OK;
}

}  // namespace kslam
