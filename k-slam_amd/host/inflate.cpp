// inflate.cpp -- include/kslam_inflate.h on the host: finding the members of a BGZF file.  Nothing is inflated here (that
// is csrc/inflate.hip, one wavefront per member); the walk only reads each member's 18-byte header and 8-byte trailer.
#include "inflate.hpp"

#include <string>

#include "../../include/kslam_inflate.h"
#include "workers.hpp"

namespace kslam_host {

namespace {
uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
uint32_t le32(const uint8_t *p) { return le16(p) | (le16(p + 2) << 16); }
std::string where(uint64_t member, uint64_t at) { return "BGZF member " + std::to_string(member) + " (byte offset " + std::to_string(at) + ")"; }
}  // namespace

void bgzf_walk(const uint8_t *data, uint64_t len, std::vector<BgzfMember> *members, uint64_t *n_members, uint64_t *text_len) {
  uint64_t at = 0, n = 0, text = 0;
  while (at < len) {
    const uint8_t *h = data + at;
    const uint64_t left = len - at;
    if (left < 2 || h[0] != 0x1f || h[1] != 0x8b) fail(KSLAM_ERR_ARG, where(n, at) + ": no gzip magic (1f 8b)" + (n ? ": data after the last member" : ""));
    if (left < BGZF_HEADER) fail(KSLAM_ERR_ARG, where(n, at) + ": truncated inside the header (" + std::to_string(left) + " of 18 bytes)");
    // htslib's check (bgzf.c: check_header): deflate, FEXTRA alone, one 6-byte extra field 'B' 'C' of 2 bytes
    if (h[2] != 8) fail(KSLAM_ERR_UNSUPPORTED, where(n, at) + ": compression method " + std::to_string(h[2]) + " is not deflate");
    if (h[3] != 4 || le16(h + 10) != 6 || h[12] != 'B' || h[13] != 'C' || le16(h + 14) != 2)
      fail(KSLAM_ERR_UNSUPPORTED, where(n, at) + ": the file is plain gzip, not BGZF (no 'BC' extra field): its members cannot be inflated in parallel; "
                                                  "re-block it with bgzip (zcat FILE | bgzip > FILE.bgz.gz)");
    const uint32_t size = le16(h + 16) + 1;
    if (size < BGZF_HEADER + BGZF_TRAILER) fail(KSLAM_ERR_ARG, where(n, at) + ": BSIZE " + std::to_string(size - 1) + " is too small for a member");
    if (size > left)
      fail(KSLAM_ERR_ARG, where(n, at) + ": BSIZE " + std::to_string(size - 1) + " runs past the end of the data (" + std::to_string(left) +
                              " bytes left): the file is truncated");
    BgzfMember m{at, size, le32(h + size - 4), le32(h + size - 8)};
    if (m.isize > BGZF_MAX_ISIZE) fail(KSLAM_ERR_ARG, where(n, at) + ": ISIZE " + std::to_string(m.isize) + " is above BGZF's 65536");
    if (members) members->push_back(m);
    text += m.isize;
    at += size;
    n++;
  }
  if (n_members) *n_members = n;
  if (text_len) *text_len = text;
}

}  // namespace kslam_host

using namespace kslam_host;

extern "C" {

int kslam_bgzf_is_gzip(const void *data, uint64_t len) {
  const uint8_t *p = static_cast<const uint8_t *>(data);
  return p && len >= 2 && p[0] == 0x1f && p[1] == 0x8b;
}

kslam_status kslam_bgzf_scan(const void *data, uint64_t len, uint64_t *n_members, uint64_t *text_len) {
  if (n_members) *n_members = 0;
  if (text_len) *text_len = 0;
  return guarded([&] {
    if (len && !data) fail(KSLAM_ERR_ARG, "null argument");
    bgzf_walk(static_cast<const uint8_t *>(data), len, nullptr, n_members, text_len);
  });
}

}  // extern "C"
