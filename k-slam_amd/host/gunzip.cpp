// gunzip.cpp -- include/kslam_gunzip.h on the host: the RFC 1952 header walk (csrc/gzip_header.h, shared with the device)
// behind kslam_gunzip_header, and the walk along the chain of block starts.  Nothing is inflated here: that is
// csrc/gunzip.hip.  The count pass leaves one GunzipLink per start; only the links on the chain from the file's first block
// are trusted, because only those come from waves that started at a true block start.
#include "gunzip.hpp"

#include "../../include/kslam_gunzip.h"
#include "../csrc/gzip_header.h"
#include "workers.hpp"

namespace kslam_host {

std::string gunzip_error_text(uint64_t member, uint64_t at, const char *kind) {
  return "gzip member " + std::to_string(member) + " (byte offset " + std::to_string(at) + "): " + kind;
}

const char *gunzip_kind_name(uint32_t kind) {
  switch (kind) {
    case GZK_HEADER: return "gzip header";
    case GZK_NOT_MEMBER: return "not a gzip member";
    case GZK_SPAN: return "more than 2^32 bits of deflate data without a block start that a wave could be started on";
    default: return nullptr;
  }
}

GunzipChain gunzip_chain_walk(const GunzipLink *links, uint32_t n, uint32_t first) {
  GunzipChain c;
  uint64_t out = 0, member = 0;
  uint64_t member_at = 0, member_out = 0;   // of the member the next span starts in: its header, its first text byte
  uint32_t i = first;
  for (;;) {
    if (i >= n) {   // (a table that does not hold the first start)
      c.state = GunzipChain::BROKEN;
      c.broken_at = i;
      return c;
    }
    const GunzipLink &l = links[i];
    const bool hit = l.status == GZL_HIT;
    if ((l.status != GZL_HIT && l.status != GZL_EOF && l.status != GZL_ERROR) || (hit && (l.next <= i || l.next >= n))) {
      c.state = GunzipChain::BROKEN;
      c.broken_at = i;
      return c;
    }
    if (l.need_back > out - member_out) {   // a match of this member reached before the member's first byte
      c.state = GunzipChain::FAILED;
      c.bad_member = member;
      c.bad_at = member_at;
      c.bad_kind = GZK_DISTANCE;
      return c;
    }
    if (l.status == GZL_ERROR) {
      c.state = GunzipChain::FAILED;
      c.bad_member = member + l.members;
      c.bad_at = l.members ? l.member_at : member_at;
      c.bad_kind = l.kind;
      return c;
    }
    c.spans.push_back(GunzipSpan{i, out, l.out_bytes, member, l.members});
    if (l.members) {
      member += l.members;
      member_at = l.member_at;
      member_out = out + l.member_out;
    }
    out += l.out_bytes;
    if (!hit) break;
    i = l.next;
  }
  c.members = member;
  c.text_len = out;
  return c;
}

}  // namespace kslam_host

using namespace kslam_host;

extern "C" {

kslam_status kslam_gunzip_header(const void *data, uint64_t len, uint64_t *deflate_at) {
  if (deflate_at) *deflate_at = 0;
  return guarded([&] {
    if (!deflate_at || (len && !data)) fail(KSLAM_ERR_ARG, "null argument");
    const uint32_t e = kslam::gzip_header_walk(static_cast<const uint8_t *>(data), 0, len, deflate_at);
    if (e) fail(KSLAM_ERR_ARG, gunzip_error_text(0, 0, gunzip_kind_name(e == kslam::GZH_HEADER ? GZK_HEADER : GZK_NOT_MEMBER)));
  });
}

}  // extern "C"
