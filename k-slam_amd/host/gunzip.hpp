// gunzip.hpp -- the host's side of include/kslam_gunzip.h (host/gunzip.cpp): the RFC 1952 header walk, and the walk along
// the chain of block starts that the device's count pass (csrc/gunzip.hip) leaves behind.  Plain C++, no device code, so that
// tools/gunzip_check.cpp runs it alone.
#ifndef KSLAM_HOST_GUNZIP_HPP_
#define KSLAM_HOST_GUNZIP_HPP_
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/kslam.h"

namespace kslam_host {

// What stopped a wave of the count pass.  Kinds below 32 are csrc/inflate.h's InflateError.
enum GunzipKind : uint32_t {
  GZK_DISTANCE = 6,         // INF_DISTANCE
  GZK_DATA_LENGTH = 10,     // INF_DATA_LENGTH
  GZK_HEADER = 32,          // "gzip header"
  GZK_NOT_MEMBER = 33,      // "not a gzip member"
  GZK_SPAN = 34,            // one wave would have to cover more than 2^32 bits: KSLAM_ERR_UNSUPPORTED
};
enum GunzipLinkStatus : uint32_t {
  GZL_NONE = 0,             // the wave never ran, or did not finish
  GZL_HIT = 1,              // a block of its ended exactly on start `next`
  GZL_EOF = 2,              // its last member ended, and behind it came nothing but zero bytes
  GZL_ABANDONED = 3,        // it used up its budget of bits without meeting a start
  GZL_ERROR = 4,            // `kind` says why it stopped
};

// One per start, written by the wave that decoded from it (lengths only).
struct GunzipLink {
  uint32_t status, kind;
  uint32_t next;            // GZL_HIT: the number of the start it ended on (> its own)
  uint32_t need_back;       // the furthest a match of the member it STARTED in reached before the wave's first output byte
  uint64_t out_bytes;       // text bytes from its start to its end
  uint64_t members;         // members that ended on the way
  uint64_t member_at;       // members > 0: byte offset of the header of the last member that began on the way ...
  uint64_t member_out;      // ... and the wave's output bytes before that member's first
};
static_assert(sizeof(GunzipLink) == 48, "the device writes these");

// One live start: a stretch of the text that one wave decodes.
struct GunzipSpan {
  uint32_t start;           // its number among the starts
  uint64_t out, n_out;      // its text: offset and length
  uint64_t member0;         // the member it starts in ...
  uint64_t n_members;       // ... and how many members end inside it
};

struct GunzipChain {
  enum State { COMPLETE, BROKEN, FAILED } state = COMPLETE;
  uint32_t broken_at = 0;               // BROKEN: the live start whose wave has to run again, without a budget
  uint64_t bad_member = 0, bad_at = 0;  // FAILED: the member, the byte offset of its header, the kind
  uint32_t bad_kind = 0;
  std::vector<GunzipSpan> spans;        // COMPLETE: the live starts in order
  uint64_t members = 0, text_len = 0;
};

// Follows links[first] -> links[links[first].next] -> ... to the end of the file.  A link on the chain that is missing,
// abandoned or points nowhere breaks it (BROKEN: everything before it stands, the caller decodes on from there); an error on
// the chain is the file's (FAILED); links off the chain -- false starts -- are never looked at.
GunzipChain gunzip_chain_walk(const GunzipLink *links, uint32_t n, uint32_t first);

// "gzip member 3 (byte offset 1234): CRC mismatch"
std::string gunzip_error_text(uint64_t member, uint64_t at, const char *kind);
// the names of GZK_HEADER / GZK_NOT_MEMBER / GZK_SPAN; nullptr for a kind that is csrc/inflate.h's
const char *gunzip_kind_name(uint32_t kind);

}  // namespace kslam_host
#endif  // KSLAM_HOST_GUNZIP_HPP_
