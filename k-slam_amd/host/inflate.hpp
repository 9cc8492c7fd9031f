// inflate.hpp -- the host's walk over the members of a BGZF file (host/inflate.cpp), shared with the C ABI entry that
// inflates them on the device (csrc/api_tail.hip: kslam_bgzf_inflate).  Plain C++, no device code.
#ifndef KSLAM_HOST_INFLATE_HPP_
#define KSLAM_HOST_INFLATE_HPP_
#include <cstdint>
#include <vector>

#include "../../include/kslam.h"

namespace kslam_host {

struct BgzfMember {
  uint64_t at;       // byte offset of the member (its 1f 8b)
  uint32_t size;     // BSIZE + 1: header (18) + deflate data + trailer (8)
  uint32_t isize;    // inflated length, from the trailer
  uint32_t crc;      // CRC-32 of the inflated bytes, from the trailer
};
constexpr uint32_t BGZF_HEADER = 18, BGZF_TRAILER = 8, BGZF_MAX_ISIZE = 65536;

// The members of data[0 .. len) by htslib's rule; throws HostError (workers.hpp) as include/kslam_inflate.h says.
// members may be null (count only).
void bgzf_walk(const uint8_t *data, uint64_t len, std::vector<BgzfMember> *members, uint64_t *n_members, uint64_t *text_len);

}  // namespace kslam_host
#endif  // KSLAM_HOST_INFLATE_HPP_
