// inflate.h -- interface of inflate.hip (BGZF members inflated on the device, include/kslam_inflate.h)
#pragma once
#include "common.h"

namespace kslam {

constexpr uint32_t INFLATE_WAVES = 4;             // waves (= members) per workgroup
constexpr uint32_t INFLATE_ROUND = 4096;          // members per launch round unless KSLAM_INFLATE_ROUND says otherwise
constexpr uint32_t INFLATE_MAX_ISIZE = 65536;     // what BGZF allows a member to inflate to

// what stopped a member (0 = it inflated to its ISIZE and CRC-32); the names are inflate_error_name's
enum InflateError : uint32_t {
  INF_OK = 0,
  INF_BAD_BLOCK_TYPE = 1,
  INF_STORED_LENGTH = 2,
  INF_OVERSUBSCRIBED = 3,
  INF_INCOMPLETE = 4,
  INF_INVALID_SYMBOL = 5,
  INF_DISTANCE = 6,
  INF_OUTPUT_OVERRUN = 7,
  INF_OUTPUT_UNDERRUN = 8,
  INF_CRC = 9,
  INF_DATA_LENGTH = 10,
};
const char *inflate_error_name(uint32_t kind);

struct InflateMember {   // one member of a round, filled by the host from the member's header and trailer
  uint32_t in_off;       // its deflate data inside the round's compressed bytes ...
  uint32_t in_len;       // ... and their length (BSIZE + 1 - 26)
  uint32_t out_off;      // its place inside the round's text: the exclusive sum of the ISIZE fields
  uint32_t isize, crc;   // the trailer
  uint32_t pad;
};

struct InflateWork {   // scratch, grown once and kept by the context
  DevBuf in, out, members, first_bad;
};

// The n members described by d_members: d_in (4-byte aligned, 4 readable bytes behind the last member) -> d_out.
// *d_first_bad (u64, set to ~0 by the caller) takes the minimum of (member number << 8 | InflateError) over the members that failed.
void inflate_members_device(const uint8_t *d_in, const InflateMember *d_members, uint32_t n, uint8_t *d_out, uint64_t *d_first_bad,
                            hipStream_t s);

}  // namespace kslam
