// bgzf.h -- interface of bgzf.hip (BGZF compression of a device byte string, include/kslam_bgzf.h)
#pragma once
#include "common.h"
#include "../../include/kslam_bgzf.h"

namespace kslam {

constexpr uint32_t BGZF_MEMBER_IN = 65280;      // input bytes per member (htslib's BGZF_BLOCK_SIZE)
constexpr uint32_t BGZF_SLOT = 65536;           // the largest member BSIZE can describe
constexpr uint32_t BGZF_ROUND = 1024;           // members per launch round (sizes the scratch below)

struct BgzfWork {   // scratch, grown once and kept by the context
  DevBuf cand;      // u16 per input position of a round: distance to the match candidate, 0 = none
  DevBuf slots;     // BGZF_SLOT bytes per member of a round (+ padding): the members before they are packed
  DevBuf sizes, offs, scan_tmp, totals;   // u32 member sizes, their u64 exclusive scan; totals[0] = round, [1] = output so far
};

// d_in[0 .. n) -> out[0 .. *out_len): BGZF members of BGZF_MEMBER_IN input bytes each, no EOF marker; n == 0 gives 0 bytes.
// deflate: KSLAM_BGZF_DEFLATE_FIXED or _DYNAMIC.  The bytes depend on the input and the mode alone.  Waits for the stream (the
// length is read back).
void bgzf_compress_device(const char *d_in, uint64_t n, int deflate, BgzfWork &W, DevBuf &out, uint64_t *out_len, hipStream_t s);

// kslam_debug_bgzf_code_lengths: the code builder of the dynamic mode alone.  counts[0 .. n), 2 <= n <= 286, limit <= 15 with
// 2^limit >= n, the counts' sum below 2^32 -> lengths[0 .. n), all on the device.
void bgzf_code_lengths_device(const uint32_t *d_counts, uint32_t n, uint32_t limit, uint8_t *d_lengths, hipStream_t s);

}  // namespace kslam
