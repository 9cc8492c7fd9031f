// wave_add.h -- counter adds combined inside the wavefront, for the tables whose rows are four 64-bit counters per key
// (coverage.hip: per entry; genes.hip: per gene).  Real samples are skewed -- a few keys take most records -- so the lanes of a
// wavefront that share a key go to memory as ONE 64-bit atomic add per field.
#pragma once
#include "common.h"

namespace kslam {

__device__ inline uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// rows[key][f_one] += the number of lanes with `one`, rows[key][f_sum] += their `sum`s, for the lanes with `has`: lanes that
// share a key go to memory as one add each.  Called by every lane of the wavefront (has = false for those with nothing).
__device__ inline void wave_add(bool has, uint32_t key, bool one, uint64_t sum, unsigned long long *rows, int f_one, int f_sum) {
  uint64_t pending = __ballot(has);
  const int lane = threadIdx.x & 63;
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    const uint32_t k0 = __shfl(key, leader);
    const bool same = has && key == k0;
    const uint64_t m = __ballot(same);
    const uint64_t ones = __popcll(__ballot(same && one));
    const uint64_t total = (m & (m - 1)) ? wave_sum(same ? sum : 0ull) : sum;   // (one lane: its own sum)
    if (lane == leader) {
      if (ones) atomicAdd(rows + 4ull * k0 + f_one, (unsigned long long)ones);
      if (total) atomicAdd(rows + 4ull * k0 + f_sum, (unsigned long long)total);
    }
    pending &= ~m;
  }
}

}  // namespace kslam
