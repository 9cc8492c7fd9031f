// crc32.h -- the CRC-32 of gzip (polynomial 0xedb88320, reflected) in pieces, for kernels that compute it in parallel:
// bgzf.hip (the writer) and inflate.hip (the reader) both take a byte range per thread or lane by a byte table, move each
// part to its place by a multiplication with x^(8 * bytes after it) mod P over GF(2), and XOR the parts together
// (crc(A || B) = crc(A) * x^(8 |B|) ^ crc(B), zlib's crc32_combine).
#pragma once
#include "common.h"

namespace kslam {

constexpr uint32_t CRC_POLY = 0xedb88320u;

#ifdef __HIPCC__
namespace {
// x^(2^k) mod P, P the CRC-32 polynomial in reflected form (zlib's x2n_table)
__constant__ uint32_t X2N[32] = {
    0x40000000u, 0x20000000u, 0x08000000u, 0x00800000u, 0x00008000u, 0xedb88320u, 0xb1e6b092u, 0xa06a2517u,
    0xed627daeu, 0x88d14467u, 0xd7bbfe6au, 0xec447f11u, 0x8e7ea170u, 0x6427800eu, 0x4d47bae0u, 0x09fe548fu,
    0x83852d0fu, 0x30362f1au, 0x7b5a9cc3u, 0x31fec169u, 0x9fec022au, 0x6c8dedc4u, 0x15d6874du, 0x5fde7a4eu,
    0xbad90e37u, 0x2e4e5eefu, 0x4eaba214u, 0xa8a472c0u, 0x429a969eu, 0x148d302au, 0xc40ba6d0u, 0xc4e22c3cu};
}  // namespace

__device__ inline uint32_t multmodp(uint32_t a, uint32_t b) {   // a * b mod P
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}

__device__ inline uint32_t x8nmodp(uint32_t n) {   // x^(8 n) mod P
  uint32_t p = 0x80000000u;
  for (uint32_t k = 3; n; n >>= 1, k++)
    if (n & 1u) p = multmodp(X2N[k & 31], p);
  return p;
}

// entry t of the byte table (256 entries): one per thread of a 256-thread workgroup
__device__ inline uint32_t crc_table_entry(uint32_t t) {
  uint32_t c = t;
  for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
  return c;
}
#endif

}  // namespace kslam
