// crc32.hip.h -- CRC-32 arithmetic in GF(2) shared by checksum.hip (chunks of a segment) and
// deflate_join.hip (segments of a buffer): crc(A||B) = x^(8|B|) * crc(A) + crc(B) mod P,
// zlib's crc32_combine.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bitar_hip {
namespace cks {

constexpr uint32_t kPoly = 0xEDB88320u;  // reflected CRC-32 (zlib)
constexpr uint32_t kBase = 65521u;       // Adler-32 modulus

// a * b mod P in the reflected representation (zlib multmodp)
__device__ __forceinline__ uint32_t multmodp(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = b & 1u ? (b >> 1) ^ kPoly : b >> 1;
  }
  return p;
}
// x^(8 n) mod P
__device__ __forceinline__ uint32_t x8nmodp(uint32_t n) {
  uint32_t p = 1u << 31;    // x^0
  uint32_t sq = 1u << 23;   // x^8
  while (n) {
    if (n & 1u) p = multmodp(sq, p);
    sq = multmodp(sq, sq);
    n >>= 1;
  }
  return p;
}

}  // namespace cks
}  // namespace bitar_hip
