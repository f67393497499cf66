// rans.hip.h -- what the rANS codecs' files (rans.hip, ransplane.hip) share: the coder's
// constants, unaligned little-endian accesses, and the private histograms' counting step.
#pragma once

#include "autopack.hip.h"

namespace bitar_hip {

namespace rans {

constexpr uint32_t kScaleBits = 12, kScale = 1u << kScaleBits;
constexpr uint32_t kX0 = 1u << 16;       // every state's start, and the bound of a refill
constexpr uint32_t kCopies = 16;         // private histograms: lane t adds into copy t % 16
constexpr uint32_t kRow = 128 + 4;       // dwords of one copy, two bins of 16 bits a dword (a copy
                                         // counts at most 4112 bytes); the copies of a bin lie
                                         // 4 banks apart
constexpr uint32_t kBatch = 8;           // dwords a lane loads before it counts their bytes
constexpr uint32_t kGroup = 8;           // steps whose symbols the encoder loads together
constexpr uint32_t kRing = 512;          // words either kernel holds in LDS (the decoder: read
                                         // ahead; the encoder: not yet stored)

__device__ __forceinline__ uint32_t table_size(uint32_t nsym) { return 2u * ((12u * nsym + 15u) >> 4); }

// (streams arrive at any address on the pointer-list path)
__device__ __forceinline__ uint32_t ld16(const GMEM uint8_t* p) { return p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t ld32(const GMEM uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
__device__ __forceinline__ void st16(GMEM uint8_t* p, uint32_t v) {
  const uint16_t h = (uint16_t)v;
  __builtin_memcpy(p, &h, 2);
}
__device__ __forceinline__ void st32(GMEM uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return readlane(wave_incl_sum(v), 63); }
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// one more byte of value b in a private histogram
__device__ __forceinline__ void count(uint32_t* hist, uint32_t b) {
  atomicAdd(&hist[b >> 1], 1u << (16u * (b & 1u)));
}

}  // namespace rans

}  // namespace bitar_hip
