// autopack.hip.h -- what AUTOPACK's decode path shares with the four codecs' files: which segment
// a workgroup of a LISTED decoder takes (autopack.hip).
#pragma once

#include "wave.hip.h"

namespace bitar_hip {

constexpr uint32_t kNoSegment = 0xFFFFFFFFu;

// Workgroup b of the listed decoder of the format whose tag has the high nibble `nibble`:
//   lists form (list != null): segment list[b] while b < *count -- the route kernel put the
//     format's segments there -- and none past that;
//   tag-peek form (list == null): segment b when its stream is not empty and byte 0 has the
//     nibble, none otherwise.
// Wave-uniform.  Nothing of a stream but byte 0 is read here, and that only of a stream of at
// least one byte.
__device__ __forceinline__ uint32_t listed_segment(
    uint32_t nibble, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
    const uint8_t* const* __restrict__ srcs, const uint8_t* __restrict__ slab, uint64_t slot_stride,
    const uint32_t* __restrict__ csizes, uint32_t nseg) {
  const uint32_t b = blockIdx.x;
  if (list) return b < *count ? list[b] : kNoSegment;
  if (b >= nseg || csizes[b] == 0) return kNoSegment;
  const GMEM uint8_t* src = global_ptr(srcs ? srcs[b] : slab + (uint64_t)b * slot_stride);
  return (uint32_t)(src[0] >> 4) == nibble ? b : kNoSegment;
}

}  // namespace bitar_hip
