// autopack.hip -- AUTOPACK: per segment the smallest of the applicable column codecs' streams
// (RUNPACK, INTPACK, DICTPACK, FLTPACK), and on the way back each segment to the decoder its tag
// names (gfx950).  No reference counterpart.  DESIGN.md 4.21.
//
// AUTOPACK has no format of its own.  Compress runs the candidates' own kernels: candidate 0
// (RUNPACK) into the caller's slots, the others into a scratch slab each (in their store-less
// form, *_compress_candidate_kernel: a stored form there is never selected, it ties with
// RUNPACK's at best, so only its size is written); autopack_select_kernel
// then takes per segment the smallest size, the lowest index among equals, and copies a winner
// that is not candidate 0 over the slot.  Decompress sorts the segments by the high nibble of
// byte 0 (autopack_route_kernel) and runs each format's decoder over its own segments
// (*_decompress_listed_kernel in the four codecs' files).
#include "kernels.hip.h"
#include "../../include/bitar_hip.h"
#include "wave.hip.h"

namespace bitar_hip {

// One wavefront per segment, kSelectWaves segments per workgroup (the kernel has no LDS and no
// barrier, so the waves of a workgroup do not meet).  Segment i of the chunk: sizes[i] holds
// candidate 0's size and the slot its stream; candidate k >= 1 left its size at
// cand_sizes[(k - 1)*cand_segs + i] and its stream at cand_slab + ((k - 1)*cand_segs + i) *
// cand_stride.  Exactly `size` bytes of the winner are copied (wave_copy_global rounds nothing
// up), so past the larger of the two streams the slot is as it was.
constexpr uint32_t kSelectWaves = 4;

__global__ __launch_bounds__(64 * kSelectWaves) void autopack_select_kernel(
    const uint8_t* __restrict__ cand_slab, uint64_t cand_stride, const uint32_t* __restrict__ cand_sizes,
    uint32_t cand_segs, uint32_t ncand, uint32_t nseg, uint8_t* __restrict__ slab,
    uint64_t slot_stride, uint8_t* const* __restrict__ dsts, uint32_t* __restrict__ sizes) {
  const uint32_t i = uniform(blockIdx.x * kSelectWaves + threadIdx.x / 64u);
  if (i >= nseg) return;
  uint32_t best = sizes[i], win = 0;
  for (uint32_t k = 1; k < ncand; ++k) {
    const uint32_t s = cand_sizes[(uint64_t)(k - 1) * cand_segs + i];
    if (s < best) {  // (a tie stays with the earlier candidate)
      best = s;
      win = k;
    }
  }
  best = uniform(best);
  win = uniform(win);
  if (win == 0) return;
  GMEM uint8_t* dst = global_ptr(dsts ? dsts[i] : slab + (uint64_t)i * slot_stride);
  const GMEM uint8_t* src =
      global_ptr(cand_slab + ((uint64_t)(win - 1) * cand_segs + i) * cand_stride);
  wave_copy_global(dst, src, best);
  if (lane_id() == 0) sizes[i] = best;
}

// One lane per segment.  A segment whose stream is empty or whose byte 0 has a high nibble
// outside 4..7 is rejected here: produced[i] = BITAR_HIP_SEGMENT_ERROR, bit 0 of the error word,
// its output range untouched.  Every other segment belongs to the format f = nibble - 4 and,
// with lists, gets a place in lists[f*nseg ..): a ballot per format, one atomic add of the
// wave's count per format, a lane's place the add's result plus its rank in the ballot.  (The
// order inside a list is that of the waves' adds: the decoders do not depend on it.)  counts[4]
// start at 0.  Without lists (the tag-peek form) only the rejects are handled.
__global__ __launch_bounds__(256) void autopack_route_kernel(
    const uint8_t* const* __restrict__ srcs, const uint8_t* __restrict__ slab, uint64_t slot_stride,
    const uint32_t* __restrict__ csizes, uint32_t nseg, uint32_t* __restrict__ produced,
    uint32_t* __restrict__ err, uint32_t* __restrict__ lists, uint32_t* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t f = 5;  // no segment
  if (i < nseg) {
    f = 4;  // rejected
    if (csizes[i] != 0) {
      const GMEM uint8_t* src = global_ptr(srcs ? srcs[i] : slab + (uint64_t)i * slot_stride);
      const uint32_t nib = src[0] >> 4;
      if (nib >= 4u && nib <= 7u) f = nib - 4u;
    }
  }
  if (f == 4) produced[i] = BITAR_HIP_SEGMENT_ERROR;
  if (ballot(f == 4) != 0 && lane_id() == 0) atomicOr(err, 1u);
  if (!lists) return;
  const uint64_t below = ((uint64_t)1 << lane_id()) - 1u;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint64_t mine = ballot(f == k);
    if (mine == 0) continue;
    uint32_t base = 0;
    if (lane_id() == 0) base = atomicAdd(counts + k, (uint32_t)__popcll(mine));
    base = uniform(base);
    if (f == k) lists[(uint64_t)k * nseg + base + (uint32_t)__popcll(mine & below)] = i;
  }
}

}  // namespace bitar_hip
