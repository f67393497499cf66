// autopack.hip.h -- what the column codecs' files (intpack.hip, fltpack.hip, dictpack.hip,
// runpack.hip, cascade.hip, patchpack.hip, decpack.hip) share: the kernels around a format's
// compress_segment and decode_stream, the frame every stream starts with, and which segment a
// workgroup of one of AUTOPACK's LISTED decoders takes (autopack.hip).
// (What the bit-packing formats share below that, INTPACK's and DECPACK's whole segment encoder
// and decoder included, is in bitpack.hip.h.)
//
// A format is a traits type F, defined in the format's own file:
//   F::kNibble                          the high nibble of byte 0 of its streams
//   F::EncShared<W>, F::DecShared       the LDS of its encoder (element width W) and decoder
//   F::compress_segment<W, STORE>(src, L, dst, size_out, sh)
//   F::decode_stream(src, csize, tag, byte1, L, seg, dst, sh) -> bool
// runtime.hip includes this header with BITAR_COLUMN_DECLARATIONS_ONLY: it sees the two kernel
// templates' declarations below (the other kernels' are in kernels.hip.h) and the traits types'
// names, which stay incomplete there, and its column table (kColumn, compress_kernel<>,
// decompress_kernel<>) names the instantiations the formats' files define.
#pragma once

#include "../../include/bitar_hip.h"
#include "wave.hip.h"

namespace bitar_hip {

struct IntPack;
struct FltPack;
struct DictPack;
struct RunPack;
struct Cascade;
struct PatchPack;
struct Rans;       // (rans.hip)
struct RansPlane;  // (ransplane.hip; a decoder per element width)
template <uint32_t W> struct RansPlaneDecoder;
struct SymTab;     // (symtab.hip)
struct DecPack;    // (decpack.hip; ids from 256 on, include/bitar_hip_codecs.h)

// Segment i: min(seg, n_total - i*seg) bytes at input + i*seg -> its slot (slab + i*slot_stride,
// or dsts[i]); sizes[i] = the stream's size (at most 4 + the segment's length: never a failure).
// STORE = false is the form of a later candidate of AUTOPACK: a segment that would be stored gets
// its size only.
template <class F, uint32_t W, bool STORE>
__global__ void column_compress_kernel(const uint8_t*, uint64_t, uint32_t, uint8_t*, uint64_t,
                                       uint8_t* const*, uint32_t*);

// Segment i: csizes[i] bytes at srcs[i] (or slab + i*slot_stride) -> out + i*seg; produced[i] =
// its length, or BITAR_HIP_SEGMENT_ERROR (and bit 0 of the error word) for a stream the format
// rejects.  The element width comes from the stream's tag.
// LISTED = false: workgroup i takes segment i (list and count are not looked at).
// LISTED = true, AUTOPACK's decoder of the format: a grid of nseg workgroups of which the listed
// ones -- or, without a list, those whose stream carries the format's nibble -- do exactly the
// same for their segment; the others leave at once and write nothing.
template <class F, bool LISTED>
__global__ void column_decompress_kernel(const uint8_t* const*, const uint8_t*, uint64_t,
                                         const uint32_t*, uint32_t, uint32_t, uint8_t*, uint32_t*,
                                         uint32_t*, const uint32_t*, const uint32_t*);

#ifndef BITAR_COLUMN_DECLARATIONS_ONLY

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

template <class F, uint32_t W, bool STORE>
__global__ __launch_bounds__(64) void column_compress_kernel(
    const uint8_t* __restrict__ input, uint64_t n_total, uint32_t seg, uint8_t* __restrict__ slab,
    uint64_t slot_stride, uint8_t* const* __restrict__ dsts, uint32_t* __restrict__ sizes) {
  __shared__ typename F::template EncShared<W> sh;
  const uint32_t i = blockIdx.x;
  const uint64_t seg_off = (uint64_t)i * seg;
  if (seg_off >= n_total) return;
  const uint32_t L = (uint32_t)(n_total - seg_off < seg ? n_total - seg_off : seg);
  GMEM uint8_t* dst = global_ptr(dsts ? dsts[i] : slab + (uint64_t)i * slot_stride);
  F::template compress_segment<W, STORE>(global_ptr(input + seg_off), L, dst, sizes + i, sh);
}

// The stored form of every format: 4 header bytes, then the segment's L bytes and nothing else.
__device__ __forceinline__ bool decode_stored(const GMEM uint8_t* src, uint32_t csize, uint32_t L,
                                              GMEM uint8_t* dst) {
  if (csize != 4u + L) return false;
  wave_copy_global(dst, src + 4, L);
  return true;
}

// What every format's stream starts with: byte 0 the tag, byte 1 the format's own, bytes 2..3
// LE16(L - 1).  F::decode_stream sees a stream of at least 4 bytes; it checks the tag, byte 1 and
// L <= seg, and either takes the stored form (decode_stored) or decodes at the tag's width.
// Nothing outside the stream's csizes[i] bytes is used (an aligned dword is loaded only when one
// of its bytes is), and nothing outside the segment's seg bytes is written.
template <class F, bool LISTED>
__global__ __launch_bounds__(64) void column_decompress_kernel(
    const uint8_t* const* __restrict__ srcs, const uint8_t* __restrict__ slab, uint64_t slot_stride,
    const uint32_t* __restrict__ csizes, uint32_t nseg, uint32_t seg, uint8_t* __restrict__ out,
    uint32_t* __restrict__ produced, uint32_t* __restrict__ err, const uint32_t* __restrict__ list,
    const uint32_t* __restrict__ count) {
  __shared__ typename F::DecShared sh;
  uint32_t i = blockIdx.x;
  if constexpr (LISTED) {
    i = listed_segment(F::kNibble, list, count, srcs, slab, slot_stride, csizes, nseg);
    if (i == kNoSegment) return;
  } else {
    if (i >= nseg) return;
  }
  const GMEM uint8_t* src = global_ptr(srcs ? srcs[i] : slab + (uint64_t)i * slot_stride);
  GMEM uint8_t* dst = global_ptr(out + (uint64_t)i * seg);
  const uint32_t csize = csizes[i];
  bool ok = csize >= 4;
  uint32_t L = 0;
  if (ok) {
    const uint32_t tag = src[0], byte1 = src[1];
    L = 1u + src[2] + ((uint32_t)src[3] << 8);
    ok = F::decode_stream(src, csize, tag, byte1, L, seg, dst, sh);
  }
  if (lane_id() == 0) {
    if (ok) {
      produced[i] = L;
    } else {
      produced[i] = BITAR_HIP_SEGMENT_ERROR;
      atomicOr(err, 1u);
    }
  }
}

// The explicit instantiations of a format's file: one line per width and form.
#define BITAR_COLUMN_COMPRESS(F, W, STORE)                                                     \
  template __global__ void column_compress_kernel<F, W, STORE>(                                \
      const uint8_t*, uint64_t, uint32_t, uint8_t*, uint64_t, uint8_t* const*, uint32_t*)
#define BITAR_COLUMN_DECOMPRESS(F, LISTED)                                                     \
  template __global__ void column_decompress_kernel<F, LISTED>(                                \
      const uint8_t* const*, const uint8_t*, uint64_t, const uint32_t*, uint32_t, uint32_t,    \
      uint8_t*, uint32_t*, uint32_t*, const uint32_t*, const uint32_t*)

#endif  // BITAR_COLUMN_DECLARATIONS_ONLY

}  // namespace bitar_hip
