// filter.hip -- byte shuffle and bit shuffle of fixed-width column buffers, per segment, both
// directions (gfx950).  No reference counterpart: the filter sits in front of the codecs so
// that their 2560-byte windows see one byte position (or one bit position) of every element
// side by side.
//
// Layout of a segment S of L bytes, element width w:
//   SHUFFLE      m = L / w;  T[j*m + i] = S[i*w + j];  the last L - m*w bytes stay in place.
//   BITSHUFFLE   m8 = m & ~7;  plane p = 8j + b occupies T[p*m8/8, (p+1)*m8/8);  bit t of its
//                byte q is bit b of S[(8q + t)*w + j];  the last L - m8*w bytes stay in place.
// Either way the filtered side is `R` rows of `RL` bytes (w streams of m bytes, or 8w planes
// of m8/8 bytes) and the plain side is a run of whole elements.
//
// One 256-thread workgroup per segment, tiles of 8 KiB (apply) or 16 KiB (invert) through two
// LDS buffers:
//   plain side  <-> bufA   16 B per lane when the segment's base is 16-B aligned, 4 B when it
//                          is 4-B aligned, bytes otherwise (lanes contiguous in every case)
//   bufA        <-> bufB   each lane turns 4 elements (4w bytes) into 4 bytes of each of the w
//                          streams with v_perm_b32 (a 4x4 byte transpose per dword column)
//   bufB        <-> bufA   BITSHUFFLE only: each lane turns 32 bytes of one stream into one dword
//                          of each of its 8 planes (8x8 bit transposes in the lane + a 4x4 byte
//                          transpose)
//   rows        <-> HBM    blocks of BS bytes (16 for streams, 4 for planes) at BS-aligned
//                          ADDRESSES of each row, lanes contiguous along a row.  A row starts at
//                          j*m, so its blocks are not aligned with the tile: the LDS side is
//                          read (apply) or addressed (invert) at a byte offset and realigned
//                          with v_alignbyte_b32.  Only the head of a row before its first
//                          aligned address and the tail after its last whole block move bytewise.
// A block belongs to the tile that holds its first byte, so the apply loads BS row positions
// more than a tile (re-read from L2), and the invert loads the blocks at a tile's edges twice.
// Workgroups never wait for one another.
#include "kernels.hip.h"
#include "wave.hip.h"

// Tile bytes, measured: the apply is 11-28 % faster with 8 KiB tiles (18 KB of
// LDS, 8 workgroups per CU instead of 4), the invert 1-5 % slower (its edge blocks load twice)
#ifndef BITAR_FILTER_TILE_APPLY
#define BITAR_FILTER_TILE_APPLY 8192
#endif
#ifndef BITAR_FILTER_TILE_INVERT
#define BITAR_FILTER_TILE_INVERT 16384
#endif
// 1: the apply takes its bit planes from wave ballots instead of in-lane bit transposes (a
// measurement variant, scripts/build_variant.sh; DESIGN.md 4.14 has the numbers)
#ifndef BITAR_FILTER_BALLOT
#define BITAR_FILTER_BALLOT 0
#endif

namespace bitar_hip {

namespace flt {

constexpr uint32_t kThreads = 256;
// an LDS image holds a tile and at most: 32 elements of overlap + a group's slack (apply), 8
// bytes more per plane row (invert); + 16 for the realigning reads' last dword
constexpr uint32_t kImageSlack = 1024 + 16;

// o[k] = {d0.byte k, d1.byte k, d2.byte k, d3.byte k}: a 4x4 byte transpose (its own inverse)
__device__ __forceinline__ void transpose4x4(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3,
                                             uint32_t* o) {
  const uint32_t t0 = __builtin_amdgcn_perm(d1, d0, 0x05010400u);
  const uint32_t t1 = __builtin_amdgcn_perm(d1, d0, 0x07030602u);
  const uint32_t u0 = __builtin_amdgcn_perm(d3, d2, 0x05010400u);
  const uint32_t u1 = __builtin_amdgcn_perm(d3, d2, 0x07030602u);
  o[0] = __builtin_amdgcn_perm(u0, t0, 0x05040100u);
  o[1] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);
  o[2] = __builtin_amdgcn_perm(u1, t1, 0x05040100u);
  o[3] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);
}

// 8x8 bit-matrix transpose of the little-endian (lo, hi): bit t of output byte b = bit b of
// input byte t (its own inverse)
__device__ __forceinline__ void transpose8x8(uint32_t& lo, uint32_t& hi) {
  uint64_t x = ((uint64_t)hi << 32) | lo, t;
  t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;
  x = x ^ t ^ (t << 7);
  t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull;
  x = x ^ t ^ (t << 14);
  t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull;
  x = x ^ t ^ (t << 28);
  lo = (uint32_t)x;
  hi = (uint32_t)(x >> 32);
}

// the dword at byte offset a of an LDS image (a of any alignment; reads one dword past it)
__device__ __forceinline__ uint32_t lds_dword_at(const uint8_t* lds, uint32_t a) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(lds + (a & ~3u));
  return funnel(q[0], q[1], a);
}

// nbytes from HBM (g, the tile's plain bytes) into the LDS image, or back
template <bool TO_LDS, typename V>
__device__ __forceinline__ void linear_vec(uint8_t* lds, GMEM uint8_t* g, uint32_t nbytes,
                                           uint32_t tid) {
  const uint32_t nv = nbytes / (uint32_t)sizeof(V);
  V* l = reinterpret_cast<V*>(lds);
  GMEM V* p = reinterpret_cast<GMEM V*>(g);
  if (TO_LDS) {
    for (uint32_t v = tid; v < nv; v += 4 * kThreads) {  // 4 loads in flight per lane
      V x[4];
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k)
        if (v + k * kThreads < nv) x[k] = p[v + k * kThreads];
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k)
        if (v + k * kThreads < nv) l[v + k * kThreads] = x[k];
    }
  } else {
    for (uint32_t v = tid; v < nv; v += kThreads) p[v] = l[v];
  }
  for (uint32_t k = nv * (uint32_t)sizeof(V) + tid; k < nbytes; k += kThreads) {
    if (TO_LDS) lds[k] = g[k];
    else g[k] = lds[k];
  }
}

template <bool TO_LDS>
__device__ __forceinline__ void linear(uint8_t* lds, GMEM uint8_t* g, uint32_t nbytes,
                                       uint32_t tid) {
  const uint32_t a = (uint32_t)(uintptr_t)g;  // wave-uniform
  if ((a & 15u) == 0) linear_vec<TO_LDS, uint4>(lds, g, nbytes, tid);
  else if ((a & 3u) == 0) linear_vec<TO_LDS, uint32_t>(lds, g, nbytes, tid);
  else linear_vec<TO_LDS, uint8_t>(lds, g, nbytes, tid);
}

// Apply: rows of an LDS image (row r at r*RS, position k0 of every row at offset 0) to HBM
// (row r at tp + r*RL).  The tile owns the BS-byte blocks that start at row positions
// [k0, k0 + K) at BS-aligned addresses; the image holds K + BS positions.
template <uint32_t BS, uint32_t R, uint32_t K, uint32_t RS>
__device__ __forceinline__ void store_rows(GMEM uint8_t* tp, const uint8_t* lds, uint32_t RL,
                                           uint32_t k0, uint32_t tid) {
  constexpr uint32_t SPR = K / BS;  // blocks per row, a power of two
  for (uint32_t s = tid; s < R * SPR; s += kThreads) {
    const uint32_t r = s / SPR, t = s % SPR;
    GMEM uint8_t* row = tp + r * RL;
    const uint32_t d = (0u - (uint32_t)(uintptr_t)(row + k0)) & (BS - 1);
    const uint32_t pos = k0 + d + BS * t;  // < k0 + K
    const uint32_t a = r * RS + d + BS * t;
    if (pos + BS <= RL) {
      if (BS == 16) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(lds + (a & ~3u));
        const uint32_t x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3], x4 = q[4];
        *reinterpret_cast<GMEM uint4*>(row + pos) =
            make_uint4(funnel(x0, x1, a), funnel(x1, x2, a), funnel(x2, x3, a), funnel(x3, x4, a));
      } else {
        *reinterpret_cast<GMEM uint32_t*>(row + pos) = lds_dword_at(lds, a);
      }
    } else if (pos < RL) {  // the row's tail
      for (uint32_t k = 0; pos + k < RL; ++k) row[pos + k] = lds[a + k];
    }
    if (k0 == 0 && t == 0) {  // the row's head
      const uint32_t h = d < RL ? d : RL;
      for (uint32_t k = 0; k < h; ++k) row[k] = lds[r * RS + k];
    }
  }
}

// Invert: the blocks of every row that hold positions [k0, k0 + kc) from HBM into an LDS image
// in which row r sits at r*RS and position k0 - delta(r) at offset 0, delta(r) = the address of
// (row r, position k0) mod BS: aligned blocks land on aligned LDS offsets.
template <uint32_t BS, uint32_t R, uint32_t K, uint32_t RS>
__device__ __forceinline__ void load_rows(const GMEM uint8_t* tp, uint8_t* lds, uint32_t RL,
                                          uint32_t k0, uint32_t kc, uint32_t tid) {
  constexpr uint32_t SPR = K / BS;  // a power of two; slot SPR of a row is the shifted rest
  auto slot = [&](uint32_t r, uint32_t t) {
    const GMEM uint8_t* row = tp + r * RL;
    const uint32_t delta = (uint32_t)(uintptr_t)(row + k0) & (BS - 1);
    const int32_t pos = (int32_t)(k0 + BS * t) - (int32_t)delta;
    if (pos >= (int32_t)(k0 + kc)) return;
    uint8_t* l = lds + r * RS + BS * t;
    if (pos >= 0 && (uint32_t)pos + BS <= RL) {
      if (BS == 16) *reinterpret_cast<uint4*>(l) = *reinterpret_cast<const GMEM uint4*>(row + pos);
      else *reinterpret_cast<uint32_t*>(l) = *reinterpret_cast<const GMEM uint32_t*>(row + pos);
    } else {  // the row's head or tail
      for (uint32_t k = 0; k < BS; ++k) {
        const int32_t p = pos + (int32_t)k;
        if (p >= 0 && (uint32_t)p < RL) l[k] = row[p];
      }
    }
  };
  for (uint32_t s = tid; s < R * SPR; s += kThreads) slot(s / SPR, s % SPR);
  for (uint32_t r = tid; r < R; r += kThreads) slot(r, SPR);
}

}  // namespace flt

// Segment i: lens ? lens[i] : min(seg, n - i*seg) bytes at in + i*seg -> out + i*seg.  A length
// above min(seg, n - i*seg) (BITAR_HIP_SEGMENT_ERROR is one) moves nothing.
template <uint32_t W, bool BITS, bool INV>
__global__ __launch_bounds__(256) void filter_kernel(const uint8_t* __restrict__ in, uint64_t n,
                                                     uint32_t seg,
                                                     const uint32_t* __restrict__ lens,
                                                     uint32_t nseg, uint8_t* __restrict__ out) {
  using namespace flt;
  constexpr uint32_t kTile = INV ? BITAR_FILTER_TILE_INVERT : BITAR_FILTER_TILE_APPLY;
  constexpr uint32_t kBuf = kTile + kImageSlack;
  constexpr uint32_t E = kTile / W;  // elements per tile
  constexpr uint32_t XS = E + 32;    // stride of a stream's row in bufB
  constexpr uint32_t KP = E / 8;     // plane bytes per tile
  static_assert(E % 32 == 0 && KP % 4 == 0, "tile too small for this width");
  static_assert(W * XS + 16 <= kBuf && 8 * W * (KP + 8) + 16 <= kBuf, "LDS image too small");
  __shared__ __attribute__((aligned(16))) uint8_t bufA[kBuf];
  __shared__ __attribute__((aligned(16))) uint8_t bufB[kBuf];

  const uint32_t tid = threadIdx.x;
  const uint32_t si = blockIdx.x;
  if (si >= nseg) return;
  const uint64_t off = (uint64_t)si * seg;
  if (off >= n) return;
  const uint32_t room = (uint32_t)(n - off < seg ? n - off : seg);
  const uint32_t len = lens ? lens[si] : room;
  if (len > room) return;
  const uint32_t m = len / W;
  const uint32_t M = BITS ? m & ~7u : m;  // elements that are transposed
  const uint32_t RL = BITS ? M / 8 : M;   // bytes of a row (stream or plane)

  // sp: the plain side, tp: the filtered side
  GMEM uint8_t* sp = global_ptr(const_cast<uint8_t*>(INV ? out + off : in + off));
  GMEM uint8_t* tp = global_ptr(const_cast<uint8_t*>(INV ? in + off : out + off));

  // 4 elements of a lane <-> 4 bytes of each of the W streams
  auto to_streams = [](const uint32_t* d, uint32_t* o) {
    if constexpr (W == 2) {
      o[0] = __builtin_amdgcn_perm(d[1], d[0], 0x06040200u);
      o[1] = __builtin_amdgcn_perm(d[1], d[0], 0x07050301u);
    } else {
      constexpr uint32_t C = W / 4;  // dwords per element
#pragma unroll
      for (uint32_t c = 0; c < C; ++c)
        transpose4x4(d[c], d[C + c], d[2 * C + c], d[3 * C + c], o + 4 * c);
    }
  };
  auto to_elements = [](const uint32_t* o, uint32_t* d) {
    if constexpr (W == 2) {
      d[0] = __builtin_amdgcn_perm(o[1], o[0], 0x05010400u);
      d[1] = __builtin_amdgcn_perm(o[1], o[0], 0x07030602u);
    } else {
      constexpr uint32_t C = W / 4;
#pragma unroll
      for (uint32_t c = 0; c < C; ++c) {
        uint32_t t[4];
        transpose4x4(o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3], t);
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) d[e * C + c] = t[e];
      }
    }
  };

  if (!INV) {
    constexpr uint32_t OV = BITS ? 32 : 16;  // elements a tile loads past its own
    constexpr uint32_t PS = XS / 8;          // stride of a plane's row in bufA
    for (uint32_t i0 = 0; i0 < M; i0 += E) {
      const uint32_t cnt = M - i0 < E + OV ? M - i0 : E + OV;
      linear<true>(bufA, sp + i0 * W, cnt * W, tid);
      __syncthreads();
      for (uint32_t g = tid; g < (cnt + 3) / 4; g += kThreads) {
        uint32_t d[W], o[W];
        const uint32_t* src = reinterpret_cast<const uint32_t*>(bufA + g * 4 * W);
#pragma unroll
        for (uint32_t k = 0; k < W; ++k) d[k] = src[k];
        to_streams(d, o);
#pragma unroll
        for (uint32_t j = 0; j < W; ++j) *reinterpret_cast<uint32_t*>(bufB + j * XS + 4 * g) = o[j];
      }
      __syncthreads();
      if (BITS) {
#if BITAR_FILTER_BALLOT
        // a wave takes 64 bytes of stream j, one per lane: the ballot of bit b is 8 bytes of
        // plane 8j + b
        const uint32_t nch = (cnt + 63) / 64;
        for (uint32_t c = tid / kWave; c < W * nch; c += kThreads / kWave) {
          const uint32_t j = c / nch, u = c % nch;
          const uint32_t x = bufB[j * XS + 64 * u + (tid & 63u)];
#pragma unroll
          for (uint32_t bit = 0; bit < 8; ++bit) {
            const uint64_t mask = ballot((x >> bit) & 1u);
            uint32_t* dst = reinterpret_cast<uint32_t*>(bufA + (8 * j + bit) * PS + 8 * u);
            if ((tid & 63u) == 0) {
              dst[0] = (uint32_t)mask;
              if (8 * u + 4 < PS) dst[1] = (uint32_t)(mask >> 32);
            }
          }
        }
#else
        // 32 bytes of stream j -> one dword of each of its 8 planes (bufA is free again)
        for (uint32_t s = tid; s < W * (XS / 32); s += kThreads) {
          const uint32_t j = s / (XS / 32), u = s % (XS / 32);
          if (32 * u >= cnt) continue;
          const uint4* src = reinterpret_cast<const uint4*>(bufB + j * XS + 32 * u);
          uint4 a = src[0], b = src[1];
          transpose8x8(a.x, a.y);
          transpose8x8(a.z, a.w);
          transpose8x8(b.x, b.y);
          transpose8x8(b.z, b.w);
          uint32_t o[8];
          transpose4x4(a.x, a.z, b.x, b.z, o);
          transpose4x4(a.y, a.w, b.y, b.w, o + 4);
#pragma unroll
          for (uint32_t bit = 0; bit < 8; ++bit)
            *reinterpret_cast<uint32_t*>(bufA + (8 * j + bit) * PS + 4 * u) = o[bit];
        }
#endif
        __syncthreads();
        store_rows<4, 8 * W, KP, PS>(tp, bufA, RL, i0 / 8, tid);
      } else {
        store_rows<16, W, E, XS>(tp, bufB, RL, i0, tid);
      }
      __syncthreads();
    }
  } else {
    constexpr uint32_t PS = KP + 8;  // stride of a plane's row in bufA
    for (uint32_t i0 = 0; i0 < M; i0 += E) {
      const uint32_t cnt = M - i0 < E ? M - i0 : E;
      if (BITS) {
        load_rows<4, 8 * W, KP, PS>(tp, bufA, RL, i0 / 8, cnt / 8, tid);
        __syncthreads();
        for (uint32_t s = tid; s < W * (E / 32); s += kThreads) {
          const uint32_t j = s / (E / 32), u = s % (E / 32);
          if (32 * u >= cnt) continue;
          uint32_t o[8], lo[4], hi[4];
#pragma unroll
          for (uint32_t bit = 0; bit < 8; ++bit) {
            const uint32_t r = 8 * j + bit;
            const uint32_t delta = (uint32_t)(uintptr_t)(tp + r * RL + i0 / 8) & 3u;
            o[bit] = lds_dword_at(bufA, r * PS + delta + 4 * u);
          }
          transpose4x4(o[0], o[1], o[2], o[3], lo);
          transpose4x4(o[4], o[5], o[6], o[7], hi);
#pragma unroll
          for (uint32_t v = 0; v < 4; ++v) transpose8x8(lo[v], hi[v]);
          uint4* dst = reinterpret_cast<uint4*>(bufB + j * XS + 32 * u);
          dst[0] = make_uint4(lo[0], hi[0], lo[1], hi[1]);
          dst[1] = make_uint4(lo[2], hi[2], lo[3], hi[3]);
        }
      } else {
        load_rows<16, W, E, XS>(tp, bufB, RL, i0, cnt, tid);
      }
      __syncthreads();
      for (uint32_t g = tid; g < (cnt + 3) / 4; g += kThreads) {
        uint32_t d[W], o[W];
#pragma unroll
        for (uint32_t j = 0; j < W; ++j) {
          const uint32_t delta = BITS ? 0u : (uint32_t)(uintptr_t)(tp + j * RL + i0) & 15u;
          o[j] = lds_dword_at(bufB, j * XS + delta + 4 * g);
        }
        to_elements(o, d);
        uint32_t* dst = reinterpret_cast<uint32_t*>(bufA + g * 4 * W);
#pragma unroll
        for (uint32_t k = 0; k < W; ++k) dst[k] = d[k];
      }
      __syncthreads();
      linear<false>(bufA, sp + i0 * W, cnt * W, tid);
      __syncthreads();
    }
  }
  // what is left of the segment stays where it is
  for (uint32_t k = M * W + tid; k < len; k += kThreads) {
    if (INV) sp[k] = tp[k];
    else tp[k] = sp[k];
  }
}

#define BITAR_FILTER_INSTANCE(W, BITS, INV)                                              \
  template __global__ void filter_kernel<W, BITS, INV>(const uint8_t*, uint64_t, uint32_t, \
                                                       const uint32_t*, uint32_t, uint8_t*);
#define BITAR_FILTER_WIDTH(W)          \
  BITAR_FILTER_INSTANCE(W, false, false) \
  BITAR_FILTER_INSTANCE(W, false, true)  \
  BITAR_FILTER_INSTANCE(W, true, false)  \
  BITAR_FILTER_INSTANCE(W, true, true)
BITAR_FILTER_WIDTH(2)
BITAR_FILTER_WIDTH(4)
BITAR_FILTER_WIDTH(8)
BITAR_FILTER_WIDTH(16)

}  // namespace bitar_hip
