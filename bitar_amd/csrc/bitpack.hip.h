// bitpack.hip.h -- what the bit-packing codecs share (intpack.hip, fltpack.hip; gfx950, wave64):
// wave reductions over DPP, element loads and stores at any alignment, and the payload emitter
// that writes a miniblock's bit string as aligned dwords.
//
// Payload of a miniblock of 64 elements at width b: 8 * b bytes, element t at bits
// [t*b, (t+1)*b) of the little-endian bit string.  Lane t holds element t.
#pragma once

#include "wave.hip.h"

namespace bitar_hip {

namespace ipk {

constexpr uint32_t kMini = 64;     // elements per miniblock
constexpr uint32_t kMaxMini = 1024;  // miniblocks of a 64 KiB segment of bytes
constexpr uint32_t kMaxBlk = 256;

template <uint32_t W> struct Elem { using U = uint32_t; using S = int32_t; };
template <> struct Elem<8> { using U = uint64_t; using S = int64_t; };

// v moved by a DPP control (lanes without a source, or outside the row mask, get `idle`)
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp(uint32_t v, uint32_t idle) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)idle, (int)v, CTRL, ROWS, 0xf, false);
}
template <int CTRL, int ROWS>
__device__ __forceinline__ uint64_t dpp(uint64_t v, uint64_t idle) {
  const uint32_t lo = dpp<CTRL, ROWS>((uint32_t)v, (uint32_t)idle);
  const uint32_t hi = dpp<CTRL, ROWS>((uint32_t)(v >> 32), (uint32_t)(idle >> 32));
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t lane63(uint32_t v) { return readlane(v, 63); }
__device__ __forceinline__ uint64_t lane63(uint64_t v) {
  return ((uint64_t)readlane((uint32_t)(v >> 32), 63) << 32) | readlane((uint32_t)v, 63);
}

// reductions over the wave's 64 lanes (the DPP ladder of wave_incl_sum; lane 63 holds the result)
template <typename U>
__device__ __forceinline__ U wave_or(U x) {
  x |= dpp<0x111, 0xf>(x, (U)0);
  x |= dpp<0x112, 0xf>(x, (U)0);
  x |= dpp<0x114, 0xf>(x, (U)0);
  x |= dpp<0x118, 0xf>(x, (U)0);
  x |= dpp<0x142, 0xa>(x, (U)0);
  x |= dpp<0x143, 0xc>(x, (U)0);
  return lane63(x);
}
template <typename S>
__device__ __forceinline__ S imin(S a, S b) { return a < b ? a : b; }
template <typename S, typename U>
__device__ __forceinline__ S wave_min(S v) {
  constexpr U top = (U)(~(U)0 >> 1);  // the largest signed value: the identity
  S x = v;
  x = imin(x, (S)dpp<0x111, 0xf>((U)x, top));
  x = imin(x, (S)dpp<0x112, 0xf>((U)x, top));
  x = imin(x, (S)dpp<0x114, 0xf>((U)x, top));
  x = imin(x, (S)dpp<0x118, 0xf>((U)x, top));
  x = imin(x, (S)dpp<0x142, 0xa>((U)x, top));
  x = imin(x, (S)dpp<0x143, 0xc>((U)x, top));
  return (S)lane63((U)x);
}
template <typename U>
__device__ __forceinline__ U wave_incl_add(U x) {
  x += dpp<0x111, 0xf>(x, (U)0);
  x += dpp<0x112, 0xf>(x, (U)0);
  x += dpp<0x114, 0xf>(x, (U)0);
  x += dpp<0x118, 0xf>(x, (U)0);
  x += dpp<0x142, 0xa>(x, (U)0);
  x += dpp<0x143, 0xc>(x, (U)0);
  return x;
}

__device__ __forceinline__ uint32_t bit_length(uint32_t v) { return 32u - (uint32_t)__clz((int)v); }
__device__ __forceinline__ uint32_t bit_length(uint64_t v) {
  return 64u - (uint32_t)__clzll((long long)v);
}

// the W-byte little-endian element at p (any alignment): only aligned units that hold one of
// its bytes are loaded
template <uint32_t W>
__device__ __forceinline__ typename Elem<W>::U load_elem(const GMEM uint8_t* p) {
  const uint32_t a = (uint32_t)(uintptr_t)p;
  if constexpr (W == 1) {
    return *p;
  } else if constexpr (W == 2) {
    if ((a & 1u) == 0) return *reinterpret_cast<const GMEM uint16_t*>(p);
    return (uint32_t)p[0] | (uint32_t)p[1] << 8;
  } else {
    const GMEM uint32_t* q = reinterpret_cast<const GMEM uint32_t*>(p - (a & 3u));
    if constexpr (W == 4) {
      const uint32_t lo = q[0];
      if ((a & 3u) == 0) return lo;
      return funnel(lo, q[1], a);
    } else {
      uint32_t lo = q[0], hi = q[1];
      if ((a & 3u) != 0) {
        const uint32_t top = q[2];
        lo = funnel(lo, hi, a);
        hi = funnel(hi, top, a);
      }
      return ((uint64_t)hi << 32) | lo;
    }
  }
}

template <uint32_t W>
__device__ __forceinline__ void store_elem(GMEM uint8_t* p, typename Elem<W>::U v) {
  const uint32_t a = (uint32_t)(uintptr_t)p;
  if constexpr (W == 1) {
    *p = (uint8_t)v;
  } else if constexpr (W == 2) {
    if ((a & 1u) == 0) {
      *reinterpret_cast<GMEM uint16_t*>(p) = (uint16_t)v;
    } else {
      p[0] = (uint8_t)v;
      p[1] = (uint8_t)(v >> 8);
    }
  } else if ((a & 3u) == 0) {
    GMEM uint32_t* q = reinterpret_cast<GMEM uint32_t*>(p);
    q[0] = (uint32_t)v;
    if constexpr (W == 8) q[1] = (uint32_t)(v >> 32);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < W; ++k) p[k] = (uint8_t)(v >> (8 * k));
  }
}

// the W-byte reference of block `blk` in an LDS array of references
template <uint32_t W>
__device__ __forceinline__ typename Elem<W>::U lds_ref(const uint8_t* refs, uint32_t blk) {
  if constexpr (W == 8) return *reinterpret_cast<const uint64_t*>(&refs[blk * 8]);
  else if constexpr (W == 4) return *reinterpret_cast<const uint32_t*>(&refs[blk * 4]);
  else if constexpr (W == 2) return *reinterpret_cast<const uint16_t*>(&refs[blk * 2]);
  else return refs[blk];
}
template <uint32_t W>
__device__ __forceinline__ void set_lds_ref(uint8_t* refs, uint32_t blk, typename Elem<W>::U ref) {
  if constexpr (W == 8) *reinterpret_cast<uint64_t*>(&refs[blk * 8]) = ref;
  else if constexpr (W == 4) *reinterpret_cast<uint32_t*>(&refs[blk * 4]) = ref;
  else if constexpr (W == 2) *reinterpret_cast<uint16_t*>(&refs[blk * 2]) = (uint16_t)ref;
  else refs[blk] = (uint8_t)ref;
}

constexpr uint32_t kStageDwords = 2 * kMini + 4;  // one miniblock's bit string in LDS

// The payload of a stream, one miniblock at a time, as aligned dwords: the bit string is put
// together in LDS shifted by the payload's byte misalignment `a`, and the `a` bytes of every
// miniblock's last dword are the first bytes of the next one's (miniblocks are multiples of 8
// bytes).  Nothing before pay or at or past pay + bytes() is written.
template <uint32_t W>
struct PayloadEmitter {
  using U = typename Elem<W>::U;
  GMEM uint8_t* pay;
  uint32_t* stage;  // kStageDwords of LDS
  uint32_t a, carry = 0, off = 0;
  bool started = false;

  __device__ __forceinline__ PayloadEmitter(GMEM uint8_t* pay_, uint32_t* stage_)
      : pay(pay_), stage(stage_), a((uint32_t)(uintptr_t)pay_ & 3u) {}

  // this lane's residual r of a miniblock of width b > 0
  __device__ __forceinline__ void put(U r, uint32_t b) {
    const uint32_t lane = lane_id();
    const uint32_t nd = 2 * b;  // its dwords; dword nd holds the bytes carried over
    stage[lane] = 0;
    stage[lane + kWave] = 0;
    if (lane < 4) stage[2 * kWave + lane] = 0;
    lds_order();
    if (lane == 0) stage[0] = carry;
    lds_order();
    const uint32_t bit = 8 * a + lane * b;
    const uint32_t d = bit >> 5, s = bit & 31u;
    const uint64_t lo64 = (uint64_t)(uint32_t)r << s;
    uint32_t w0 = (uint32_t)lo64, w1 = (uint32_t)(lo64 >> 32), w2 = 0;
    if constexpr (W == 8) {
      const uint64_t hi64 = (uint64_t)(uint32_t)(r >> 32) << s;
      w1 |= (uint32_t)hi64;
      w2 = (uint32_t)(hi64 >> 32);
    }
    if (w0) atomicOr(&stage[d], w0);
    if (w1) atomicOr(&stage[d + 1], w1);
    if (w2) atomicOr(&stage[d + 2], w2);
    lds_order();
    GMEM uint32_t* q = reinterpret_cast<GMEM uint32_t*>(pay + off - a);
    for (uint32_t j = lane; j < nd; j += kWave) {
      const uint32_t v = stage[j];
      if (j == 0 && a && !started) {  // the payload's first dword: its low bytes are the header's
        for (uint32_t t = a; t < 4; ++t) pay[t - a] = (uint8_t)(v >> (8 * t));
      } else {
        q[j] = v;
      }
    }
    carry = stage[nd];
    lds_order();
    started = true;
    off += 8 * b;
  }

  // the bytes still carried; returns the payload's size
  __device__ __forceinline__ uint32_t finish() {
    const uint32_t lane = lane_id();
    if (started && lane < a) pay[off - a + lane] = (uint8_t)(carry >> (8 * lane));
    return off;
  }
};

// lane t's field of the miniblock of width b > 0 whose payload starts at mb (any alignment);
// only the dwords that hold one of the field's bits are loaded (all inside the miniblock's bytes)
template <uint32_t W>
__device__ __forceinline__ typename Elem<W>::U extract_field(const GMEM uint8_t* mb, uint32_t b) {
  using U = typename Elem<W>::U;
  const uint32_t lane = lane_id();
  const GMEM uint8_t* p = mb + ((lane * b) >> 3);
  const uint32_t al = (uint32_t)(uintptr_t)p & 3u;
  const uint32_t s = 8 * al + ((lane * b) & 7u);  // < 32
  const GMEM uint32_t* q = reinterpret_cast<const GMEM uint32_t*>(p - al);
  const uint32_t d0 = q[0];
  const uint32_t d1 = s + b > 32 ? q[1] : 0u;
  const uint64_t lo64 = ((uint64_t)d1 << 32) | d0;
  U r;
  if constexpr (W == 8) {
    const uint32_t d2 = s + b > 64 ? q[2] : 0u;
    r = lo64 >> s;
    if (s) r |= (uint64_t)d2 << (64 - s);
    if (b < 64) r &= ((uint64_t)1 << b) - 1;
  } else {
    r = (uint32_t)(lo64 >> s);
    if (b < 32) r &= (1u << b) - 1;
  }
  return r;
}

}  // namespace ipk

}  // namespace bitar_hip
