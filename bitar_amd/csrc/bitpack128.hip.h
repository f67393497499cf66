// bitpack128.hip.h -- bitpack.hip.h's pieces for 16-byte elements (decpack.hip; gfx950, wave64):
// 128-bit values over DPP, element loads and stores at any alignment, INTPACK's plan at 128 bits,
// and the payload emitter and field extractor for widths up to 128, where a field lies in up to
// five dwords of the bit string.
//
// A value is an unsigned __int128: the compiler keeps it in four VGPRs, adds and subtracts with
// one carry chain (v_add_co_u32 + 3 v_addc_co_u32), and loads an aligned one as
// global_load_dwordx4.  DPP moves a dword, so every wave step moves four.
//
// Payload of a miniblock of 64 elements at width b: 8 * b bytes, element t at bits
// [t*b, (t+1)*b) of the little-endian bit string.  Lane t holds element t.
#pragma once

#include "bitpack.hip.h"

namespace bitar_hip {

namespace dpk {

using u128 = unsigned __int128;
using s128 = __int128;

__device__ __forceinline__ uint32_t dword(u128 v, uint32_t i) { return (uint32_t)(v >> (32 * i)); }
__device__ __forceinline__ u128 from_dwords(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
  return (u128)((uint64_t)d3 << 32 | d2) << 64 | ((uint64_t)d1 << 32 | d0);
}

// v moved by a DPP control, four dwords (lanes without a source get `idle`)
template <int CTRL, int ROWS>
__device__ __forceinline__ u128 dpp(u128 v, u128 idle) {
  const uint64_t lo = ipk::dpp<CTRL, ROWS>((uint64_t)v, (uint64_t)idle);
  const uint64_t hi = ipk::dpp<CTRL, ROWS>((uint64_t)(v >> 64), (uint64_t)(idle >> 64));
  return (u128)hi << 64 | lo;
}
__device__ __forceinline__ u128 read_lane(u128 v, uint32_t l) {
  return from_dwords(readlane(dword(v, 0), l), readlane(dword(v, 1), l),
                     readlane(dword(v, 2), l), readlane(dword(v, 3), l));
}
__device__ __forceinline__ u128 lane63(u128 v) { return read_lane(v, 63); }

// the smallest of the wave's 64 values read as signed (the compare carries across the dwords)
__device__ __forceinline__ s128 imin(s128 a, s128 b) { return a < b ? a : b; }
__device__ __forceinline__ s128 wave_min(s128 v) {
  constexpr u128 top = ~(u128)0 >> 1;  // the largest signed value: the identity
  s128 x = v;
  x = imin(x, (s128)dpp<0x111, 0xf>((u128)x, top));
  x = imin(x, (s128)dpp<0x112, 0xf>((u128)x, top));
  x = imin(x, (s128)dpp<0x114, 0xf>((u128)x, top));
  x = imin(x, (s128)dpp<0x118, 0xf>((u128)x, top));
  x = imin(x, (s128)dpp<0x142, 0xa>((u128)x, top));
  x = imin(x, (s128)dpp<0x143, 0xc>((u128)x, top));
  return (s128)lane63((u128)x);
}
// inclusive sum mod 2^128 over the wave's 64 lanes (the add carries across the dwords)
__device__ __forceinline__ u128 wave_incl_add(u128 x) {
  x += dpp<0x111, 0xf>(x, (u128)0);
  x += dpp<0x112, 0xf>(x, (u128)0);
  x += dpp<0x114, 0xf>(x, (u128)0);
  x += dpp<0x118, 0xf>(x, (u128)0);
  x += dpp<0x142, 0xa>(x, (u128)0);
  x += dpp<0x143, 0xc>(x, (u128)0);
  return x;
}

__device__ __forceinline__ uint32_t bit_length(u128 v) {
  const uint64_t hi = (uint64_t)(v >> 64);
  return hi ? 64u + ipk::bit_length(hi) : ipk::bit_length((uint64_t)v);
}
// the bit length of the OR of the wave's values = the largest of their bit lengths: one dword
// per DPP step where the OR itself would move four
__device__ __forceinline__ uint32_t wave_bit_length(u128 v) {
  return readlane(wave_incl_max(bit_length(v)), 63);
}

// the 16-byte little-endian element at p (any alignment): one 16-byte load when p is 16-byte
// aligned, else only the aligned dwords that hold one of its bytes
__device__ __forceinline__ u128 load_elem(const GMEM uint8_t* p) {
  const uint32_t a = (uint32_t)(uintptr_t)p;
  if ((a & 15u) == 0) {
    const uint4 x = *reinterpret_cast<const GMEM uint4*>(p);
    return from_dwords(x.x, x.y, x.z, x.w);
  }
  const GMEM uint32_t* q = reinterpret_cast<const GMEM uint32_t*>(p - (a & 3u));
  uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
  if ((a & 3u) != 0) {
    const uint32_t top = q[4];
    d0 = funnel(d0, d1, a);
    d1 = funnel(d1, d2, a);
    d2 = funnel(d2, d3, a);
    d3 = funnel(d3, top, a);
  }
  return from_dwords(d0, d1, d2, d3);
}

__device__ __forceinline__ void store_elem(GMEM uint8_t* p, u128 v) {
  const uint32_t a = (uint32_t)(uintptr_t)p;
  if ((a & 15u) == 0) {
    *reinterpret_cast<GMEM uint4*>(p) = make_uint4(dword(v, 0), dword(v, 1), dword(v, 2), dword(v, 3));
  } else if ((a & 3u) == 0) {
    GMEM uint32_t* q = reinterpret_cast<GMEM uint32_t*>(p);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) q[k] = dword(v, k);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) p[k] = (uint8_t)(v >> (8 * k));
  }
}

// the x of this lane's element idx of the m elements at src: the element (mode 0) or its
// difference to the one before (mode 1), mod 2^128; lanes at or past m get 0
__device__ __forceinline__ void load_values(const GMEM uint8_t* src, uint32_t idx, uint32_t m,
                                            u128& plain, u128& delta) {
  const uint32_t lane = lane_id();
  u128 v = 0;
  if (idx < m) v = load_elem(src + (uint64_t)idx * 16);
  uint32_t p0 = wave_shr1(dword(v, 0)), p1 = wave_shr1(dword(v, 1));
  uint32_t p2 = wave_shr1(dword(v, 2)), p3 = wave_shr1(dword(v, 3));
  // (The shifted value stays a move of its own: folded into a subtraction as a DPP operand, the
  // first miniblock's differences came out negated on gfx950 in cascade.hip's single-read path,
  // bitpack.hip.h load_values.  Four moves per miniblock are cheap next to a carry chain that
  // depends on which form the compiler picks.)
  __asm__ volatile("" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3));
  u128 prev = from_dwords(p0, p1, p2, p3);
  if (lane == 0 && idx > 0 && idx < m) prev = load_elem(src + (uint64_t)(idx - 1) * 16);
  u128 d = v - prev;
  if (idx < ipk::kMini) {  // the first miniblock: x_0 = x_1, or 0 when there is no element 1
    const u128 d1 = read_lane(d, 1);
    if (idx == 0) d = m > 1 ? d1 : (u128)0;
  }
  plain = v;
  delta = idx < m ? d : (u128)0;
}

// Block `blk` (miniblocks 4 blk .. 4 blk + 3) of the m elements at src in both modes: the
// block's reference and the miniblocks' widths (0 for a miniblock past the last)
struct BlockPlan {
  u128 ref[2];
  uint32_t b[2][4];
};
__device__ __forceinline__ void plan_block(const GMEM uint8_t* src, uint32_t blk, uint32_t m,
                                           BlockPlan& p) {
  const uint32_t lane = lane_id();
  constexpr s128 top = (s128)(~(u128)0 >> 1);
  u128 x[2][4];
  s128 lo[2] = {top, top};
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t idx = (blk * 4 + j) * ipk::kMini + lane;
    load_values(src, idx, m, x[0][j], x[1][j]);
    if (idx < m) {
      lo[0] = imin(lo[0], (s128)x[0][j]);
      lo[1] = imin(lo[1], (s128)x[1][j]);
    }
  }
#pragma unroll
  for (uint32_t md = 0; md < 2; ++md) {
    p.ref[md] = (u128)wave_min(lo[md]);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t idx = (blk * 4 + j) * ipk::kMini + lane;
      p.b[md][j] = wave_bit_length(idx < m ? x[md][j] - p.ref[md] : (u128)0);
    }
  }
}

// one miniblock's bit string in LDS: 64 fields of up to 128 bits, and the dword that holds the
// bytes carried over to the next miniblock
constexpr uint32_t kStageDwords = 4 * ipk::kMini + 4;

// bitpack.hip.h's PayloadEmitter for fields of up to 128 bits: the bit string (up to 1 KiB) is
// put together in LDS shifted by the payload's byte misalignment `a`, and leaves as aligned
// dwords; the `a` bytes of every miniblock's last dword are the first bytes of the next one's
// (miniblocks are multiples of 8 bytes).  Nothing before pay or at or past pay + bytes() is
// written.
struct PayloadEmitter {
  GMEM uint8_t* pay;
  uint32_t* stage;  // kStageDwords of LDS
  uint32_t a, carry = 0, off = 0;
  bool started = false;

  __device__ __forceinline__ PayloadEmitter(GMEM uint8_t* pay_, uint32_t* stage_)
      : pay(pay_), stage(stage_), a((uint32_t)(uintptr_t)pay_ & 3u) {}

  // this lane's residual r < 2^b of a miniblock of width b, 1..128
  __device__ __forceinline__ void put(u128 r, uint32_t b) {
    const uint32_t lane = lane_id();
    const uint32_t nd = 2 * b;  // its dwords; dword nd holds the bytes carried over
    // (the last bit of the shifted string is bit 8a + 64b - 1 < 32 (nd + 1): dwords 0..nd)
    for (uint32_t j = lane; j <= nd; j += kWave) stage[j] = 0;
    lds_order();
    if (lane == 0) stage[0] = carry;
    lds_order();
    const uint32_t bit = 8 * a + lane * b;
    const uint32_t d = bit >> 5, s = bit & 31u;
    // r << s, 160 bits: dword i takes the high half of (r_i : r_(i-1)) << s
    const uint32_t r0 = dword(r, 0), r1 = dword(r, 1), r2 = dword(r, 2), r3 = dword(r, 3);
    const uint32_t w0 = r0 << s;
    const uint32_t w1 = (uint32_t)((((uint64_t)r1 << 32 | r0) << s) >> 32);
    const uint32_t w2 = (uint32_t)((((uint64_t)r2 << 32 | r1) << s) >> 32);
    const uint32_t w3 = (uint32_t)((((uint64_t)r3 << 32 | r2) << s) >> 32);
    const uint32_t w4 = (uint32_t)(((uint64_t)r3 << s) >> 32);
    // (a dword that is not zero holds a bit of the field, so it is one of dwords 0..nd)
    if (w0) atomicOr(&stage[d], w0);
    if (w1) atomicOr(&stage[d + 1], w1);
    if (w2) atomicOr(&stage[d + 2], w2);
    if (w3) atomicOr(&stage[d + 3], w3);
    if (w4) atomicOr(&stage[d + 4], w4);
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

// lane t's field of the miniblock of width b, 1..128, whose payload starts at mb (any
// alignment); only the dwords that hold one of the field's bits are loaded (all of them hold a
// byte of the miniblock)
__device__ __forceinline__ u128 extract_field(const GMEM uint8_t* mb, uint32_t b) {
  const uint32_t lane = lane_id();
  const GMEM uint8_t* p = mb + ((lane * b) >> 3);
  const uint32_t al = (uint32_t)(uintptr_t)p & 3u;
  const uint32_t s = 8 * al + ((lane * b) & 7u);  // < 32
  const GMEM uint32_t* q = reinterpret_cast<const GMEM uint32_t*>(p - al);
  const uint32_t d0 = q[0];
  const uint32_t d1 = s + b > 32 ? q[1] : 0u;
  const uint32_t d2 = s + b > 64 ? q[2] : 0u;
  const uint32_t d3 = s + b > 96 ? q[3] : 0u;
  const uint32_t d4 = s + b > 128 ? q[4] : 0u;
  u128 r = from_dwords((uint32_t)(((uint64_t)d1 << 32 | d0) >> s),
                       (uint32_t)(((uint64_t)d2 << 32 | d1) >> s),
                       (uint32_t)(((uint64_t)d3 << 32 | d2) >> s),
                       (uint32_t)(((uint64_t)d4 << 32 | d3) >> s));
  if (b < 128) r &= ((u128)1 << b) - 1;
  return r;
}

}  // namespace dpk

}  // namespace bitar_hip
