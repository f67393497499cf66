// bitpack.hip.h -- what the bit-packing codecs share (intpack.hip, fltpack.hip, cascade.hip,
// patchpack.hip, decpack.hip; gfx950, wave64), for elements of 1..16 bytes: wave reductions over
// DPP, element loads and stores at any alignment, the payload emitter that writes a miniblock's
// bit string as aligned dwords, the exception lists' rank and position check (fltpack.hip,
// patchpack.hip), INTPACK's plan and miniblock decode over elements from anywhere (intpack.hip,
// cascade.hip, patchpack.hip), and the frame-of-reference segment encoder and decoder themselves
// (intpack.hip at 1..8 bytes, decpack.hip at 16).
//
// Payload of a miniblock of 64 elements at width b: 8 * b bytes, element t at bits
// [t*b, (t+1)*b) of the little-endian bit string.  Lane t holds element t.
//
// A 16-byte value is an unsigned __int128: the compiler keeps it in four VGPRs, adds and
// subtracts with one carry chain (v_add_co_u32 + 3 v_addc_co_u32), and loads an aligned one as
// global_load_dwordx4.  DPP moves a dword, so every wave step moves four.
#pragma once

#include "wave.hip.h"

namespace bitar_hip {

namespace ipk {

constexpr uint32_t kMini = 64;     // elements per miniblock
constexpr uint32_t kMaxMini = 1024;  // miniblocks of a 64 KiB segment of bytes
constexpr uint32_t kMaxBlk = 256;

template <uint32_t W> struct Elem { using U = uint32_t; using S = int32_t; };
template <> struct Elem<8> { using U = uint64_t; using S = int64_t; };
template <> struct Elem<16> { using U = unsigned __int128; using S = __int128; };
using u128 = unsigned __int128;

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
template <int CTRL, int ROWS>
__device__ __forceinline__ u128 dpp(u128 v, u128 idle) {
  const uint64_t lo = dpp<CTRL, ROWS>((uint64_t)v, (uint64_t)idle);
  const uint64_t hi = dpp<CTRL, ROWS>((uint64_t)(v >> 64), (uint64_t)(idle >> 64));
  return (u128)hi << 64 | lo;
}
// lane l's v (16 bytes: l is wave-uniform, __shfl moves at most 8)
__device__ __forceinline__ uint32_t read_lane(uint32_t v, uint32_t l) { return __shfl(v, l); }
__device__ __forceinline__ uint64_t read_lane(uint64_t v, uint32_t l) { return __shfl(v, l); }
__device__ __forceinline__ u128 read_lane(u128 v, uint32_t l) {
  u128 r = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) r |= (u128)readlane((uint32_t)(v >> (32 * i)), l) << (32 * i);
  return r;
}
// v as the compiler must leave it: in VGPRs of its own, no part of the instruction that uses it
template <typename U>
__device__ __forceinline__ void keep_in_vgprs(U& v) { __asm__ volatile("" : "+v"(v)); }
__device__ __forceinline__ void keep_in_vgprs(u128& v) {
  uint64_t lo = (uint64_t)v, hi = (uint64_t)(v >> 64);  // (no 16-byte operands)
  __asm__ volatile("" : "+v"(lo), "+v"(hi));
  v = (u128)hi << 64 | lo;
}
__device__ __forceinline__ uint32_t lane63(uint32_t v) { return readlane(v, 63); }
__device__ __forceinline__ uint64_t lane63(uint64_t v) {
  return ((uint64_t)readlane((uint32_t)(v >> 32), 63) << 32) | readlane((uint32_t)v, 63);
}
__device__ __forceinline__ u128 lane63(u128 v) { return read_lane(v, 63); }

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
__device__ __forceinline__ uint32_t bit_length(u128 v) {
  const uint64_t hi = (uint64_t)(v >> 64);
  return hi ? 64u + bit_length(hi) : bit_length((uint64_t)v);
}
// the bit length of the OR of the wave's values.  At 16 bytes it is taken as the largest of
// their bit lengths: one dword per DPP step where the OR itself would move four.
template <uint32_t W>
__device__ __forceinline__ uint32_t wave_width(typename Elem<W>::U v) {
  if constexpr (W == 16) return readlane(wave_incl_max(bit_length(v)), 63);
  else return bit_length(wave_or<typename Elem<W>::U>(v));
}

// the W-byte little-endian element at p (any alignment): only aligned units that hold one of
// its bytes are loaded (16 bytes: one 16-byte load when p is 16-byte aligned)
template <uint32_t W>
__device__ __forceinline__ typename Elem<W>::U load_elem(const GMEM uint8_t* p) {
  const uint32_t a = (uint32_t)(uintptr_t)p;
  if constexpr (W == 1) {
    return *p;
  } else if constexpr (W == 2) {
    if ((a & 1u) == 0) return *reinterpret_cast<const GMEM uint16_t*>(p);
    return (uint32_t)p[0] | (uint32_t)p[1] << 8;
  } else if constexpr (W == 16) {
    uint32_t d0, d1, d2, d3;  // (four dwords on every path: as one 16-byte value, the aligned
                              // load's result is copied and waited for where the paths meet)
    if ((a & 15u) == 0) {
      const uint4 x = *reinterpret_cast<const GMEM uint4*>(p);
      d0 = x.x, d1 = x.y, d2 = x.z, d3 = x.w;
    } else {
      const GMEM uint32_t* q = reinterpret_cast<const GMEM uint32_t*>(p - (a & 3u));
      d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
      if ((a & 3u) != 0) {
        const uint32_t top = q[4];
        d0 = funnel(d0, d1, a);
        d1 = funnel(d1, d2, a);
        d2 = funnel(d2, d3, a);
        d3 = funnel(d3, top, a);
      }
    }
    return (u128)((uint64_t)d3 << 32 | d2) << 64 | ((uint64_t)d1 << 32 | d0);
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
  } else if (W == 16 && (a & 15u) == 0) {
    *reinterpret_cast<GMEM typename Elem<W>::U*>(p) = v;  // one 16-byte store
  } else if ((a & 3u) == 0) {
    GMEM uint32_t* q = reinterpret_cast<GMEM uint32_t*>(p);
#pragma unroll
    for (uint32_t k = 0; k < W / 4; ++k) q[k] = (uint32_t)(v >> (32 * k));
  } else {
#pragma unroll
    for (uint32_t k = 0; k < W; ++k) p[k] = (uint8_t)(v >> (8 * k));
  }
}

// the W-byte reference of block `blk` in an LDS array of references
template <uint32_t W>
__device__ __forceinline__ typename Elem<W>::U lds_ref(const uint8_t* refs, uint32_t blk) {
  if constexpr (W == 16) return *reinterpret_cast<const u128*>(&refs[blk * 16]);
  else if constexpr (W == 8) return *reinterpret_cast<const uint64_t*>(&refs[blk * 8]);
  else if constexpr (W == 4) return *reinterpret_cast<const uint32_t*>(&refs[blk * 4]);
  else if constexpr (W == 2) return *reinterpret_cast<const uint16_t*>(&refs[blk * 2]);
  else return refs[blk];
}
template <uint32_t W>
__device__ __forceinline__ void set_lds_ref(uint8_t* refs, uint32_t blk, typename Elem<W>::U ref) {
  if constexpr (W == 16) *reinterpret_cast<u128*>(&refs[blk * 16]) = ref;
  else if constexpr (W == 8) *reinterpret_cast<uint64_t*>(&refs[blk * 8]) = ref;
  else if constexpr (W == 4) *reinterpret_cast<uint32_t*>(&refs[blk * 4]) = ref;
  else if constexpr (W == 2) *reinterpret_cast<uint16_t*>(&refs[blk * 2]) = (uint16_t)ref;
  else refs[blk] = (uint8_t)ref;
}

// one miniblock's bit string in LDS: 64 fields of up to 64 bits (128 at W = 16), and the dword
// that holds the bytes carried over to the next miniblock
constexpr uint32_t stage_rows(uint32_t W) { return W == 16 ? 4 : 2; }  // of 64 dwords
constexpr uint32_t stage_dwords(uint32_t W) { return stage_rows(W) * kMini + 4; }
constexpr uint32_t kStageDwords = stage_dwords(8);

// The payload of a stream, one miniblock at a time, as aligned dwords: the bit string is put
// together in LDS shifted by the payload's byte misalignment `a`, and the `a` bytes of every
// miniblock's last dword are the first bytes of the next one's (miniblocks are multiples of 8
// bytes).  Nothing before pay or at or past pay + bytes() is written.
template <uint32_t W>
struct PayloadEmitter {
  using U = typename Elem<W>::U;
  static constexpr uint32_t kDwords = sizeof(U) / 4;  // of a field; shifted, it touches one more
  GMEM uint8_t* pay;
  uint32_t* stage;  // stage_dwords(W) of LDS
  uint32_t a, carry = 0, off = 0;
  bool started = false;

  __device__ __forceinline__ PayloadEmitter(GMEM uint8_t* pay_, uint32_t* stage_)
      : pay(pay_), stage(stage_), a((uint32_t)(uintptr_t)pay_ & 3u) {}

  // this lane's residual r < 2^b of a miniblock of width b > 0
  __device__ __forceinline__ void put(U r, uint32_t b) {
    const uint32_t lane = lane_id();
    const uint32_t nd = 2 * b;  // its dwords; dword nd holds the bytes carried over
#pragma unroll
    for (uint32_t j = 0; j < stage_rows(W); ++j) stage[lane + j * kWave] = 0;
    if (lane < 4) stage[stage_rows(W) * kWave + lane] = 0;
    lds_order();
    if (lane == 0) stage[0] = carry;
    lds_order();
    const uint32_t bit = 8 * a + lane * b;
    const uint32_t d = bit >> 5, s = bit & 31u;
    // r << s: dword i of r, shifted, lies in dwords i and i + 1.  (Scalars, no loop over the
    // dwords: the loop forms tried give the 1..8-byte kernels other code.)
    const uint64_t lo64 = (uint64_t)(uint32_t)r << s;
    uint32_t w0 = (uint32_t)lo64, w1 = (uint32_t)(lo64 >> 32), w2 = 0, w3 = 0, w4 = 0;
    if constexpr (kDwords >= 2) {
      const uint64_t hi64 = (uint64_t)(uint32_t)(r >> 32) << s;
      w1 |= (uint32_t)hi64;
      w2 = (uint32_t)(hi64 >> 32);
    }
    if constexpr (kDwords == 4) {
      const uint64_t p2 = (uint64_t)(uint32_t)(r >> 64) << s, p3 = (uint64_t)(uint32_t)(r >> 96) << s;
      w2 |= (uint32_t)p2;
      w3 = (uint32_t)(p2 >> 32) | (uint32_t)p3;
      w4 = (uint32_t)(p3 >> 32);
    }
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

// lane t's field of the miniblock of width b > 0 whose payload starts at mb (any alignment);
// only the dwords that hold one of the field's bits are loaded (all inside the miniblock's bytes)
template <uint32_t W>
__device__ __forceinline__ typename Elem<W>::U extract_field(const GMEM uint8_t* mb, uint32_t b) {
  using U = typename Elem<W>::U;
  constexpr uint32_t kDwords = sizeof(U) / 4;
  const uint32_t lane = lane_id();
  const GMEM uint8_t* p = mb + ((lane * b) >> 3);
  const uint32_t al = (uint32_t)(uintptr_t)p & 3u;
  const uint32_t s = 8 * al + ((lane * b) & 7u);  // < 32
  const GMEM uint32_t* q = reinterpret_cast<const GMEM uint32_t*>(p - al);
  // (scalars and branches, no loop over the kDwords + 1 dwords: the loop forms tried give the
  // 1..8-byte kernels other code)
  const uint32_t d0 = q[0];
  const uint32_t d1 = s + b > 32 ? q[1] : 0u;
  const uint64_t lo64 = ((uint64_t)d1 << 32) | d0;
  U r;
  if constexpr (kDwords == 1) {
    r = (uint32_t)(lo64 >> s);
  } else {  // the field's own dwords >> s, and above them the low bits of the one after
    const uint32_t d2 = s + b > 64 ? q[2] : 0u;
    if constexpr (kDwords == 2) {
      r = lo64 >> s;
      if (s) r |= (uint64_t)d2 << (64 - s);
    } else {
      const uint32_t d3 = s + b > 96 ? q[3] : 0u;
      const uint32_t d4 = s + b > 128 ? q[4] : 0u;
      r = ((U)((uint64_t)d3 << 32 | d2) << 64 | lo64) >> s;
      if (s) r |= (U)d4 << (128 - s);
    }
  }
  if (b < 8 * sizeof(U)) r &= ((U)1 << b) - 1;
  return r;
}

// ---- exceptions: elements kept raw behind the payload, pos[] (LE16, increasing) and val[] -----
// (fltpack.hip: the values that are no decimal; patchpack.hip: the residuals too long to pack.)

// the set bits of a wave mask below this lane: an exception's rank among its miniblock's
__device__ __forceinline__ uint32_t rank_in(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                   __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The decoder's check of a position list, 64 at a time with neighbours across lanes: each of
// the nx LE16 positions at pos is below m and above the one before.  sink(p) gets every position
// p < m, from its lane, whether or not the list turns out valid; false for a list that must be
// rejected.  Nothing is written but what the sink writes.
template <class SINK>
__device__ __forceinline__ bool check_positions(const GMEM uint8_t* pos, uint32_t nx, uint32_t m,
                                                SINK&& sink) {
  const uint32_t lane = lane_id();
  bool bad = false;
  uint32_t last = 0;
  for (uint32_t j0 = 0; j0 < nx; j0 += kWave) {
    const uint32_t j = j0 + lane;
    uint32_t p = 0;
    if (j < nx) p = pos[2 * j] | (uint32_t)pos[2 * j + 1] << 8;
    uint32_t before = wave_shr1(p);
    if (lane == 0) before = last;
    if (j < nx) {
      bad = bad || p >= m || (j > 0 && p <= before);
      if (p < m) sink(p);
    }
    last = readlane(p, 63);  // (used only when a full chunk came before)
  }
  return ballot(bad) == 0;
}

// ... into a bitmap in LDS (zeroed by the caller up to bit m): bit p = element p is an exception
__device__ __forceinline__ bool mark_positions(const GMEM uint8_t* pos, uint32_t nx, uint32_t m,
                                               uint32_t* exc) {
  return check_positions(pos, nx, m, [&](uint32_t p) { atomicOr(&exc[p >> 5], 1u << (p & 31u)); });
}

// the 64 bits of miniblock k in the bitmap: bit t = this miniblock's element t is an exception
__device__ __forceinline__ uint64_t exception_mask(const uint32_t* exc, uint32_t k) {
  return (uint64_t)uniform(exc[2 * k + 1]) << 32 | uniform(exc[2 * k]);
}

// ---- INTPACK's plan and its miniblock decode, over elements from anywhere ---------------------
// (intpack.hip takes them from the segment in global memory and puts them back there;
// cascade.hip plans the runs its head scan leaves in LDS and decodes into LDS.)
// A source of elements is a callable: src(idx) is element idx < m; kKeepShift: see load_values.

template <uint32_t W>
struct GlobalElems {
  static constexpr bool kKeepShift = false;
  const GMEM uint8_t* p;
  __device__ __forceinline__ typename Elem<W>::U operator()(uint32_t idx) const {
    return load_elem<W>(p + (uint64_t)idx * W);
  }
};

// the x of this lane's element idx: the element (mode 0) or its difference to the one before
// (mode 1), mod 2^(8W); lanes at or past m get 0
template <uint32_t W, class SRC>
__device__ __forceinline__ void load_values(const SRC& src, uint32_t idx, uint32_t m,
                                            typename Elem<W>::U& plain, typename Elem<W>::U& delta) {
  using U = typename Elem<W>::U;
  constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
  const uint32_t lane = lane_id();
  U v = 0;
  if (idx < m) v = src(idx);
  U prev = dpp<0x138, 0xf>(v, (U)0);  // wave_shr:1
  // (A source may ask for the shifted value to stay a move of its own.  Folded into the
  // subtraction as v_subrev_u32_dpp, which the compiler does where element idx - 1 never needs a
  // second load, the first miniblock's differences came out negated on gfx950: cascade.hip's
  // single-read path.  INTPACK's kernels never get that form, and the barrier costs them time.
  // At 16 bytes it always stays: four moves are cheap next to a carry chain that depends on
  // which form the compiler picks.)
  if constexpr (SRC::kKeepShift || W == 16) keep_in_vgprs(prev);
  if (lane == 0 && idx > 0 && idx < m) prev = src(idx - 1);
  U d = (v - prev) & mask;
  if (idx < kMini) {  // the first miniblock: x_0 = x_1, or 0 when there is no element 1
    const U d1 = read_lane(d, 1);
    if (idx == 0) d = m > 1 ? d1 : 0;
  }
  plain = v;
  delta = idx < m ? d : 0;
}

template <uint32_t W>
__device__ __forceinline__ typename Elem<W>::S as_signed(typename Elem<W>::U x) {
  using S = typename Elem<W>::S;
  constexpr uint32_t sh = 8 * sizeof(S) - 8 * W;
  return (S)(x << sh) >> sh;
}

// Block `blk` (miniblocks 4 blk .. 4 blk + 3) of m elements in both modes: this lane's x, the
// block's reference and the miniblocks' widths (0 for a miniblock past the last)
template <uint32_t W>
struct BlockPlan {
  typename Elem<W>::U x[2][4], ref[2];
  uint32_t b[2][4];
  // this lane's residual in miniblock 4 blk + j (0 at or past m)
  __device__ __forceinline__ typename Elem<W>::U residual(uint32_t md, uint32_t j, bool in) const {
    using U = typename Elem<W>::U;
    constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
    return in ? (U)((x[md][j] - ref[md]) & mask) : (U)0;
  }
};
template <uint32_t W, class SRC>
__device__ __forceinline__ void plan_block(const SRC& src, uint32_t blk, uint32_t m,
                                           BlockPlan<W>& p) {
  using U = typename Elem<W>::U;
  using S = typename Elem<W>::S;
  constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
  const uint32_t lane = lane_id();
  S lo[2] = {(S)(~(U)0 >> 1), (S)(~(U)0 >> 1)};
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t idx = (blk * 4 + j) * kMini + lane;
    load_values<W>(src, idx, m, p.x[0][j], p.x[1][j]);
    if (idx < m) {
      lo[0] = imin(lo[0], as_signed<W>(p.x[0][j]));
      lo[1] = imin(lo[1], as_signed<W>(p.x[1][j]));
    }
  }
#pragma unroll
  for (uint32_t md = 0; md < 2; ++md) {
    p.ref[md] = (U)wave_min<S, U>(lo[md]) & mask;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t idx = (blk * 4 + j) * kMini + lane;
      p.b[md][j] = wave_width<W>(p.residual(md, j, idx < m));
    }
  }
}

// Where the parts of a stream of L bytes at width W lie
template <uint32_t W>
struct Layout {
  uint32_t m, tail, nmb, nblk, wid_at, ref_at, pay_at;
  static constexpr uint32_t base_at = 4;
  __device__ __forceinline__ Layout(uint32_t L, uint32_t mode) {
    m = L / W;
    tail = L - m * W;
    nmb = (m + kMini - 1) / kMini;
    nblk = (nmb + 3) / 4;
    wid_at = 4 + (mode == 1 ? W : 0);
    ref_at = wid_at + nmb;
    pay_at = ref_at + nblk * W;
  }
};

// mode: delta only when strictly smaller, stored (mode 2, size 4 + L) when nothing is gained;
// sum[md] = the payload bytes of mode md
template <uint32_t W>
__device__ __forceinline__ uint32_t choose_mode(uint32_t L, const uint32_t (&sum)[2], uint32_t& size) {
  const Layout<W> lay(L, 0);
  const uint32_t fixed = lay.pay_at + lay.tail;
  const uint32_t size0 = fixed + sum[0], size1 = fixed + W + sum[1];
  const uint32_t mode = size1 < size0 ? 1u : 0u;
  size = mode ? size1 : size0;
  if (size < 4u + L) return mode;
  size = 4u + L;
  return 2u;
}

// the low two bits of a tag: log2(W) for INTPACK's widths (nibble 4), log2(W) - 4 for DECPACK's
// one (nibble 0xD)
template <uint32_t W>
constexpr uint32_t kWidthBits = W == 1 || W == 16 ? 0 : W == 2 ? 1 : W == 4 ? 2 : 3;

// the first dword of a stream
template <uint32_t W, uint32_t NIBBLE = 4>
__device__ __forceinline__ uint32_t stream_head(uint32_t mode, uint32_t L) {
  return NIBBLE << 4 | mode << 2 | kWidthBits<W> | (L - 1) << 16;
}
// what a decoder accepts of bytes 0 and 1 (the width bits apart)
__device__ __forceinline__ bool valid_head(uint32_t tag, uint32_t rsv, uint32_t nibble = 4) {
  return (tag >> 4) == nibble && ((tag >> 2) & 3u) != 3u && rsv == 0;
}

// The widths of a packed stream of csize bytes (mode 0 or 1): false for a stream that must be
// rejected -- too short for its header arrays, a width above 8 W, a size other than what the
// widths add up to.  sink(k, b, off) gets this lane's miniblock k < nmb, its width and the byte
// offset of its payload; `run` becomes the payload's size.
template <uint32_t W, class SINK>
__device__ __forceinline__ bool scan_widths(const GMEM uint8_t* src, uint32_t csize,
                                            const Layout<W>& lay, uint32_t& run, SINK&& sink) {
  const uint32_t lane = lane_id();
  if (csize < lay.pay_at + lay.tail) return false;  // (so the header arrays lie inside the stream)
  run = 0;
  bool bad = false;
  for (uint32_t k0 = 0; k0 < lay.nmb; k0 += kWave) {
    const uint32_t k = k0 + lane;
    const uint32_t b = k < lay.nmb ? src[lay.wid_at + k] : 0u;
    bad = bad || b > 8 * W;
    const uint32_t incl = wave_incl_sum(8u * b);
    if (k < lay.nmb) sink(k, b, run + incl - 8u * b);
    run += readlane(incl, 63);
  }
  if (ballot(bad) != 0) return false;  // (each width <= 8 W: run <= 64 KiB * 8, no overflow)
  return lay.pay_at + run + lay.tail == csize;
}

// this lane's element of miniblock k of width b whose payload starts at mb; `carry` is the last
// element so far (mode 1); block_ref: the block's reference where the caller has loaded it
template <uint32_t W>
__device__ __forceinline__ typename Elem<W>::U unpack_miniblock(
    const GMEM uint8_t* src, const Layout<W>& lay, uint32_t mode, uint32_t k, uint32_t b,
    const GMEM uint8_t* mb, typename Elem<W>::U& carry,
    const typename Elem<W>::U* block_ref = nullptr) {
  using U = typename Elem<W>::U;
  constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
  const uint32_t idx = k * kMini + lane_id();
  U r = 0;
  if (b) r = extract_field<W>(mb, b);
  const U ref = block_ref ? *block_ref : load_elem<W>(src + lay.ref_at + (k / 4) * W);
  U v = (r + ref) & mask;
  if (mode) {
    if (idx == 0) v = load_elem<W>(src + lay.base_at);
    v = wave_incl_add<U>(v) + carry;
    carry = lane63(v);
  }
  return v;
}

// ---- the frame-of-reference segment codec (intpack.hip at 1..8 bytes, decpack.hip at 16) ------
// NIBBLE: the stream's tag nibble.  LDS: for 64 KiB segments of elements of WMIN..WMAX bytes.

template <uint32_t WMIN, uint32_t WMAX>
struct EncLds {
  uint8_t wid[2][kMaxMini / WMIN];                                     // widths of mode 0 / mode 1
  __attribute__((aligned(16))) uint8_t ref[2][kMaxBlk / WMIN * WMAX];  // references, W bytes each
  uint32_t stage[stage_dwords(WMAX)];                                  // one miniblock's bit string
};
template <uint32_t WMIN>
struct DecLds {
  uint8_t wid[kMaxMini / WMIN];
  uint32_t off[kMaxMini / WMIN];  // byte offset of every miniblock in the payload
};

// STORE = false is AUTOPACK's candidate form (autopack.hip): a segment that takes the stored form
// writes its size alone -- a later candidate's stored form is never selected, it ties with
// RUNPACK's at best -- and every other segment is written as ever.
template <uint32_t W, bool STORE, uint32_t NIBBLE, class LDS>
__device__ __forceinline__ void compress_segment(const GMEM uint8_t* src, uint32_t L,
                                                 GMEM uint8_t* dst, uint32_t* size_out, LDS& sh) {
  using U = typename Elem<W>::U;
  constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
  const uint32_t lane = lane_id();
  const Layout<W> lay(L, 0);
  const uint32_t m = lay.m, tail = lay.tail, nmb = lay.nmb, nblk = lay.nblk;
  const GlobalElems<W> elems{src};

  // ---- plan: both modes' references and widths in one sweep ---------------------------------
  uint32_t sum[2] = {0, 0};
  for (uint32_t blk = 0; blk < nblk; ++blk) {
    BlockPlan<W> p;
    plan_block<W>(elems, blk, m, p);
#pragma unroll
    for (uint32_t md = 0; md < 2; ++md) {
      if (lane == 0) set_lds_ref<W>(sh.ref[md], blk, p.ref[md]);
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t k = blk * 4 + j;
        if (k < nmb) {
          if (lane == 0) sh.wid[md][k] = (uint8_t)p.b[md][j];
          sum[md] += 8u * p.b[md][j];
        }
      }
    }
  }
  lds_order();

  // ---- mode: delta only when strictly smaller, stored when nothing is gained ---------------
  uint32_t total;
  const uint32_t mode = choose_mode<W>(L, sum, total);
  GMEM uint32_t* head = reinterpret_cast<GMEM uint32_t*>(dst);  // (slots are 16-B aligned)
  if (mode == 2) {
    if (lane == 0) {
      if constexpr (STORE) *head = stream_head<W, NIBBLE>(2, L);
      *size_out = total;
    }
    if constexpr (STORE) wave_copy_global(dst + 4, src, L);
    return;
  }
  if (lane == 0) {
    *head = stream_head<W, NIBBLE>(mode, L);
    *size_out = total;
  }
  uint32_t pos = 4;
  if (mode) {
    if (lane < W) dst[pos + lane] = src[lane];
    pos += W;
  }
  for (uint32_t k = lane; k < nmb; k += kWave) dst[pos + k] = sh.wid[mode][k];
  pos += nmb;
  for (uint32_t k = lane; k < nblk * W; k += kWave) dst[pos + k] = sh.ref[mode][k];
  pos += nblk * W;

  // ---- emit: the payload as aligned dwords ---------------------------------------------------
  GMEM uint8_t* pay = dst + pos;
  PayloadEmitter<W> emit(pay, sh.stage);
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t b = sh.wid[mode][k];
    if (b == 0) continue;
    const uint32_t idx = k * kMini + lane;
    U xs[2];
    load_values<W>(elems, idx, m, xs[0], xs[1]);
    const U ref = lds_ref<W>(sh.ref[mode], k / 4);
    const U r = idx < m ? (U)(((mode ? xs[1] : xs[0]) - ref) & mask) : (U)0;
    emit.put(r, b);
  }
  const uint32_t off = emit.finish();
  if (lane < tail) pay[off + lane] = src[m * W + lane];
}

// the packed form: src holds csize bytes, the header is valid and L <= seg.  Returns false for a
// stream that must be rejected (checked before anything is written).
template <uint32_t W, class LDS>
__device__ __forceinline__ bool decompress_packed(const GMEM uint8_t* src, uint32_t csize,
                                                  uint32_t L, uint32_t mode, GMEM uint8_t* dst,
                                                  LDS& sh) {
  using U = typename Elem<W>::U;
  const uint32_t lane = lane_id();
  const Layout<W> lay(L, mode);
  const uint32_t m = lay.m, tail = lay.tail, nmb = lay.nmb;

  // widths -> offsets; the stream's size must be exactly what they add up to
  uint32_t run;
  if (!scan_widths<W>(src, csize, lay, run, [&](uint32_t k, uint32_t b, uint32_t off) {
        sh.wid[k] = (uint8_t)b;
        sh.off[k] = off;
      }))
    return false;
  lds_order();

  const GMEM uint8_t* pay = src + lay.pay_at;
  U carry = 0, ref = 0;
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t idx = k * kMini + lane;
    const uint32_t b = sh.wid[k];
    // (at 16 bytes the reference is loaded once per block, after the width and ahead of the
    // fields, whose loads then go out while it is on its way; the narrow kernels keep the load
    // per miniblock that their code has)
    if constexpr (W == 16)
      if ((k & 3u) == 0) ref = load_elem<W>(src + lay.ref_at + (k / 4) * W);
    const U v = unpack_miniblock<W>(src, lay, mode, k, b, pay + sh.off[k], carry,
                                    W == 16 ? &ref : nullptr);
    if (idx < m) store_elem<W>(dst + (uint64_t)idx * W, v);
  }
  if (lane < tail) dst[m * W + lane] = pay[run + lane];
  return true;
}

}  // namespace ipk

}  // namespace bitar_hip
