// runs.hip.h -- what the run-length codecs share (runpack.hip, cascade.hip; gfx950, wave64): the
// chunk reader, the head scan of the encoders and the window expansion of the decoders.
//
// Both directions work in CHUNKS: chunk c is bytes [16c, 16c + 16) of the segment, E = 16 / W
// whole elements, and lane t of a step holds chunk 64*step + t, so a step moves 1 KiB at every
// element width W.
#pragma once

#include "bitpack.hip.h"
#include "wave.hip.h"

namespace bitar_hip {

namespace rpk {

__device__ __forceinline__ uint32_t pick(const uint4& v, uint32_t k) {  // (no indexed registers)
  return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
}

// bytes [s, s + 16) of the 32-byte little-endian pair (x, y), s in 0..16 and wave-uniform
__device__ __forceinline__ uint4 window16(const uint4& x, const uint4& y, uint32_t s) {
  const uint32_t r = s;  // (funnel keeps the low two bits)
  switch (s >> 2) {
    case 0: return make_uint4(funnel(x.x, x.y, r), funnel(x.y, x.z, r), funnel(x.z, x.w, r), funnel(x.w, y.x, r));
    case 1: return make_uint4(funnel(x.y, x.z, r), funnel(x.z, x.w, r), funnel(x.w, y.x, r), funnel(y.x, y.y, r));
    case 2: return make_uint4(funnel(x.z, x.w, r), funnel(x.w, y.x, r), funnel(y.x, y.y, r), funnel(y.y, y.z, r));
    case 3: return make_uint4(funnel(x.w, y.x, r), funnel(y.x, y.y, r), funnel(y.y, y.z, r), funnel(y.z, y.w, r));
    default: return y;
  }
}

// every lane gets the lane below's v; lane 0 gets `carry` (wave-uniform)
__device__ __forceinline__ uint4 from_below(const uint4& v, const uint4& carry) {
  uint4 p = make_uint4(wave_shr1(v.x), wave_shr1(v.y), wave_shr1(v.z), wave_shr1(v.w));
  if (lane_id() == 0) p = carry;
  return p;
}
__device__ __forceinline__ uint4 lane63(const uint4& v) {
  return make_uint4(readlane(v.x, 63), readlane(v.y, 63), readlane(v.z, 63), readlane(v.w, 63));
}

// The segment's chunks, for a segment at any address: aligned 16-byte blocks, a lane's second
// block taken from the lane above.  A block is loaded only when it holds a byte of the segment.
struct ChunkReader {
  const GMEM uint4* sa;
  uint32_t sh, L;
  __device__ __forceinline__ ChunkReader(const GMEM uint8_t* src, uint32_t L_)
      : sh((uint32_t)(uintptr_t)src & 15u), L(L_) {
    sa = reinterpret_cast<const GMEM uint4*>(src - sh);
  }
  // chunk c of this lane (zeros where c starts past the segment; bytes past L are arbitrary)
  __device__ __forceinline__ uint4 load(uint32_t c) const {
    const bool act = 16u * c < L;
    uint4 x = make_uint4(0, 0, 0, 0);
    if (act) x = sa[c];
    if (sh == 0) return x;
    uint4 y = make_uint4(shfl_down1(x.x), shfl_down1(x.y), shfl_down1(x.z), shfl_down1(x.w));
    // the block above: from the lane above when that lane loaded it, else from memory when it
    // holds a byte of the segment (it starts at byte 16(c+1) - sh of it)
    const bool own = lane_id() == kWave - 1 || !(16u * (c + 1) < L);
    if (act && own && 16u * (c + 1) < L + sh) y = sa[c + 1];
    return window16(x, y, sh);
  }
};

// bit j: element j of chunk `ch` differs from its predecessor (element 0's is the last element
// of `prev`, the chunk before)
template <uint32_t W>
__device__ __forceinline__ uint32_t head_mask(const uint4& ch, const uint4& prev) {
  if constexpr (W == 16) {
    return (((ch.x ^ prev.x) | (ch.y ^ prev.y) | (ch.z ^ prev.z) | (ch.w ^ prev.w)) != 0) ? 1u : 0u;
  } else if constexpr (W == 8) {
    const uint32_t a = (ch.x ^ prev.z) | (ch.y ^ prev.w), b = (ch.z ^ ch.x) | (ch.w ^ ch.y);
    return (a ? 1u : 0u) | (b ? 2u : 0u);
  } else if constexpr (W == 4) {
    return (ch.x != prev.w ? 1u : 0u) | (ch.y != ch.x ? 2u : 0u) | (ch.z != ch.y ? 4u : 0u) |
           (ch.w != ch.z ? 8u : 0u);
  } else {
    const uint32_t w[5] = {prev.w, ch.x, ch.y, ch.z, ch.w};
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      // every element of the dword against the one before it, 8*W bits down the byte string
      const uint32_t d = w[k + 1] ^ (w[k + 1] << (8 * W) | w[k] >> (32 - 8 * W));
      if constexpr (W == 2) {
        mask |= ((d & 0xFFFFu) ? 1u : 0u) << (2 * k) | ((d >> 16) ? 2u : 0u) << (2 * k);
      } else {
        // bit 7 of each byte that is not 0, then those four bits gathered by a multiply
        // (partial products land on distinct bits: 3, 10, 17, 24 | 11, 18, 25 | 19, 26 | 27)
        const uint32_t t = (((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;
        mask |= (((t >> 7) * 0x01020408u) >> 24) << (4 * k);
      }
    }
    return mask;
  }
}

// element j of a chunk, in the low dwords of the result
template <uint32_t W>
__device__ __forceinline__ uint4 element(const uint4& ch, uint32_t j) {
  if constexpr (W == 16) return ch;
  else if constexpr (W == 8) return j ? make_uint4(ch.z, ch.w, 0, 0) : make_uint4(ch.x, ch.y, 0, 0);
  else if constexpr (W == 4) return make_uint4(pick(ch, j), 0, 0, 0);
  else if constexpr (W == 2) return make_uint4((pick(ch, j >> 1) >> (16 * (j & 1u))) & 0xFFFFu, 0, 0, 0);
  else return make_uint4((pick(ch, j >> 2) >> (8 * (j & 3u))) & 0xFFu, 0, 0, 0);
}

// One step of an encoder pass: this lane's chunk, its head bits, and where the heads are.
template <uint32_t W>
struct HeadScan {
  static constexpr uint32_t E = 16 / W;
  ChunkReader rd;
  uint32_t m;
  uint4 carry = make_uint4(0, 0, 0, 0);  // the chunk of lane 63 of the step before
  uint32_t last = 0;                     // position of the last head so far (element 0 is one)
  uint4 ch;
  uint32_t mask;

  __device__ __forceinline__ HeadScan(const GMEM uint8_t* src, uint32_t L, uint32_t m_)
      : rd(src, L), m(m_) {}

  // loads the step's chunks; returns false when none of its elements is a head
  __device__ __forceinline__ bool step(uint32_t c) {
    ch = rd.load(c);
    const uint4 prev = from_below(ch, carry);
    carry = lane63(ch);
    mask = head_mask<W>(ch, prev);
    if (c == 0) mask |= 1u;
    const uint32_t e0 = c * E;
    const uint32_t nv = e0 >= m ? 0u : (m - e0 < E ? m - e0 : E);  // elements of the segment
    mask &= (1u << nv) - 1u;
    return ballot(mask != 0) != 0;
  }
  // (after a step with heads) the position of the last head below this lane's chunk, and the
  // new `last`
  __device__ __forceinline__ uint32_t head_below(uint32_t c) {
    const uint32_t top = mask ? c * E + (31u - (uint32_t)__clz((int)mask)) + 1u : 0u;
    const uint32_t incl = wave_incl_max(top);
    const uint32_t below = max(wave_shr1(incl), last + 1u) - 1u;
    last = readlane(incl, 63) - 1u;
    return below;
  }
};

__device__ __forceinline__ uint32_t byte_of(const uint4& v, uint32_t t) {
  return ((t < 4 ? v.x : t < 8 ? v.y : t < 12 ? v.z : v.w) >> (8 * (t & 3u))) & 0xFFu;
}

// The expansion of r runs whose lengths add up to m (the caller has checked that) into m
// elements at dst, one window of 64 chunks (64 * E elements) per step.  `map` is 32 dwords of LDS.
// Where the runs come from is the caller's RUNS:
//   length_of(k)       run k's length, wave-uniform k < r
//   lengths_from(s)    this lane's length of run s + lane, 0 at or past r
//   repeated(k)        run k's value repeated over 16 bytes
//   stage(cur, s)      runs cur .. s - 1 (at most 64 * E of them) are about to be gathered
//   values()           the LDS they are gathered from, and
//   slot(i)            where run cur + i lies in it, in elements
// Block b of the output is its bytes [16b - a, 16b - a + 16), a = the output's misalignment: the
// top a bytes of chunk b - 1 and the rest of chunk b.  Lane t of a step makes chunk 64*step + t
// and stores that block, 16 bytes at once unless it crosses an end of the output.
template <uint32_t W, class RUNS>
__device__ __forceinline__ void expand_runs(RUNS& runs, uint32_t r, uint32_t m, GMEM uint8_t* dst,
                                            uint32_t* map) {
  constexpr uint32_t E = 16 / W;
  const uint32_t lane = lane_id();
  const uint32_t a = (uint32_t)(uintptr_t)dst & 15u;
  const uint32_t T = m * W;
  const uint32_t nblk = (T + a + 15u) / 16u;
  uint32_t cur = 0;                      // the run that holds the window's first element
  uint32_t cur_end = runs.length_of(0);  // where it ends
  uint32_t rep_run = 0;
  uint4 rep = runs.repeated(0);          // run rep_run's value over 16 bytes
  uint4 carry = make_uint4(0, 0, 0, 0);
  for (uint32_t b0 = 0; b0 < nblk; b0 += kWave) {
    const uint32_t ws = b0 * E;
    uint4 ch = rep;
    if (ws < m) {
      const uint32_t we = ws + kWave * E < m ? ws + kWave * E : m;
      if (cur_end >= we) {
        // one run covers the window: every lane stores its value
        if (rep_run != cur) {
          rep = runs.repeated(cur);
          rep_run = cur;
        }
        ch = rep;
      } else {
        // mark where the runs after `cur` start, 64 runs per step, up to the window's end
        if (lane < 32) map[lane] = 0;
        lds_order();
        uint32_t s = cur + 1u, pos = cur_end;
        while (pos < we) {  // (then s < r: the lengths add up to m)
          const uint32_t k = s + lane;
          const uint32_t v = runs.lengths_from(s);
          const uint32_t incl = wave_incl_sum(v);
          const uint32_t start = pos + incl - v;
          const bool in = (k < r) & (start < we);
          if (in) atomicOr(&map[(start - ws) >> 5], 1u << ((start - ws) & 31u));
          const uint32_t n_in = (uint32_t)__popcll(ballot(in));  // >= 1: lane 0 starts at pos
          if (n_in == 0) break;              // (so never taken: the loop ends by construction)
          pos += readlane(incl, n_in - 1u);  // the end of the last of them
          s += n_in;
        }
        // the values of runs cur .. s - 1 (at most 64 * E of them) in LDS
        runs.stage(cur, s);
        lds_order();
        const uint32_t* vals = runs.values();
        // an element's run is `cur` plus the number of starts at or before it
        const uint32_t bits = (map[(lane * E) >> 5] >> ((lane * E) & 31u)) & ((1u << E) - 1u);
        const uint32_t cnt = (uint32_t)__popc(bits);
        const uint32_t base = wave_incl_sum(cnt) - cnt;
        uint32_t idx[E];
#pragma unroll
        for (uint32_t j = 0; j < E; ++j)
          idx[j] = runs.slot(base + (uint32_t)__popc(bits & ((2u << j) - 1u)));
        if constexpr (W == 16) {
          ch = *reinterpret_cast<const uint4*>(&vals[idx[0] * 4]);
        } else if constexpr (W == 8) {
          ch = make_uint4(vals[idx[0] * 2], vals[idx[0] * 2 + 1], vals[idx[1] * 2],
                          vals[idx[1] * 2 + 1]);
        } else if constexpr (W == 4) {
          ch = make_uint4(vals[idx[0]], vals[idx[1]], vals[idx[2]], vals[idx[3]]);
        } else {
          uint32_t w[4];
#pragma unroll
          for (uint32_t q = 0; q < 4; ++q) {
            w[q] = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4 / W; ++j) {
              uint32_t e;
              if constexpr (W == 2) e = reinterpret_cast<const uint16_t*>(vals)[idx[q * 2 + j]];
              else e = reinterpret_cast<const uint8_t*>(vals)[idx[q * 4 + j]];
              w[q] |= e << (8 * W * j);
            }
          }
          ch = make_uint4(w[0], w[1], w[2], w[3]);
        }
        lds_order();
        cur = s - 1u;
        cur_end = pos;
      }
      if (cur_end == we && we < m) {  // the next window starts a run
        ++cur;
        cur_end += runs.length_of(cur);
      }
    }
    const uint4 below = from_below(ch, carry);
    carry = lane63(ch);
    const uint4 o = window16(below, ch, 16u - a);
    const int32_t lo = (int32_t)(16u * (b0 + lane)) - (int32_t)a;
    if (lo >= 0 && (uint32_t)lo + 16u <= T) {
      *reinterpret_cast<GMEM uint4*>(dst + lo) = o;
    } else {
#pragma unroll
      for (uint32_t t = 0; t < 16; ++t) {
        const int32_t at = lo + (int32_t)t;
        if (at >= 0 && (uint32_t)at < T) dst[at] = (uint8_t)byte_of(o, t);
      }
    }
  }
}

}  // namespace rpk

}  // namespace bitar_hip
