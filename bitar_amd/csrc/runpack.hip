// runpack.hip -- RUNPACK: per-segment run-length coding of fixed-width elements, for sorted or
// clustered columns whose values come in long runs (partition and dimension keys, coarse
// timestamps, status and flag bytes, byte-per-value validity), both directions (gfx950).  No
// reference counterpart.
//
// Stream of a segment of L bytes, element width W in {1, 2, 4, 8, 16}, m = L / W elements
// compared as byte patterns:
//   byte 0      0x70 | mode << 3 | log2(W)     mode 0 runs, 1 stored
//   byte 1      bl, bytes per run length: 1 or 2 (0 in the stored form)
//   bytes 2..3  LE16(L - 1)
//   stored:     L raw bytes                                                  size = 4 + L
//   runs:       LE16(r - 1)  values[r] (W bytes each)  lengths[r] (length - 1, bl bytes LE)  tail
//               size = 6 + r*(W + bl) + (L - m*W)
// Runs are maximal, bl is 1 when no run is longer than 256, and the runs form is taken when its
// size is strictly below 4 + L (a tie is stored).
//
// One wavefront per segment.  Both kernels work in CHUNKS (runs.hip.h, shared with cascade.hip:
// the chunk reader, the head scan and the decoder's window expansion): chunk c is bytes
// [16c, 16c + 16) of the segment, E = 16 / W whole elements, and lane t of a step holds chunk
// 64*step + t, so a step moves 1 KiB at every width.  The encoder counts the runs in one pass and keeps the first
// heads in LDS; a segment with more of them than fit there is read a second time to emit.  A step
// without a head -- the common case of the columns this codec is for -- costs the load, the
// compare and one ballot in either pass.  The
// decoder builds chunks from the runs and stores them as 16-byte blocks aligned in the OUTPUT,
// whatever the alignment of the segment.
#include "../../include/bitar_hip.h"
#include "autopack.hip.h"
#include "bitpack.hip.h"
#include "runs.hip.h"

namespace bitar_hip {

namespace rpk {

// a run's value into the stream (values start 6 bytes into a 16-B aligned slot: elements of 4
// bytes and more sit at 2 mod 4 and get halfword and dword stores)
template <uint32_t W>
__device__ __forceinline__ void store_value(GMEM uint8_t* p, const uint4& v) {
  const uint32_t a = (uint32_t)(uintptr_t)p;
  if constexpr (W == 1) {
    *p = (uint8_t)v.x;
  } else if constexpr (W == 2) {
    if ((a & 1u) == 0) {
      *reinterpret_cast<GMEM uint16_t*>(p) = (uint16_t)v.x;
    } else {
      p[0] = (uint8_t)v.x;
      p[1] = (uint8_t)(v.x >> 8);
    }
  } else {
    constexpr uint32_t N = W / 4;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if ((a & 3u) == 2) {
      *reinterpret_cast<GMEM uint16_t*>(p) = (uint16_t)w[0];
      GMEM uint32_t* q = reinterpret_cast<GMEM uint32_t*>(p + 2);
#pragma unroll
      for (uint32_t k = 0; k + 1 < N; ++k) q[k] = w[k] >> 16 | w[k + 1] << 16;
      *reinterpret_cast<GMEM uint16_t*>(p + W - 2) = (uint16_t)(w[N - 1] >> 16);
    } else if ((a & 3u) == 0) {
      GMEM uint32_t* q = reinterpret_cast<GMEM uint32_t*>(p);
#pragma unroll
      for (uint32_t k = 0; k < N; ++k) q[k] = w[k];
    } else {
#pragma unroll
      for (uint32_t k = 0; k < W; ++k) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3u)));
    }
  }
}

// (length - 1) of a run, bl bytes little-endian, wherever it falls
__device__ __forceinline__ void store_length(GMEM uint8_t* p, uint32_t v, uint32_t bl) {
  if (bl == 1) {
    *p = (uint8_t)v;
  } else if (((uint32_t)(uintptr_t)p & 1u) == 0) {
    *reinterpret_cast<GMEM uint16_t*>(p) = (uint16_t)v;
  } else {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
  }
}

__device__ __forceinline__ void store_header(GMEM uint8_t* dst, uint32_t mode, uint32_t lg,
                                             uint32_t bl, uint32_t L) {
  // (slots are 16-B aligned)
  *reinterpret_cast<GMEM uint32_t*>(dst) = 0x70u | mode << 3 | lg | bl << 8 | (L - 1) << 16;
}

// The heads pass one meets, while there are at most kCap of them: their positions and values.
// A segment of long runs -- what the codec is for -- is then written from here and read once.
// (A second read is a second read from HBM at scale: the 8192 segments in flight are 512 MiB,
// twice the Infinity Cache.)  kCap keeps the LDS of a one-wave workgroup at 6 KiB or less.
template <uint32_t W>
struct EncShared {
  static constexpr uint32_t kCap = W <= 4 ? 1024 : 256;
  __attribute__((aligned(16))) uint32_t val[kCap * W / 4];
  uint16_t pos[kCap];  // (a position is below 65536)

  __device__ __forceinline__ void put(uint32_t k, uint32_t at, const uint4& v) {
    pos[k] = (uint16_t)at;
    if constexpr (W == 16) *reinterpret_cast<uint4*>(&val[4 * k]) = v;
    else if constexpr (W == 8) *reinterpret_cast<uint2*>(&val[2 * k]) = make_uint2(v.x, v.y);
    else if constexpr (W == 4) val[k] = v.x;
    else if constexpr (W == 2) reinterpret_cast<uint16_t*>(val)[k] = (uint16_t)v.x;
    else reinterpret_cast<uint8_t*>(val)[k] = (uint8_t)v.x;
  }
  __device__ __forceinline__ uint4 value(uint32_t k) const {
    if constexpr (W == 16) return *reinterpret_cast<const uint4*>(&val[4 * k]);
    else if constexpr (W == 8) return make_uint4(val[2 * k], val[2 * k + 1], 0, 0);
    else if constexpr (W == 4) return make_uint4(val[k], 0, 0, 0);
    else if constexpr (W == 2) return make_uint4(reinterpret_cast<const uint16_t*>(val)[k], 0, 0, 0);
    else return make_uint4(reinterpret_cast<const uint8_t*>(val)[k], 0, 0, 0);
  }
};

template <uint32_t W>
__device__ __forceinline__ void compress_segment(const GMEM uint8_t* src, uint32_t L,
                                                 GMEM uint8_t* dst, uint32_t* size_out,
                                                 EncShared<W>& sh) {
  constexpr uint32_t kCap = EncShared<W>::kCap;
  constexpr uint32_t E = 16 / W;
  constexpr uint32_t kLog = W == 1 ? 0 : W == 2 ? 1 : W == 4 ? 2 : W == 8 ? 3 : 4;
  const uint32_t lane = lane_id();
  const uint32_t m = L / W, tail = L - m * W;
  const uint32_t nch = (m * W + 15u) / 16u;

  // ---- pass one: the number of runs, and whether one is longer than 256 ---------------------
  uint32_t r = 0, bl = 1;
  bool stored = m == 0;
  if (!stored) {
    HeadScan<W> hs(src, L, m);
    bool wide = false;
    for (uint32_t c0 = 0; c0 < nch; c0 += kWave) {
      const uint32_t c = c0 + lane;
      if (!hs.step(c)) continue;
      const uint32_t below = hs.head_below(c);
      // the run that ends at this lane's first head (runs inside a chunk are shorter than 16)
      const uint32_t first = c * E + (uint32_t)__builtin_ctz(hs.mask | 0x10000u);
      if (ballot((hs.mask != 0) & (first - below > 256u)) != 0) wide = true;
      const uint32_t cnt = (uint32_t)__popc(hs.mask);
      const uint32_t incl = wave_incl_sum(cnt);
      if (r < kCap) {  // head k, when it is one of the first kCap, is kept
        uint32_t k = r + incl - cnt;
        for (uint32_t mk = hs.mask; mk; mk &= mk - 1u, ++k) {
          const uint32_t j = (uint32_t)__builtin_ctz(mk);
          if (k < kCap) sh.put(k, c * E + j, element<W>(hs.ch, j));
        }
      }
      r += readlane(incl, 63);
      // the smallest runs form of r runs is no smaller than the stored one: no need to go on
      if (6u + r * (W + 1u) >= 4u + L) {
        stored = true;
        break;
      }
    }
    if (!stored) {
      if (m - hs.last > 256u) wide = true;
      bl = wide ? 2u : 1u;
      stored = !(6u + r * (W + bl) + tail < 4u + L);  // a tie is stored
    }
  }
  if (stored) {
    if (lane == 0) {
      store_header(dst, 1, kLog, 0, L);
      *size_out = 4u + L;
    }
    wave_copy_global(dst + 4, src, L);
    return;
  }

  if (lane == 0) {
    store_header(dst, 0, kLog, bl, L);
    *reinterpret_cast<GMEM uint16_t*>(dst + 4) = (uint16_t)(r - 1);
    *size_out = 6u + r * (W + bl) + tail;
  }
  GMEM uint8_t* vals = dst + 6;
  GMEM uint8_t* lens = vals + r * W;
  if (lane < tail) lens[r * bl + lane] = src[m * W + lane];

  // ---- every head was kept: run k is lane k's, its length the distance to the next head ------
  if (r <= kCap) {
    lds_order();
    for (uint32_t k = lane; k < r; k += kWave) {
      const uint32_t at = sh.pos[k], next = k + 1u < r ? (uint32_t)sh.pos[k + 1u] : m;
      store_value<W>(vals + k * W, sh.value(k));
      store_length(lens + k * bl, next - at - 1u, bl);
    }
    return;
  }

  // ---- pass two: head k writes values[k] and, from the head before it, lengths[k - 1] --------
  HeadScan<W> hs(src, L, m);
  uint32_t done = 0;
  for (uint32_t c0 = 0; c0 < nch; c0 += kWave) {
    const uint32_t c = c0 + lane;
    if (!hs.step(c)) continue;
    uint32_t prev = hs.head_below(c);
    const uint32_t cnt = (uint32_t)__popc(hs.mask);
    const uint32_t incl = wave_incl_sum(cnt);
    uint32_t k = done + incl - cnt;
    done += readlane(incl, 63);
    for (uint32_t mk = hs.mask; mk; mk &= mk - 1u) {
      const uint32_t j = (uint32_t)__builtin_ctz(mk);
      const uint32_t pos = c * E + j;
      store_value<W>(vals + k * W, element<W>(hs.ch, j));
      if (k) store_length(lens + (k - 1u) * bl, pos - prev - 1u, bl);
      prev = pos;
      ++k;
    }
  }
  if (lane == 0) store_length(lens + (r - 1u) * bl, m - hs.last - 1u, bl);
}

struct DecShared {
  __attribute__((aligned(16))) uint32_t vals[(1024 + 16) / 4];  // the values of a window's runs
  uint32_t map[32];  // bit e: a run starts at element e of the window
};

__device__ __forceinline__ uint32_t load_length(const GMEM uint8_t* lens, uint32_t k, uint32_t bl) {
  if (bl == 1) return 1u + lens[k];
  return 1u + lens[2 * k] + ((uint32_t)lens[2 * k + 1] << 8);
}

// the W-byte value at p (any alignment) repeated over 16 bytes
template <uint32_t W>
__device__ __forceinline__ uint4 load_repeated(const GMEM uint8_t* p) {
  if constexpr (W == 1) {
    const uint32_t v = (uint32_t)*p * 0x01010101u;
    return make_uint4(v, v, v, v);
  } else if constexpr (W == 2) {
    const uint32_t v = ((uint32_t)p[0] | (uint32_t)p[1] << 8) * 0x00010001u;
    return make_uint4(v, v, v, v);
  } else if constexpr (W == 4) {
    const uint32_t v = ipk::load_elem<4>(p);
    return make_uint4(v, v, v, v);
  } else if constexpr (W == 8) {
    const uint32_t lo = ipk::load_elem<4>(p), hi = ipk::load_elem<4>(p + 4);
    return make_uint4(lo, hi, lo, hi);
  } else {
    return make_uint4(ipk::load_elem<4>(p), ipk::load_elem<4>(p + 4), ipk::load_elem<4>(p + 8),
                      ipk::load_elem<4>(p + 12));
  }
}

// The runs of a stream in global memory, as expand_runs takes them (runs.hip.h): the values of a
// window's runs are copied side by side into LDS.
template <uint32_t W>
struct GlobalRuns {
  const GMEM uint8_t* vals;
  const GMEM uint8_t* lens;
  uint32_t bl, r;
  uint32_t* lds;  // DecShared::vals
  __device__ __forceinline__ uint32_t length_of(uint32_t k) const { return load_length(lens, k, bl); }
  __device__ __forceinline__ uint32_t lengths_from(uint32_t s) const {
    const uint32_t k = s + lane_id();
    return k < r ? load_length(lens, k, bl) : 0u;
  }
  __device__ __forceinline__ uint4 repeated(uint32_t k) const { return load_repeated<W>(vals + k * W); }
  __device__ __forceinline__ void stage(uint32_t cur, uint32_t s) const {
    const uint32_t lane = lane_id();
    const GMEM uint8_t* p = vals + cur * W;
    const uint32_t nbytes = (s - cur) * W;
    for (uint32_t j = lane; j < nbytes / 4u; j += kWave) lds[j] = ipk::load_elem<4>(p + 4u * j);
    if (lane < (nbytes & 3u))
      reinterpret_cast<uint8_t*>(lds)[(nbytes & ~3u) + lane] = p[(nbytes & ~3u) + lane];
  }
  __device__ __forceinline__ const uint32_t* values() const { return lds; }
  __device__ __forceinline__ uint32_t slot(uint32_t i) const { return i; }
};

// The runs form: src holds csize >= 4 bytes, the header's tag is valid and L <= seg.  Returns
// false, having written nothing, for a stream that must be rejected.
template <uint32_t W>
__device__ __forceinline__ bool decompress_runs(const GMEM uint8_t* src, uint32_t csize, uint32_t bl,
                                                uint32_t L, GMEM uint8_t* dst, DecShared& sh) {
  const uint32_t lane = lane_id();
  const uint32_t m = L / W, tail = L - m * W;
  if (csize < 6 || (bl != 1 && bl != 2)) return false;
  const uint32_t r = 1u + src[4] + ((uint32_t)src[5] << 8);
  if (r > m || csize != 6u + r * (W + bl) + tail) return false;
  const GMEM uint8_t* vals = src + 6;
  const GMEM uint8_t* lens = vals + r * W;

  // ---- the run lengths must add up to m.  The true sum can reach 2^32 (W = 1, r = 65536, every
  // length 65536) and no further, so a 32-bit sum is wrong only there, where it wraps to 0:
  // still rejected, because m >= r >= 1.  (Partial sums are 32 bits wide everywhere.)
  uint32_t part = 0;
  for (uint32_t k = lane; k < r; k += kWave) part += load_length(lens, k, bl);
  if (readlane(wave_incl_sum(part), 63) != m) return false;

  // ---- expansion (runs.hip.h), the runs taken from the stream in global memory -----------------
  GlobalRuns<W> runs{vals, lens, bl, r, sh.vals};
  expand_runs<W>(runs, r, m, dst, sh.map);
  const uint32_t T = m * W;
  if (lane < tail) dst[T + lane] = lens[r * bl + lane];
  return true;
}

}  // namespace rpk

// RUNPACK as the shared kernels see it (autopack.hip.h).  The encoder writes nothing at or past
// the stream's size in its slot, and it has the storing form alone: as AUTOPACK's first candidate
// it writes into the caller's slot.  The decoder leaves a rejected segment's output range
// untouched and writes nothing outside the segment's first L bytes.
struct RunPack {
  static constexpr uint32_t kNibble = 7;
  template <uint32_t W> using EncShared = rpk::EncShared<W>;
  using DecShared = rpk::DecShared;

  template <uint32_t W, bool STORE>
  static constexpr auto compress_segment = &rpk::compress_segment<W>;  // (STORE alone)

  static __device__ __forceinline__ bool decode_stream(const GMEM uint8_t* src, uint32_t csize,
                                                       uint32_t tag, uint32_t bl, uint32_t L,
                                                       uint32_t seg, GMEM uint8_t* dst,
                                                       DecShared& sh) {
    const uint32_t lg = tag & 7u;
    bool ok = (tag >> 4) == kNibble && lg <= 4u && L <= seg;
    if (ok && (tag & 8u)) {
      ok = bl == 0 && decode_stored(src, csize, L, dst);
    } else if (ok) {
      switch (lg) {
        case 0: ok = rpk::decompress_runs<1>(src, csize, bl, L, dst, sh); break;
        case 1: ok = rpk::decompress_runs<2>(src, csize, bl, L, dst, sh); break;
        case 2: ok = rpk::decompress_runs<4>(src, csize, bl, L, dst, sh); break;
        case 3: ok = rpk::decompress_runs<8>(src, csize, bl, L, dst, sh); break;
        default: ok = rpk::decompress_runs<16>(src, csize, bl, L, dst, sh); break;
      }
    }
    return ok;
  }
};

BITAR_COLUMN_COMPRESS(RunPack, 1, true);
BITAR_COLUMN_COMPRESS(RunPack, 2, true);
BITAR_COLUMN_COMPRESS(RunPack, 4, true);
BITAR_COLUMN_COMPRESS(RunPack, 8, true);
BITAR_COLUMN_COMPRESS(RunPack, 16, true);
BITAR_COLUMN_DECOMPRESS(RunPack, false);
BITAR_COLUMN_DECOMPRESS(RunPack, true);

}  // namespace bitar_hip
