// ransplane.hip -- RANSPLANE: RANS (rans.hip) with one order-0 table per byte plane of an element
// of W = 2, 4 or 8 bytes, for float and integer columns whose byte planes have different
// histograms (a float's exponent byte against its low mantissa bytes), both directions (gfx950).
// No filter pass: 64 is a multiple of W, so lane t codes plane t % W for the whole segment and
// the input is read contiguously.  No reference counterpart.
//
// Stream of a segment of L bytes (tests/ransplane_model.py restates it in numpy):
//   byte 0      0xB0 | mode << 3 | lg           mode 0 planes, 1 stored; W = 1 << lg
//   byte 1      0
//   bytes 2..3  LE16(L - 1)
//   stored:     L raw bytes                                                  size = 4 + L
//   planes:     bitmaps[W][32]  freqs of plane 0 .. W - 1 (tsize_p bytes each)
//               words[nw] (LE16)  states[64] (LE32)
//               size = 4 + 32 W + sum(tsize_p) + 2*nw + 256,  tsize_p = 2 * ceil(12 * nsym_p / 16)
// Plane p holds the bytes i < L with i % W == p, n_p of them; its frequencies are RANS's over
// those: f = 1 + floor(c * (4096 - nsym_p) / n_p), the deficit to the plane's most frequent
// symbol.  The coder is RANS's with the f and cum of plane i % W for symbol i.  The planes form is
// taken when L >= W and its size is strictly below 4 + L.
//
// One wavefront per segment, one launch each way, no scratch in HBM.  The kernels are the column
// codecs' (autopack.hip.h); the decoder has one traits type per width, so that its LDS is the
// width's own and an id decodes its own width alone.
#include "../../include/bitar_hip.h"
#include "rans.hip.h"

namespace bitar_hip {

namespace ransplane {

using namespace rans;

constexpr uint32_t kNibble = 0xB;

template <uint32_t W>
struct Width {
  static_assert(W == 2 || W == 4 || W == 8, "element widths of 2, 4 and 8 bytes");
  static constexpr uint32_t kLg = W == 2 ? 1 : W == 4 ? 2 : 3;
  static constexpr uint32_t kTables = 4u + 32u * W;         // where the first freqs field starts
  static constexpr uint32_t kFixed = kTables + 256u;        // header, bitmaps and states
  static constexpr uint32_t kHead = kTables + 384u * W;     // header, bitmaps and freqs at most
  static constexpr uint32_t kPlaneCopies = kCopies / W;     // private histograms of one plane
};

// ---- encoder --------------------------------------------------------------------------------
template <uint32_t W>
struct EncShared {
  union {
    // copy c of plane p is row p * (16 / W) + c
    __attribute__((aligned(16))) uint32_t hist[kCopies * kRow];
    __attribute__((aligned(16))) uint32_t head[(Width<W>::kHead + 3) / 4];
  };
  // per plane and symbol: .x = f | cum << 16, .y = floor((2^32 - 1) / f)
  __attribute__((aligned(8))) uint2 tab[W * 256];
  uint16_t ring[kRing];  // emitted words not yet stored, word k at k % kRing
};
static_assert(sizeof(uint32_t) * kCopies * kRow >= Width<8>::kHead, "head fits the histograms' LDS");

template <uint32_t W>
__device__ __forceinline__ void store_segment(const GMEM uint8_t* src, uint32_t L, GMEM uint8_t* dst,
                                              uint32_t* size_out) {
  if (lane_id() == 0) {
    dst[0] = (uint8_t)(kNibble << 4 | 8u | Width<W>::kLg);
    dst[1] = 0;
    dst[2] = (uint8_t)(L - 1);
    dst[3] = (uint8_t)((L - 1) >> 8);
    *size_out = 4u + L;
  }
  wave_copy_global(dst + 4, src, L);
}

template <uint32_t W>
__device__ __forceinline__ void compress_segment(const GMEM uint8_t* src, uint32_t L,
                                                 GMEM uint8_t* dst, uint32_t* size_out,
                                                 EncShared<W>& sh) {
  using Wd = Width<W>;
  const uint32_t lane = lane_id();
  // (no planes form is smaller than one symbol's table a plane and the states; and L >= W here)
  if (Wd::kFixed + 2u * W >= 4u + L) return store_segment<W>(src, L, dst, size_out);

  // ---- histograms: aligned dwords of the segment, the bytes outside it masked ---------------
  for (uint32_t k = lane; k < kCopies * kRow / 4; k += kWave)
    reinterpret_cast<uint4*>(sh.hist)[k] = make_uint4(0, 0, 0, 0);
  lds_order();
  {
    const uint32_t mis = (uint32_t)((uintptr_t)src & 3u);
    const GMEM uint32_t* words = reinterpret_cast<const GMEM uint32_t*>(src - mis);
    const uint32_t nd = (mis + L + 3u) >> 2;
    // dword d holds the segment's bytes 4d - mis + j, of plane (4d - mis + j) % W.  Every dword
    // of this lane has the lane's parity (a block is 512 dwords), so the plane of its byte j is
    // (4 lane + j - mis) % W whatever d is.  A plane's copies take 4 W lanes each: for W = 8 the
    // lanes of one parity, which alone count into the plane at a byte position, are split by
    // the lane's bit 1.
    const uint32_t copy = W == 8 ? (lane >> 1 & 1u) : (lane & (Wd::kPlaneCopies - 1));
    uint32_t* mine[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
      mine[j] = sh.hist + (((4u * lane + j + W - mis) & (W - 1)) * Wd::kPlaneCopies + copy) * kRow;
    const uint32_t inner_end = (mis + L) >> 2;  // dwords [1, inner_end) lie inside whatever mis is
    for (uint32_t base = 0; base < nd; base += kBatch * kWave) {
      uint32_t v[kBatch];
#pragma unroll
      for (uint32_t j = 0; j < kBatch; ++j) {
        const uint32_t d = base + j * kWave + lane;
        v[j] = d < nd ? words[d] : 0u;
      }
      if (base >= 1 && base + kBatch * kWave <= inner_end) {
#pragma unroll
        for (uint32_t j = 0; j < kBatch; ++j) {
          count(mine[0], v[j] & 255u);
          count(mine[1], v[j] >> 8 & 255u);
          count(mine[2], v[j] >> 16 & 255u);
          count(mine[3], v[j] >> 24);
        }
      } else {
#pragma unroll
        for (uint32_t j = 0; j < kBatch; ++j) {
          const uint32_t at = 4u * (base + j * kWave + lane) - mis;  // (past L where d >= nd)
#pragma unroll
          for (uint32_t k = 0; k < 4; ++k)
            if (at + k < L) count(mine[k], v[j] >> (8 * k) & 255u);
        }
      }
    }
  }
  lds_order();

  // ---- the planes' counts: lane t has the symbols 4t .. 4t + 3 of each ----------------------
  uint32_t c[W][4];
#pragma unroll
  for (uint32_t p = 0; p < W; ++p) {
    c[p][0] = c[p][1] = c[p][2] = c[p][3] = 0;
#pragma unroll
    for (uint32_t k = 0; k < Wd::kPlaneCopies; ++k) {
      const uint2 v =
          *reinterpret_cast<const uint2*>(sh.hist + (p * Wd::kPlaneCopies + k) * kRow + 2 * lane);
      c[p][0] += v.x & 0xFFFFu;
      c[p][1] += v.x >> 16;
      c[p][2] += v.y & 0xFFFFu;
      c[p][3] += v.y >> 16;
    }
  }
  lds_order();  // (head shares the histograms' LDS)
  for (uint32_t k = lane; k < (Wd::kHead + 3) / 4; k += kWave) sh.head[k] = 0;
  lds_order();
  if (lane == 0) sh.head[0] = (kNibble << 4 | Wd::kLg) | (L - 1) << 16;

  // ---- normalisation and tables, RANS's a plane ---------------------------------------------
  uint32_t words_at = Wd::kTables;  // where plane p's freqs field starts; the words' in the end
#pragma unroll
  for (uint32_t p = 0; p < W; ++p) {
    const uint32_t np = (L - p + W - 1) / W;  // the plane's bytes (L > p)
    uint32_t here = 0, best = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      here += c[p][k] != 0;
      // the most frequent, the lowest value on a tie (a count is at most 2^16)
      best = max(best, c[p][k] << 8 | (255u - (4 * lane + k)));
    }
    const uint32_t rank_incl = wave_incl_sum(here);
    const uint32_t nsym = readlane(rank_incl, 63);
    const uint32_t top = 255u - (readlane(wave_incl_max(best), 63) & 255u);
    uint32_t f[4], fsum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      f[k] = c[p][k] ? 1u + c[p][k] * (kScale - nsym) / np : 0u;  // (the product is below 2^28)
      fsum += f[k];
    }
    const uint32_t deficit = kScale - wave_sum(fsum);
    if (lane == top >> 2) {
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k)
        if (k == (top & 3u)) f[k] += deficit;
    }
    fsum = f[0] + f[1] + f[2] + f[3];
    uint32_t cum = wave_incl_sum(fsum) - fsum;
    uint32_t k12 = 8u * words_at + 12u * (rank_incl - here);  // the bit of this lane's first f
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      sh.tab[p * 256 + 4 * lane + k] = make_uint2(f[k] | cum << 16, f[k] ? 0xFFFFFFFFu / f[k] : 0u);
      cum += f[k];
      if (f[k]) {
        bits |= 1u << k;
        const uint32_t sft = k12 & 31u;
        atomicOr(&sh.head[k12 >> 5], (f[k] - 1u) << sft);
        if (sft > 20u) atomicOr(&sh.head[(k12 >> 5) + 1], (f[k] - 1u) >> (32u - sft));
        k12 += 12u;
      }
    }
    // byte b of the plane's bitmap holds the symbols of lanes 2b and 2b + 1
    atomicOr(&sh.head[1 + 8 * p + (lane >> 3)], bits << (4u * (lane & 7u)));
    words_at += table_size(nsym);
  }
  if (words_at + 256u >= 4u + L) return store_segment<W>(src, L, dst, size_out);
  lds_order();
  for (uint32_t k = lane; k < words_at; k += kWave)
    dst[k] = reinterpret_cast<const uint8_t*>(sh.head)[k];

  // ---- the coder: steps T - 1 .. 0, words placed by the ballot's prefix ----------------------
  // the largest nw whose planes form is still strictly below 4 + L
  const uint32_t max_words = (4u + L - 1u - words_at - 256u) >> 1;
  GMEM uint8_t* wp = dst + words_at;
  const uint2* tab = sh.tab + (lane & (W - 1)) * 256;  // the table of this lane's plane
  uint32_t x = kX0, q = 0, stored = 0;  // words emitted, and those of them in the slot
  // the symbols of kGroup steps are loaded together, a group ahead of the one being coded: a
  // step then waits for no load of its own
  const uint32_t T = (L + kWave - 1) / kWave;
  auto load_group = [&](uint32_t g, uint32_t (&sy)[kGroup]) {
#pragma unroll
    for (uint32_t j = 0; j < kGroup; ++j) {
      const uint32_t i = (g * kGroup + j) * kWave + lane;
      sy[j] = i < L ? src[i] : 0u;
    }
  };
  uint32_t cur[kGroup], nxt[kGroup];
  uint32_t g = (T + kGroup - 1) / kGroup;
  load_group(g - 1, cur);
  while (g-- > 0) {
    if (g) load_group(g - 1, nxt);
#pragma unroll
    for (uint32_t j = kGroup; j-- > 0;) {
      const uint32_t t = g * kGroup + j;
      if (t >= T) continue;  // (the last group alone)
      const bool act = t * kWave + lane < L;
      const uint2 e = tab[cur[j]];
      const uint32_t fs = e.x & 0xFFFFu;
      // x >= f << 20 without the wrap at f = 4096 (x >> 20 is below 4096: that lane never emits)
      const bool emit = act && (x >> 20) >= fs;
      const uint64_t mask = ballot(emit);
      const uint32_t nq = q + (uint32_t)__builtin_popcountll(mask);
      if (BITAR_RARE(nq > max_words)) return store_segment<W>(src, L, dst, size_out);
      if (emit) {
        sh.ring[(q + lanes_below(mask)) & (kRing - 1u)] = (uint16_t)x;
        x >>= 16;
      }
      q = nq;
      // the words go to the slot kRing - 64 at a time: a step waits for no store of its own
      if (BITAR_RARE(q - stored >= kRing - kWave)) {
        lds_order();
#pragma unroll
        for (uint32_t k = 0; k < (kRing - kWave) / kWave; ++k) {
          const uint32_t at = stored + k * kWave + lane;
          st16(wp + 2u * at, sh.ring[at & (kRing - 1u)]);
        }
        stored += kRing - kWave;
        lds_order();
      }
      // x / f from the symbol's reciprocal m = floor((2^32 - 1) / f): 2^32/f - 1 <= m <= 2^32/f,
      // so mulhi(x, m) is the quotient or one below it.  (An inactive lane's symbol 0 may be
      // absent from its plane: f = 0 there, and nothing of the lane's is kept.)
      uint32_t d = __umulhi(x, e.y);
      uint32_t r = x - d * fs;
      if (r >= fs) {
        ++d;
        r -= fs;
      }
      if (act) x = (d << kScaleBits) + r + (e.x >> 16);
    }
#pragma unroll
    for (uint32_t j = 0; j < kGroup; ++j) cur[j] = nxt[j];
  }
  lds_order();
  for (uint32_t at = stored + lane; at < q; at += kWave)
    st16(wp + 2u * at, sh.ring[at & (kRing - 1u)]);
  st32(wp + 2u * q + 4u * lane, x);
  if (lane == 0) *size_out = words_at + 2u * q + 256u;
}

// ---- decoder --------------------------------------------------------------------------------
template <uint32_t W>
struct DecShared {
  __attribute__((aligned(16))) uint32_t sym[W * kScale / 4];  // plane, slot -> symbol, a byte each
  uint32_t tab[W * 256];                                       // plane, symbol -> f | cum << 16
  uint16_t ring[kRing];                                        // word k at k % kRing
};

// the symbols 4 lane .. 4 lane + 3 that plane p's bitmap has, as 4 bits
__device__ __forceinline__ uint32_t plane_bits(const GMEM uint8_t* src, uint32_t p, uint32_t lane) {
  return src[4u + 32u * p + (lane >> 1)] >> (4u * (lane & 1u)) & 15u;
}

template <uint32_t W>
__device__ __forceinline__ bool decompress_planes(const GMEM uint8_t* src, uint32_t csize,
                                                  uint32_t L, GMEM uint8_t* dst,
                                                  DecShared<W>& sh) {
  using Wd = Width<W>;
  const uint32_t lane = lane_id();
  if (L < W || csize < Wd::kFixed + 2u * W) return false;
  // ---- the sizes of the freqs fields, from the bitmaps ---------------------------------------
  uint32_t tables = 0;
  for (uint32_t p = 0; p < W; ++p) {
    const uint32_t nsym = wave_sum((uint32_t)__builtin_popcount(plane_bits(src, p, lane)));
    if (nsym == 0) return false;
    tables += table_size(nsym);
  }
  if (csize < Wd::kFixed + tables || ((csize - Wd::kFixed - tables) & 1u)) return false;
  const uint32_t nw = (csize - Wd::kFixed - tables) >> 1;
  const GMEM uint8_t* words = src + Wd::kTables + tables;
  uint32_t x = ld32(words + 2u * nw + 4u * lane);
  if (ballot(x < kX0)) return false;

  // ---- a plane's tables: lane t has the symbols 4t .. 4t + 3 ---------------------------------
  const GMEM uint8_t* freqs = src + Wd::kTables;
  for (uint32_t p = 0; p < W; ++p) {
    const uint32_t bits = plane_bits(src, p, lane);
    const uint32_t here = (uint32_t)__builtin_popcount(bits);
    const uint32_t rank_incl = wave_incl_sum(here);
    const uint32_t nsym = readlane(rank_incl, 63);
    const uint32_t tsize = table_size(nsym);
    // the bits of `freqs` past the last frequency, in its last 16-bit word
    const uint32_t pad = (16u - (12u * nsym & 15u)) & 15u;
    if (pad && (ld16(freqs + tsize - 2) >> (16u - pad))) return false;
    uint32_t f[4], fsum = 0;
    {
      uint32_t k12 = 12u * (rank_incl - here);
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        f[k] = 0;
        if (bits >> k & 1u) {
          f[k] = 1u + (ld16(freqs + (k12 >> 3)) >> (k12 & 7u) & 0xFFFu);
          k12 += 12u;
        }
        fsum += f[k];
      }
    }
    const uint32_t cum_incl = wave_incl_sum(fsum);
    if (readlane(cum_incl, 63) != kScale) return false;  // (so every cum below is under 4096)
    freqs += tsize;

    // slot -> symbol: every symbol marks its first slot, then a running maximum along the slots
    // (symbols ascend with their slots); lane t scans the slots 64t .. 64t + 63
    uint32_t* sym = sh.sym + p * (kScale / 4);
    for (uint32_t k = lane; k < kScale / 16; k += kWave)
      reinterpret_cast<uint4*>(sym)[k] = make_uint4(0, 0, 0, 0);
    lds_order();
    {
      uint32_t cum = cum_incl - fsum;
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        sh.tab[p * 256 + 4 * lane + k] = f[k] | cum << 16;
        if (f[k]) reinterpret_cast<uint8_t*>(sym)[cum] = (uint8_t)(4 * lane + k);
        cum += f[k];
      }
    }
    lds_order();
    {
      uint32_t w[16];
      uint32_t top = 0;
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        const uint4 v = reinterpret_cast<const uint4*>(sym)[4 * lane + k];
        w[4 * k] = v.x;
        w[4 * k + 1] = v.y;
        w[4 * k + 2] = v.z;
        w[4 * k + 3] = v.w;
      }
#pragma unroll
      for (uint32_t k = 0; k < 16; ++k)
        top = max(max(top, w[k] & 255u), max(max(w[k] >> 8 & 255u, w[k] >> 16 & 255u), w[k] >> 24));
      uint32_t m = wave_shr1(wave_incl_max(top));  // the last symbol marked before this lane's slots
#pragma unroll
      for (uint32_t k = 0; k < 16; ++k) {
        uint32_t o = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          m = max(m, w[k] >> (8 * j) & 255u);
          o |= m << (8 * j);
        }
        w[k] = o;
      }
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k)
        reinterpret_cast<uint4*>(sym)[4 * lane + k] =
            make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    }
    lds_order();
  }

  // ---- the coder: steps 0 .. T - 1, refills read backward from the end of `words` ----------
  // The words [lo, p) not yet used are in the LDS ring, at least min(64, p) of them before every
  // step: a refill waits for LDS alone, and the ring is filled 448 words at a time.
  const uint8_t* sym = reinterpret_cast<const uint8_t*>(sh.sym) + (lane & (W - 1)) * kScale;
  const uint32_t* tab = sh.tab + (lane & (W - 1)) * 256;
  uint32_t p = nw, lo = nw;
  const uint32_t T = (L + kWave - 1) / kWave;
  for (uint32_t t = 0; t < T; ++t) {
    if (BITAR_RARE(p - lo < kWave && lo > 0)) {
      constexpr uint32_t kFill = kRing - kWave;
      const uint32_t from = lo > kFill ? lo - kFill : 0u;
      uint32_t v[kFill / kWave];
#pragma unroll
      for (uint32_t j = 0; j < kFill / kWave; ++j) {
        const uint32_t k = from + j * kWave + lane;
        v[j] = k < lo ? ld16(words + 2u * k) : 0u;
      }
#pragma unroll
      for (uint32_t j = 0; j < kFill / kWave; ++j) {
        const uint32_t k = from + j * kWave + lane;
        if (k < lo) sh.ring[k & (kRing - 1u)] = (uint16_t)v[j];
      }
      lo = from;
      lds_order();
    }
    const uint32_t i = t * kWave + lane;
    if (i < L) {
      const uint32_t slot = x & (kScale - 1u);
      const uint32_t s = sym[slot];
      const uint32_t e = tab[s];
      x = (e & 0xFFFFu) * (x >> kScaleBits) + slot - (e >> 16);
      dst[i] = (uint8_t)s;
    }
    const bool need = x < kX0;
    const uint64_t mask = ballot(need);
    if (mask) {
      const uint32_t n = (uint32_t)__builtin_popcountll(mask);
      if (BITAR_RARE(n > p)) return false;
      p -= n;
      if (need) x = x << 16 | sh.ring[(p + lanes_below(mask)) & (kRing - 1u)];
    }
  }
  // rANS's own check: the decoder lands where the encoder began
  return p == 0 && !ballot(x != kX0);
}

}  // namespace ransplane

// The codec as the column kernels see it.  The encoder writes nothing past 4 + L bytes of its
// slot (a planes form is left for the stored one before its words reach that size); the decoder
// writes nothing outside the segment's first L bytes.
struct RansPlane {
  template <uint32_t W> using EncShared = ransplane::EncShared<W>;

  template <uint32_t W, bool STORE>
  static constexpr auto compress_segment = &ransplane::compress_segment<W>;
};

// The decoder of the id of width W: a stream of another width is rejected, not decoded.
template <uint32_t W>
struct RansPlaneDecoder {
  static constexpr uint32_t kNibble = ransplane::kNibble;
  using DecShared = ransplane::DecShared<W>;

  static __device__ __forceinline__ bool decode_stream(const GMEM uint8_t* src, uint32_t csize,
                                                       uint32_t tag, uint32_t byte1, uint32_t L,
                                                       uint32_t seg, GMEM uint8_t* dst,
                                                       DecShared& sh) {
    if ((tag >> 4) != kNibble || (tag & 7u) != ransplane::Width<W>::kLg || byte1 != 0 || L > seg)
      return false;
    if (tag & 8u) return decode_stored(src, csize, L, dst);
    return ransplane::decompress_planes<W>(src, csize, L, dst, sh);
  }
};

BITAR_COLUMN_COMPRESS(RansPlane, 2, true);
BITAR_COLUMN_COMPRESS(RansPlane, 4, true);
BITAR_COLUMN_COMPRESS(RansPlane, 8, true);
BITAR_COLUMN_DECOMPRESS(RansPlaneDecoder<2>, false);
BITAR_COLUMN_DECOMPRESS(RansPlaneDecoder<4>, false);
BITAR_COLUMN_DECOMPRESS(RansPlaneDecoder<8>, false);

}  // namespace bitar_hip
