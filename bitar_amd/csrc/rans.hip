// rans.hip -- RANS: an order-0 rANS entropy coder with 64 interleaved states, one per lane, for
// byte segments whose gain is their histogram and not their repeats (shuffled floats, embeddings,
// noisy sensor words, residuals), both directions (gfx950).  No reference counterpart.
//
// Stream of a segment of L bytes (tests/rans_model.py restates it in numpy):
//   byte 0      0xA0 | mode                     mode 0 rans, 1 stored
//   byte 1      0
//   bytes 2..3  LE16(L - 1)
//   stored:     L raw bytes                                                  size = 4 + L
//   rans:       bitmap[32]  freqs[tsize]  words[nw] (LE16)  states[64] (LE32)
//               size = 36 + tsize + 2*nw + 256,  tsize = 2 * ceil(12 * nsym / 16)
// Frequencies sum to 4096: f = 1 + floor(c * (4096 - nsym) / L), the deficit to the most frequent
// symbol.  Symbol i is lane i % 64's at step i / 64; the encoder runs the steps backward from
// states of 2^16, a lane emits its low 16 bits when x >= f << 20, and a step's words are stored in
// lane order; the decoder runs forward and refills, from the end of `words`, the lanes that fell
// below 2^16.  The rans form is taken when its size is strictly below 4 + L.
//
// One wavefront per segment, one launch each way, no scratch in HBM.  The kernels are the column
// codecs' (autopack.hip.h) with this format's traits: the element width is always 1.
#include "../../include/bitar_hip.h"
#include "rans.hip.h"

namespace bitar_hip {

namespace rans {

constexpr uint32_t kFixed = 36u + 256u;  // header, bitmap and states

// ---- encoder --------------------------------------------------------------------------------
struct EncShared {
  union {
    __attribute__((aligned(16))) uint32_t hist[kCopies * kRow];
    __attribute__((aligned(16))) uint32_t head[(36 + 384) / 4];  // header, bitmap and freqs
  };
  // per symbol: .x = f | cum << 16, .y = floor((2^32 - 1) / f)
  __attribute__((aligned(8))) uint2 tab[256];
  uint16_t ring[kRing];  // emitted words not yet stored, word k at k % kRing
};

__device__ __forceinline__ void store_segment(const GMEM uint8_t* src, uint32_t L, GMEM uint8_t* dst,
                                              uint32_t* size_out) {
  if (lane_id() == 0) {
    dst[0] = 0xA1;
    dst[1] = 0;
    dst[2] = (uint8_t)(L - 1);
    dst[3] = (uint8_t)((L - 1) >> 8);
    *size_out = 4u + L;
  }
  wave_copy_global(dst + 4, src, L);
}

__device__ __forceinline__ void compress_segment(const GMEM uint8_t* src, uint32_t L,
                                                 GMEM uint8_t* dst, uint32_t* size_out,
                                                 EncShared& sh) {
  const uint32_t lane = lane_id();
  // (no rans form is smaller than one symbol's table and the states)
  if (kFixed + 2u >= 4u + L) return store_segment(src, L, dst, size_out);

  // ---- histogram: aligned dwords of the segment, the bytes outside it masked --------------
  for (uint32_t k = lane; k < kCopies * kRow / 4; k += kWave)
    reinterpret_cast<uint4*>(sh.hist)[k] = make_uint4(0, 0, 0, 0);
  lds_order();
  {
    const uint32_t mis = (uint32_t)((uintptr_t)src & 3u);
    const GMEM uint32_t* words = reinterpret_cast<const GMEM uint32_t*>(src - mis);
    const uint32_t nd = (mis + L + 3u) >> 2;
    uint32_t* mine = sh.hist + (lane & (kCopies - 1)) * kRow;
    // dword d holds the segment's bytes 4d - mis + j.  A block of kBatch x 64 dwords is loaded
    // before any of it is counted, and a block of interior dwords takes no compare
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
          count(mine, v[j] & 255u);
          count(mine, v[j] >> 8 & 255u);
          count(mine, v[j] >> 16 & 255u);
          count(mine, v[j] >> 24);
        }
      } else {
#pragma unroll
        for (uint32_t j = 0; j < kBatch; ++j) {
          const uint32_t at = 4u * (base + j * kWave + lane) - mis;  // (past L where d >= nd)
#pragma unroll
          for (uint32_t k = 0; k < 4; ++k)
            if (at + k < L) count(mine, v[j] >> (8 * k) & 255u);
        }
      }
    }
  }
  lds_order();

  // ---- normalisation: lane t has the symbols 4t .. 4t + 3 -----------------------------------
  uint32_t c[4] = {0, 0, 0, 0};
#pragma unroll
  for (uint32_t k = 0; k < kCopies; ++k) {
    const uint2 v = *reinterpret_cast<const uint2*>(sh.hist + k * kRow + 2 * lane);
    c[0] += v.x & 0xFFFFu;
    c[1] += v.x >> 16;
    c[2] += v.y & 0xFFFFu;
    c[3] += v.y >> 16;
  }
  lds_order();  // (head shares the histogram's LDS)
  uint32_t here = 0, best = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    here += c[k] != 0;
    // the most frequent, the lowest value on a tie (a count is at most 2^16)
    best = max(best, c[k] << 8 | (255u - (4 * lane + k)));
  }
  const uint32_t rank_incl = wave_incl_sum(here);
  const uint32_t nsym = readlane(rank_incl, 63);
  const uint32_t top = 255u - (readlane(wave_incl_max(best), 63) & 255u);
  uint32_t f[4], fsum = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    f[k] = c[k] ? 1u + c[k] * (kScale - nsym) / L : 0u;  // (the product is below 2^28)
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

  const uint32_t tsize = table_size(nsym);
  const uint32_t words_at = 36u + tsize;
  if (words_at + 256u >= 4u + L) return store_segment(src, L, dst, size_out);

  // ---- header, bitmap and freqs, staged in LDS ----------------------------------------------
  for (uint32_t k = lane; k < (36 + 384) / 4; k += kWave) sh.head[k] = 0;
  lds_order();
  if (lane == 0) sh.head[0] = 0xA0u | (L - 1) << 16;
  {
    uint32_t k12 = 12u * (rank_incl - here);  // the bit of this lane's first present symbol
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      sh.tab[4 * lane + k] = make_uint2(f[k] | cum << 16, f[k] ? 0xFFFFFFFFu / f[k] : 0u);
      cum += f[k];
      if (f[k]) {
        bits |= 1u << k;
        const uint32_t at = 36u * 8u + k12, sft = at & 31u;
        atomicOr(&sh.head[at >> 5], (f[k] - 1u) << sft);
        if (sft > 20u) atomicOr(&sh.head[(at >> 5) + 1], (f[k] - 1u) >> (32u - sft));
        k12 += 12u;
      }
    }
    // bitmap byte b holds the symbols of lanes 2b and 2b + 1
    atomicOr(&sh.head[1 + (lane >> 3)], bits << (4u * (lane & 7u)));
  }
  lds_order();
  for (uint32_t k = lane; k < words_at; k += kWave)
    dst[k] = reinterpret_cast<const uint8_t*>(sh.head)[k];

  // ---- the coder: steps T - 1 .. 0, words placed by the ballot's prefix ----------------------
  // the largest nw whose rans form is still strictly below 4 + L
  const uint32_t max_words = (4u + L - 1u - words_at - 256u) >> 1;
  GMEM uint8_t* wp = dst + words_at;
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
      const uint2 e = sh.tab[cur[j]];
      const uint32_t fs = e.x & 0xFFFFu;
      // x >= f << 20 without the wrap at f = 4096 (x >> 20 is below 4096: that lane never emits)
      const bool emit = act && (x >> 20) >= fs;
      const uint64_t mask = ballot(emit);
      const uint32_t nq = q + (uint32_t)__builtin_popcountll(mask);
      if (BITAR_RARE(nq > max_words)) return store_segment(src, L, dst, size_out);
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
      // so mulhi(x, m) is the quotient or one below it
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
struct DecShared {
  __attribute__((aligned(16))) uint32_t sym[kScale / 4];  // slot -> symbol, a byte each
  uint32_t tab[256];                                       // symbol -> f | cum << 16
  uint16_t ring[kRing];                                    // word k at k % kRing
};

__device__ __forceinline__ bool decompress_rans(const GMEM uint8_t* src, uint32_t csize, uint32_t L,
                                                GMEM uint8_t* dst, DecShared& sh) {
  const uint32_t lane = lane_id();
  if (csize < kFixed + 2u) return false;
  // ---- the table: lane t has the symbols 4t .. 4t + 3 ---------------------------------------
  const uint32_t bits = src[4u + (lane >> 1)] >> (4u * (lane & 1u)) & 15u;
  const uint32_t here = (uint32_t)__builtin_popcount(bits);
  const uint32_t rank_incl = wave_incl_sum(here);
  const uint32_t nsym = readlane(rank_incl, 63);
  if (nsym == 0) return false;
  const uint32_t tsize = table_size(nsym);
  if (csize < kFixed + tsize || ((csize - kFixed - tsize) & 1u)) return false;
  const uint32_t nw = (csize - kFixed - tsize) >> 1;
  const GMEM uint8_t* freqs = src + 36;
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
  if (readlane(cum_incl, 63) != kScale) return false;
  const GMEM uint8_t* words = src + 36 + tsize;
  uint32_t x = ld32(words + 2u * nw + 4u * lane);
  if (ballot(x < kX0)) return false;

  // slot -> symbol: every symbol marks its first slot, then a running maximum along the slots
  // (symbols ascend with their slots); lane t scans the slots 64t .. 64t + 63
  for (uint32_t k = lane; k < kScale / 16; k += kWave)
    reinterpret_cast<uint4*>(sh.sym)[k] = make_uint4(0, 0, 0, 0);
  lds_order();
  {
    uint32_t cum = cum_incl - fsum;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      sh.tab[4 * lane + k] = f[k] | cum << 16;
      if (f[k]) reinterpret_cast<uint8_t*>(sh.sym)[cum] = (uint8_t)(4 * lane + k);
      cum += f[k];
    }
  }
  lds_order();
  {
    uint32_t w[16];
    uint32_t top = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint4 v = reinterpret_cast<const uint4*>(sh.sym)[4 * lane + k];
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
      reinterpret_cast<uint4*>(sh.sym)[4 * lane + k] =
          make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
  }
  lds_order();

  // ---- the coder: steps 0 .. T - 1, refills read backward from the end of `words` ----------
  // The words [lo, p) not yet used are in the LDS ring, at least min(64, p) of them before every
  // step: a refill waits for LDS alone, and the ring is filled 448 words at a time.
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
      const uint32_t s = reinterpret_cast<const uint8_t*>(sh.sym)[slot];
      const uint32_t e = sh.tab[s];
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

}  // namespace rans

// The codec as the column kernels see it: one "width", the storing form alone.  The encoder
// writes nothing past 4 + L bytes of its slot (a rans form is left for the stored one before its
// words reach that size); the decoder writes nothing outside the segment's first L bytes.
struct Rans {
  static constexpr uint32_t kNibble = 0xA;
  template <uint32_t W> using EncShared = rans::EncShared;
  using DecShared = rans::DecShared;

  template <uint32_t W, bool STORE>
  static constexpr auto compress_segment = &rans::compress_segment;

  static __device__ __forceinline__ bool decode_stream(const GMEM uint8_t* src, uint32_t csize,
                                                       uint32_t tag, uint32_t byte1, uint32_t L,
                                                       uint32_t seg, GMEM uint8_t* dst,
                                                       DecShared& sh) {
    if ((tag >> 4) != kNibble || (tag & 15u) > 1u || byte1 != 0 || L > seg) return false;
    if (tag & 1u) return decode_stored(src, csize, L, dst);
    return rans::decompress_rans(src, csize, L, dst, sh);
  }
};

BITAR_COLUMN_COMPRESS(Rans, 1, true);
BITAR_COLUMN_DECOMPRESS(Rans, false);

}  // namespace bitar_hip
