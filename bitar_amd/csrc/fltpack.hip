// fltpack.hip -- FLTPACK: decimal-scaled bit packing of floating-point columns, per segment,
// both directions (gfx950).  No reference counterpart.  A value that is an integer n over 10^e
// is stored as n, packed the way INTPACK packs (a signed reference per block of 256 elements,
// residuals at the bit length of the largest one per miniblock of 64); every other value (NaN,
// infinities, -0.0, denormals, non-decimal fractions) is an exception, kept raw behind the
// payload with its position.
//
// Stream of a segment of L bytes, element width W (4: float, 8: double), m = L / W elements
// (DESIGN.md 4.16):
//   byte 0      0x50 | mode << 2 | log2(W)     mode 0 packed, 2 stored
//   byte 1      e, the decimal exponent, 0..15 (0 in the stored form)
//   bytes 2..3  LE16(L - 1)
//   stored:     L raw bytes
//   packed:     LE16 nx  widths[nmb]  refs[nblk] (W bytes each)  payload  pos[nx] (LE16)
//               val[nx] (W bytes each)  tail
//
// Arithmetic: encode is one multiply, one rint and the conversion to an integer; decode is the
// conversion back and one true division.  Both must give IEEE results (the numpy model is
// compared bit for bit), so this file takes no fast-math flag, no reciprocal multiply and no
// approximate intrinsic.
//
// One wavefront per segment, lane t = element t of the current miniblock.  The encoder passes
// over its segment three times: score the sample (every 16th element, held in 4 KiB of LDS, at
// each of the 16 exponents), plan (references, widths, exceptions, size), emit.  The emit pass
// recomputes n from the input, which by then comes from L2 / Infinity Cache, and does not stash
// it: a stash of a 64 KiB segment's integers takes 64 KiB of LDS, which leaves two one-wave
// workgroups per CU (160 KiB), against the 6 KiB this kernel needs; the recomputation is one
// multiply, one rint and one division per element, hidden behind the loads of the many waves
// that then fit.  The decoder merges the exceptions before it stores: the validated position
// list becomes a bitmap in LDS, a lane whose bit is set takes its value from val[] (its rank
// among the set bits, through mbcnt, plus a running base) in place of the computed one, so every
// element is stored once, by one lane, and nothing has to be waited for.
#include "../../include/bitar_hip.h"
#include "autopack.hip.h"
#include "bitpack.hip.h"

namespace bitar_hip {

namespace fpk {

using namespace ipk;

constexpr uint32_t kMaxMiniF = 256;             // miniblocks of 64 KiB of floats
constexpr uint32_t kMaxSample = 1024;           // every 16th of 16384 floats
constexpr uint32_t kMaxExp = 15;

__device__ const double kPow10[16] = {1e0, 1e1, 1e2,  1e3,  1e4,  1e5,  1e6,  1e7,
                                      1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};

template <uint32_t W>
__device__ __forceinline__ double to_double(typename Elem<W>::U bits) {
  if constexpr (W == 8) return __longlong_as_double((long long)bits);
  else return (double)__uint_as_float(bits);
}

// the element that n stands for at the scale P = 10^e
template <uint32_t W>
__device__ __forceinline__ typename Elem<W>::U from_int(typename Elem<W>::S n, double P) {
  const double q = (double)n / P;
  if constexpr (W == 8) return (uint64_t)__double_as_longlong(q);
  else return __float_as_uint((float)q);  // round to nearest even
}

// n of the element `bits` at the scale P; false when the element is not encodable there (its
// decode would not give back exactly these bits)
template <uint32_t W>
__device__ __forceinline__ bool to_int(typename Elem<W>::U bits, double P,
                                       typename Elem<W>::S& n) {
  using S = typename Elem<W>::S;
  constexpr double lim = W == 8 ? 9007199254740992.0 : 2147483647.0;  // 2^53, 2^31 - 1
  const double t = rint(to_double<W>(bits) * P);
  const bool in = fabs(t) <= lim;  // false for NaN and the infinities too
  n = (S)(in ? t : 0.0);           // (converting a value out of range is undefined)
  return in && from_int<W>(n, P) == bits;
}

struct Shared {
  __attribute__((aligned(8))) uint8_t sample[kMaxSample * 4];  // every 16th element
  __attribute__((aligned(8))) uint8_t ref[kMaxMiniF * 2];      // references, W bytes each
  uint8_t wid[kMaxMiniF];                                      // widths
  uint8_t xcnt[kMaxMiniF];                                     // exceptions per miniblock
  uint32_t stage[kStageDwords];                                // one miniblock's bit string
};

// STORE = false is AUTOPACK's candidate form (autopack.hip): a segment that takes the stored form
// writes its size alone -- a later candidate's stored form is never selected, it ties with
// RUNPACK's at best -- and every other segment is written as ever.
template <uint32_t W, bool STORE = true>
__device__ __forceinline__ void compress_segment(const GMEM uint8_t* src, uint32_t L,
                                                 GMEM uint8_t* dst, uint32_t* size_out,
                                                 Shared& sh) {
  using U = typename Elem<W>::U;
  using S = typename Elem<W>::S;
  constexpr uint32_t kLog = W == 4 ? 2 : 3;
  constexpr S top = (S)(~(U)0 >> 1);
  const uint32_t lane = lane_id();
  const uint32_t m = L / W, tail = L - m * W;
  const uint32_t nmb = (m + kMini - 1) / kMini, nblk = (nmb + 3) / 4;

  // ---- score: the cost of every exponent on the sample (elements 0, 16, 32, ...) ------------
  const uint32_t ns = (m + 15) / 16;
  U* samp = reinterpret_cast<U*>(sh.sample);
  for (uint32_t j = lane; j < ns; j += kWave) samp[j] = load_elem<W>(src + (uint64_t)j * 16 * W);
  lds_order();
  uint32_t e = 0, best = ~0u;
  for (uint32_t c = 0; c <= kMaxExp && ns; ++c) {
    const double P = kPow10[c];
    S lo = top, nhi = top;  // the smallest n and the smallest -n of this lane's samples
    uint32_t bad = 0;
    for (uint32_t j0 = 0; j0 < ns; j0 += kWave) {
      const uint32_t j = j0 + lane;
      S n = 0;
      const bool ok = j < ns && to_int<W>(samp[j < ns ? j : 0], P, n);
      bad += (uint32_t)__popcll(ballot(j < ns) & ~ballot(ok));
      if (ok) {
        lo = imin(lo, n);
        nhi = imin(nhi, (S)-n);
      }
    }
    uint32_t b = 0;
    if (bad < ns) {
      const S mn = wave_min<S, U>(lo), mx = (S)-wave_min<S, U>(nhi);
      b = bit_length((U)((U)mx - (U)mn));
    }
    const uint32_t cost = bad * (8 * W + 16) + (ns - bad) * b;
    if (cost < best) {  // (a tie stays with the smaller exponent)
      best = cost;
      e = c;
    }
  }
  const double P = kPow10[e];

  // ---- plan: references, widths, exceptions ---------------------------------------------------
  uint32_t sum = 0, nx = 0;
  for (uint32_t blk = 0; blk < nblk; ++blk) {
    S n[4];
    bool ok[4];
    S lo = top;
    uint64_t any = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t k = blk * 4 + j;
      const uint32_t idx = k * kMini + lane;
      U bits = 0;
      if (idx < m) bits = load_elem<W>(src + (uint64_t)idx * W);
      n[j] = 0;
      ok[j] = idx < m && to_int<W>(bits, P, n[j]);
      if (ok[j]) lo = imin(lo, n[j]);
      const uint64_t good = ballot(ok[j]);
      const uint32_t cnt = (uint32_t)__popcll(ballot(idx < m) & ~good);
      any |= good;
      if (k < nmb) {
        if (lane == 0) sh.xcnt[k] = (uint8_t)cnt;  // (at most 64)
        nx += cnt;
      }
    }
    const U least = (U)wave_min<S, U>(lo);
    const U ref = any ? least : (U)0;  // (a block of exceptions only: 0)
    if (lane == 0) set_lds_ref<W>(sh.ref, blk, ref);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t k = blk * 4 + j;
      const U r = ok[j] ? (U)((U)n[j] - ref) : (U)0;
      const uint32_t b = bit_length(wave_or<U>(r));
      if (k < nmb) {
        if (lane == 0) sh.wid[k] = (uint8_t)b;
        sum += 8u * b;
      }
    }
  }
  lds_order();

  // ---- stored when nothing is gained (m = 0 included) -----------------------------------------
  const uint32_t pay_at = 6u + nmb + nblk * W;
  const uint32_t total = pay_at + sum + nx * (2u + W) + tail;
  if (!(total < 4u + L)) {
    const uint32_t h = 0x50u | 2u << 2 | kLog | (L - 1) << 16;
    if (lane == 0) *size_out = 4u + L;
    if constexpr (STORE) {
      if (lane < 4) dst[lane] = (uint8_t)(h >> (8 * lane));
      wave_copy_global(dst + 4, src, L);
    }
    return;
  }
  const uint64_t h = 0x50u | kLog | e << 8 | (L - 1) << 16 | (uint64_t)nx << 32;
  if (lane < 6) dst[lane] = (uint8_t)(h >> (8 * lane));
  if (lane == 0) *size_out = total;
  for (uint32_t k = lane; k < nmb; k += kWave) dst[6 + k] = sh.wid[k];
  for (uint32_t k = lane; k < nblk * W; k += kWave) dst[6 + nmb + k] = sh.ref[k];

  // ---- emit: the payload as aligned dwords (bitpack.hip.h); the exceptions in position order, -
  // ---- a lane's slot = the exceptions of earlier miniblocks + those of lower lanes            -
  PayloadEmitter<W> emit(dst + pay_at, sh.stage);
  GMEM uint8_t* pos_out = dst + pay_at + sum;
  GMEM uint8_t* val_out = pos_out + 2 * nx;
  uint32_t xbase = 0;
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t b = sh.wid[k], c = sh.xcnt[k];
    if (b == 0 && c == 0) continue;
    const uint32_t idx = k * kMini + lane;
    U bits = 0;
    if (idx < m) bits = load_elem<W>(src + (uint64_t)idx * W);
    S n = 0;
    const bool ok = idx < m && to_int<W>(bits, P, n);
    if (c) {
      const uint64_t bad = ballot(idx < m) & ~ballot(ok);
      if (idx < m && !ok) {
        const uint32_t i = xbase + rank_in(bad);  // < nx
        pos_out[2 * i] = (uint8_t)idx;
        pos_out[2 * i + 1] = (uint8_t)(idx >> 8);
        store_elem<W>(val_out + i * W, bits);
      }
      xbase += c;
    }
    if (b) {
      const U ref = lds_ref<W>(sh.ref, k / 4);
      emit.put(ok ? (U)((U)n - ref) : (U)0, b);
    }
  }
  emit.finish();
  if (lane < tail) val_out[nx * W + lane] = src[m * W + lane];
}

struct DecShared {
  uint8_t wid[kMaxMiniF];
  uint32_t off[kMaxMiniF];   // byte offset of every miniblock in the payload
  uint32_t exc[2 * kMaxMiniF];  // bit p: element p is an exception
};

// the packed form: src holds csize >= 4 bytes, the header's first four bytes are valid and
// L <= seg.  Returns false for a stream that must be rejected (checked before anything is
// written).
template <uint32_t W>
__device__ __forceinline__ bool decompress_packed(const GMEM uint8_t* src, uint32_t csize,
                                                  uint32_t L, uint32_t e, GMEM uint8_t* dst,
                                                  DecShared& sh) {
  using U = typename Elem<W>::U;
  using S = typename Elem<W>::S;
  const uint32_t lane = lane_id();
  const uint32_t m = L / W, tail = L - m * W;
  const uint32_t nmb = (m + kMini - 1) / kMini, nblk = (nmb + 3) / 4;
  if (csize < 6) return false;
  const uint32_t nx = src[4] | (uint32_t)src[5] << 8;
  if (nx > m) return false;
  const uint32_t wid_at = 6, ref_at = wid_at + nmb, pay_at = ref_at + nblk * W;
  const uint32_t after = nx * (2u + W) + tail;  // what follows the payload
  if (csize < pay_at + after) return false;     // (so the header arrays lie inside the stream)

  // widths -> offsets; the stream's size must be exactly what they add up to
  uint32_t run = 0;
  bool bad = false;
  for (uint32_t k0 = 0; k0 < nmb; k0 += kWave) {
    const uint32_t k = k0 + lane;
    const uint32_t b = k < nmb ? src[wid_at + k] : 0u;
    bad = bad || b > 8 * W;
    const uint32_t incl = wave_incl_sum(8u * b);
    if (k < nmb) {
      sh.wid[k] = (uint8_t)b;
      sh.off[k] = run + incl - 8u * b;
      sh.exc[2 * k] = 0;
      sh.exc[2 * k + 1] = 0;
    }
    run += readlane(incl, 63);
  }
  if (ballot(bad) != 0) return false;  // (each width <= 64: run <= 64 KiB * 8, no overflow)
  if (pay_at + run + after != csize) return false;
  lds_order();

  // positions: each below m and above the one before (chunks of 64, neighbours across lanes)
  const uint32_t pos_at = pay_at + run, val_at = pos_at + 2 * nx;
  if (!mark_positions(src + pos_at, nx, m, sh.exc)) return false;
  lds_order();

  const double P = kPow10[e];
  const GMEM uint8_t* pay = src + pay_at;
  uint32_t xi = 0;  // exceptions of the miniblocks before this one
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t b = sh.wid[k];
    const uint32_t idx = k * kMini + lane;
    U r = 0;
    if (b) r = extract_field<W>(pay + sh.off[k], b);
    const U ref = load_elem<W>(src + ref_at + (k / 4) * W);
    U v = from_int<W>((S)(U)(r + ref), P);
    const uint64_t mask = exception_mask(sh.exc, k);
    if (mask) {
      if ((mask >> lane) & 1u) v = load_elem<W>(src + val_at + (xi + rank_in(mask)) * W);
      xi += (uint32_t)__popcll(mask);
    }
    if (idx < m) store_elem<W>(dst + (uint64_t)idx * W, v);
  }
  if (lane < tail) dst[m * W + lane] = src[val_at + nx * W + lane];
  return true;
}

}  // namespace fpk

// FLTPACK as the shared kernels see it (autopack.hip.h).  Slots have any alignment.
struct FltPack {
  static constexpr uint32_t kNibble = 5;
  template <uint32_t W> using EncShared = fpk::Shared;
  using DecShared = fpk::DecShared;

  template <uint32_t W, bool STORE>
  static constexpr auto compress_segment = &fpk::compress_segment<W, STORE>;

  static __device__ __forceinline__ bool decode_stream(const GMEM uint8_t* src, uint32_t csize,
                                                       uint32_t tag, uint32_t e, uint32_t L,
                                                       uint32_t seg, GMEM uint8_t* dst,
                                                       DecShared& sh) {
    const uint32_t mode = (tag >> 2) & 3u, lg = tag & 3u;
    bool ok = (tag >> 4) == kNibble && (mode == 0u || mode == 2u) && lg >= 2u &&
              e <= fpk::kMaxExp && L <= seg;
    if (ok && mode == 2) {
      ok = e == 0 && decode_stored(src, csize, L, dst);
    } else if (ok) {
      ok = lg == 2 ? fpk::decompress_packed<4>(src, csize, L, e, dst, sh)
                   : fpk::decompress_packed<8>(src, csize, L, e, dst, sh);
    }
    return ok;
  }
};

BITAR_COLUMN_COMPRESS(FltPack, 4, true);
BITAR_COLUMN_COMPRESS(FltPack, 8, true);
BITAR_COLUMN_COMPRESS(FltPack, 4, false);
BITAR_COLUMN_COMPRESS(FltPack, 8, false);
BITAR_COLUMN_DECOMPRESS(FltPack, false);
BITAR_COLUMN_DECOMPRESS(FltPack, true);

}  // namespace bitar_hip
