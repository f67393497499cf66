// intpack.hip -- INTPACK: frame-of-reference bit packing of integer columns, per segment, both
// directions (gfx950).  No reference counterpart and no match search: one pass finds, for the
// plain values and for their deltas, a signed minimum per block of 256 elements and the bit
// length of the largest residual per miniblock of 64; the smaller of the two forms is emitted.
//
// Stream of a segment of L bytes, element width W, m = L / W elements:
//   byte 0      0x40 | mode << 2 | log2(W)     mode 0 packed, 1 packed with delta, 2 stored
//   byte 1      0
//   bytes 2..3  LE16(L - 1)
//   stored:     L raw bytes
//   packed:     [mode 1: element 0]  widths[nmb]  refs[nblk] (W bytes each)  payload  tail
//               nmb = ceil(m / 64), nblk = ceil(nmb / 4); miniblock k's payload is 8 * widths[k]
//               bytes, element t at bits [t*b, (t+1)*b) of the little-endian bit string
//
// One wavefront per segment, lane t = element t of the current miniblock.  The encoder reads
// its segment twice (plan, then emit): the second read comes from L2 / Infinity Cache, and an
// LDS copy of a 64 KiB segment would leave two waves per CU.  Element and payload addresses
// have any alignment: loads take the aligned dwords that hold a needed byte and realign, the
// payload leaves as aligned dwords with the bytes shared between two miniblocks carried over.
// (Reductions, element loads and stores and the payload emitter: bitpack.hip.h, shared with
// fltpack.hip.)
#include "../../include/bitar_hip.h"
#include "autopack.hip.h"
#include "bitpack.hip.h"

namespace bitar_hip {

namespace ipk {

// the x of this lane's element idx: the element (mode 0) or its difference to the one before
// (mode 1), mod 2^(8W); lanes at or past m get 0
template <uint32_t W>
__device__ __forceinline__ void load_values(const GMEM uint8_t* src, uint32_t idx, uint32_t m,
                                            typename Elem<W>::U& plain, typename Elem<W>::U& delta) {
  using U = typename Elem<W>::U;
  constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
  const uint32_t lane = lane_id();
  U v = 0;
  if (idx < m) v = load_elem<W>(src + (uint64_t)idx * W);
  U prev = dpp<0x138, 0xf>(v, (U)0);  // wave_shr:1
  if (lane == 0 && idx > 0 && idx < m) prev = load_elem<W>(src + (uint64_t)(idx - 1) * W);
  U d = (v - prev) & mask;
  if (idx < kMini) {  // the first miniblock: x_0 = x_1, or 0 when there is no element 1
    const U d1 = (U)__shfl(d, 1);
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

struct Shared {
  uint8_t wid[2][kMaxMini];                                // widths of mode 0 / mode 1
  __attribute__((aligned(8))) uint8_t ref[2][kMaxBlk * 8]; // references, W bytes each
  uint32_t stage[kStageDwords];                            // one miniblock's bit string
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
  constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
  constexpr uint32_t kLog = W == 1 ? 0 : W == 2 ? 1 : W == 4 ? 2 : 3;
  const uint32_t lane = lane_id();
  const uint32_t m = L / W, tail = L - m * W;
  const uint32_t nmb = (m + kMini - 1) / kMini, nblk = (nmb + 3) / 4;

  // ---- plan: both modes' references and widths in one sweep -------------------------------
  uint32_t sum[2] = {0, 0};
  for (uint32_t blk = 0; blk < nblk; ++blk) {
    U x[2][4];
    S lo[2] = {(S)(~(U)0 >> 1), (S)(~(U)0 >> 1)};
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t idx = (blk * 4 + j) * kMini + lane;
      load_values<W>(src, idx, m, x[0][j], x[1][j]);
      if (idx < m) {
        lo[0] = imin(lo[0], as_signed<W>(x[0][j]));
        lo[1] = imin(lo[1], as_signed<W>(x[1][j]));
      }
    }
#pragma unroll
    for (uint32_t md = 0; md < 2; ++md) {
      const U ref = (U)wave_min<S, U>(lo[md]) & mask;
      if (lane == 0) set_lds_ref<W>(sh.ref[md], blk, ref);
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t k = blk * 4 + j;
        const uint32_t idx = k * kMini + lane;
        const U r = idx < m ? (U)((x[md][j] - ref) & mask) : (U)0;
        const uint32_t b = bit_length(wave_or<U>(r));
        if (k < nmb) {
          if (lane == 0) sh.wid[md][k] = (uint8_t)b;
          sum[md] += 8u * b;
        }
      }
    }
  }
  lds_order();

  // ---- mode: delta only when strictly smaller, stored when nothing is gained ---------------
  const uint32_t fixed = 4u + nmb + nblk * W + tail;
  const uint32_t size0 = fixed + sum[0], size1 = fixed + W + sum[1];
  const uint32_t mode = size1 < size0 ? 1u : 0u;
  const uint32_t total = mode ? size1 : size0;
  GMEM uint32_t* head = reinterpret_cast<GMEM uint32_t*>(dst);  // (slots are 16-B aligned)
  if (!(total < 4u + L)) {
    if (lane == 0) {
      if constexpr (STORE) *head = 0x40u | 2u << 2 | kLog | (L - 1) << 16;
      *size_out = 4u + L;
    }
    if constexpr (STORE) wave_copy_global(dst + 4, src, L);
    return;
  }
  if (lane == 0) {
    *head = 0x40u | mode << 2 | kLog | (L - 1) << 16;
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

  // ---- emit: the payload as aligned dwords (bitpack.hip.h) -----------------------------------
  GMEM uint8_t* pay = dst + pos;
  PayloadEmitter<W> emit(pay, sh.stage);
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t b = sh.wid[mode][k];
    if (b == 0) continue;
    const uint32_t idx = k * kMini + lane;
    U xs[2];
    load_values<W>(src, idx, m, xs[0], xs[1]);
    const U ref = lds_ref<W>(sh.ref[mode], k / 4);
    const U r = idx < m ? (U)(((mode ? xs[1] : xs[0]) - ref) & mask) : (U)0;
    emit.put(r, b);
  }
  const uint32_t off = emit.finish();
  if (lane < tail) pay[off + lane] = src[m * W + lane];
}

struct DecShared {
  uint8_t wid[kMaxMini];
  uint32_t off[kMaxMini];  // byte offset of every miniblock in the payload
};

// the packed form: src holds csize bytes, the header is valid and L <= seg.  Returns false for a
// stream that must be rejected (checked before anything is written).
template <uint32_t W>
__device__ __forceinline__ bool decompress_packed(const GMEM uint8_t* src, uint32_t csize,
                                                  uint32_t L, uint32_t mode, GMEM uint8_t* dst,
                                                  DecShared& sh) {
  using U = typename Elem<W>::U;
  constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
  const uint32_t lane = lane_id();
  const uint32_t m = L / W, tail = L - m * W;
  const uint32_t nmb = (m + kMini - 1) / kMini, nblk = (nmb + 3) / 4;
  const uint32_t base_at = 4, wid_at = 4 + (mode ? W : 0), ref_at = wid_at + nmb;
  const uint32_t pay_at = ref_at + nblk * W;
  if (csize < pay_at + tail) return false;  // (so the header arrays lie inside the stream)

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
    }
    run += readlane(incl, 63);
  }
  if (ballot(bad) != 0) return false;  // (each width <= 64: run <= 64 KiB * 8, no overflow)
  if (pay_at + run + tail != csize) return false;
  lds_order();

  const GMEM uint8_t* pay = src + pay_at;
  U carry = 0;
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t b = sh.wid[k];
    const uint32_t idx = k * kMini + lane;
    U r = 0;
    if (b) r = extract_field<W>(pay + sh.off[k], b);
    const U ref = load_elem<W>(src + ref_at + (k / 4) * W);
    U v = (r + ref) & mask;
    if (mode) {
      if (idx == 0) v = load_elem<W>(src + base_at);
      v = wave_incl_add<U>(v) + carry;
      carry = lane63(v);
    }
    if (idx < m) store_elem<W>(dst + (uint64_t)idx * W, v);
  }
  if (lane < tail) dst[m * W + lane] = pay[run + lane];
  return true;
}

}  // namespace ipk

// INTPACK as the shared kernels see it (autopack.hip.h).
struct IntPack {
  static constexpr uint32_t kNibble = 4;
  template <uint32_t W> using EncShared = ipk::Shared;
  using DecShared = ipk::DecShared;

  template <uint32_t W, bool STORE>
  static constexpr auto compress_segment = &ipk::compress_segment<W, STORE>;

  static __device__ __forceinline__ bool decode_stream(const GMEM uint8_t* src, uint32_t csize,
                                                       uint32_t tag, uint32_t rsv, uint32_t L,
                                                       uint32_t seg, GMEM uint8_t* dst,
                                                       DecShared& sh) {
    const uint32_t mode = (tag >> 2) & 3u;
    bool ok = (tag >> 4) == kNibble && mode != 3u && rsv == 0 && L <= seg;
    if (ok && mode == 2) {
      ok = decode_stored(src, csize, L, dst);
    } else if (ok) {
      switch (tag & 3u) {
        case 0: ok = ipk::decompress_packed<1>(src, csize, L, mode, dst, sh); break;
        case 1: ok = ipk::decompress_packed<2>(src, csize, L, mode, dst, sh); break;
        case 2: ok = ipk::decompress_packed<4>(src, csize, L, mode, dst, sh); break;
        default: ok = ipk::decompress_packed<8>(src, csize, L, mode, dst, sh); break;
      }
    }
    return ok;
  }
};

BITAR_COLUMN_COMPRESS(IntPack, 1, true);
BITAR_COLUMN_COMPRESS(IntPack, 2, true);
BITAR_COLUMN_COMPRESS(IntPack, 4, true);
BITAR_COLUMN_COMPRESS(IntPack, 8, true);
BITAR_COLUMN_COMPRESS(IntPack, 1, false);
BITAR_COLUMN_COMPRESS(IntPack, 2, false);
BITAR_COLUMN_COMPRESS(IntPack, 4, false);
BITAR_COLUMN_COMPRESS(IntPack, 8, false);
BITAR_COLUMN_DECOMPRESS(IntPack, false);
BITAR_COLUMN_DECOMPRESS(IntPack, true);

}  // namespace bitar_hip
