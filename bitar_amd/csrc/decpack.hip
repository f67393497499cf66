// decpack.hip -- DECPACK: INTPACK's frame-of-reference bit packing for 16-byte integers (Arrow
// decimal128), per segment, both directions (gfx950).  The rules are INTPACK's (intpack.hip) at
// 128 bits: a signed minimum per block of 256 elements, the bit length of the largest residual
// per miniblock of 64, plain values or their deltas, whichever is smaller.
//
// Stream of a segment of L bytes, m = L / 16 elements (include/bitar_hip_codecs.h):
//   byte 0      0xD0 | mode << 2                mode 0 packed, 1 packed with delta, 2 stored
//   byte 1      0
//   bytes 2..3  LE16(L - 1)
//   stored:     L raw bytes
//   packed:     [mode 1: element 0]  widths[nmb]  refs[nblk] (16 bytes each)  payload  tail
//               nmb = ceil(m / 64), nblk = ceil(nmb / 4); miniblock k's payload is 8 * widths[k]
//               bytes (widths 0..128), element t at bits [t*b, (t+1)*b) of the little-endian
//               bit string
//
// One wavefront per segment, lane t = element t of the current miniblock; the encoder reads its
// segment twice (plan, then emit), as INTPACK's does.  What is new here is the arithmetic: a value
// is four dwords, so the wave's minimum, OR and inclusive add move four dwords per DPP step, the
// signed compare and the add carry across them, and a field of up to 128 bits lies in up to five
// dwords of the bit string (bitpack128.hip.h).  The stream's layout, the mode choice and the
// widths' scan are bitpack.hip.h's at W = 16.
#include "../../include/bitar_hip_codecs.h"
#include "autopack.hip.h"
#include "bitpack128.hip.h"

namespace bitar_hip {

namespace dpk {

using ipk::kMini;
using Layout = ipk::Layout<16>;
constexpr uint32_t kMaxMini = 64;  // miniblocks of a 64 KiB segment of 16-byte elements
constexpr uint32_t kMaxBlk = 16;

struct Shared {
  uint8_t wid[2][kMaxMini];  // widths of mode 0 / mode 1
  u128 ref[2][kMaxBlk];      // references
  uint32_t stage[kStageDwords];  // one miniblock's bit string
};

// the first dword of a stream
__device__ __forceinline__ uint32_t stream_head(uint32_t mode, uint32_t L) {
  return 0xD0u | mode << 2 | (L - 1) << 16;
}

template <uint32_t W, bool STORE>
__device__ __forceinline__ void compress_segment(const GMEM uint8_t* src, uint32_t L,
                                                 GMEM uint8_t* dst, uint32_t* size_out,
                                                 Shared& sh) {
  static_assert(W == 16 && STORE, "DECPACK: 16-byte elements, no store-less form");
  const uint32_t lane = lane_id();
  const Layout lay(L, 0);
  const uint32_t m = lay.m, tail = lay.tail, nmb = lay.nmb, nblk = lay.nblk;

  // ---- plan: both modes' references and widths in one sweep --------------------------------
  uint32_t sum[2] = {0, 0};
  for (uint32_t blk = 0; blk < nblk; ++blk) {
    BlockPlan p;
    plan_block(src, blk, m, p);
#pragma unroll
    for (uint32_t md = 0; md < 2; ++md) {
      if (lane == 0) sh.ref[md][blk] = p.ref[md];
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
  const uint32_t mode = ipk::choose_mode<16>(L, sum, total);
  GMEM uint32_t* head = reinterpret_cast<GMEM uint32_t*>(dst);  // (slots are 16-B aligned)
  if (lane == 0) {
    *head = stream_head(mode, L);
    *size_out = total;
  }
  if (mode == 2) {
    wave_copy_global(dst + 4, src, L);
    return;
  }
  uint32_t pos = 4;
  if (mode) {
    if (lane < 16) dst[pos + lane] = src[lane];
    pos += 16;
  }
  for (uint32_t k = lane; k < nmb; k += kWave) dst[pos + k] = sh.wid[mode][k];
  pos += nmb;
  const uint8_t* refs = reinterpret_cast<const uint8_t*>(sh.ref[mode]);
  for (uint32_t k = lane; k < nblk * 16; k += kWave) dst[pos + k] = refs[k];
  pos += nblk * 16;

  // ---- emit: the payload as aligned dwords ---------------------------------------------------
  GMEM uint8_t* pay = dst + pos;
  PayloadEmitter emit(pay, sh.stage);
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t b = sh.wid[mode][k];
    if (b == 0) continue;
    const uint32_t idx = k * kMini + lane;
    u128 xs[2];
    load_values(src, idx, m, xs[0], xs[1]);
    const u128 ref = sh.ref[mode][k / 4];
    const u128 r = idx < m ? (mode ? xs[1] : xs[0]) - ref : (u128)0;
    emit.put(r, b);
  }
  const uint32_t off = emit.finish();
  if (lane < tail) pay[off + lane] = src[m * 16 + lane];
}

struct DecShared {
  uint8_t wid[kMaxMini];
  uint32_t off[kMaxMini];  // byte offset of every miniblock in the payload
};

// the packed form: src holds csize bytes, the header is valid and L <= seg.  Returns false for a
// stream that must be rejected (checked before anything is written).
__device__ __forceinline__ bool decompress_packed(const GMEM uint8_t* src, uint32_t csize,
                                                  uint32_t L, uint32_t mode, GMEM uint8_t* dst,
                                                  DecShared& sh) {
  const uint32_t lane = lane_id();
  const Layout lay(L, mode);
  const uint32_t m = lay.m, tail = lay.tail, nmb = lay.nmb;

  // widths -> offsets; the stream's size must be exactly what they add up to
  uint32_t run;
  if (!ipk::scan_widths<16>(src, csize, lay, run, [&](uint32_t k, uint32_t b, uint32_t off) {
        sh.wid[k] = (uint8_t)b;
        sh.off[k] = off;
      }))
    return false;
  lds_order();

  const GMEM uint8_t* pay = src + lay.pay_at;
  u128 carry = 0;
  u128 ref = 0;
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t idx = k * kMini + lane;
    const uint32_t b = sh.wid[k];
    if ((k & 3u) == 0) ref = load_elem(src + lay.ref_at + (k / 4) * 16);  // (once per block)
    u128 r = 0;
    if (b) r = extract_field(pay + sh.off[k], b);
    u128 v = r + ref;
    if (mode) {
      if (idx == 0) v = load_elem(src + Layout::base_at);
      v = wave_incl_add(v) + carry;
      carry = lane63(v);
    }
    if (idx < m) store_elem(dst + (uint64_t)idx * 16, v);
  }
  if (lane < tail) dst[m * 16 + lane] = pay[run + lane];
  return true;
}

}  // namespace dpk

// DECPACK as the shared kernels see it (autopack.hip.h).
struct DecPack {
  static constexpr uint32_t kNibble = 0xD;
  template <uint32_t W> using EncShared = dpk::Shared;
  using DecShared = dpk::DecShared;

  template <uint32_t W, bool STORE>
  static constexpr auto compress_segment = &dpk::compress_segment<W, STORE>;

  static __device__ __forceinline__ bool decode_stream(const GMEM uint8_t* src, uint32_t csize,
                                                       uint32_t tag, uint32_t rsv, uint32_t L,
                                                       uint32_t seg, GMEM uint8_t* dst,
                                                       DecShared& sh) {
    const uint32_t mode = (tag >> 2) & 3u;
    // (the low two bits are log2(w) - 4: 0, the one width there is)
    if ((tag >> 4) != kNibble || mode == 3u || (tag & 3u) != 0 || rsv != 0 || L > seg) return false;
    if (mode == 2) return decode_stored(src, csize, L, dst);
    return dpk::decompress_packed(src, csize, L, mode, dst, sh);
  }
};

BITAR_COLUMN_COMPRESS(DecPack, 16, true);
BITAR_COLUMN_DECOMPRESS(DecPack, false);

}  // namespace bitar_hip
