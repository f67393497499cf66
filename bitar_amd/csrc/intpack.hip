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
  constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
  const uint32_t lane = lane_id();
  const Layout<W> lay(L, 0);
  const uint32_t m = lay.m, tail = lay.tail, nmb = lay.nmb, nblk = lay.nblk;
  const GlobalElems<W> elems{src};

  // ---- plan: both modes' references and widths in one sweep (bitpack.hip.h) -----------------
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
      if constexpr (STORE) *head = stream_head<W>(2, L);
      *size_out = total;
    }
    if constexpr (STORE) wave_copy_global(dst + 4, src, L);
    return;
  }
  if (lane == 0) {
    *head = stream_head<W>(mode, L);
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
    load_values<W>(elems, idx, m, xs[0], xs[1]);
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
  U carry = 0;
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t idx = k * kMini + lane;
    const U v = unpack_miniblock<W>(src, lay, mode, k, sh.wid[k], pay + sh.off[k], carry);
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
    bool ok = ipk::valid_head(tag, rsv) && L <= seg;
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
