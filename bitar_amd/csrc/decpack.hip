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
// segment twice (plan, then emit).  The code is INTPACK's too, bitpack.hip.h's templates at
// W = 16: a value is four dwords there, so the wave's minimum and inclusive add move four dwords
// per DPP step, the signed compare and the add carry across them, and a field of up to 128 bits
// lies in up to five dwords of the bit string.
#include "../../include/bitar_hip_codecs.h"
#include "autopack.hip.h"
#include "bitpack.hip.h"

namespace bitar_hip {

// DECPACK as the shared kernels see it (autopack.hip.h).
struct DecPack {
  static constexpr uint32_t kNibble = 0xD;
  template <uint32_t W> using EncShared = ipk::EncLds<16, 16>;
  using DecShared = ipk::DecLds<16>;

  template <uint32_t W, bool STORE>
  static __device__ __forceinline__ void compress_segment(const GMEM uint8_t* src, uint32_t L,
                                                          GMEM uint8_t* dst, uint32_t* size_out,
                                                          EncShared<W>& sh) {
    static_assert(W == 16 && STORE, "DECPACK: 16-byte elements, no store-less form");
    ipk::compress_segment<W, STORE, kNibble>(src, L, dst, size_out, sh);
  }

  static __device__ __forceinline__ bool decode_stream(const GMEM uint8_t* src, uint32_t csize,
                                                       uint32_t tag, uint32_t rsv, uint32_t L,
                                                       uint32_t seg, GMEM uint8_t* dst,
                                                       DecShared& sh) {
    // (the low two bits are log2(w) - 4: 0, the one width there is)
    if (!ipk::valid_head(tag, rsv, kNibble) || (tag & 3u) != 0 || L > seg) return false;
    if ((tag >> 2 & 3u) == 2) return decode_stored(src, csize, L, dst);
    return ipk::decompress_packed<16>(src, csize, L, tag >> 2 & 3u, dst, sh);
  }
};

BITAR_COLUMN_COMPRESS(DecPack, 16, true);
BITAR_COLUMN_DECOMPRESS(DecPack, false);

}  // namespace bitar_hip
