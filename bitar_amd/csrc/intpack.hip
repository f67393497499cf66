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
// (All of it is in bitpack.hip.h: the segment encoder and decoder, shared with decpack.hip, and
// under them the reductions, element loads and stores and the payload emitter, shared with
// fltpack.hip, cascade.hip and patchpack.hip.)
#include "../../include/bitar_hip.h"
#include "autopack.hip.h"
#include "bitpack.hip.h"

namespace bitar_hip {

// INTPACK as the shared kernels see it (autopack.hip.h).  One LDS size for every width.
struct IntPack {
  static constexpr uint32_t kNibble = 4;
  template <uint32_t W> using EncShared = ipk::EncLds<1, 8>;
  using DecShared = ipk::DecLds<1>;

  template <uint32_t W, bool STORE>
  static constexpr auto compress_segment = &ipk::compress_segment<W, STORE, kNibble, EncShared<W>>;

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
