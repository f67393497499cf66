/*
 * bitar_hip_codecs.h -- codec ids from 256 on of the MI355X segment codec engine
 * (libbitar_hip.so).  The ids below 256 and every entry point are in bitar_hip.h; the ids here
 * are passed to the same entry points (bitar_hip_compress, bitar_hip_decompress,
 * bitar_hip_slot_size, ...) as plain uint32_t values.  They are additive: BITAR_HIP_ABI_VERSION
 * and the symbol list of bitar_hip.h are as they were.  This header stands alone: it neither
 * includes bitar_hip.h nor is included by it.
 */
#ifndef BITAR_HIP_CODECS_H_
#define BITAR_HIP_CODECS_H_

enum bitar_hip_codec_256 {
  /* DECPACK: INTPACK's frame-of-reference bit packing for 16-byte integer
   * columns -- Arrow decimal128, a 16-byte little-endian two's-complement integer.  A family's
   * id is base + log2(element width): 256 + 4; 261 is left free for a 32-byte width, and 256..259
   * are no codecs.  No match search, no exceptions for outliers, no candidate of AUTOPACK.
   *
   * One stream per segment of L bytes (1..65536), w = 16, m = L / 16 elements read as
   * little-endian integers mod 2^128; the last L - 16 m bytes are the tail:
   *   byte 0      0xD0 | mode << 2 | (log2(w) - 4)   mode 0 plain, 1 delta, 2 stored; low two bits 0
   *   byte 1      0
   *   bytes 2..3  LE16(L - 1)
   *   stored:     L raw bytes                                              size = 4 + L
   *   packed:     [mode 1: element 0, 16 bytes]
   *               widths[nmb]  one byte, 0..128, per miniblock of 64 elements, nmb = ceil(m / 64)
   *               refs[nblk]   16 bytes each, per block of 4 miniblocks, nblk = ceil(nmb / 4)
   *               payload      miniblock k = 8 * widths[k] bytes, element t at bits
   *                            [t*b, (t+1)*b) of a little-endian bit string (INTPACK's
   *                            packing), slots past m as 0
   *               tail
   *   size = 4 + [16] + nmb + 16 nblk + 8 sum(widths) + (L - 16 m)
   * mode 0: x_i = v_i.  mode 1: x_i = v_i - v_(i-1) mod 2^128, x_0 = x_1 (0 when m = 1; the
   * decoder ignores it and starts from element 0).  ref = the block's smallest x read as signed
   * 128-bit; residual = x - ref mod 2^128; widths[k] = the bit length of the miniblock's largest
   * residual.  Mode 1 only when strictly smaller than mode 0; stored when the winner is not
   * strictly below 4 + L (m = 0 included).  A slot is therefore seg + 4 rounded up to 256, and
   * the max distance is 0 ("none").
   *
   * The decoder rejects (BITAR_HIP_SEGMENT_ERROR, the segment's output untouched): a high nibble
   * other than 0xD, mode 3, non-zero low two bits, byte 1 != 0, L > seg, a stored form whose
   * size is not 4 + L, a stream too short for its header arrays, a width above 128, a size that
   * is not exactly the formula.  Everything else decodes: widths larger than needed, a mode
   * that is not the smallest, a packed form above 4 + L.  Nothing outside the stream is read,
   * nothing outside the segment's first L output bytes is written. */
  BITAR_HIP_CODEC_DECPACK128 = 260
};

/* The DECPACK id of an element width of 16 bytes. */
#define BITAR_HIP_CODEC_DECPACK(width) (BITAR_HIP_CODEC_DECPACK128)

#endif /* BITAR_HIP_CODECS_H_ */
