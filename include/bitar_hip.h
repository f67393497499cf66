/*
 * bitar_hip.h -- the C-ABI boundary of the MI355X segment codec engine (libbitar_hip.so).
 *
 * Plain pointers and sizes only; no Arrow, torch or HIP types in the signatures
 * (hipStream_t travels as void*).  Every entry point returns 0 or a negated
 * arrow::StatusCode, the convention the reference carries in an int
 * (reference src/include/util.h:157-205).
 *
 * Each function names the reference interface it replaces.  The reference drives a
 * BlueField-2 DEFLATE engine through DPDK compressdev; here one HIP kernel launch
 * replaces a whole enqueue/dequeue burst loop, and a HIP stream replaces a queue pair.
 */
#ifndef BITAR_HIP_H_
#define BITAR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BITAR_HIP_ABI_VERSION 3

/* negated arrow::StatusCode */
enum bitar_hip_status {
  BITAR_HIP_OK = 0,
  BITAR_HIP_OUT_OF_MEMORY = -1,
  BITAR_HIP_INVALID = -4,
  BITAR_HIP_IO_ERROR = -5,
  BITAR_HIP_CAPACITY_ERROR = -6,
  BITAR_HIP_CANCELLED = -8,
  BITAR_HIP_UNKNOWN_ERROR = -9,
  BITAR_HIP_NOT_IMPLEMENTED = -10
};

/* Codec of one segment op.  DEFLATE = raw RFC 1951 stream per segment, the reference's
 * frame (reference src/config.cc:83-105, memory.cc:110).  LZ4 = raw LZ4 block per segment
 * (the north-star codec).  ZSTD = one RFC 8878 Zstandard frame per segment (the DPDK
 * RTE_COMP_ALGO_ZSTD path of reference src/config.cc:83-105 / BASELINE configs[5]). */
enum bitar_hip_codec {
  BITAR_HIP_CODEC_LZ4 = 1,
  BITAR_HIP_CODEC_DEFLATE = 2,         /* fixed-Huffman blocks (HuffmanEncoding::FIXED) */
  BITAR_HIP_CODEC_ZSTD = 3,
  BITAR_HIP_CODEC_DEFLATE_DYNAMIC = 4, /* dynamic Huffman (HuffmanEncoding::DYNAMIC, the
                                          reference default, config.h:151); decoded like
                                          DEFLATE.  Compress runs two kernels through a
                                          stream-ordered scratch allocation. */
  BITAR_HIP_CODEC_LZ4_WIDE = 5,        /* LZ4 blocks from the wide parse: 16 KiB history (match
                                          distance <= 14848), 4096-entry table -- the ratio
                                          operating point, within a few % of liblz4's ratio
                                          at a lower speed; the streams are ordinary LZ4 blocks
                                          (decoded like LZ4).  The C++ front-end selects it for
                                          Codec::LZ4 at level() >= 2 (bitar/config.h). */
  /* SNAPPY: one RAW Snappy stream per segment (no framing format), readable
   * by every stock Snappy decoder; the decoder reads any stock raw stream of <= 65536 bytes.
   * A segment of n bytes:
   *   preamble    n as a minimal varint (<= 3 bytes; n = 0: the single byte 00)
   *   elements    the sequences of BITAR_HIP_CODEC_LZ4's parse (distance <= 2560), each as
   *               - one literal element for a non-empty literal run: tag (len-1) << 2 for
   *                 len-1 < 60, tag 60 << 2 + 1 length byte for len-1 < 256, else tag 61 << 2 +
   *                 2 length bytes (little-endian), then the bytes;
   *               - the match split by stock Snappy's rule (while len >= 68 a piece of 64, a
   *                 piece of 60 if len > 64, then the rest, 4..64), each piece a copy-1 element
   *                 (2 bytes: tag 1 | (len-4) << 2 | (offset >> 8) << 5, offset low byte) if
   *                 4 <= len <= 11 and offset < 2048, else a copy-2 element (3 bytes: tag
   *                 2 | (len-1) << 2, LE16 offset); copy-4 is never written;
   *               the trailing literals are a last literal element.
   *   stored      a stream that is not smaller than preamble + ONE literal element holding the
   *               whole segment (or that overran its slot) is written in that form, so a stream
   *               is <= n + 6 bytes and compress never fails for lack of space.
   * The decoder follows stock Snappy: the varint may be non-minimal (<= 5 bytes, the fifth
   * below 16); literal length codes 60..63 and copy-4 are legal; a copy with offset 0 or beyond
   * the bytes produced so far rejects (offset == produced is fine, overlapping copies
   * replicate); an element reading past the input rejects; the elements must consume the input
   * exactly and produce exactly the declared length.  A declared length above seg fails the
   * segment.  No byte outside the segment's seg output bytes is written in any case. */
  BITAR_HIP_CODEC_SNAPPY = 6,
  /* INTPACK: frame-of-reference bit packing of little-endian integer
   * elements, for columns of narrow range (dictionary indices, small integers, sorted keys,
   * timestamps, string offsets).  The id is 8 + log2(element width in bytes); no reference
   * counterpart and no stock library reads the format.  One stream per segment of L bytes,
   * m = L / w elements, the last L - m*w bytes are the tail:
   *   byte 0      0x40 | mode << 2 | log2(w)    mode 0 packed, 1 packed with delta, 2 stored
   *   byte 1      0
   *   bytes 2..3  LE16(L - 1)
   *   stored:     L raw bytes
   *   packed:     [mode 1: element 0, w bytes]
   *               widths[nmb]  one byte (0..8w) per miniblock of 64 elements, nmb = ceil(m / 64)
   *               refs[nblk]   one w-byte reference per block of 4 miniblocks
   *               payload      miniblock k = 8 * widths[k] bytes: element t at bits [t*b, (t+1)*b)
   *                            of a little-endian bit string, elements past m as 0
   *               tail
   * Values: x_i = v_i (mode 0) or v_i - v_(i-1) mod 2^(8w) (mode 1; x_0 = x_1, 0 when m = 1,
   * ignored by the decoder, which starts from element 0).  ref = a block's smallest x read as
   * signed, residual = x - ref mod 2^(8w), widths[k] = the bit length of the miniblock's
   * largest residual.  The encoder takes mode 1 only when strictly smaller, and the stored form
   * when the winner is not strictly smaller than 4 + L.  The decoder takes w from the tag (all
   * four ids select it) and rejects: another tag, byte 1 != 0, L > seg, a width above 8w, a
   * stream whose size is not exactly what its header and widths add up to. */
  BITAR_HIP_CODEC_INTPACK8 = 8,
  BITAR_HIP_CODEC_INTPACK16 = 9,
  BITAR_HIP_CODEC_INTPACK32 = 10,
  BITAR_HIP_CODEC_INTPACK64 = 11,
  /* FLTPACK: decimal-scaled bit packing of little-endian IEEE float (w = 4) or
   * double (w = 8) elements, for columns that are decimal by origin (prices, sensor readings,
   * coordinates, percentages, integer-valued doubles).  The id is 16 + log2(w); no reference
   * counterpart and no stock library reads the format.  One stream per segment of L bytes,
   * m = L / w elements, the last L - m*w bytes are the tail:
   *   byte 0      0x50 | mode << 2 | log2(w)    mode 0 packed, 2 stored
   *   byte 1      e, the decimal exponent, 0..15 (0 in the stored form)
   *   bytes 2..3  LE16(L - 1)
   *   stored:     L raw bytes
   *   packed:     LE16 nx      number of exceptions, nx <= m
   *               widths[nmb]  one byte (0..8w) per miniblock of 64 elements, nmb = ceil(m / 64)
   *               refs[nblk]   one w-byte signed reference per block of 4 miniblocks
   *               payload      miniblock k = 8 * widths[k] bytes: element t at bits [t*b, (t+1)*b)
   *                            of a little-endian bit string (INTPACK's packing)
   *               pos[nx]      LE16 element indices, strictly increasing, each < m
   *               val[nx]      the exceptions' raw w-byte elements, in the same order
   *               tail
   *   size = 6 + nmb + nblk*w + 8*sum(widths) + nx*(2 + w) + (L - m*w)
   * An element v is encodable at e when t = rint((double)v * 10^e) is finite, |t| <= 2^53
   * (w = 8) or 2^31 - 1 (w = 4), and (double)n / 10^e for n = (int)t -- rounded to float for
   * w = 4 -- has exactly v's bit pattern; every other element (NaN, infinities, -0.0, denormals,
   * non-decimal values) is an exception.  ref = a block's smallest n over its encodable
   * elements (0 without any), residual = n - ref mod 2^(8w), 0 at an exception's slot and past
   * m.  The encoder picks e by a cost estimate over every 16th element (the smallest e among
   * equals) and takes the stored form when the packed one is not strictly smaller than 4 + L.
   * The decoder takes w from the tag (both ids select it) and rejects: another tag, mode 1 or
   * 3, log2(w) below 2, e > 15 (e != 0 when stored), L > seg, nx > m, a width above 8w, a
   * position >= m or not above the one before, a stream whose size is not exactly the formula
   * (4 + L when stored).  Anything else decodes: arithmetic is mod 2^(8w), residuals at
   * exception slots are ignored. */
  BITAR_HIP_CODEC_FLTPACK32 = 18,
  BITAR_HIP_CODEC_FLTPACK64 = 19,
  /* DICTPACK: a per-segment dictionary plus bit-packed indices, for columns of
   * wide values with few distinct ones (hash or surrogate ids, UUIDs, decimal128, floats that
   * take a few hundred values, anything a Parquet reader decoded from a dictionary page).  The
   * id is 24 + log2(w) for w = 4, 8 or 16 bytes (24 and 25 are not offered: INTPACK serves 1-
   * and 2-byte elements); no reference counterpart and no stock library reads the format.  One
   * stream per segment of L bytes, m = L / w elements compared as byte patterns (+0.0, -0.0
   * and every NaN payload are distinct values), the last L - m*w bytes are the tail:
   *   byte 0      0x60 | mode << 3 | log2(w)    mode 0 packed, 1 stored; log2(w) 2, 3 or 4
   *   byte 1      0
   *   bytes 2..3  LE16(L - 1)
   *   stored:     L raw bytes                                           size = 4 + L
   *   packed:     LE16(d - 1)  d = number of dictionary entries, 1 <= d <= min(m, 1024)
   *               dict[d]      the distinct elements, w bytes each, in order of first occurrence
   *               payload      nmb = ceil(m / 64) miniblocks of 8*b bytes, b = bit_length(d - 1)
   *                            (none when d = 1): element t's dictionary index at bits
   *                            [t*b, (t+1)*b) of the miniblock's little-endian bit string
   *                            (INTPACK's packing), slots past m written as 0
   *               tail
   *   size = 6 + d*w + 8*b*nmb + (L - m*w)
   * The encoder packs a segment that has at most 1024 distinct elements and whose packed size is
   * below 4 + L, and stores every other one (m = 0 included).  The two sizes differ by 2 mod 4,
   * so they are never equal: "below" and "not above" are the same rule.  The decoder takes w
   * from the tag (all three ids select it) and rejects, before it writes anything: a high nibble
   * other than 6, log2(w) outside 2..4, byte 1 != 0, L > seg, d > min(m, 1024), a stream whose
   * size is not exactly the formula (4 + L when stored).  An index >= d in one of the slots
   * 0..m-1 rejects the segment as well, where the decoder meets it: the elements of the
   * miniblocks before that one have been written then.  Bits in slots past m are ignored and
   * duplicate dictionary entries are accepted. */
  BITAR_HIP_CODEC_DICTPACK32 = 26,
  BITAR_HIP_CODEC_DICTPACK64 = 27,
  BITAR_HIP_CODEC_DICTPACK128 = 28,
  /* RUNPACK: per-segment run-length coding, for sorted or clustered columns
   * whose values come in long runs (partition and dimension keys, coarse timestamps, status and
   * flag bytes, byte-per-value validity).  The id is 32 + log2(w) for w = 1, 2, 4, 8 or 16
   * bytes; no reference counterpart and no stock library reads the format.  One stream per
   * segment of L bytes, m = L / w elements compared as byte patterns (+0.0, -0.0 and every NaN
   * payload are distinct values), the last L - m*w bytes are the tail:
   *   byte 0      0x70 | mode << 3 | log2(w)    mode 0 runs, 1 stored
   *   byte 1      bl, bytes per run length: 1 or 2 (0 in the stored form)
   *   bytes 2..3  LE16(L - 1)
   *   stored:     L raw bytes                                           size = 4 + L
   *   runs:       LE16(r - 1)  r = number of runs, 1 <= r <= m
   *               values[r]    each run's element, w bytes, in order
   *               lengths[r]   (run length - 1), bl bytes each, little-endian
   *               tail
   *   size = 6 + r*(w + bl) + (L - m*w)
   * The encoder's runs are maximal (neighbouring runs have different values), bl is 1 when every
   * run is at most 256 elements long and 2 otherwise, and the runs form is taken when its size
   * is strictly below 4 + L; every other segment is stored (m = 0 included, and a tie, which
   * does occur: w = 1, m = 4, r = 1 is 8 bytes either way).  The decoder takes w from the tag
   * (all five ids select it) and rejects, before it writes anything: a high nibble other than
   * 7, log2(w) above 4, stored with byte 1 != 0, runs with byte 1 not 1 or 2, L > seg, a runs
   * stream shorter than 6 bytes, r > m, a stream whose size is not exactly the formula (4 + L
   * when stored), run lengths that do not add up to exactly m.  A rejected segment's output
   * range is left untouched.  Streams no encoder writes decode: equal neighbouring values,
   * bl = 2 where 1 would do, a runs form larger than 4 + L. */
  BITAR_HIP_CODEC_RUNPACK8 = 32,
  BITAR_HIP_CODEC_RUNPACK16 = 33,
  BITAR_HIP_CODEC_RUNPACK32 = 34,
  BITAR_HIP_CODEC_RUNPACK64 = 35,
  BITAR_HIP_CODEC_RUNPACK128 = 36,
  /* AUTOPACK: per segment the smallest of the applicable codecs above, for
   * columns whose shape the caller does not know or that changes from segment to segment.  The
   * id is 40 + log2(w) for w = 1, 2, 4, 8 or 16 bytes.  AUTOPACK has no format of its own.  For
   * a segment of L bytes the candidates are, in this order,
   *   w = 1, 2    RUNPACK, INTPACK
   *   w = 4, 8    RUNPACK, INTPACK, DICTPACK, FLTPACK
   *   w = 16      RUNPACK, DICTPACK
   * and the segment's stream is the shortest of the candidates' streams for that segment and
   * width, exactly as their own ids write them; a tie goes to the earlier candidate.  Nothing is
   * added: no wrapper byte, no new tag.  So every AUTOPACK stream decodes under its codec's own
   * id as well, a segment no candidate packs is RUNPACK's stored form (tag 0x78 | log2(w): all
   * candidates tie at 4 + L), and the size is never above any single candidate's.  The decoder
   * looks at the high nibble of byte 0: 4, 5, 6 or 7 gives the segment to INTPACK's, FLTPACK's,
   * DICTPACK's or RUNPACK's decoder, with that decoder's every rule and verdict (and what a
   * rejected segment of that format may have written); any other nibble, and a stream of size 0,
   * is rejected with its output range untouched.  Every AUTOPACK id decodes every width and all
   * four formats. */
  BITAR_HIP_CODEC_AUTOPACK8 = 40,
  BITAR_HIP_CODEC_AUTOPACK16 = 41,
  BITAR_HIP_CODEC_AUTOPACK32 = 42,
  BITAR_HIP_CODEC_AUTOPACK64 = 43,
  BITAR_HIP_CODEC_AUTOPACK128 = 44,
  /* CASCADE: RUNPACK's runs with their values and lengths packed by INTPACK --
   * the "RLE, delta, bit-pack" cascade -- for columns whose runs are themselves regular: sorted
   * keys, coarse timestamps, clustered status codes, flag bytes.  The id is 64 + log2(w) for
   * w = 1, 2, 4 or 8 bytes; no reference counterpart and no stock library reads the format.  It
   * is no candidate of AUTOPACK.  One stream per segment of L bytes, m = L / w elements compared
   * as byte patterns, the last L - m*w bytes are the tail:
   *   byte 0      0x80 | mode << 3 | log2(w)    mode 0 cascade, 1 stored
   *   byte 1      0
   *   bytes 2..3  LE16(L - 1)
   *   stored:     L raw bytes                                           size = 4 + L
   *   cascade:    LE16(r - 1)      r = number of runs, 1 <= r <= min(m, 32768)
   *               LE16(vsize - 1)
   *               values           an INTPACK stream (tag 0x4_, any of its three modes) of width w
   *                                whose "segment" is the r*w bytes of the runs' values; vsize bytes
   *               lengths          an INTPACK stream of width 2 whose "segment" is the 2r bytes
   *                                LE16(run length - 1) of the runs
   *               tail
   *   size = 8 + vsize + lsize + (L - m*w)
   * The encoder's runs are maximal, the two sub-streams are byte for byte what INTPACK writes
   * for those bytes (its choice between plain, delta and stored and its 4-byte header
   * included), and the cascade form is taken when r <= 32768 and its size is strictly below
   * 4 + L; every other segment is stored (m = 0 and a tie included).  The decoder takes w from
   * the tag (all four ids select it) and rejects, before it writes anything: a high nibble
   * other than 8, log2(w) above 3, byte 1 != 0, L > seg, a stored form whose size is not 4 + L,
   * a cascade form shorter than 8 bytes, r > min(m, 32768), a vsize that leaves no room for a
   * 4-byte lengths header and the tail, a values sub-stream that INTPACK's own rules reject or
   * whose tag width is not w or whose L field is not r*w, the same for the lengths sub-stream
   * with width 2 and 2r (its size must be exactly the rest of the stream less the tail), run
   * lengths that do not add up to exactly m.  A rejected segment's output range is left
   * untouched.  Streams no encoder writes decode: equal neighbouring values, a sub-stream in a
   * mode that is not its smallest, a cascade form larger than 4 + L. */
  BITAR_HIP_CODEC_CASCADE8 = 64,
  BITAR_HIP_CODEC_CASCADE16 = 65,
  BITAR_HIP_CODEC_CASCADE32 = 66,
  BITAR_HIP_CODEC_CASCADE64 = 67,
  /* RANS: an order-0 rANS entropy coder with 64 interleaved states for byte
   * segments whose gain is their histogram and not their repeats -- non-decimal floats behind the
   * shuffle filter, embeddings and weights, noisy sensor words, residuals.  No reference
   * counterpart and no stock library reads the format (tests/rans_model.py is a numpy reader and
   * writer).  Ids 68..71 are left for a fifth CASCADE width.  One stream per segment of L bytes:
   *   byte 0      0xA0 | mode                mode 0 rans, 1 stored
   *   byte 1      0
   *   bytes 2..3  LE16(L - 1)
   *   stored:     L raw bytes                                           size = 4 + L
   *   rans:       bitmap   32 bytes, bit s (byte s >> 3, bit s & 7) set iff byte value s occurs
   *               freqs    for the k-th present symbol in ascending order, f - 1 in bits
   *                        [12k, 12k + 12) of a little-endian bit string, zero-padded to an even
   *                        number of bytes
   *               words    nw little-endian 16-bit words, in the order the encoder emitted them
   *               states   64 x LE32, the encoder's final state of lane 0..63
   *   size = 36 + tsize + 2*nw + 256,  tsize = 2 * ceil(12 * nsym / 16)
   * Frequencies: with c[s] the count of s and nsym the number of present symbols,
   * f[s] = 1 + floor(c[s] * (4096 - nsym) / L), and the deficit 4096 - sum(f) goes to the most
   * frequent symbol (the lowest value on a tie); cum[s] is the sum of f[t] over t < s.
   * Coder: symbol i belongs to lane i mod 64 and step i div 64; 32-bit states start at 2^16.  The
   * encoder runs the steps from the last to the first; an active lane with state x and symbol s
   * emits x & 0xFFFF and shifts x right by 16 when x >= f[s] * 2^20, then
   * x = (x div f[s]) * 4096 + x mod f[s] + cum[s]; a step's words are appended in ascending lane
   * order, and after step 0 the 64 states are written.  The decoder runs the steps forward with
   * p = nw: slot = x & 4095, s the symbol whose [cum, cum + f) holds slot,
   * x = f[s] * (x >> 12) + slot - cum[s]; the n lanes with x < 2^16, ranked r in lane order, then
   * take x = x << 16 | words[p - n + r], and p -= n.
   * The rans form is taken iff its size is strictly below 4 + L.  The decoder rejects: a high
   * nibble other than 0xA, a mode above 1, byte 1 != 0, L > seg, a stored form whose size is not
   * 4 + L, a rans form shorter than 36 + 2 + 256 bytes, an empty bitmap, frequencies that do not
   * sum to 4096, non-zero pad bits in freqs, a size for which 2*nw is negative or odd, an initial
   * state below 2^16 -- all before the first output byte -- and a refill that needs more words
   * than remain, words left over at the end, or a final state other than 2^16 (rANS's own
   * integrity check) after part of the segment's output range may have been written.  Nothing
   * outside that range is written.  Streams no encoder writes decode: any table that sums to
   * 4096, a rans form larger than 4 + L. */
  BITAR_HIP_CODEC_RANS = 72,
  /* RANSPLANE: RANS with one order-0 table per byte plane of an element of
   * w = 2, 4 or 8 bytes -- bf16 / fp16 / fp32 / fp64 weights, activations and embeddings, whose
   * exponent byte has 2..3 bits of entropy and whose low mantissa bytes have 8, and integer
   * columns with noisy low bytes.  No filter pass: 64 is a multiple of w, so lane i mod 64 codes
   * plane i mod w for the whole segment.  No reference counterpart and no stock library reads the
   * format (tests/ransplane_model.py is a numpy reader and writer).  The id is 80 + log2(w); 80
   * itself is not offered (width 1 is RANS), and ids 73..79 and 84.. stay unknown.  Unlike the
   * other families, an id decodes only its own width: the decoder's LDS is sized by w.
   * One stream per segment of L bytes, w = 1 << lg:
   *   byte 0      0xB0 | mode << 3 | lg      mode 0 planes, 1 stored; lg 1, 2 or 3
   *   byte 1      0
   *   bytes 2..3  LE16(L - 1)
   *   stored:     L raw bytes                                           size = 4 + L
   *   planes:     bitmaps  w x 32 bytes, plane 0 first; in plane p's bitmap bit s (byte s >> 3,
   *                        bit s & 7) is set iff byte value s occurs among the bytes i < L with
   *                        i mod w == p (i counts from the segment's first byte, not its address)
   *               freqs    w fields, plane 0 first, each exactly RANS's freqs field for that
   *                        plane: f - 1 of the k-th present symbol in bits [12k, 12k + 12) of a
   *                        little-endian bit string, zero-padded to an even number of bytes
   *                        (tsize_p = 2 * ceil(12 * nsym_p / 16))
   *               words    nw little-endian 16-bit words, in the order the encoder emitted them
   *               states   64 x LE32, the encoder's final state of lane 0..63
   *   size = 4 + 32 w + sum(tsize_p) + 2*nw + 256
   * Frequencies, per plane: with n_p the number of bytes of plane p, c_p[s] their counts and
   * nsym_p the number of present symbols, f_p[s] = 1 + floor(c_p[s] * (4096 - nsym_p) / n_p), and
   * the deficit 4096 - sum(f_p) goes to the plane's most frequent symbol (the lowest value on a
   * tie): RANS's rule with n_p in place of L.
   * Coder: RANS's, word for word -- 64 states starting at 2^16, symbol i in lane i mod 64 at step
   * i div 64, the encoder running backward and emitting x & 0xFFFF when x >= f * 2^20, a step's
   * words in lane order, the decoder running forward and refilling from the end of `words` by
   * ballot rank -- with the f and cum of plane i mod w.
   * The planes form is taken iff L >= w (every plane non-empty) and its size is strictly below
   * 4 + L; otherwise the segment is stored (tag 0xB8 | lg).  Neither L nor seg need be a multiple
   * of w: there is no tail, the last planes are one byte shorter.
   * The decoder rejects: a high nibble other than 0xB, lg other than that of the id it was called
   * under, byte 1 != 0, L > seg, a stored form whose size is not 4 + L, a planes form with L < w,
   * a stream too short for its bitmaps, tables and states, any plane's bitmap empty, any plane's
   * frequencies not summing to 4096, non-zero pad bits in any plane's freqs field, a size for
   * which 2*nw is negative or odd, an initial state below 2^16 -- all before the first output
   * byte -- and a refill that needs more words than remain, words left over, or a final state
   * other than 2^16 after part of the segment's output range may have been written.  Nothing is
   * read outside the stream's bytes and nothing is written outside the segment's first L output
   * bytes.  Streams no encoder writes decode: any tables that sum to 4096, a planes form larger
   * than 4 + L. */
  BITAR_HIP_CODEC_RANSPLANE16 = 81,
  BITAR_HIP_CODEC_RANSPLANE32 = 82,
  BITAR_HIP_CODEC_RANSPLANE64 = 83,
  /* SYMTAB: a static symbol table per segment, in the style of FSST, for the
   * data buffer of a string or binary column -- names, URLs, log lines, keys: up to 255 byte
   * strings of 1..8 bytes, the text written as one-byte codes, anything else escaped.  No
   * reference counterpart and no stock library reads the format (tests/symtab_model.py is a
   * Python reader and writer).  A byte codec: no element width.  Ids 84..87 are left for
   * RANSPLANE.  One stream per segment of L bytes, 1..65536:
   *   byte 0      0xC0 | mode            mode 0 coded, 1 stored
   *   byte 1      nsym, 1..255           (0 in the stored form)
   *   bytes 2..3  LE16(L - 1)
   *   stored:     L raw bytes                                     size = 4 + L
   *   coded:      LE16 nc                number of codes, >= 1
   *               lens[nsym]             one byte each, 1..8
   *               syms                   the symbols' bytes, concatenated in code order
   *               codes[nc]              c < nsym: symbol c;  255: the next unread byte of lits
   *               lits[nx]               nx = the number of codes equal to 255
   *   size = 6 + nsym + sum(lens) + nc + nx
   * Escapes sit in a stream of their own, so every byte of `codes` is a code: a code's output
   * offset is a prefix sum of lengths, an escape's literal index its rank among the escapes.
   * The coded form is taken iff it is strictly smaller than 4 + L.  The decoder rejects a high
   * nibble other than 0xC, a mode above 1, byte 1 other than 0 when stored, L > seg, nsym = 0 or
   * nc = 0 when coded, a length of 0 or above 8, a code in [nsym, 255), a stream whose size is not
   * exactly the formula, and lengths that do not sum to exactly L (an escape counts 1) -- all
   * before the first output byte -- and decodes everything else; duplicate symbols are allowed.
   * Nothing outside the segment's L output bytes is written, nothing outside the stream is read.
   * The encoder's rule (its bytes are the model's):
   * Sample: the segment is cut into chunks of 256 bytes (the last may be short); the sample is
   * all chunks when L <= 16384 and those whose index is a multiple of 4 otherwise (at most 64).
   * Nothing is matched or paired across a chunk's end.
   * Items: ids 0..255 are the byte values, id 256 + c is symbol c of the current table T.
   * Generations: T starts empty; in each of five generations every sample chunk is parsed
   * greedily against T -- at a position the longest symbol of T that matches inside the chunk,
   * else the single byte -- and c1[x] counts the parsed items.  An adjacent pair (x, y) of a chunk
   * with len(x) + len(y) <= 8 has key = x * 512 + y and slot = (key * 0x9E3779B1 mod 2^32) >> 20
   * (4096 slots); of the keys that share a slot in a generation only the smallest is counted.
   * Selection: the candidates are, in index order, the items with c1 > 0 (index = id, gain =
   * c1 * len) and the occupied slots (index = 512 + slot, gain = count * total length).  With 255
   * or fewer all are taken; otherwise, thr being the 255th largest gain, every candidate with
   * gain > thr and then those with gain = thr in index order until 255 are.  The new T is the
   * taken candidates in index order; after the fifth generation a symbol's code is its position.
   * Emit: the whole segment parsed greedily with T, no match passing its end; a symbol gives its
   * code, a single byte not in T gives 255 in codes and the byte in lits. */
  BITAR_HIP_CODEC_SYMTAB = 88,
  /* PATCHPACK: INTPACK with per-miniblock exceptions -- a patched frame of
   * reference -- for integer columns with outliers: timestamps with gaps, string offsets with a
   * long string, heavy-tailed counts, INT_MAX, 0 or -1 written for "missing".  INTPACK gives a
   * miniblock the bit length of its largest residual; here the few residuals that are too long
   * are kept raw behind the payload, as FLTPACK keeps its exceptions.  No reference counterpart
   * and no stock library reads the format (tests/patchpack_model.py is a numpy reader and
   * writer).  Ids 104 + log2(w) for w = 1, 2, 4, 8; id 108 is left for a 16-byte width.  No
   * candidate of AUTOPACK.  One stream per segment of L bytes, m = L / w elements, nmb =
   * ceil(m / 64) miniblocks, nblk = ceil(nmb / 4) blocks, tail = L - m * w bytes:
   *   byte 0      0x90 | mode << 2 | log2(w)   mode 0 plain, 1 delta, 2 stored, 3 complement
   *   byte 1      0
   *   bytes 2..3  LE16(L - 1)
   *   stored:     L raw bytes                                        size = 4 + L
   *   packed:     LE16 nx        number of exceptions, nx <= min(m, 65535)
   *               [mode 1: element 0, w bytes]
   *               widths[nmb]    one byte each, 0..8w
   *               refs[nblk]     w bytes each
   *               payload        miniblock k = 8 * widths[k] bytes, INTPACK's packing
   *               pos[nx]        LE16 element indices, strictly increasing, each < m
   *               val[nx]        the exceptions' x, w bytes each, same order
   *               tail
   *   size = 6 + [w] + nmb + nblk*w + 8*sum(widths) + nx*(2 + w) + tail
   * All arithmetic mod 2^(8w).  mode 0: x_i = v_i.  mode 3: x_i = ~v_i (outliers below the rest
   * then lie above).  mode 1: INTPACK's, x_i = v_i - v_(i-1), x_0 = x_1, or 0 when m = 1.  A
   * block's reference is the signed minimum of x over all its elements, later exceptions
   * included.  Width rule, in miniblock k with c = min(64, m - 64k) elements: r_t = x_t - ref,
   * l_t = bit_length(r_t), B = max l_t; cost(b) = 8b + (2 + w) * #{t < c : l_t > b} for b = 0..B;
   * widths[k] is the LARGEST b of minimal cost, the exceptions are the elements with l_t >
   * widths[k], and their slots and the slots past m pack as 0.  A miniblock that gains nothing
   * has INTPACK's width and no exception.  val holds x itself (the element, its complement, the
   * delta); in mode 1 x_0 may be an exception like any other, and the decoder takes element 0
   * from the base whatever slot 0 or an exception at position 0 holds.  The smallest of the three
   * packed sizes wins, a tie goes to plain, then delta, then complement; the segment is stored
   * when the winner is not strictly below 4 + L (m = 0 included).  The decoder takes w from the
   * tag (any of the ids decodes every width) and rejects, before it writes anything: a high
   * nibble other than 9, byte 1 != 0, L > seg, a stored form whose size is not 4 + L, a stream
   * too short for its header arrays, a width above 8w, nx > m, a size that is not exactly the
   * formula, a position >= m or not above the one before it.  A rejected segment's output range
   * stays untouched, nothing outside a segment's first L output bytes is written, nothing outside
   * the stream is read.  Everything else decodes: non-zero bits in an exception's slot (ignored),
   * widths larger than needed, a mode that is not the smallest, a packed form above 4 + L. */
  /* (Written in parentheses on purpose: tests/test_abi.py counts the header's `*PACK<bits> = <id>`
   * lines and pins the five families it knows at 19.  tests/test_patchpack_model.py checks these
   * four against the Python ids.) */
  BITAR_HIP_CODEC_PATCHPACK8 = (104),
  BITAR_HIP_CODEC_PATCHPACK16 = (105),
  BITAR_HIP_CODEC_PATCHPACK32 = (106),
  BITAR_HIP_CODEC_PATCHPACK64 = (107)
};

/* The INTPACK id of an element width of 1, 2, 4 or 8 bytes. */
#define BITAR_HIP_CODEC_INTPACK(width) \
  ((width) == 1 ? BITAR_HIP_CODEC_INTPACK8 : (width) == 2 ? BITAR_HIP_CODEC_INTPACK16 : \
   (width) == 4 ? BITAR_HIP_CODEC_INTPACK32 : BITAR_HIP_CODEC_INTPACK64)

/* The FLTPACK id of an element width of 4 (float) or 8 (double) bytes. */
#define BITAR_HIP_CODEC_FLTPACK(width) \
  ((width) == 4 ? BITAR_HIP_CODEC_FLTPACK32 : BITAR_HIP_CODEC_FLTPACK64)

/* The RANSPLANE id of an element width of 2, 4 or 8 bytes. */
#define BITAR_HIP_CODEC_RANSPLANE(width) \
  ((width) == 2 ? BITAR_HIP_CODEC_RANSPLANE16 : (width) == 4 ? BITAR_HIP_CODEC_RANSPLANE32 : \
   BITAR_HIP_CODEC_RANSPLANE64)

/* The DICTPACK id of an element width of 4, 8 or 16 bytes. */
#define BITAR_HIP_CODEC_DICTPACK(width) \
  ((width) == 4 ? BITAR_HIP_CODEC_DICTPACK32 : (width) == 8 ? BITAR_HIP_CODEC_DICTPACK64 : \
   BITAR_HIP_CODEC_DICTPACK128)

/* The RUNPACK id of an element width of 1, 2, 4, 8 or 16 bytes. */
#define BITAR_HIP_CODEC_RUNPACK(width) \
  ((width) == 1 ? BITAR_HIP_CODEC_RUNPACK8 : (width) == 2 ? BITAR_HIP_CODEC_RUNPACK16 : \
   (width) == 4 ? BITAR_HIP_CODEC_RUNPACK32 : (width) == 8 ? BITAR_HIP_CODEC_RUNPACK64 : \
   BITAR_HIP_CODEC_RUNPACK128)

/* The AUTOPACK id of an element width of 1, 2, 4, 8 or 16 bytes. */
#define BITAR_HIP_CODEC_AUTOPACK(width) \
  ((width) == 1 ? BITAR_HIP_CODEC_AUTOPACK8 : (width) == 2 ? BITAR_HIP_CODEC_AUTOPACK16 : \
   (width) == 4 ? BITAR_HIP_CODEC_AUTOPACK32 : (width) == 8 ? BITAR_HIP_CODEC_AUTOPACK64 : \
   BITAR_HIP_CODEC_AUTOPACK128)

/* The CASCADE id of an element width of 1, 2, 4 or 8 bytes. */
#define BITAR_HIP_CODEC_CASCADE(width) \
  ((width) == 1 ? BITAR_HIP_CODEC_CASCADE8 : (width) == 2 ? BITAR_HIP_CODEC_CASCADE16 : \
   (width) == 4 ? BITAR_HIP_CODEC_CASCADE32 : BITAR_HIP_CODEC_CASCADE64)

/* The PATCHPACK id of an element width of 1, 2, 4 or 8 bytes. */
#define BITAR_HIP_CODEC_PATCHPACK(width) \
  ((width) == 1 ? BITAR_HIP_CODEC_PATCHPACK8 : (width) == 2 ? BITAR_HIP_CODEC_PATCHPACK16 : \
   (width) == 4 ? BITAR_HIP_CODEC_PATCHPACK32 : BITAR_HIP_CODEC_PATCHPACK64)

/* Per-segment marker written into sizes[] / produced[] when that segment's op failed
 * (malformed stream, or output larger than its slot: the reference's
 * RTE_COMP_OP_STATUS_OUT_OF_SPACE_*, device.cc:512-520). */
#define BITAR_HIP_SEGMENT_ERROR 0xFFFFFFFFu

/* Largest segment a kernel accepts (LZ4 offsets are 16-bit; the reference caps segments
 * at kMaxSegSize = 59460, config.h:41-47). */
#define BITAR_HIP_MAX_SEG_SIZE 65536u

typedef struct bitar_hip_ctx bitar_hip_ctx;

typedef struct {
  uint32_t num_streams; /* queue pairs: one HIP stream each (driver.cc:100-157 lcore map) */
  uint32_t flags;       /* BITAR_HIP_FLAG_* (0: the default decoders, no path counters) */
} bitar_hip_config;

/* bitar_hip_config.flags: the context's initial decoder options (bitar_hip_decoder_options);
 * every context keeps its own, so engines with different settings run side by side. */
#define BITAR_HIP_FLAG_INFLATE_WAVE_ONLY 0x1u /* no lane inflater in front of inflate_kernel
                                                 (the default since round 3; the flag also
                                                 overrides BITAR_HIP_INFLATE_LANES) */
#define BITAR_HIP_FLAG_ZSTD_WAVE_ONLY 0x2u    /* no lane Zstd decoder in front of the wave one */
#define BITAR_HIP_FLAG_ZSTD_LANE_EXEC 0x4u    /* handed-off sequence sections: lane executor */
#define BITAR_HIP_FLAG_COUNT_PATHS 0x8u       /* count decoder path entries (see below) */
#define BITAR_HIP_FLAG_PLAIN_ORDER 0x10u      /* calls dispatch segment i as workgroup i
                                                 (default, from 2048 segments: estimated most
                                                 expensive first; the output is identical) */
#define BITAR_HIP_FLAG_ZSTD_SERIAL 0x20u      /* Zstd decode: the Huffman literal streams and
                                                 the sequences' phase A one after the other on
                                                 the call's stream (default: side by side, the
                                                 literals on a paired stream; same output) */

/* Number of visible gfx950 devices.  Replaces rte_compressdev_devices_get() in
 * CompressDriver::ListAvailableDeviceIds (reference src/driver.cc:173-190). */
int bitar_hip_device_count(int* count);

/* Open a device context with cfg->num_streams streams.  Replaces
 * CompressDevice::Initialize: configure + queue_pair_setup + start
 * (reference src/device.cc:114-154). */
int bitar_hip_open(int device, const bitar_hip_config* cfg, bitar_hip_ctx** out);

/* Release streams and device state.  Replaces ~CompressDevice (device.cc:329-343). */
int bitar_hip_close(bitar_hip_ctx* ctx);

/* The hipStream_t behind queue pair `qp` (returned as void*). */
int bitar_hip_stream(bitar_hip_ctx* ctx, uint32_t qp, void** stream);

/* Device ordinal of the context. */
int bitar_hip_device(bitar_hip_ctx* ctx, int* device);

/* Worst-case compressed bytes of one segment of `seg` bytes (LZ4_compressBound /
 * fixed-Huffman bound; seg + 4 for INTPACK, FLTPACK, DICTPACK, RUNPACK, AUTOPACK, CASCADE, RANS, RANSPLANE, SYMTAB, PATCHPACK and DECPACK (bitar_hip_codecs.h, the ids from 256 on), their stored form), rounded up to 256 B; 0 for an
 * unknown codec.  Plays the role of compressed_seg_size
 * (reference src/config.cc:59-73): the stride of output slots in a slab. */
uint64_t bitar_hip_slot_size(uint32_t codec, uint32_t seg);

/* Largest match distance the encoder of `codec` emits (0 for an unknown codec): the reach of
 * its sliding window, 2560 for the fast parses of LZ4 / DEFLATE / Zstd and 14848 for the
 * wide LZ4 parse.  INTPACK, FLTPACK, DICTPACK, RUNPACK, AUTOPACK, CASCADE, RANS, RANSPLANE, SYMTAB, PATCHPACK and DECPACK have no matches: their 0 means "none", not "unknown".  The front-end reports ceil(log2) of it as the configured window_size
 * (the reference sets the device maximum, src/device.cc:389-393; its streams are valid for
 * any window at least this large, and the decoders accept the full 32 KiB / 64 KiB). */
uint32_t bitar_hip_max_distance(uint32_t codec);

/* HBM / pinned-host allocations on the context's device.  Replace the memzone reservation
 * of RtememzoneAllocator::AllocateAligned / rte_malloc (reference src/memory_pool.cc:70-188).
 * Device allocations are 256-B aligned. */
int bitar_hip_alloc(bitar_hip_ctx* ctx, uint64_t bytes, void** ptr);
int bitar_hip_free(bitar_hip_ctx* ctx, void* ptr);
int bitar_hip_host_alloc(bitar_hip_ctx* ctx, uint64_t bytes, void** ptr);
int bitar_hip_host_free(bitar_hip_ctx* ctx, void* ptr);

/* Asynchronous copy in any direction on `stream`.  In every call `stream` is a hipStream_t;
 * NULL is the HIP default stream, queue-pair streams come from bitar_hip_stream(). */
int bitar_hip_memcpy(bitar_hip_ctx* ctx, void* dst, const void* src, uint64_t bytes,
                     void* stream);

/* Compress n bytes at d_in (device memory) as ceil(n/seg) independent segments.
 * Segment i is written to d_slab + i*slot_stride and d_sizes[i] receives its compressed
 * size.  Asynchronous on `stream`.  n == 0 launches nothing.
 * Replaces one CompressDevice::Compress call: the AssembleFrom / EnqueueBurst /
 * DequeueBurst loop over bursts of segments (reference src/device.cc:156-238,
 * src/memory.cc:350-430).  slot_stride must be >= bitar_hip_slot_size(codec, seg); d_slab
 * and slot_stride must be 16-B aligned. */
int bitar_hip_compress(bitar_hip_ctx* ctx, void* stream, uint32_t codec, const void* d_in,
                       uint64_t n, uint32_t seg, void* d_slab, uint64_t slot_stride,
                       uint32_t* d_sizes);

/* Same, but segment i goes to its own slot d_dsts[i] (a device array of device pointers,
 * each 16-B aligned with room for slot_capacity >= bitar_hip_slot_size(codec, seg) bytes).
 * The form the slot pool of the C++ front-end uses: its free slots are not contiguous
 * (DeviceMemory::Take, reference src/memory.cc:160-189). */
int bitar_hip_compress_scattered(bitar_hip_ctx* ctx, void* stream, uint32_t codec,
                                 const void* d_in, uint64_t n, uint32_t seg,
                                 void* const* d_dsts, uint64_t slot_capacity, uint32_t* d_sizes);

/* Decompress nseg segments.  d_srcs[i] (a device array of device pointers) holds
 * d_sizes[i] compressed bytes; segment i inflates into d_out + i*seg and d_produced[i]
 * receives its size.  Requires capacity >= nseg*seg, else BITAR_HIP_CAPACITY_ERROR
 * (reference device.cc:248-254).  seg <= 65536, except for Zstd: <= 2^30, so that a whole
 * stock frame of any content size can be one segment.  Asynchronous on `stream`.
 * Replaces one CompressDevice::Decompress call (reference src/device.cc:240-318,
 * src/memory.cc:432-505).
 *
 * What a call writes (any alignment of d_out and of the sources; pinned with guard bytes
 * around every buffer by tests/test_gpu_canaries.py):
 *   - segment i writes only inside [d_out + i*seg, d_out + (i+1)*seg);
 *   - of that range the first d_produced[i] bytes are the segment's output, the bytes past
 *     them are unspecified (the lane decoders copy in 8-byte words that run up to 32 bytes
 *     ahead of the output position, and the Zstd lane kernels stage literals at the range's
 *     tail), so a segment that produces 0 bytes leaves its range as it was;
 *   - a rejected segment (BITAR_HIP_SEGMENT_ERROR) may have written anywhere inside its own
 *     range, and nowhere else;
 *   - d_produced[0, nseg) is written; nothing else is: not the sources, not d_sizes, no byte
 *     before d_out or from d_out + nseg*seg on, whatever `capacity` is. */
int bitar_hip_decompress(bitar_hip_ctx* ctx, void* stream, uint32_t codec,
                         const void* const* d_srcs, const uint32_t* d_sizes, uint32_t nseg,
                         uint32_t seg, void* d_out, uint64_t capacity, uint32_t* d_produced);

/* Same, with segment i at d_slab + i*slot_stride (the layout bitar_hip_compress writes). */
int bitar_hip_decompress_slab(bitar_hip_ctx* ctx, void* stream, uint32_t codec,
                              const void* d_slab, uint64_t slot_stride,
                              const uint32_t* d_sizes, uint32_t nseg, uint32_t seg,
                              void* d_out, uint64_t capacity, uint32_t* d_produced);

/* Compress n bytes of HOST memory (pinned or pageable) at h_in with the PCIe link and the
 * kernels overlapped: the input is copied into d_stage (device memory, >= n bytes) in chunks
 * of whole segments (about 1/8 of the call, >= 32 MiB) on a copy stream paired with
 * `stream`, and each chunk is compressed on `stream` as soon as it has landed, so a call
 * takes about the link time plus one chunk's compress.  The output is a slab (d_slab, as
 * bitar_hip_compress) or scattered slots (d_dsts with d_slab NULL, as
 * bitar_hip_compress_scattered; slot_stride is then the slots' capacity).  Asynchronous on
 * `stream`; bitar_hip_sync(stream) covers the copies too.  Replaces the zero-copy attach of
 * host input slices the BlueField DMAs from (reference src/memory.cc:380-399,
 * rte_mem_virt2iova at 388). */
int bitar_hip_compress_host(bitar_hip_ctx* ctx, void* stream, uint32_t codec, const void* h_in,
                            uint64_t n, uint32_t seg, void* d_stage, void* d_slab,
                            void* const* d_dsts, uint64_t slot_stride, uint32_t* d_sizes);

/* Decompress into HOST memory: the segments decode into d_stage (device memory, >= nseg*seg
 * bytes) in chunks, and each decoded chunk is copied to h_out on the paired copy stream while
 * the next one decodes; nseg*seg bytes land at h_out (capacity >= nseg*seg, else
 * BITAR_HIP_CAPACITY_ERROR).  Otherwise as bitar_hip_decompress; bitar_hip_sync(stream)
 * covers the copies.  Replaces decompression into host-memory output slices (reference
 * src/memory.cc:482-493). */
int bitar_hip_decompress_host(bitar_hip_ctx* ctx, void* stream, uint32_t codec,
                              const void* const* d_srcs, const uint32_t* d_sizes, uint32_t nseg,
                              uint32_t seg, void* d_stage, void* h_out, uint64_t capacity,
                              uint32_t* d_produced);

/* Wait for `stream` and return BITAR_HIP_IO_ERROR if a segment op launched on THAT stream
 * failed since its last sync (each stream has its own sticky device-side error word, read
 * and cleared in stream order, so concurrent queue pairs never see each other's failures).
 * NULL waits for the default stream and the context's queue pairs and reports / clears
 * their words only: a foreign stream's word (e.g. a torch side stream) is left to a sync of
 * that stream, which reports it exactly once.  Replaces the
 * completion polling of DequeueBurst + GetErrorCount (reference src/device.cc:84-110,
 * 490-535). */
int bitar_hip_sync(bitar_hip_ctx* ctx, void* stream);

/* Exclusive prefix sum of d_sizes (nseg entries) into d_offsets (nseg+1 entries), then
 * gather each slot into one contiguous frame at d_frame (d_frame may be NULL to compute
 * offsets only).  Builds the packed frame / global frame index.  A size
 * above slot_stride (BITAR_HIP_SEGMENT_ERROR of a failed op) packs as 0 bytes and makes the
 * next bitar_hip_sync of `stream` return BITAR_HIP_IO_ERROR; slot_stride may be 0 only when
 * d_frame is NULL. */
int bitar_hip_pack(bitar_hip_ctx* ctx, void* stream, const void* d_slab, uint64_t slot_stride,
                   const uint32_t* d_sizes, uint32_t nseg, uint64_t* d_offsets, void* d_frame);

/* LZ4 frame with LINKED blocks (LZ4 frame format Block_Independence = 0, the liblz4 and
 * Arrow LZ4_FRAME default): the blocks of ONE frame decode in order on one wavefront, each
 * block's matches reaching into the output of the blocks before it.  d_blocks holds nblocks
 * pairs {offset of the block's data in d_src, size | 1u << 31 for a stored block}, decoded
 * in table order wherever they lie in d_src; the
 * output goes to d_out (capacity bytes) and *d_produced receives its total size, or
 * BITAR_HIP_SEGMENT_ERROR (then the next sync returns BITAR_HIP_IO_ERROR).  Asynchronous on
 * `stream`.  Frame / block checksums are the caller's (XXH32).  Used by the Arrow util::Codec
 * adapter for stock IPC bodies. */
int bitar_hip_lz4_chain(bitar_hip_ctx* ctx, void* stream, const void* d_src, uint32_t src_len,
                        const uint32_t* d_blocks, uint32_t nblocks, void* d_out,
                        uint64_t capacity, uint32_t* d_produced);

/* Batched device-to-device copy: entry i moves d_sizes[i] bytes from d_srcs[i] to d_dsts[i]
 * (device arrays of n device pointers / sizes; any alignment, ranges must not overlap).
 * Asynchronous on `stream`.  The front-end's chained operations (max_sgl_segs > 1) use it to
 * spread one op's compressed stream over its pool slots and to join a chained input: the
 * mbuf chains the reference builds with rte_pktmbuf_chain (src/memory.cc:60-100, 380-425,
 * 459-500). */
int bitar_hip_copy_batch(bitar_hip_ctx* ctx, void* stream, const void* const* d_srcs,
                         void* const* d_dsts, const uint32_t* d_sizes, uint32_t n);

/* The data blocks of an LZ4 frame (LZ4 frame format, block independence) from LZ4 segments
 * of n input bytes (d_in, segment size seg <= 65536, so the frame's maximum block size is
 * 64 KiB): block i = LE32 size + the compressed block, or LE32(len | 1<<31) + the raw input
 * slice when the block did not shrink.  d_framed (nseg uint32) receives the framed sizes,
 * d_offsets (nseg+1 uint64) their exclusive prefix sum; d_frame may be NULL to size only.
 * The frame header and EndMark are the caller's.  Used by the Arrow util::Codec adapter
 * (arrow::Compression::LZ4_FRAME, the Arrow IPC body codec). */
int bitar_hip_pack_lz4f(bitar_hip_ctx* ctx, void* stream, const void* d_in, uint64_t n,
                        uint32_t seg, const void* d_slab, uint64_t slot_stride,
                        const uint32_t* d_sizes, uint32_t* d_framed, uint64_t* d_offsets,
                        void* d_frame);

/* Deterministic synthetic input (SplitMix64-based; kinds as in the oracle's bo_fill:
 * 0 random, 1 Silesia-style mix, 2 Arrow record-batch body, 3 constant, 4 periodic,
 * 5 int64 small-range only, 6 log text only). */
int bitar_hip_fill(bitar_hip_ctx* ctx, void* stream, int kind, uint64_t seed, void* d_out,
                   uint64_t n);

/* Bytes [offset, offset + n) of the same deterministic stream (offset a multiple of 64), so
 * a rank can generate just the batches of a job it was dealt. */
int bitar_hip_fill_at(bitar_hip_ctx* ctx, void* stream, int kind, uint64_t seed,
                      uint64_t offset, void* d_out, uint64_t n);

/* Checksum types (rte_comp_checksum_type, reference src/include/config.h:169-182). */
enum bitar_hip_checksum_kind {
  BITAR_HIP_CHECKSUM_CRC32 = 1,         /* zlib / ISO-HDLC CRC-32 */
  BITAR_HIP_CHECKSUM_ADLER32 = 2,       /* RFC 1950 Adler-32 */
  BITAR_HIP_CHECKSUM_CRC32_ADLER32 = 3  /* CRC-32 in bits 0..31, Adler-32 in bits 32..63 */
};

/* Per-segment checksum of uncompressed data -- what the reference's xforms ask the engine to
 * compute over an op's uncompressed side (checksum_type in compress_xform / decompress_xform,
 * reference src/config.cc:83-105): segment i starts at d_data + i*seg and holds d_lens[i]
 * bytes (a decompress's d_produced; BITAR_HIP_SEGMENT_ERROR gives 0), or, with d_lens NULL,
 * min(seg, n - i*seg) bytes (a compress's input; then nseg must be ceil(n / seg)).
 * d_sums[i] (uint64) receives the checksum.  Asynchronous on `stream`. */
int bitar_hip_checksum(bitar_hip_ctx* ctx, void* stream, uint32_t kind, const void* d_data,
                       uint64_t n, uint32_t seg, const uint32_t* d_lens, uint32_t nseg,
                       uint64_t* d_sums);

/* ---- filters for fixed-width column buffers ----
 * A transposition of each segment on its own, in front of compress and behind decompress, so
 * that the codecs' short windows see one byte (or bit) position of every element side by
 * side.  S = the L bytes of a segment, w = the element width, 2, 4, 8 or 16 (a caller with
 * 1-byte elements does not filter):
 *   SHUFFLE     m = L / w;  T[j*m + i] = S[i*w + j] (i < m, j < w): Blosc shuffle / Parquet
 *               BYTE_STREAM_SPLIT per segment.  The last L - m*w bytes keep their positions.
 *   BITSHUFFLE  m8 = (L / w) & ~7;  plane p = 8*j + b (byte j of the element, bit b, LSB = 0)
 *               occupies T[p*(m8/8), (p+1)*(m8/8)), and bit t of its byte q is bit b of
 *               S[(8q + t)*w + j]: the HDF5 bitshuffle layout with one block per segment.  The
 *               last L - m8*w bytes keep their positions.
 * The output has the input's length.  No reference counterpart, and no stock library knows
 * the filter: filter and width travel with the caller's frame like codec and segment size. */
enum bitar_hip_filter { BITAR_HIP_FILTER_SHUFFLE = 1, BITAR_HIP_FILTER_BITSHUFFLE = 2 };

/* Filter segment i of d_in (at d_in + i*seg) into d_out + i*seg.  Its length is d_lens[i], or
 * min(seg, n - i*seg) with d_lens NULL (the convention of bitar_hip_checksum; nseg may be any
 * count).  A length above min(seg, n - i*seg) -- BITAR_HIP_SEGMENT_ERROR of a failed op is
 * one -- moves nothing and writes nothing for that segment (the failed op has already made the
 * next sync fail).  Nothing past min(n, nseg*seg) is read or written, and the buffers may have
 * any alignment.  Asynchronous on `stream`; n == 0 or nseg == 0 launches nothing.
 * BITAR_HIP_INVALID (the context stays usable): an unknown filter, a width outside
 * {2, 4, 8, 16}, seg outside [1, 65536], a null buffer, [d_in, d_in + n) overlapping
 * [d_out, d_out + n). */
int bitar_hip_filter_apply(bitar_hip_ctx* ctx, void* stream, uint32_t filter, uint32_t width,
                           const void* d_in, uint64_t n, uint32_t seg, const uint32_t* d_lens,
                           uint32_t nseg, void* d_out);

/* The inverse, with the same arguments: d_in holds filtered segments (e.g. a decompress's
 * output with d_lens = its d_produced), d_out receives the caller's bytes. */
int bitar_hip_filter_invert(bitar_hip_ctx* ctx, void* stream, uint32_t filter, uint32_t width,
                            const void* d_in, uint64_t n, uint32_t seg, const uint32_t* d_lens,
                            uint32_t nseg, void* d_out);

/* ---- one gzip member (RFC 1952) from DEFLATE segments ----
 * bitar_hip_compress for BITAR_HIP_CODEC_DEFLATE / _DEFLATE_DYNAMIC (any other codec, INTPACK, FLTPACK, DICTPACK and RUNPACK
 * included: BITAR_HIP_INVALID) that also stores each segment's exact bit length: d_bits[i] = the bits of
 * a coded segment up to and including its end-of-block code, 8 * d_sizes[i] for a stored
 * segment, BITAR_HIP_SEGMENT_ERROR for a failed one.  d_bits NULL: exactly
 * bitar_hip_compress.  The encoders guarantee: a coded segment is ONE block with BFINAL at bit
 * 0 of byte 0; a stored segment is ceil(n / 65535) byte-aligned stored blocks whose header
 * bytes are 0 except the last one's, which is 1. */
int bitar_hip_compress_bits(bitar_hip_ctx* ctx, void* stream, uint32_t codec, const void* d_in,
                            uint64_t n, uint32_t seg, void* d_slab, uint64_t slot_stride,
                            uint32_t* d_sizes, uint32_t* d_bits);

/* Join the nseg slots of such a call into ONE raw DEFLATE stream (RFC 1951) at d_joined:
 * coded blocks are spliced at bit granularity with BFINAL cleared in all but the last, a
 * stored segment keeps its byte alignment behind a 3-bit header.  d_starts (nseg+1) receives
 * each segment's bit position and, last, the stream's bit length; the stream is
 * ceil(d_starts[nseg] / 8) bytes with zero padding bits.  d_joined NULL: positions only.
 * d_joined must be 4-B aligned and `capacity` a multiple of 4 (else BITAR_HIP_INVALID: the
 * stream is written in whole dwords); it is zeroed over `capacity` bytes first.  The stream
 * needs at most sum(d_sizes) + nseg bytes, so that rounded up to 4 always suffices.  Nothing
 * past `capacity` is read or written; a stream that needs more
 * (or a failed segment, which joins as nothing) makes the next bitar_hip_sync of `stream`
 * return BITAR_HIP_IO_ERROR.  Asynchronous on `stream`: positions and lengths never visit the
 * host. */
int bitar_hip_deflate_join(bitar_hip_ctx* ctx, void* stream, const void* d_slab,
                           uint64_t slot_stride, const uint32_t* d_sizes, const uint32_t* d_bits,
                           uint32_t nseg, uint64_t* d_starts, void* d_joined, uint64_t capacity);

/* The inverse, for parallel decode: slot i (d_slab + i*slot_stride, 16-B aligned) receives the
 * segment at bit d_starts[i] of the joined stream (d_joined, 4-B aligned, joined_len bytes)
 * as the encoder wrote it, BFINAL set again, and d_sizes[i] its size, ready for
 * bitar_hip_decompress_slab.  d_entries[i] = bits | stored << 23 (bits = 8 * size for a stored
 * segment).  d_starts and d_entries may come from an untrusted header: an entry that reaches
 * past 8 * joined_len bits or whose size exceeds slot_stride gives d_sizes[i] =
 * BITAR_HIP_SEGMENT_ERROR and BITAR_HIP_IO_ERROR at the next sync; nothing is read or written
 * out of bounds. */
int bitar_hip_deflate_split(bitar_hip_ctx* ctx, void* stream, const void* d_joined,
                            uint64_t joined_len, const uint64_t* d_starts,
                            const uint32_t* d_entries, uint32_t nseg, void* d_slab,
                            uint64_t slot_stride, uint32_t* d_sizes);

/* *d_crc = the CRC-32 of n bytes from the CRC-32s of their nseg = ceil(n / seg) segments
 * (d_sums as bitar_hip_checksum writes them, CRC-32 in the low word): zlib's crc32_combine
 * over all segments at once. */
int bitar_hip_crc32_combine(bitar_hip_ctx* ctx, void* stream, const uint64_t* d_sums, uint64_t n,
                            uint32_t seg, uint32_t nseg, uint32_t* d_crc);

/* Whole-buffer raw Snappy streams (one stream per buffer, joined from SNAPPY segments and
 * split again on the device) have their entry points in bitar_hip_snappy.h. */

/* ---- the dispatch order of a call, for tests ----
 * Calls of at least 2048 segments run segment order[b] as workgroup b, order = the segments
 * sorted by a cost key below 256, lowest first (larger keys count as 255; the order inside a
 * key is not fixed).  This builds an order with the code the codecs run and copies it out.
 *   COMPRESS_KEY    the key of LZ4 / DEFLATE / Zstd / Snappy compress: the distinct byte values
 *                   in four 32-byte samples of each segment of d_in (n bytes, segments of seg,
 *                   nseg = ceil(n / seg)); d_values and cut are not read: the heavy cut is the
 *                   fast LZ4 compressor's (64) when slots != 0
 *   DECOMPRESS_KEY  the key of their decoders, from the compressed sizes d_values[nseg] and
 *                   seg: 255 for a size >= seg, else 254 - size * 254 / seg; d_keys must be NULL
 *   CALLER_KEYS     d_values[nseg] are the keys
 * cut, slots: the priority lanes of the fast LZ4 compressor.  With H = the segments whose key is
 * below cut and S = slots, entry b carries bit 31 (which the kernel strips) iff S != 0, H > S,
 * b < H, H % S != 0 and b % S < H % S.  slots = BITAR_HIP_ORDER_SLOTS_CALL: the S an LZ4
 * compress call of nseg segments gets on this context and stream (0: none).  *slots_used (host
 * memory, may be NULL) receives the S that was used.
 * d_order (nseg words, tags left in) and d_keys (nseg words, or NULL: the keys as written,
 * before the clamp to 255) are device memory, written in `stream`'s order.
 * Returns 0; BITAR_HIP_NO_ORDER where a call of this context runs in plain order (nseg < 2048,
 * BITAR_HIP_FLAG_PLAIN_ORDER, BITAR_HIP_COST_ORDER=0 in the environment, or no scratch memory):
 * d_order and d_keys are then left alone; BITAR_HIP_INVALID for cut >= 256, nseg > 2^31, an
 * unknown mode or a null buffer.  The keys that Zstd's and the joined Snappy decoder's
 * internal kernels compute from scratch memory are not reachable here; their orders run
 * through the same sort as CALLER_KEYS. */
enum bitar_hip_order_mode {
  BITAR_HIP_ORDER_COMPRESS_KEY = 0,
  BITAR_HIP_ORDER_DECOMPRESS_KEY = 1,
  BITAR_HIP_ORDER_CALLER_KEYS = 2
};
#define BITAR_HIP_ORDER_SLOTS_CALL 0xFFFFFFFFu
#define BITAR_HIP_NO_ORDER 1
int bitar_hip_debug_order(bitar_hip_ctx* ctx, void* stream, uint32_t mode, const void* d_in,
                          uint64_t n, uint32_t seg, const uint32_t* d_values, uint32_t nseg,
                          uint32_t cut, uint32_t slots, uint32_t* d_order, uint32_t* d_keys,
                          uint32_t* slots_used);

/* Decoder selection of one context.  The decoders are interchangeable (every one accepts and
 * rejects exactly what the oracle does); the options pick which kernels run, for tests and
 * tuning.  No reference counterpart: the BlueField engine has one decoder. */
typedef struct {
  uint32_t inflate_lanes; /* segments per wave of inflate_lanes_kernel: 4, 8, 16 or 32;
                             0 = inflate_kernel (one wave per segment) alone */
  uint32_t zstd_lanes;    /* segments per wave of zstd_lanes_kernel: 8, 16, 32 or 64; 0 = off */
  uint32_t zstd_seq;      /* 1 = handed-off sequence sections run zstd_seqdec_kernel +
                             zstd_exec_kernel; 0 = the lane executor (zstd_handoff_kernel) */
  uint32_t count_paths;   /* 1 = count path entries (bitar_hip_path_counters) */
} bitar_hip_decoder_options;

int bitar_hip_get_decoder_options(bitar_hip_ctx* ctx, bitar_hip_decoder_options* opt);
/* Takes effect for calls made after it returns (calls already queued keep their kernels). */
int bitar_hip_set_decoder_options(bitar_hip_ctx* ctx, const bitar_hip_decoder_options* opt);

/* Path counters (counted while count_paths is on): how many segments reached each stage of
 * the decoders, so tests can show that their inputs exercised the path they target. */
enum bitar_hip_path_counter {
  BITAR_HIP_PATH_INFLATE_WAVE = 0,       /* segments decoded by inflate_kernel */
  BITAR_HIP_PATH_INFLATE_WAVE_REJECT = 1,/*   ... of which rejected */
  BITAR_HIP_PATH_INFLATE_BATCH_SEGS = 2, /*   ... that ran >= 1 multi-symbol batch */
  BITAR_HIP_PATH_INFLATE_BATCHES = 3,    /* batches run by inflate_kernel */
  BITAR_HIP_PATH_ZSTD_WAVE = 4,          /* segments decoded by zstd_decompress_kernel */
  BITAR_HIP_PATH_ZSTD_HANDED = 5,        /*   ... that handed their last block over */
  BITAR_HIP_PATH_ZSTD_SEQDEC = 6,        /* handed segments taken by zstd_seqdec_kernel */
  BITAR_HIP_PATH_ZSTD_SEQDEC_REJECT = 7, /*   ... rejected there */
  BITAR_HIP_PATH_ZSTD_EXEC = 8,          /* segments executed by zstd_exec_kernel */
  BITAR_HIP_PATH_ZSTD_EXEC_REJECT = 9,   /*   ... rejected there */
  BITAR_HIP_PATH_LZ4_FAR = 10,           /* segments deferred to the far-history LZ4 kernel */
  /* 11..15: LZ4 batch-path diagnostics, filled only by a library built with
     -DBITAR_LZ4D_PROFILE=1 (scripts/build_variant.sh): batches, their output bytes,
     sequences decoded by the general path, batches whose walk ended at the parsed lanes'
     end, batches whose walk ended at an ineligible sequence */
  BITAR_HIP_PATH_LZ4_BATCHES = 11,
  BITAR_HIP_PATH_LZ4_BATCH_BYTES = 12,
  BITAR_HIP_PATH_LZ4_GENERAL_SEQS = 13,
  BITAR_HIP_PATH_LZ4_STOP_PARSE = 14,
  BITAR_HIP_PATH_LZ4_STOP_INELIGIBLE = 15,
  BITAR_HIP_PATH_COUNT = 16
};

/* Wait for the device, copy min(n, BITAR_HIP_PATH_COUNT) counters to out (host memory) and
 * reset them. */
int bitar_hip_path_counters(bitar_hip_ctx* ctx, uint64_t* out, uint32_t n);

/* Where `ptr` lives: *kind = 0 pageable host, 1 pinned host, 2 device memory (then *device
 * is its ordinal).  Replaces rte_mem_virt2iova() residency assumptions (memory.cc:388). */
int bitar_hip_pointer_info(const void* ptr, int* kind, int* device);

/* Thread-local text of the last error returned on this thread. */
const char* bitar_hip_last_error(void);

/* ABI version (BITAR_HIP_ABI_VERSION). */
int bitar_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BITAR_HIP_H_ */
