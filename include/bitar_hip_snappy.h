/*
 * bitar_hip_snappy.h -- whole-buffer raw Snappy streams on the MI355X segment codec engine
 * (libbitar_hip.so): entry points beside the core C ABI of bitar_hip.h, with its conventions
 * (plain pointers and sizes, 0 or a negated arrow::StatusCode, hipStream_t as void*).  They are
 * additive: BITAR_HIP_ABI_VERSION and the symbol list of bitar_hip.h are as they were.
 */
#ifndef BITAR_HIP_SNAPPY_H_
#define BITAR_HIP_SNAPPY_H_

#include "bitar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one raw Snappy stream from SNAPPY segments, and back ----
 * A whole-buffer raw Snappy stream (what Arrow, Parquet and every stock library write per
 * buffer) has one preamble and no segment index.  The join writes one from the slots of a
 * compress at 64 KiB segments; the split finds where each 64 KiB block of output begins in
 * ANY raw stream, on the device and without a serial walk; the decode reads the fragments
 * between those positions in one launch.  Stock writers cut their input at 64 KiB and start
 * every block's history afresh, so their streams decode this way too. */

/* Join the slots that bitar_hip_compress(..., BITAR_HIP_CODEC_SNAPPY, ...) wrote for n bytes at
 * seg == 65536 (any other seg: BITAR_HIP_INVALID) into ONE raw Snappy stream at d_joined: the
 * minimal varint of n, then every segment's stream less its own preamble (a stored segment
 * keeps its single literal element).  d_offsets (ceil(n / seg) + 1 entries) receives the
 * exclusive prefix sum of those body sizes, *d_joined_len (device memory, may be NULL) the
 * stream's length: preamble + d_offsets[nseg], at most n + 4 * nseg + 5.  d_joined NULL:
 * offsets and length only.  A stream above `capacity` is not written, and a segment whose
 * size is BITAR_HIP_SEGMENT_ERROR joins as nothing: either makes the next bitar_hip_sync of
 * `stream` return BITAR_HIP_IO_ERROR.  n == 0 gives the 1-byte stream 00.  Asynchronous on
 * `stream`; nothing visits the host. */
int bitar_hip_snappy_join(bitar_hip_ctx* ctx, void* stream, const void* d_slab,
                          uint64_t slot_stride, const uint32_t* d_sizes, uint64_t n, uint32_t seg,
                          uint64_t* d_offsets, void* d_joined, uint64_t capacity,
                          uint64_t* d_joined_len);

/* *d_status of bitar_hip_snappy_split */
enum bitar_hip_snappy_split_status {
  BITAR_HIP_SNAPPY_SPLIT_OK = 0,          /* every fragment start found, the chain is a valid stream */
  BITAR_HIP_SNAPPY_SPLIT_UNSUPPORTED = 1, /* valid, but an element straddles a multiple of 65536
                                             output bytes: no independent fragments */
  BITAR_HIP_SNAPPY_SPLIT_INVALID = 2,     /* no preamble, an element reads past the stream, or the
                                             elements' output is not exactly n bytes */
  BITAR_HIP_SNAPPY_SPLIT_INCOMPLETE = 3   /* the rounds ran out and the serial finish was forbidden */
};
/* ORed into max_rounds: no serial finish after the last round (tests and measurements) */
#define BITAR_HIP_SNAPPY_NO_SERIAL_FINISH 0x80000000u

/* The fragment starts of the raw Snappy stream d_joined[0, len) whose preamble declares n
 * bytes (the caller reads it: a varint of <= 5 bytes): d_starts[k], k < nfrag = ceil(n / 65536),
 * receives the stream offset at which output position k * 65536 begins, d_starts[nfrag] = len,
 * and *d_status (device memory) one of bitar_hip_snappy_split_status.  Unless the status is OK
 * the entries are unspecified, except that an entry no element start was found for is all
 * ones.  Copy offsets are not looked at (the fragment decoder checks them).  The method is
 * speculate-and-verify over tiles of 4096 stream bytes, at most max_rounds rounds (0: the
 * default, 64) and then one serial walk of what is not settled, so the result never depends
 * on max_rounds; d_stats (device memory, 4 words, may be NULL) receives the rounds run, the
 * tile walks, the tiles and whether the serial walk ran.  Reads nothing outside
 * [d_joined, d_joined + len), any alignment.  len above 4293918720: BITAR_HIP_NOT_IMPLEMENTED.
 * Asynchronous on `stream`; nothing visits the host. */
int bitar_hip_snappy_split(bitar_hip_ctx* ctx, void* stream, const void* d_joined, uint64_t len,
                           uint64_t n, uint32_t max_rounds, uint64_t* d_starts,
                           uint32_t* d_status, uint32_t* d_stats);

/* Decode the nfrag fragments of such a stream in one launch: fragment k is the stream's bytes
 * [d_starts[k], d_starts[k + 1]) -- elements only, no preamble -- and must produce exactly
 * min(65536, n - k * 65536) bytes at d_out + k * 65536; d_produced[k] receives that count.
 * Otherwise it is the segment decoder of BITAR_HIP_CODEC_SNAPPY, with its rules and its
 * contract on what is written (bitar_hip_decompress): offset 0, an offset beyond the bytes
 * produced in THIS fragment (stock streams have none; a copy reaching into the block before
 * is not decoded), an element past the fragment, leftover input and short output reject the
 * fragment -- d_produced[k] = BITAR_HIP_SEGMENT_ERROR, BITAR_HIP_IO_ERROR at the next sync --
 * as do starts that are not ascending positions inside the stream.  capacity >= n, else
 * BITAR_HIP_CAPACITY_ERROR; nothing from d_out + n on is written.  Call it only after a split
 * whose status is OK. */
int bitar_hip_snappy_decompress_joined(bitar_hip_ctx* ctx, void* stream, const void* d_joined,
                                       uint64_t len, uint64_t n, const uint64_t* d_starts,
                                       void* d_out, uint64_t capacity, uint32_t* d_produced);

#ifdef __cplusplus
}
#endif
#endif /* BITAR_HIP_SNAPPY_H_ */
