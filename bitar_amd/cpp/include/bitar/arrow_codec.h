// bitar/arrow_codec.h -- arrow::util::Codec adapters over the MI355X engine (SURVEY.md §8f
// rank 2: the Arrow IPC body-compression hook the reference demo leaves commented out,
// apps/demo_app.cc:148-150).
//
//   auto codec = bitar::MakeArrowCodec(arrow::Compression::ZSTD);    // or LZ4_FRAME, GZIP
//   auto snappy = bitar::MakeArrowSnappyCodec();                     // Compression::SNAPPY
//   auto opts = arrow::ipc::IpcWriteOptions::Defaults();
//   opts.codec = std::shared_ptr<arrow::util::Codec>(std::move(*codec));
//   // ... arrow::ipc::MakeStreamWriter(sink, schema, opts): bodies compressed on the GPU
//
// Compress cuts the input into 64 KiB segments, compresses them on the device and writes a
// standard stream any Arrow / libzstd / liblz4 / zlib reader decodes:
//   ZSTD       one Zstandard frame per segment, concatenated (RFC 8878 allows a stream of
//              frames; ZSTD_decompress and Arrow's ZSTD codec decode it whole);
//   LZ4_FRAME  one LZ4 frame (version 01, independent blocks, 64 KiB maximum block size, no
//              checksums) whose data blocks are the segments (a block that does not shrink
//              is stored uncompressed, as the frame format requires);
//   GZIP       ONE gzip member (RFC 1952; Arrow's one-shot GZIP decoder reads exactly one):
//              the segments' dynamic-Huffman DEFLATE streams joined at bit granularity into
//              one RFC 1951 stream on the device, CRC-32 and ISIZE in the trailer, and a
//              private FEXTRA subfield 'B','T' with each segment's bit length, by which this
//              codec splits the stream again and inflates the segments in parallel (layout:
//              src/gzip_frame.h).  Buffers above 21841 segments (about
//              1.33 GiB: the index must fit the 16-bit XLEN) are NotImplemented.
//   SNAPPY     (from MakeArrowSnappyCodec) ONE raw Snappy stream (no framing format; Parquet's default page codec): the
//              varint of the length, then the elements of every segment's stream, joined on
//              the device.  MaxCompressedLen is stock Snappy's 32 + n + n/6 (the stream is at
//              most n + 4 per segment + 5; a smaller output buffer is taken when the stream
//              fits, else CapacityError).  Decompress reads the varint, finds on the device
//              where each 64 KiB block of output begins (a boundary scan: no index exists and
//              none is needed) and decodes the blocks in one launch.  It takes every stream
//              whose elements do not cross a multiple of 64 KiB of output and whose copies stay
//              inside their block -- what stock writers produce.  Invalid: no preamble, a
//              declared length above the output buffer, an element past the end, a wrong total;
//              NotImplemented: "Snappy element across a 64 KiB block"; IOError: a block did not
//              decode (corrupt, or a copy that reaches before its 64 KiB block).
// Decompress walks the frame / block / member headers on the host (sizes only, no decoding)
// and decodes every segment on the device.  Beyond what Compress writes it takes the streams
// stock writers produce: Zstd frames of any content size up to 1 GiB (one segment each; a
// frame without a content size only as the stream's single frame), with or without a content
// checksum; LZ4 frames with linked or independent blocks of <= 64 KiB, block checksums,
// content size and content checksum (XXH32, verified); gzip members of <= 64 KiB content
// (any stock gzip of a small buffer) and concatenations of members whose lengths are known
// (BGZF files, by their 'B','C' subfield), CRC-32 and ISIZE verified.  What it cannot decode
// on the device -- Zstd / LZ4 dictionaries, LZ4 blocks above 64 KiB, a stock gzip member above
// 64 KiB (no index to decode it in parallel by) -- is NotImplemented, never a silent CPU
// fallback.  Host and HBM buffers are both accepted (host data is staged through HBM).
// Streaming compressors are NotImplemented.  The device context is opened by the first Compress
// or Decompress: making a codec and asking for MaxCompressedLen need no device.
#pragma once

#include <arrow/result.h>
#include <arrow/util/compression.h>

#include <memory>

namespace bitar {

/// A Codec for arrow::Compression::ZSTD, LZ4_FRAME or GZIP on HIP device `device`.  SNAPPY has a
/// factory of its own, below: here it is NotImplemented, as before that codec existed.
arrow::Result<std::unique_ptr<arrow::util::Codec>> MakeArrowCodec(
    arrow::Compression::type type, int device = 0);

/// A Codec for arrow::Compression::SNAPPY (one raw Snappy stream per buffer) on HIP device
/// `device`.
arrow::Result<std::unique_ptr<arrow::util::Codec>> MakeArrowSnappyCodec(int device = 0);

}  // namespace bitar
