// arrow_codec.cc -- arrow::util::Codec adapters (ZSTD, LZ4_FRAME, GZIP, SNAPPY) over the C ABI.
// See include/bitar/arrow_codec.h for the stream layouts.  Every payload byte is compressed
// and decompressed on the device; the host only walks frame / block / member headers (sizes)
// and writes the 7-byte LZ4 frame header and EndMark, or the gzip member header and trailer
// (gzip_frame.h); of a Snappy stream it reads the preamble alone.
#include "bitar/arrow_codec.h"

#include <arrow/status.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "bitar_hip.h"
#include "bitar_hip_snappy.h"
#include "gzip_frame.h"
#include "hip_ctx.h"

namespace bitar {

namespace {

constexpr uint32_t kSeg = 65536;  // segment = Zstd frame content = LZ4 frame block
constexpr uint32_t kZstdMagic = 0xFD2FB528u, kLz4fMagic = 0x184D2204u;
constexpr uint32_t kSkippableMagic = 0x184D2A50u;  // ..5F: skippable frames of both formats

uint32_t Rd32(const uint8_t* p) {
  return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

// XXH32 (the LZ4 frame descriptor's header checksum is its second byte; header bytes only)
uint32_t Xxh32(const uint8_t* p, size_t n, uint32_t seed) {
  constexpr uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u,
                     P5 = 374761393u;
  auto rotl = [](uint32_t x, int r) { return (x << r) | (x >> (32 - r)); };
  size_t i = 0;
  uint32_t h;
  if (n >= 16) {
    uint32_t v[4] = {seed + P1 + P2, seed + P2, seed, seed - P1};
    for (; i + 16 <= n; i += 16)
      for (int k = 0; k < 4; ++k) v[k] = rotl(v[k] + Rd32(p + i + 4 * k) * P2, 13) * P1;
    h = rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18);
  } else {
    h = seed + P5;
  }
  h += static_cast<uint32_t>(n);
  for (; i + 4 <= n; i += 4) h = rotl(h + Rd32(p + i) * P3, 17) * P4;
  for (; i < n; ++i) h = rotl(h + p[i] * P5, 11) * P1;
  h ^= h >> 15;
  h *= P2;
  h ^= h >> 13;
  h *= P3;
  h ^= h >> 16;
  return h;
}

// one segment of a compressed stream: csize bytes at offset; raw = stored (LZ4 frame);
// content = its decompressed size when the header states it (Zstd), else 0
struct Piece {
  uint64_t offset;
  uint32_t csize;
  uint32_t content;
  bool raw;
};

// one frame of a stock stream (the unit the stock writers emit per buffer)
struct Frame {
  uint64_t offset = 0, csize = 0;  // the whole frame
  uint64_t content = 0;            // declared content size (has_content)
  bool has_content = false;
  bool linked = false;             // LZ4: blocks depend on the previous ones
  bool content_checksum = false;   // LZ4: XXH32 of the content follows the EndMark
  uint32_t checksum = 0;
  std::vector<Piece> blocks;       // LZ4 data blocks
};

class HipCodec : public arrow::util::Codec {
 public:
  HipCodec(arrow::Compression::type type, int device) : type_(type), device_(device) {}
  ~HipCodec() override {
    if (!ctx_) return;
    for (void* p : {d_in_, d_slab_, d_sizes_, d_off_, d_frame_, d_out_, d_srcs_, d_aux_, d_join_,
                    d_meta_})
      if (p) bitar_hip_free(ctx_, p);
    bitar_hip_close(ctx_);
  }

  int minimum_compression_level() const override { return 1; }
  int maximum_compression_level() const override { return 1; }
  int default_compression_level() const override { return 1; }
  int compression_level() const override { return 1; }
  arrow::Compression::type compression_type() const override { return type_; }

  int64_t MaxCompressedLen(int64_t input_len, const uint8_t*) override {
    const uint64_t nseg = (static_cast<uint64_t>(input_len) + kSeg - 1) / kSeg;
    if (type_ == arrow::Compression::SNAPPY)  // stock Snappy's bound (ours: n + 4 nseg + 5)
      return 32 + input_len + input_len / 6;
    if (type_ == arrow::Compression::ZSTD)
      return static_cast<int64_t>(9 + nseg * bitar_hip_slot_size(BITAR_HIP_CODEC_ZSTD, kSeg));
    if (type_ == arrow::Compression::GZIP)  // header + index, the joined stream, trailer
      return static_cast<int64_t>(std::max<uint64_t>(
          gzf::HeaderLen(nseg) + nseg * (gzf::SlotSize(kSeg) + 1) + gzf::kTrailerLen,
          gzf::EmptyMemberLen()));
    return static_cast<int64_t>(7 + nseg * (4 + kSeg) + 4);
  }

  arrow::Result<std::shared_ptr<arrow::util::Compressor>> MakeCompressor() override {
    return arrow::Status::NotImplemented("streaming compression on the HIP codec");
  }
  arrow::Result<std::shared_ptr<arrow::util::Decompressor>> MakeDecompressor() override {
    return arrow::Status::NotImplemented("streaming decompression on the HIP codec");
  }

  arrow::Result<int64_t> Compress(int64_t input_len, const uint8_t* input,
                                  int64_t output_buffer_len, uint8_t* output) override;
  arrow::Result<int64_t> Decompress(int64_t input_len, const uint8_t* input,
                                    int64_t output_buffer_len, uint8_t* output) override;

 private:
  // The device context is opened by the first Compress or Decompress (under mu_), so a codec
  // can be made, asked for its bounds and handed to a writer on a host that has no device.
  arrow::Status Open() {
    if (ctx_) return arrow::Status::OK();
    bitar_hip_config cfg{1, 0};
    BITAR_ABI(bitar_hip_open(device_, &cfg, &ctx_), "bitar_hip_open");
    return arrow::Status::OK();
  }
  // grow-only HBM scratch
  arrow::Status Reserve(void*& p, uint64_t& cap, uint64_t bytes) {
    if (bytes <= cap) return arrow::Status::OK();
    if (p) bitar_hip_free(ctx_, p);
    p = nullptr;
    cap = 0;
    BITAR_ABI(bitar_hip_alloc(ctx_, bytes, &p), "bitar_hip_alloc");
    cap = bytes;
    return arrow::Status::OK();
  }
  bool OnDevice(const void* p) const {
    int kind = 0, dev = -1;
    return bitar_hip_pointer_info(p, &kind, &dev) == 0 && kind == 2 && dev == device_;
  }
  arrow::Status Copy(void* dst, const void* src, uint64_t n) {
    if (n) BITAR_ABI(bitar_hip_memcpy(ctx_, dst, src, n, nullptr), "bitar_hip_memcpy");
    return arrow::Status::OK();
  }
  arrow::Status Sync() {
    BITAR_ABI(bitar_hip_sync(ctx_, nullptr), "segment codec");
    return arrow::Status::OK();
  }
  arrow::Result<std::vector<Frame>> WalkZstd(const uint8_t* p, uint64_t n) const;
  arrow::Result<std::vector<Frame>> WalkLz4f(const uint8_t* p, uint64_t n) const;
  arrow::Result<int64_t> DecompressZstd(const std::vector<Frame>& frames, const uint8_t* d_in,
                                        int64_t output_buffer_len, uint8_t* output);
  arrow::Result<int64_t> DecompressLz4f(const std::vector<Frame>& frames, const uint8_t* d_in,
                                        uint64_t n, int64_t output_buffer_len, uint8_t* output);
  arrow::Result<int64_t> CompressGzip(uint64_t n, const uint8_t* input, int64_t output_buffer_len,
                                      uint8_t* output);
  arrow::Result<int64_t> DecompressGzip(uint64_t n, const uint8_t* input,
                                        int64_t output_buffer_len, uint8_t* output);
  arrow::Result<int64_t> CompressSnappy(uint64_t n, const uint8_t* input,
                                        int64_t output_buffer_len, uint8_t* output);
  arrow::Result<int64_t> DecompressSnappy(uint64_t n, const uint8_t* input,
                                          int64_t output_buffer_len, uint8_t* output);
  arrow::Status GzipIndexed(const gzf::Member& m, const uint8_t* input, uint8_t* output);
  arrow::Status GzipSingles(const std::vector<gzf::Member>& ms, size_t m0, size_t m1,
                            const uint8_t* d_in, uint8_t* output);
  // the frame's independent 64 KiB blocks, in parallel, to dout; returns the content size
  arrow::Result<uint64_t> Lz4Independent(const Frame& f, const uint8_t* d_in, uint8_t* dout);

  arrow::Compression::type type_;
  int device_;
  bitar_hip_ctx* ctx_ = nullptr;
  std::mutex mu_;  // one stream per codec; Arrow may share a codec between threads
  void *d_in_ = nullptr, *d_slab_ = nullptr, *d_sizes_ = nullptr, *d_off_ = nullptr,
       *d_frame_ = nullptr, *d_out_ = nullptr, *d_srcs_ = nullptr, *d_aux_ = nullptr,
       *d_join_ = nullptr, *d_meta_ = nullptr;
  uint64_t c_in_ = 0, c_slab_ = 0, c_sizes_ = 0, c_off_ = 0, c_frame_ = 0, c_out_ = 0,
           c_srcs_ = 0, c_aux_ = 0, c_join_ = 0, c_meta_ = 0;
};

arrow::Result<int64_t> HipCodec::Compress(int64_t input_len, const uint8_t* input,
                                          int64_t output_buffer_len, uint8_t* output) {
  const std::lock_guard<std::mutex> lock(mu_);
  if (input_len < 0) return arrow::Status::Invalid("negative input length");
  // (SNAPPY takes any buffer its stream fits: CapacityError once the length is known)
  if (type_ != arrow::Compression::SNAPPY && output_buffer_len < MaxCompressedLen(input_len, input))
    return arrow::Status::Invalid("output buffer smaller than MaxCompressedLen");
  if (output_buffer_len < 0) return arrow::Status::Invalid("negative output buffer length");
  ARROW_RETURN_NOT_OK(Open());
  const uint64_t n = static_cast<uint64_t>(input_len);
  if (type_ == arrow::Compression::GZIP) return CompressGzip(n, input, output_buffer_len, output);
  if (type_ == arrow::Compression::SNAPPY)
    return CompressSnappy(n, input, output_buffer_len, output);
  const uint64_t nseg = (n + kSeg - 1) / kSeg;
  const bool zstd = type_ == arrow::Compression::ZSTD;
  const bool out_dev = OnDevice(output);
  // LZ4 frame header: magic, FLG (version 01, independent blocks), BD (64 KiB blocks), HC
  uint8_t hdr[7] = {0x04, 0x22, 0x4D, 0x18, 0x60, 0x40, 0};
  hdr[6] = static_cast<uint8_t>((Xxh32(hdr + 4, 2, 0) >> 8) & 0xFF);
  const uint64_t head = zstd ? 0 : sizeof hdr;
  if (n == 0) {
    // an empty stream: one empty frame (Zstd: single segment, content size 0, one empty
    // last raw block), or the LZ4 frame header + EndMark
    static const uint8_t kEmptyZstd[9] = {0x28, 0xB5, 0x2F, 0xFD, 0x20, 0x00, 0x01, 0x00, 0x00};
    uint8_t lz4[11];
    std::memcpy(lz4, hdr, 7);
    std::memset(lz4 + 7, 0, 4);
    const uint8_t* src = zstd ? kEmptyZstd : lz4;
    const uint64_t len = zstd ? sizeof kEmptyZstd : sizeof lz4;
    if (out_dev) ARROW_RETURN_NOT_OK(Copy(output, src, len));
    else std::memcpy(output, src, len);
    return static_cast<int64_t>(len);
  }
  const uint32_t codec = zstd ? BITAR_HIP_CODEC_ZSTD : BITAR_HIP_CODEC_LZ4;
  const uint64_t stride = bitar_hip_slot_size(codec, kSeg);
  const void* d_in = input;
  if (!OnDevice(input)) {
    ARROW_RETURN_NOT_OK(Reserve(d_in_, c_in_, n));
    ARROW_RETURN_NOT_OK(Copy(d_in_, input, n));
    d_in = d_in_;
  }
  ARROW_RETURN_NOT_OK(Reserve(d_slab_, c_slab_, nseg * stride));
  ARROW_RETURN_NOT_OK(Reserve(d_sizes_, c_sizes_, nseg * 4));
  ARROW_RETURN_NOT_OK(Reserve(d_aux_, c_aux_, nseg * 4));
  ARROW_RETURN_NOT_OK(Reserve(d_off_, c_off_, (nseg + 1) * 8));
  ARROW_RETURN_NOT_OK(Reserve(d_frame_, c_frame_, head + nseg * (stride > kSeg + 4 ? stride : kSeg + 4) + 4));
  auto* sizes = static_cast<uint32_t*>(d_sizes_);
  auto* offs = static_cast<uint64_t*>(d_off_);
  auto* frame = static_cast<uint8_t*>(d_frame_);
  BITAR_ABI(bitar_hip_compress(ctx_, nullptr, codec, d_in, n, kSeg, d_slab_, stride, sizes),
            "bitar_hip_compress");
  if (zstd) {
    BITAR_ABI(bitar_hip_pack(ctx_, nullptr, d_slab_, stride, sizes, static_cast<uint32_t>(nseg),
                             offs, frame),
              "bitar_hip_pack");
  } else {
    BITAR_ABI(bitar_hip_pack_lz4f(ctx_, nullptr, d_in, n, kSeg, d_slab_, stride, sizes,
                                  static_cast<uint32_t*>(d_aux_), offs, frame + head),
              "bitar_hip_pack_lz4f");
  }
  ARROW_RETURN_NOT_OK(Sync());
  uint64_t body = 0;
  ARROW_RETURN_NOT_OK(Copy(&body, offs + nseg, sizeof body));
  ARROW_RETURN_NOT_OK(Sync());
  const uint64_t total = head + body + (zstd ? 0 : 4);
  if (total > static_cast<uint64_t>(output_buffer_len))
    return arrow::Status::CapacityError("compressed stream exceeds the output buffer");
  if (out_dev) {
    if (!zstd) ARROW_RETURN_NOT_OK(Copy(output, hdr, head));
    ARROW_RETURN_NOT_OK(Copy(output + head, frame + head, body));
    if (!zstd) {
      static const uint8_t kEnd[4] = {0, 0, 0, 0};
      ARROW_RETURN_NOT_OK(Copy(output + head + body, kEnd, 4));
    }
  } else {
    if (!zstd) std::memcpy(output, hdr, head);
    ARROW_RETURN_NOT_OK(Copy(output + head, frame + head, body));
    if (!zstd) std::memset(output + head + body, 0, 4);
  }
  ARROW_RETURN_NOT_OK(Sync());
  return static_cast<int64_t>(total);
}

// Zstandard frames (any content size; a frame without one only as the stream's single
// frame, sized by the caller's output buffer)
arrow::Result<std::vector<Frame>> HipCodec::WalkZstd(const uint8_t* p, uint64_t n) const {
  std::vector<Frame> v;
  uint64_t pos = 0;
  while (pos < n) {
    Frame f;
    f.offset = pos;
    if (n - pos < 4) return arrow::Status::Invalid("truncated Zstandard frame header");
    if ((Rd32(p + pos) & 0xFFFFFFF0u) == kSkippableMagic)
      return arrow::Status::NotImplemented("skippable frame at offset ", pos);
    if (Rd32(p + pos) != kZstdMagic)
      return arrow::Status::Invalid("not a Zstandard frame at offset ", pos);
    if (n - pos < 6) return arrow::Status::Invalid("truncated Zstandard frame header");
    pos += 4;
    const uint32_t fhd = p[pos++];
    const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u, did_flag = fhd & 3u;
    if (fhd & 8u) return arrow::Status::Invalid("Zstandard frame with reserved bit set");
    if (did_flag) return arrow::Status::NotImplemented("Zstandard dictionaries");
    if (!single) pos += 1;
    const uint32_t fsz = fcs_flag == 0 ? (single ? 1u : 0u) : fcs_flag == 1 ? 2u
                         : fcs_flag == 2 ? 4u : 8u;
    if (pos + fsz > n) return arrow::Status::Invalid("truncated Zstandard frame header");
    for (uint32_t k = 0; k < fsz; ++k) f.content |= uint64_t(p[pos + k]) << (8 * k);
    if (fsz == 2) f.content += 256;
    f.has_content = fsz != 0;
    pos += fsz;
    for (bool last = false; !last;) {
      if (pos + 3 > n) return arrow::Status::Invalid("truncated Zstandard block header");
      const uint32_t bh = uint32_t(p[pos]) | uint32_t(p[pos + 1]) << 8 | uint32_t(p[pos + 2]) << 16;
      last = bh & 1u;
      const uint32_t type = (bh >> 1) & 3u, bsz = bh >> 3;
      if (type == 3) return arrow::Status::Invalid("reserved Zstandard block type");
      pos += 3 + (type == 1 ? 1u : bsz);
    }
    if ((fhd >> 2) & 1u) pos += 4;  // content checksum (verified on the device)
    if (pos > n) return arrow::Status::Invalid("truncated Zstandard frame");
    f.csize = pos - f.offset;
    v.push_back(f);
  }
  return v;
}

// LZ4 frames: version 01, blocks of <= 64 KiB (independent or linked), optional block
// checksums, content size and content checksum (both checksums verified here: XXH32)
arrow::Result<std::vector<Frame>> HipCodec::WalkLz4f(const uint8_t* p, uint64_t n) const {
  std::vector<Frame> v;
  uint64_t pos = 0;
  while (pos < n) {
    Frame f;
    f.offset = pos;
    if (n - pos < 4) return arrow::Status::Invalid("truncated LZ4 frame header");
    if ((Rd32(p + pos) & 0xFFFFFFF0u) == kSkippableMagic)
      return arrow::Status::NotImplemented("skippable frame at offset ", pos);
    if (Rd32(p + pos) != kLz4fMagic)
      return arrow::Status::Invalid("not an LZ4 frame at offset ", pos);
    if (n - pos < 7) return arrow::Status::Invalid("truncated LZ4 frame header");
    // Everything the format forbids is Invalid before anything this codec leaves out is
    // NotImplemented: a frame that no reader takes is never called a missing feature.
    const uint32_t flg = p[pos + 4], bd = p[pos + 5];
    if ((flg >> 6) != 1) return arrow::Status::Invalid("LZ4 frame version");
    if (flg & 2u) return arrow::Status::Invalid("LZ4 frame with a reserved FLG bit set");
    if (bd & 0x8Fu) return arrow::Status::Invalid("LZ4 frame with a reserved BD bit set");
    if (((bd >> 4) & 7) < 4) return arrow::Status::Invalid("LZ4 block size id below 4");
    f.linked = !((flg >> 5) & 1);
    const bool block_cks = (flg >> 4) & 1;
    f.content_checksum = (flg >> 2) & 1;
    const bool has_size = (flg >> 3) & 1, has_dict = flg & 1;
    const uint64_t dlen = 2 + (has_size ? 8 : 0) + (has_dict ? 4 : 0);
    if (pos + 4 + dlen + 1 > n) return arrow::Status::Invalid("truncated LZ4 frame header");
    if (((Xxh32(p + pos + 4, dlen, 0) >> 8) & 0xFF) != p[pos + 4 + dlen])
      return arrow::Status::Invalid("LZ4 frame header checksum");
    if (has_dict) return arrow::Status::NotImplemented("LZ4 dictionary id");
    if (((bd >> 4) & 7) != 4) return arrow::Status::NotImplemented("LZ4 blocks larger than 64 KiB");
    if (has_size) {
      f.has_content = true;
      for (int k = 0; k < 8; ++k) f.content |= uint64_t(p[pos + 6 + k]) << (8 * k);
    }
    pos += 4 + dlen + 1;
    for (;;) {
      if (pos + 4 > n) return arrow::Status::Invalid("truncated LZ4 frame");
      const uint32_t bs = Rd32(p + pos);
      pos += 4;
      if (bs == 0) break;  // EndMark
      const uint32_t len = bs & 0x7FFFFFFFu;
      if (len > kSeg || pos + len > n) return arrow::Status::Invalid("bad LZ4 block size");
      if (block_cks) {
        if (pos + len + 4 > n) return arrow::Status::Invalid("truncated LZ4 block checksum");
        if (Xxh32(p + pos, len, 0) != Rd32(p + pos + len))
          return arrow::Status::IOError("LZ4 block checksum mismatch");
      }
      // (a stored block of no bytes, 0x80000000, is valid and is nothing to decode: dropped
      // here, so that neither block mode sees it)
      if (len) f.blocks.push_back({pos, len, 0, (bs >> 31) != 0});
      pos += len + (block_cks ? 4 : 0);
    }
    if (f.content_checksum) {
      if (pos + 4 > n) return arrow::Status::Invalid("truncated LZ4 content checksum");
      f.checksum = Rd32(p + pos);
      pos += 4;
    }
    f.csize = pos - f.offset;
    v.push_back(std::move(f));
  }
  return v;
}

arrow::Result<int64_t> HipCodec::Decompress(int64_t input_len, const uint8_t* input,
                                            int64_t output_buffer_len, uint8_t* output) {
  const std::lock_guard<std::mutex> lock(mu_);
  if (input_len < 0 || output_buffer_len < 0) return arrow::Status::Invalid("negative length");
  ARROW_RETURN_NOT_OK(Open());
  const uint64_t n = static_cast<uint64_t>(input_len);
  if (type_ == arrow::Compression::GZIP)
    return DecompressGzip(n, input, output_buffer_len, output);
  if (type_ == arrow::Compression::SNAPPY)
    return DecompressSnappy(n, input, output_buffer_len, output);
  const bool zstd = type_ == arrow::Compression::ZSTD;
  const bool in_dev = OnDevice(input);
  // the header walk needs the bytes on the host
  std::vector<uint8_t> host;
  const uint8_t* hp = input;
  if (in_dev) {
    host.resize(n);
    ARROW_RETURN_NOT_OK(Copy(host.data(), input, n));
    ARROW_RETURN_NOT_OK(Sync());
    hp = host.data();
  }
  std::vector<Frame> frames;
  if (zstd) {
    ARROW_ASSIGN_OR_RAISE(frames, WalkZstd(hp, n));
  } else {
    ARROW_ASSIGN_OR_RAISE(frames, WalkLz4f(hp, n));
  }
  if (frames.empty()) return 0;
  const uint8_t* d_in = input;
  if (!in_dev) {
    ARROW_RETURN_NOT_OK(Reserve(d_in_, c_in_, n + 16));
    ARROW_RETURN_NOT_OK(Copy(d_in_, input, n));
    d_in = static_cast<const uint8_t*>(d_in_);
  }
  if (zstd) return DecompressZstd(frames, d_in, output_buffer_len, output);
  return DecompressLz4f(frames, d_in, n, output_buffer_len, output);
}

// Zstandard: every frame is one segment of the wave decoder; segments are as large as the
// largest frame (frames of 64 KiB, the shape this codec writes, are the common case)
arrow::Result<int64_t> HipCodec::DecompressZstd(const std::vector<Frame>& frames,
                                                const uint8_t* d_in, int64_t output_buffer_len,
                                                uint8_t* output) {
  const uint64_t nfr = frames.size();
  const uint64_t cap = static_cast<uint64_t>(output_buffer_len);
  // Declared content sizes come from untrusted headers: their sum must fit the caller's
  // buffer BEFORE anything is reserved (a frame without one: only as the single frame, sized
  // by the output buffer).
  uint64_t declared = 0;
  for (const Frame& f : frames) {
    if (!f.has_content && nfr > 1)
      return arrow::Status::NotImplemented("Zstandard frames without content size");
    const uint64_t c = f.has_content ? f.content : cap;
    if (c > (1ull << 30)) return arrow::Status::NotImplemented("Zstandard frame larger than 1 GiB");
    declared += c;
    if (declared > cap)
      return arrow::Status::Invalid("declared Zstandard content exceeds the output buffer (",
                                    output_buffer_len, ")");
  }
  // Frames are decoded in groups of consecutive frames, one launch each; a group's staging
  // is (frames) x (its largest frame), kept within the declared total + 64 KiB, so mixed
  // frame sizes never reserve more than about the output itself (equal-size frames, what
  // this codec writes: one group).
  const uint64_t budget = declared + kSeg;
  auto rnd = [](uint64_t c) { return std::max<uint64_t>((c + 15) & ~15ull, 16); };
  uint64_t total = 0;
  for (uint64_t g0 = 0; g0 < nfr;) {
    uint64_t g1 = g0, seg = 0;
    while (g1 < nfr) {
      const uint64_t c = rnd(frames[g1].has_content ? frames[g1].content : cap);
      const uint64_t s2 = std::max(seg, c);
      if (g1 > g0 && ((g1 - g0 + 1) * s2 > budget || g1 - g0 + 1 > 0x7FFFFFFFull)) break;
      seg = s2;
      ++g1;
    }
    const uint64_t nseg = g1 - g0;
    std::vector<const uint8_t*> srcs(nseg);
    std::vector<uint32_t> csz(nseg);
    for (uint64_t i = 0; i < nseg; ++i) {
      const Frame& f = frames[g0 + i];
      if (f.csize > 0xFFFFFFFFull) return arrow::Status::Invalid("Zstandard frame over 4 GiB");
      srcs[i] = d_in + f.offset;
      csz[i] = static_cast<uint32_t>(f.csize);
    }
    ARROW_RETURN_NOT_OK(Reserve(d_srcs_, c_srcs_, nseg * sizeof(void*)));
    ARROW_RETURN_NOT_OK(Reserve(d_sizes_, c_sizes_, nseg * 4));
    ARROW_RETURN_NOT_OK(Reserve(d_off_, c_off_, nseg * 4));  // produced sizes
    ARROW_RETURN_NOT_OK(Reserve(d_out_, c_out_, nseg * seg));
    ARROW_RETURN_NOT_OK(Copy(d_srcs_, srcs.data(), nseg * sizeof(void*)));
    ARROW_RETURN_NOT_OK(Copy(d_sizes_, csz.data(), nseg * 4));
    auto* dout = static_cast<uint8_t*>(d_out_);
    BITAR_ABI(bitar_hip_decompress(ctx_, nullptr, BITAR_HIP_CODEC_ZSTD,
                                   reinterpret_cast<const void* const*>(d_srcs_),
                                   static_cast<const uint32_t*>(d_sizes_),
                                   static_cast<uint32_t>(nseg), static_cast<uint32_t>(seg), dout,
                                   nseg * seg, static_cast<uint32_t*>(d_off_)),
              "bitar_hip_decompress");
    std::vector<uint32_t> prod(nseg);
    ARROW_RETURN_NOT_OK(Copy(prod.data(), d_off_, nseg * 4));
    ARROW_RETURN_NOT_OK(Sync());
    for (uint64_t i = 0; i < nseg; ++i) {
      const Frame& f = frames[g0 + i];
      if (f.has_content && prod[i] != f.content)
        return arrow::Status::IOError("Zstandard frame ", g0 + i, " decoded to a wrong size");
      if (total + prod[i] > cap)
        return arrow::Status::Invalid("decompressed size exceeds the output buffer (",
                                      output_buffer_len, ")");
      // frame i's output sits at i * seg: gather them back to back
      ARROW_RETURN_NOT_OK(Copy(output + total, dout + i * seg, prod[i]));
      total += prod[i];
    }
    ARROW_RETURN_NOT_OK(Sync());
    g0 = g1;
  }
  return static_cast<int64_t>(total);
}

arrow::Result<uint64_t> HipCodec::Lz4Independent(const Frame& f, const uint8_t* d_in,
                                                 uint8_t* dout) {
  const uint64_t nseg = f.blocks.size();
  if (nseg == 0) return 0;
  // a stored block decodes as an empty one (a lone 0x00 token) and is copied after
  ARROW_RETURN_NOT_OK(Reserve(d_aux_, c_aux_, 16));
  static const uint8_t kEmptyBlock[16] = {0};
  ARROW_RETURN_NOT_OK(Copy(d_aux_, kEmptyBlock, 16));
  const uint8_t* empty = static_cast<const uint8_t*>(d_aux_);
  std::vector<const uint8_t*> srcs(nseg);
  std::vector<uint32_t> csz(nseg);
  for (uint64_t i = 0; i < nseg; ++i) {
    const bool raw = f.blocks[i].raw;
    srcs[i] = raw ? empty : d_in + f.blocks[i].offset;
    csz[i] = raw ? 1u : f.blocks[i].csize;
  }
  ARROW_RETURN_NOT_OK(Reserve(d_srcs_, c_srcs_, nseg * sizeof(void*)));
  ARROW_RETURN_NOT_OK(Reserve(d_sizes_, c_sizes_, nseg * 4));
  ARROW_RETURN_NOT_OK(Reserve(d_off_, c_off_, nseg * 4));  // produced sizes
  ARROW_RETURN_NOT_OK(Copy(d_srcs_, srcs.data(), nseg * sizeof(void*)));
  ARROW_RETURN_NOT_OK(Copy(d_sizes_, csz.data(), nseg * 4));
  BITAR_ABI(bitar_hip_decompress(ctx_, nullptr, BITAR_HIP_CODEC_LZ4,
                                 reinterpret_cast<const void* const*>(d_srcs_),
                                 static_cast<const uint32_t*>(d_sizes_),
                                 static_cast<uint32_t>(nseg), kSeg, dout, nseg * kSeg,
                                 static_cast<uint32_t*>(d_off_)),
            "bitar_hip_decompress");
  for (uint64_t i = 0; i < nseg; ++i)
    if (f.blocks[i].raw)
      ARROW_RETURN_NOT_OK(Copy(dout + i * kSeg, d_in + f.blocks[i].offset, f.blocks[i].csize));
  ARROW_RETURN_NOT_OK(Sync());
  std::vector<uint32_t> prod(nseg);
  ARROW_RETURN_NOT_OK(Copy(prod.data(), d_off_, nseg * 4));
  ARROW_RETURN_NOT_OK(Sync());
  uint64_t total = 0;
  for (uint64_t i = 0; i < nseg; ++i) {
    const uint32_t got = f.blocks[i].raw ? f.blocks[i].csize : prod[i];
    if (i + 1 < nseg && got != kSeg)
      return arrow::Status::NotImplemented("LZ4 frame blocks of other than 64 KiB");
    total += got;
  }
  return total;
}

// LZ4 frames in order: independent blocks decode in parallel (one segment each), linked
// ones in order on one wavefront (bitar_hip_lz4_chain); content checksums checked (XXH32)
arrow::Result<int64_t> HipCodec::DecompressLz4f(const std::vector<Frame>& frames,
                                                const uint8_t* d_in, uint64_t n,
                                                int64_t output_buffer_len, uint8_t* output) {
  const uint64_t cap = static_cast<uint64_t>(output_buffer_len);
  uint64_t most = 0;  // staging: the output, plus a full last block of slack
  for (const Frame& f : frames) most += f.blocks.size() * kSeg;
  ARROW_RETURN_NOT_OK(Reserve(d_out_, c_out_, std::max<uint64_t>(std::min(most, cap + kSeg), 16)));
  auto* dout = static_cast<uint8_t*>(d_out_);
  uint64_t total = 0;
  for (const Frame& f : frames) {
    uint64_t got = 0;
    if (f.blocks.empty()) {
      got = 0;
    } else if (!f.linked) {
      if (total + f.blocks.size() * kSeg > c_out_)
        return arrow::Status::Invalid("LZ4 stream exceeds the output buffer");
      ARROW_ASSIGN_OR_RAISE(got, Lz4Independent(f, d_in, dout + total));
    } else {
      // the kernel takes 32-bit offsets: relative to the frame, whose size must fit
      if (f.csize > 0xFFFFFFFFull)
        return arrow::Status::NotImplemented("linked-block LZ4 frame over 4 GiB");
      std::vector<uint32_t> tab(2 * f.blocks.size());
      for (size_t b = 0; b < f.blocks.size(); ++b) {
        tab[2 * b] = static_cast<uint32_t>(f.blocks[b].offset - f.offset);
        tab[2 * b + 1] = f.blocks[b].csize | (f.blocks[b].raw ? 0x80000000u : 0u);
      }
      ARROW_RETURN_NOT_OK(Reserve(d_srcs_, c_srcs_, tab.size() * 4));
      ARROW_RETURN_NOT_OK(Reserve(d_off_, c_off_, 4));
      ARROW_RETURN_NOT_OK(Copy(d_srcs_, tab.data(), tab.size() * 4));
      // The kernel has no per-block output limit (liblz4: 64 KiB); the frame as a whole gets
      // 64 KiB per block, and never more than the caller's buffer plus the slack reserved
      // above: a bound the stream and the caller set, not what earlier calls left in d_out_.
      const uint64_t room = std::min<uint64_t>(
          {f.blocks.size() * uint64_t{kSeg}, cap + kSeg - total, c_out_ - total});
      BITAR_ABI(bitar_hip_lz4_chain(ctx_, nullptr, d_in + f.offset, static_cast<uint32_t>(f.csize),
                                    static_cast<const uint32_t*>(d_srcs_),
                                    static_cast<uint32_t>(f.blocks.size()), dout + total, room,
                                    static_cast<uint32_t*>(d_off_)),
                "bitar_hip_lz4_chain");
      ARROW_RETURN_NOT_OK(Sync());
      uint32_t prod = 0;
      ARROW_RETURN_NOT_OK(Copy(&prod, d_off_, 4));
      ARROW_RETURN_NOT_OK(Sync());
      got = prod;
    }
    if (f.has_content && got != f.content)
      return arrow::Status::IOError("LZ4 frame decoded to a wrong size");
    if (total + got > cap)
      return arrow::Status::Invalid("decompressed size exceeds the output buffer (",
                                    output_buffer_len, ")");
    if (f.content_checksum) {
      std::vector<uint8_t> back(got);
      ARROW_RETURN_NOT_OK(Copy(back.data(), dout + total, got));
      ARROW_RETURN_NOT_OK(Sync());
      if (Xxh32(back.data(), got, 0) != f.checksum)
        return arrow::Status::IOError("LZ4 content checksum mismatch");
    }
    total += got;
  }
  ARROW_RETURN_NOT_OK(Copy(output, dout, total));
  ARROW_RETURN_NOT_OK(Sync());
  return static_cast<int64_t>(total);
}

// ---- GZIP (RFC 1952; layout and index in gzip_frame.h) ----

arrow::Status FromGzf(const gzf::Status& st) {
  if (st.ok()) return arrow::Status::OK();
  return st.code == gzf::Code::kNotImplemented ? arrow::Status::NotImplemented(st.msg)
                                               : arrow::Status::Invalid(st.msg);
}

// One member: the segments' dynamic-Huffman streams (the reference default) joined into one
// raw DEFLATE stream on the device, the 'BT' index of their bit lengths in FEXTRA, CRC-32 of
// the input from its segments' CRC-32s.  Only the bit lengths, the stream's length and the
// CRC visit the host.
arrow::Result<int64_t> HipCodec::CompressGzip(uint64_t n, const uint8_t* input,
                                              int64_t output_buffer_len, uint8_t* output) {
  const bool out_dev = OnDevice(output);
  const uint64_t nseg = (n + kSeg - 1) / kSeg;
  if (n == 0) {
    uint8_t empty[64];
    static_assert(sizeof empty >= 24 + 2 + 8, "empty member");
    gzf::WriteEmptyMember(empty);
    const uint64_t len = gzf::EmptyMemberLen();
    if (out_dev) {
      ARROW_RETURN_NOT_OK(Copy(output, empty, len));
      ARROW_RETURN_NOT_OK(Sync());
    } else {
      std::memcpy(output, empty, len);
    }
    return static_cast<int64_t>(len);
  }
  // never write a stream this codec could not read back in parallel
  if (nseg > gzf::kMaxIndexSegs)
    return arrow::Status::NotImplemented(
        "GZIP buffers above ", uint64_t(gzf::kMaxIndexSegs) * kSeg,
        " bytes: the segment index must fit the 16-bit XLEN of one gzip member");
  const uint32_t codec = BITAR_HIP_CODEC_DEFLATE_DYNAMIC;
  const uint64_t stride = bitar_hip_slot_size(codec, kSeg);
  const uint64_t cap = (nseg * (stride + 1) + 3) & ~3ull;
  const void* d_in = input;
  if (!OnDevice(input)) {
    ARROW_RETURN_NOT_OK(Reserve(d_in_, c_in_, n));
    ARROW_RETURN_NOT_OK(Copy(d_in_, input, n));
    d_in = d_in_;
  }
  ARROW_RETURN_NOT_OK(Reserve(d_slab_, c_slab_, nseg * stride));
  ARROW_RETURN_NOT_OK(Reserve(d_sizes_, c_sizes_, nseg * 4));
  ARROW_RETURN_NOT_OK(Reserve(d_aux_, c_aux_, nseg * 4));
  ARROW_RETURN_NOT_OK(Reserve(d_off_, c_off_, (nseg + 1) * 8));
  ARROW_RETURN_NOT_OK(Reserve(d_join_, c_join_, cap));
  ARROW_RETURN_NOT_OK(Reserve(d_meta_, c_meta_, nseg * 8 + 8 + nseg));
  // tables of a batched copy that gathers byte 0 of every slot (BTYPE: stored or coded)
  ARROW_RETURN_NOT_OK(Reserve(d_srcs_, c_srcs_, nseg * (2 * sizeof(void*) + 4)));
  auto* sizes = static_cast<uint32_t*>(d_sizes_);
  auto* bits = static_cast<uint32_t*>(d_aux_);
  auto* starts = static_cast<uint64_t*>(d_off_);
  auto* sums = static_cast<uint64_t*>(d_meta_);
  auto* d_crc = reinterpret_cast<uint32_t*>(sums + nseg);
  const uint32_t ns = static_cast<uint32_t>(nseg);
  BITAR_ABI(bitar_hip_compress_bits(ctx_, nullptr, codec, d_in, n, kSeg, d_slab_, stride, sizes,
                                    bits),
            "bitar_hip_compress_bits");
  BITAR_ABI(bitar_hip_deflate_join(ctx_, nullptr, d_slab_, stride, sizes, bits, ns, starts,
                                   d_join_, cap),
            "bitar_hip_deflate_join");
  BITAR_ABI(bitar_hip_checksum(ctx_, nullptr, BITAR_HIP_CHECKSUM_CRC32, d_in, n, kSeg, nullptr, ns,
                               sums),
            "bitar_hip_checksum");
  BITAR_ABI(bitar_hip_crc32_combine(ctx_, nullptr, sums, n, kSeg, ns, d_crc),
            "bitar_hip_crc32_combine");
  auto* d_first = reinterpret_cast<uint8_t*>(d_crc + 2);
  {
    std::vector<const void*> tab(2 * nseg);
    std::vector<uint32_t> ones(nseg, 1u);
    for (uint64_t i = 0; i < nseg; ++i) {
      tab[i] = static_cast<const uint8_t*>(d_slab_) + i * stride;
      tab[nseg + i] = d_first + i;
    }
    auto* d_tab = static_cast<void**>(d_srcs_);
    ARROW_RETURN_NOT_OK(Copy(d_tab, tab.data(), 2 * nseg * sizeof(void*)));
    ARROW_RETURN_NOT_OK(Copy(d_tab + 2 * nseg, ones.data(), nseg * 4));
    BITAR_ABI(bitar_hip_copy_batch(ctx_, nullptr, d_tab, d_tab + nseg,
                                   reinterpret_cast<const uint32_t*>(d_tab + 2 * nseg), ns),
              "bitar_hip_copy_batch");
  }
  std::vector<uint32_t> entries(nseg);
  std::vector<uint8_t> first(nseg);
  uint64_t end_bits = 0;
  uint32_t crc = 0;
  ARROW_RETURN_NOT_OK(Copy(entries.data(), bits, nseg * 4));
  ARROW_RETURN_NOT_OK(Copy(first.data(), d_first, nseg));
  ARROW_RETURN_NOT_OK(Copy(&end_bits, starts + nseg, 8));
  ARROW_RETURN_NOT_OK(Copy(&crc, d_crc, 4));
  ARROW_RETURN_NOT_OK(Sync());
  for (uint64_t i = 0; i < nseg; ++i) {
    if (entries[i] == 0 || entries[i] > gzf::kBitsMask)
      return arrow::Status::IOError("segment ", i, " failed to compress");
    if ((first[i] & 6u) == 0) entries[i] |= gzf::kStoredBit;  // BTYPE 00, as the join reads it
  }
  const uint64_t head = gzf::HeaderLen(nseg), body = (end_bits + 7) / 8;
  const uint64_t total = head + body + gzf::kTrailerLen;
  if (total > static_cast<uint64_t>(output_buffer_len))
    return arrow::Status::CapacityError("compressed stream exceeds the output buffer");
  std::vector<uint8_t> hdr(head);
  gzf::WriteHeader(kSeg, ns, entries.data(), hdr.data());
  uint8_t trailer[8];
  gzf::Wr32(trailer, crc);
  gzf::Wr32(trailer + 4, static_cast<uint32_t>(n));
  if (out_dev) {
    ARROW_RETURN_NOT_OK(Copy(output, hdr.data(), head));
    ARROW_RETURN_NOT_OK(Copy(output + head + body, trailer, 8));
  } else {
    std::memcpy(output, hdr.data(), head);
    std::memcpy(output + head + body, trailer, 8);
  }
  ARROW_RETURN_NOT_OK(Copy(output + head, d_join_, body));
  ARROW_RETURN_NOT_OK(Sync());
  return static_cast<int64_t>(total);
}

// An indexed member: split the joined stream back into slots, inflate them in parallel,
// check sizes and the CRC-32, copy the content out.
arrow::Status HipCodec::GzipIndexed(const gzf::Member& m, const uint8_t* input, uint8_t* output) {
  if (m.nseg == 0) return arrow::Status::OK();
  const uint64_t nseg = m.nseg, stride = bitar_hip_slot_size(BITAR_HIP_CODEC_DEFLATE, m.seg);
  ARROW_RETURN_NOT_OK(Reserve(d_join_, c_join_, m.deflate_len + 16));
  ARROW_RETURN_NOT_OK(Reserve(d_slab_, c_slab_, nseg * stride));
  ARROW_RETURN_NOT_OK(Reserve(d_sizes_, c_sizes_, nseg * 4));
  ARROW_RETURN_NOT_OK(Reserve(d_aux_, c_aux_, nseg * 4));
  ARROW_RETURN_NOT_OK(Reserve(d_off_, c_off_, (nseg + 1) * 8));
  ARROW_RETURN_NOT_OK(Reserve(d_out_, c_out_, nseg * m.seg));
  ARROW_RETURN_NOT_OK(Reserve(d_meta_, c_meta_, nseg * 8 + 8 + nseg * 4));
  auto* sums = static_cast<uint64_t*>(d_meta_);
  auto* d_crc = reinterpret_cast<uint32_t*>(sums + nseg);
  auto* d_prod = d_crc + 2;
  auto* dout = static_cast<uint8_t*>(d_out_);
  // (the stream starts wherever the header ends: the split wants it 4-B aligned)
  ARROW_RETURN_NOT_OK(Copy(d_join_, input + m.deflate_off, m.deflate_len));
  ARROW_RETURN_NOT_OK(Copy(d_off_, m.starts.data(), (nseg + 1) * 8));
  ARROW_RETURN_NOT_OK(Copy(d_aux_, m.entries.data(), nseg * 4));
  BITAR_ABI(bitar_hip_deflate_split(ctx_, nullptr, d_join_, m.deflate_len,
                                    static_cast<const uint64_t*>(d_off_),
                                    static_cast<const uint32_t*>(d_aux_), m.nseg, d_slab_, stride,
                                    static_cast<uint32_t*>(d_sizes_)),
            "bitar_hip_deflate_split");
  BITAR_ABI(bitar_hip_decompress_slab(ctx_, nullptr, BITAR_HIP_CODEC_DEFLATE_DYNAMIC, d_slab_,
                                      stride, static_cast<const uint32_t*>(d_sizes_), m.nseg,
                                      m.seg, dout, nseg * m.seg, d_prod),
            "bitar_hip_decompress_slab");
  BITAR_ABI(bitar_hip_checksum(ctx_, nullptr, BITAR_HIP_CHECKSUM_CRC32, dout, m.isize, m.seg,
                               nullptr, m.nseg, sums),
            "bitar_hip_checksum");
  BITAR_ABI(bitar_hip_crc32_combine(ctx_, nullptr, sums, m.isize, m.seg, m.nseg, d_crc),
            "bitar_hip_crc32_combine");
  std::vector<uint32_t> prod(nseg);
  uint32_t crc = 0;
  ARROW_RETURN_NOT_OK(Copy(prod.data(), d_prod, nseg * 4));
  ARROW_RETURN_NOT_OK(Copy(&crc, d_crc, 4));
  ARROW_RETURN_NOT_OK(Sync());  // (a segment that failed to inflate: IOError here)
  for (uint64_t i = 0; i < nseg; ++i)
    if (prod[i] != std::min<uint64_t>(m.seg, m.isize - i * m.seg))
      return arrow::Status::IOError("gzip segment ", i, " decoded to a wrong size");
  if (crc != m.crc) return arrow::Status::IOError("gzip CRC-32 mismatch");
  ARROW_RETURN_NOT_OK(Copy(output, dout, m.isize));
  return Sync();
}

// Members ms[m0, m1) without an index (ISIZE <= 64 KiB each: small stock members, BGZF
// blocks): one segment each, one launch.
arrow::Status HipCodec::GzipSingles(const std::vector<gzf::Member>& ms, size_t m0, size_t m1,
                                    const uint8_t* d_in, uint8_t* output) {
  const uint64_t nseg = m1 - m0;
  std::vector<const uint8_t*> srcs(nseg);
  std::vector<uint32_t> csz(nseg);
  for (uint64_t i = 0; i < nseg; ++i) {
    const gzf::Member& m = ms[m0 + i];
    if (m.deflate_len > 0xFFFFFFFFull) return arrow::Status::Invalid("gzip member over 4 GiB");
    srcs[i] = d_in + m.deflate_off;
    csz[i] = static_cast<uint32_t>(m.deflate_len);
  }
  ARROW_RETURN_NOT_OK(Reserve(d_srcs_, c_srcs_, nseg * sizeof(void*)));
  ARROW_RETURN_NOT_OK(Reserve(d_sizes_, c_sizes_, nseg * 4));
  ARROW_RETURN_NOT_OK(Reserve(d_out_, c_out_, nseg * kSeg));
  ARROW_RETURN_NOT_OK(Reserve(d_meta_, c_meta_, nseg * 8 + nseg * 4));
  // the members' contents are gathered back to back on the device (one batched copy: a BGZF
  // file has one member per 64 KiB) and leave in one copy; ISIZE <= 64 KiB each (gzf::Walk)
  uint64_t total = 0;
  for (uint64_t i = 0; i < nseg; ++i) total += ms[m0 + i].isize;
  ARROW_RETURN_NOT_OK(Reserve(d_join_, c_join_, total + 16));
  ARROW_RETURN_NOT_OK(Reserve(d_off_, c_off_, nseg * (2 * sizeof(void*) + 4)));
  auto* sums = static_cast<uint64_t*>(d_meta_);
  auto* d_prod = reinterpret_cast<uint32_t*>(sums + nseg);
  auto* dout = static_cast<uint8_t*>(d_out_);
  ARROW_RETURN_NOT_OK(Copy(d_srcs_, srcs.data(), nseg * sizeof(void*)));
  ARROW_RETURN_NOT_OK(Copy(d_sizes_, csz.data(), nseg * 4));
  BITAR_ABI(bitar_hip_decompress(ctx_, nullptr, BITAR_HIP_CODEC_DEFLATE_DYNAMIC,
                                 reinterpret_cast<const void* const*>(d_srcs_),
                                 static_cast<const uint32_t*>(d_sizes_),
                                 static_cast<uint32_t>(nseg), kSeg, dout, nseg * kSeg, d_prod),
            "bitar_hip_decompress");
  BITAR_ABI(bitar_hip_checksum(ctx_, nullptr, BITAR_HIP_CHECKSUM_CRC32, dout, nseg * kSeg, kSeg,
                               d_prod, static_cast<uint32_t>(nseg), sums),
            "bitar_hip_checksum");
  {
    std::vector<const void*> tab(2 * nseg);
    std::vector<uint32_t> len(nseg);
    uint64_t at = 0;
    for (uint64_t i = 0; i < nseg; ++i) {
      tab[i] = dout + i * kSeg;
      tab[nseg + i] = static_cast<uint8_t*>(d_join_) + at;
      len[i] = ms[m0 + i].isize;
      at += len[i];
    }
    auto* d_tab = static_cast<void**>(d_off_);
    ARROW_RETURN_NOT_OK(Copy(d_tab, tab.data(), 2 * nseg * sizeof(void*)));
    ARROW_RETURN_NOT_OK(Copy(d_tab + 2 * nseg, len.data(), nseg * 4));
    BITAR_ABI(bitar_hip_copy_batch(ctx_, nullptr, d_tab, d_tab + nseg,
                                   reinterpret_cast<const uint32_t*>(d_tab + 2 * nseg),
                                   static_cast<uint32_t>(nseg)),
              "bitar_hip_copy_batch");
  }
  std::vector<uint32_t> prod(nseg);
  std::vector<uint64_t> crcs(nseg);
  ARROW_RETURN_NOT_OK(Copy(prod.data(), d_prod, nseg * 4));
  ARROW_RETURN_NOT_OK(Copy(crcs.data(), sums, nseg * 8));
  ARROW_RETURN_NOT_OK(Sync());
  for (uint64_t i = 0; i < nseg; ++i) {
    const gzf::Member& m = ms[m0 + i];
    if (prod[i] != m.isize) return arrow::Status::IOError("gzip member decoded to a wrong size");
    if (static_cast<uint32_t>(crcs[i]) != m.crc)
      return arrow::Status::IOError("gzip CRC-32 mismatch");
  }
  ARROW_RETURN_NOT_OK(Copy(output, d_join_, total));
  return Sync();
}

arrow::Result<int64_t> HipCodec::DecompressGzip(uint64_t n, const uint8_t* input,
                                                int64_t output_buffer_len, uint8_t* output) {
  const bool in_dev = OnDevice(input);
  std::vector<uint8_t> host;  // the member walk needs the bytes on the host
  const uint8_t* hp = input;
  if (in_dev) {
    host.resize(n);
    ARROW_RETURN_NOT_OK(Copy(host.data(), input, n));
    ARROW_RETURN_NOT_OK(Sync());
    hp = host.data();
  }
  std::vector<gzf::Member> ms;
  ARROW_RETURN_NOT_OK(FromGzf(gzf::Walk(hp, n, &ms)));
  // ISIZE comes from untrusted trailers: the sum must fit the caller's buffer before
  // anything is reserved
  uint64_t declared = 0;
  bool singles = false;
  for (const gzf::Member& m : ms) {
    declared += m.isize;
    singles = singles || !m.indexed;
    if (declared > static_cast<uint64_t>(output_buffer_len))
      return arrow::Status::Invalid("declared gzip content exceeds the output buffer (",
                                    output_buffer_len, ")");
  }
  const uint8_t* d_in = input;
  if (singles && !in_dev) {
    ARROW_RETURN_NOT_OK(Reserve(d_in_, c_in_, n + 16));
    ARROW_RETURN_NOT_OK(Copy(d_in_, input, n));
    d_in = static_cast<const uint8_t*>(d_in_);
  }
  constexpr size_t kBatch = 8192;  // 512 MiB of staging per launch of small members
  uint64_t total = 0;
  for (size_t k = 0; k < ms.size();) {
    if (ms[k].indexed) {
      ARROW_RETURN_NOT_OK(GzipIndexed(ms[k], input, output + total));
      total += ms[k].isize;
      ++k;
      continue;
    }
    size_t k1 = k;
    uint64_t bytes = 0;
    while (k1 < ms.size() && !ms[k1].indexed && k1 - k < kBatch) bytes += ms[k1++].isize;
    ARROW_RETURN_NOT_OK(GzipSingles(ms, k, k1, d_in, output + total));
    total += bytes;
    k = k1;
  }
  return static_cast<int64_t>(total);
}

// ---- SNAPPY (one raw stream per buffer) ----

// The segments' raw streams joined on the device: varint(n), then every segment's elements.
// Only the stream's length visits the host.
arrow::Result<int64_t> HipCodec::CompressSnappy(uint64_t n, const uint8_t* input,
                                                int64_t output_buffer_len, uint8_t* output) {
  if (n > 0xFFFFFFFFull)
    return arrow::Status::NotImplemented("Snappy buffers of 4 GiB and above (a 32-bit preamble)");
  const uint64_t nseg = (n + kSeg - 1) / kSeg;
  const uint64_t stride = bitar_hip_slot_size(BITAR_HIP_CODEC_SNAPPY, kSeg);
  const uint64_t cap = n + 4 * nseg + 5;
  const void* d_in = input;
  if (n && !OnDevice(input)) {
    ARROW_RETURN_NOT_OK(Reserve(d_in_, c_in_, n));
    ARROW_RETURN_NOT_OK(Copy(d_in_, input, n));
    d_in = d_in_;
  }
  ARROW_RETURN_NOT_OK(Reserve(d_slab_, c_slab_, nseg * stride));
  ARROW_RETURN_NOT_OK(Reserve(d_sizes_, c_sizes_, nseg * 4));
  ARROW_RETURN_NOT_OK(Reserve(d_off_, c_off_, (nseg + 2) * 8));
  ARROW_RETURN_NOT_OK(Reserve(d_join_, c_join_, cap));
  auto* sizes = static_cast<uint32_t*>(d_sizes_);
  auto* offs = static_cast<uint64_t*>(d_off_);
  BITAR_ABI(bitar_hip_compress(ctx_, nullptr, BITAR_HIP_CODEC_SNAPPY, d_in, n, kSeg, d_slab_,
                               stride, sizes),
            "bitar_hip_compress");
  BITAR_ABI(bitar_hip_snappy_join(ctx_, nullptr, d_slab_, stride, sizes, n, kSeg, offs, d_join_,
                                  cap, offs + nseg + 1),
            "bitar_hip_snappy_join");
  uint64_t total = 0;
  ARROW_RETURN_NOT_OK(Copy(&total, offs + nseg + 1, sizeof total));
  ARROW_RETURN_NOT_OK(Sync());
  if (total > static_cast<uint64_t>(output_buffer_len))
    return arrow::Status::CapacityError("compressed stream exceeds the output buffer");
  ARROW_RETURN_NOT_OK(Copy(output, d_join_, total));
  ARROW_RETURN_NOT_OK(Sync());
  return static_cast<int64_t>(total);
}

// Any raw Snappy stream whose elements do not cross a multiple of 64 KiB of output (every
// stock writer's, and this codec's): the boundary scan finds the fragments on the device, one
// launch decodes them.  The host reads the preamble, the scan's status and the produced sizes.
arrow::Result<int64_t> HipCodec::DecompressSnappy(uint64_t n, const uint8_t* input,
                                                  int64_t output_buffer_len, uint8_t* output) {
  const bool in_dev = OnDevice(input);
  uint8_t head[5] = {0, 0, 0, 0, 0};
  const uint64_t nhead = std::min<uint64_t>(n, sizeof head);
  if (in_dev) {
    ARROW_RETURN_NOT_OK(Copy(head, input, nhead));
    ARROW_RETURN_NOT_OK(Sync());
  } else {
    std::memcpy(head, input, nhead);
  }
  // the preamble, by the segment decoder's rule: <= 5 bytes, the fifth below 16, any padding
  uint64_t declared = 0;
  bool have = false;
  for (uint64_t k = 0; k < nhead && !have; ++k) {
    if (k == 4 && head[k] >= 16) break;
    declared |= uint64_t(head[k] & 127u) << (7 * k);
    have = head[k] < 128;
  }
  if (!have) return arrow::Status::Invalid("Snappy stream without a length preamble");
  if (declared > static_cast<uint64_t>(output_buffer_len))
    return arrow::Status::Invalid("declared Snappy length ", declared,
                                  " exceeds the output buffer (", output_buffer_len, ")");
  const uint64_t nfrag = (declared + kSeg - 1) / kSeg;
  const uint8_t* d_in = input;
  if (!in_dev) {
    ARROW_RETURN_NOT_OK(Reserve(d_in_, c_in_, n + 16));
    ARROW_RETURN_NOT_OK(Copy(d_in_, input, n));
    d_in = static_cast<const uint8_t*>(d_in_);
  }
  const bool out_dev = OnDevice(output);
  uint8_t* dout = output;
  if (!out_dev) {
    ARROW_RETURN_NOT_OK(Reserve(d_out_, c_out_, std::max<uint64_t>(declared, 16)));
    dout = static_cast<uint8_t*>(d_out_);
  }
  ARROW_RETURN_NOT_OK(Reserve(d_off_, c_off_, (nfrag + 1) * 8));
  ARROW_RETURN_NOT_OK(Reserve(d_sizes_, c_sizes_, std::max<uint64_t>(nfrag * 4, 16)));
  ARROW_RETURN_NOT_OK(Reserve(d_meta_, c_meta_, 16));
  auto* starts = static_cast<uint64_t*>(d_off_);
  auto* d_status = static_cast<uint32_t*>(d_meta_);
  BITAR_ABI(bitar_hip_snappy_split(ctx_, nullptr, d_in, n, declared, 0, starts, d_status, nullptr),
            "bitar_hip_snappy_split");
  uint32_t status = 0;
  ARROW_RETURN_NOT_OK(Copy(&status, d_status, sizeof status));
  ARROW_RETURN_NOT_OK(Sync());
  if (status == BITAR_HIP_SNAPPY_SPLIT_UNSUPPORTED)
    return arrow::Status::NotImplemented("Snappy element across a 64 KiB block");
  if (status != BITAR_HIP_SNAPPY_SPLIT_OK)
    return arrow::Status::Invalid("corrupt Snappy stream: an element reads past its end, or its ",
                                  "elements do not produce the declared ", declared, " bytes");
  if (declared == 0) return 0;
  auto* d_prod = static_cast<uint32_t*>(d_sizes_);
  BITAR_ABI(bitar_hip_snappy_decompress_joined(ctx_, nullptr, d_in, n, declared, starts, dout,
                                               declared, d_prod),
            "bitar_hip_snappy_decompress_joined");
  std::vector<uint32_t> prod(nfrag);
  ARROW_RETURN_NOT_OK(Copy(prod.data(), d_prod, nfrag * 4));
  const int rc = bitar_hip_sync(ctx_, nullptr);
  if (rc != 0 && rc != BITAR_HIP_IO_ERROR) BITAR_ABI(rc, "segment codec");
  uint64_t bad = nfrag;
  for (uint64_t k = nfrag; k-- > 0;)
    if (prod[k] != std::min<uint64_t>(kSeg, declared - k * kSeg)) bad = k;
  if (rc != 0 || bad != nfrag)
    return arrow::Status::IOError("Snappy block ", bad, " of ", nfrag, " did not decode: the ",
                                  "stream is corrupt or has a copy that reaches before its ",
                                  "64 KiB block");
  if (!out_dev) {
    ARROW_RETURN_NOT_OK(Copy(output, dout, declared));
    ARROW_RETURN_NOT_OK(Sync());
  }
  return static_cast<int64_t>(declared);
}

}  // namespace

arrow::Result<std::unique_ptr<arrow::util::Codec>> MakeArrowCodec(arrow::Compression::type type,
                                                                  int device) {
  if (type == arrow::Compression::SNAPPY)
    return arrow::Status::NotImplemented(
        "HIP codec for snappy through MakeArrowCodec: use bitar::MakeArrowSnappyCodec");
  if (type != arrow::Compression::ZSTD && type != arrow::Compression::LZ4_FRAME &&
      type != arrow::Compression::GZIP)
    return arrow::Status::NotImplemented("HIP codec for ",
                                         arrow::util::Codec::GetCodecAsString(type));
  // gzip_frame.h restates the engine's DEFLATE slot size (it includes no engine header)
  for (uint32_t seg : {1u, 13u, 59460u, 65536u})
    if (gzf::SlotSize(seg) != bitar_hip_slot_size(BITAR_HIP_CODEC_DEFLATE_DYNAMIC, seg))
      return arrow::Status::UnknownError("gzip_frame.h and the engine disagree on the slot size");
  return std::unique_ptr<arrow::util::Codec>(new HipCodec(type, device));
}

arrow::Result<std::unique_ptr<arrow::util::Codec>> MakeArrowSnappyCodec(int device) {
  return std::unique_ptr<arrow::util::Codec>(new HipCodec(arrow::Compression::SNAPPY, device));
}

}  // namespace bitar
