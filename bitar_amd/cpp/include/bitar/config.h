// bitar/config.h -- device configuration (reference src/include/config.h:37-185).
//
// Same setters/getters and slot-sizing rule as the reference's Configuration<Class>; the
// DPDK rte_comp_xform / rte_comp_huffman / rte_comp_checksum_type types are replaced by
// plain enums, and the driver class MLX5_PCI by HIP_GFX950 (one MI355X = one device).
#pragma once

#include <cstdint>
#include <limits>
#include <string>
#include <string_view>
#include <type_traits>

namespace bitar {

namespace internal {

static inline constexpr auto kExpanseRatio = 1.1;  // reference config.h:41
// The reference caps segments at (65535 - RTE_PKTMBUF_HEADROOM) / 1.1 = 59460
// (config.h:42-47); kept for the uint16 API, the HIP engine also takes 65536 through
// set_decompressed_seg_size32.
static inline constexpr std::uint32_t kMaxMbufDataSize =
    std::numeric_limits<std::uint16_t>::max() - 128;
static inline constexpr std::uint32_t kMinSegSize = 8;
static inline constexpr std::uint32_t kMaxSegSize =
    static_cast<std::uint16_t>(kMaxMbufDataSize / kExpanseRatio);
static inline constexpr std::uint32_t kMaxSegSize32 = 65536;
static inline constexpr std::uint32_t kDefaultSegSize = 2048;
static inline constexpr std::uint16_t kMaxPreallocateSlots = 65535;

enum class DriverClass : std::int8_t { HIP_GFX950 };

template <typename EnumClass, typename Constant>
using IsEnumConstant = std::enable_if_t<std::is_enum_v<EnumClass> &&
                                        std::is_same_v<decltype(Constant::value), const EnumClass>>;

}  // namespace internal

using Class_HIP_GFX950 =
    std::integral_constant<internal::DriverClass, internal::DriverClass::HIP_GFX950>;

/// The segment codec (the reference hard-codes RTE_COMP_ALGO_DEFLATE, config.cc:86-88;
/// ZSTD is DPDK's RTE_COMP_ALGO_ZSTD-shaped option, BASELINE configs[5]).
/// INTPACK is the engine's integer codec (no reference or stock counterpart):
/// frame-of-reference bit packing, with optional delta, of little-endian elements of
/// HipConfiguration::element_width() bytes -- dictionary indices, small-range integers, sorted
/// keys, timestamps, string offsets.
/// FLTPACK is the engine's floating-point codec (likewise its own): values that
/// are an integer over a power of ten -- prices, sensor readings, coordinates, integer-valued
/// doubles -- are bit-packed as that integer, everything else is kept as an exception;
/// element_width() is 4 (float) or 8 (double).
/// DICTPACK is the engine's dictionary codec (likewise its own): per segment the
/// distinct elements in order of first occurrence and every element's bit-packed index -- hash
/// ids, UUIDs, decimal128, floats of a few hundred values; element_width() is 4, 8 or 16.
/// RUNPACK is the engine's run-length codec (likewise its own): per segment each
/// run's element and length -- sorted or clustered keys, coarse timestamps, flag and validity
/// bytes; element_width() is 1, 2, 4, 8 or 16.
/// AUTOPACK has no format of its own: per segment it writes the smallest of the
/// streams RUNPACK, INTPACK, DICTPACK and FLTPACK give at element_width() (1, 2, 4, 8 or 16; a
/// codec is tried at the widths it has), and decodes each segment by its tag -- for columns whose
/// shape is not known in advance or changes along the column.
/// CASCADE is the engine's cascaded run-length codec (likewise its own): RUNPACK's
/// runs with their values and lengths bit-packed by INTPACK -- sorted keys, coarse timestamps,
/// clustered status codes, flag bytes; element_width() is 1, 2, 4 or 8.  No candidate of AUTOPACK.
/// RANS is the engine's order-0 rANS entropy coder (likewise its own): 64
/// interleaved states per segment, for bytes whose gain is their histogram and not their repeats
/// -- non-decimal floats behind Filter::SHUFFLE or BITSHUFFLE, embeddings, noisy sensor words;
/// one level, no window, no chained operations; filters and checksums as for LZ4.
/// RANSPLANE is RANS with one table per byte plane of an element (likewise its own, DESIGN.md
/// 4.26): bf16 / fp16 / fp32 / fp64 weights, activations and embeddings, whose exponent byte and
/// low mantissa bytes have different histograms; element_width() is 2, 4 or 8 and, unlike the
/// other column codecs, is needed on the decompressing side too; it takes no filter.
/// SYMTAB is the engine's per-segment symbol table (likewise its own), in the
/// style of FSST: up to 255 strings of 1..8 bytes, the text written as one-byte codes -- the data
/// buffer of a string or binary column (names, URLs, log lines, keys); a byte codec with no element
/// width, one level, no window, no chained operations; filters and checksums as for LZ4.
/// PATCHPACK is INTPACK with per-miniblock exceptions (likewise its own): the few
/// residuals that would widen a miniblock are kept raw behind the payload -- timestamps with gaps,
/// string offsets with a long string, heavy-tailed counts, INT_MAX, 0 or -1 written for "missing";
/// element_width() is 1, 2, 4 or 8.  No candidate of AUTOPACK.
/// DECPACK is INTPACK's frame-of-reference bit packing for 16-byte integers (likewise its own,
/// DESIGN.md 4.30; its id is one of the ids from 256 on, include/bitar_hip_codecs.h): Arrow
/// decimal128 columns, whose values are a few bytes of digits under 12 or 13 bytes of sign
/// extension; element_width() is 16.  No exceptions for outliers, no candidate of AUTOPACK.
/// SNAPPY is one raw Snappy stream per segment: the LZ4 codec's fast parse with
/// a Snappy emitter, readable by every stock Snappy decoder; one level, chained operations and
/// checksums as for LZ4.
enum class Codec : std::uint8_t {
  DEFLATE = 1, LZ4 = 2, ZSTD = 3, INTPACK = 4, FLTPACK = 5, DICTPACK = 6, RUNPACK = 7,
  AUTOPACK = 8, SNAPPY = 9, CASCADE = 10, RANS = 11, RANSPLANE = 12, SYMTAB = 13,
  PATCHPACK = 14, DECPACK = 15
};
/// rte_comp_huffman
enum class HuffmanEncoding : std::uint8_t { DEFAULT = 0, FIXED = 1, DYNAMIC = 2 };
/// rte_comp_checksum_type
enum class ChecksumType : std::uint8_t { NONE = 0, CRC32 = 1, ADLER32 = 2, CRC32_ADLER32 = 3 };

/// A per-segment transposition of fixed-width elements in front of the codec (no reference
/// counterpart; include/bitar_hip.h bitar_hip_filter): SHUFFLE gathers byte j of every element
/// (Blosc shuffle / Parquet BYTE_STREAM_SPLIT per segment), BITSHUFFLE bit b of byte j (the
/// HDF5 bitshuffle layout).
enum class Filter : std::uint8_t { NONE = 0, SHUFFLE = 1, BITSHUFFLE = 2 };

std::string_view ToString(Codec c);
std::string_view ToString(Filter f);
std::string_view ToString(HuffmanEncoding h);
std::string_view ToString(ChecksumType c);

template <typename Class,
          typename = internal::IsEnumConstant<internal::DriverClass, Class>>
class Configuration {
 public:
  Configuration() { UpdateCompressedSegSize(); }
  Configuration(const Configuration&) = default;
  Configuration(Configuration&&) noexcept = default;
  Configuration& operator=(const Configuration&) = default;
  Configuration& operator=(Configuration&&) noexcept = default;
  virtual ~Configuration() = default;

  [[nodiscard]] virtual std::string ToString() const;
  [[nodiscard]] virtual std::string_view type_name() const noexcept = 0;

  /// Ops per burst.  The HIP engine launches one kernel per call over every segment, so the
  /// value is validated (> 0) and reported but does not cut launches.
  [[nodiscard]] auto burst_size() const noexcept { return burst_size_; }
  void set_burst_size(std::uint16_t burst_size) { burst_size_ = burst_size; }

  /// Segments chained per op (SGL, reference default 1).  k > 1: the k segments of an op are
  /// compressed as one stream and spread over k slots (device.cc, chained ops).
  [[nodiscard]] auto max_sgl_segs() const noexcept { return max_sgl_segs_; }
  void set_max_sgl_segs(std::uint16_t max_sgl_segs) { max_sgl_segs_ = max_sgl_segs; }

  /// Bytes of uncompressed data per segment.
  [[nodiscard]] std::uint32_t decompressed_seg_size() const noexcept {
    return decompressed_seg_size_;
  }
  void set_decompressed_seg_size(std::uint16_t decompressed_seg_size) {
    decompressed_seg_size_ = decompressed_seg_size;
    UpdateCompressedSegSize();
  }
  /// 32-bit form for 64 KiB segments (BASELINE's chunk size), which uint16 cannot express.
  void set_decompressed_seg_size32(std::uint32_t decompressed_seg_size) {
    decompressed_seg_size_ = decompressed_seg_size;
    UpdateCompressedSegSize();
  }

  /// The reference's slot size for compressed output (config.cc:59-73).  The HIP engine's
  /// slots are max(this, the codec's worst-case bound), see CompressDevice::slot_size().
  [[nodiscard]] std::uint32_t compressed_seg_size() const noexcept {
    return compressed_seg_size_;
  }

  /// log2 of the sliding window; 0 = the device maximum.  INTPACK, FLTPACK, DICTPACK, RUNPACK, AUTOPACK, CASCADE, RANS, RANSPLANE, SYMTAB, PATCHPACK and DECPACK have no window: Initialize
  /// ignores the value and reports 0.
  [[nodiscard]] auto window_size() const noexcept { return window_size_; }
  void set_window_size(std::uint8_t window_size) { window_size_ = window_size; }

  [[nodiscard]] auto huffman_enc() const noexcept { return huffman_enc_; }
  void set_huffman_enc(HuffmanEncoding huffman_enc) { huffman_enc_ = huffman_enc; }

  /// Output slots preallocated per device (the reference's memzones).
  [[nodiscard]] auto max_preallocate_memzones() const noexcept {
    return max_preallocate_memzones_;
  }
  void set_max_preallocate_memzones(std::uint16_t n) { max_preallocate_memzones_ = n; }

  [[nodiscard]] auto codec() const noexcept { return codec_; }
  void set_codec(Codec codec) { codec_ = codec; }

  /// Compression level, 1..9 (rte_comp_compress_xform.level; the reference always sets 1,
  /// config.cc:86-88).  LZ4: 1 = the fast parse, >= 2 = the wide parse (16 KiB history, the
  /// ratio operating point, BITAR_HIP_CODEC_LZ4_WIDE).  The other codecs have one level.
  [[nodiscard]] auto level() const noexcept { return level_; }
  void set_level(std::uint8_t level) { level_ = level; }

 private:
  /// Configuration::UpdateCompressedSegSize (reference config.cc:59-73): the highest set bit
  /// of 2*seg, or seg*1.1 when that exceeds 32 KiB.
  void UpdateCompressedSegSize() noexcept {
    const auto lower_bound = static_cast<std::uint32_t>(decompressed_seg_size_ << 1U);
    std::uint32_t num = 1U << 17;
    while (num && (num & lower_bound) == 0) num >>= 1U;
    compressed_seg_size_ =
        num > (65536U >> 1U)
            ? static_cast<std::uint32_t>(static_cast<double>(decompressed_seg_size_) *
                                         internal::kExpanseRatio)
            : num;
  }

  std::uint16_t burst_size_ = 32;
  std::uint16_t max_sgl_segs_ = 1U;
  std::uint32_t decompressed_seg_size_ = internal::kDefaultSegSize;
  std::uint32_t compressed_seg_size_{};
  std::uint8_t window_size_ = 0U;
  HuffmanEncoding huffman_enc_ = HuffmanEncoding::DYNAMIC;  // reference config.h:151
  std::uint16_t max_preallocate_memzones_ = 1024;
  Codec codec_ = Codec::DEFLATE;
  std::uint8_t level_ = 1;
};

static inline constexpr std::string_view kHipConfigurationTypeName{"hip_gfx950"};

/// Configuration of an MI355X compress device (the BlueFieldConfiguration analogue,
/// reference config.h:155-183).
class HipConfiguration : public Configuration<Class_HIP_GFX950> {
 public:
  [[nodiscard]] std::string_view type_name() const noexcept override {
    return kHipConfigurationTypeName;
  }
  [[nodiscard]] std::string ToString() const override;

  [[nodiscard]] auto checksum_type() const noexcept { return checksum_type_; }
  void set_checksum_type(ChecksumType checksum_type) { checksum_type_ = checksum_type; }

  /// Filter applied to every segment before it is compressed and undone after it is
  /// decompressed; element_width is the column's value size in bytes, 2, 4, 8 or 16.  Checksums
  /// stay over the caller's (unfiltered) bytes.  Both sides of a frame must be configured alike:
  /// filter and width travel with the frame like codec and segment size.  Not combined with
  /// chained ops (max_sgl_segs > 1).  Default: NONE, width 1.
  [[nodiscard]] auto filter() const noexcept { return filter_; }
  [[nodiscard]] auto element_width() const noexcept { return element_width_; }
  void set_filter(Filter filter, std::uint8_t element_width) {
    filter_ = filter;
    element_width_ = element_width;
  }
  /// The element width alone: what Codec::INTPACK (1, 2, 4 or 8 bytes), Codec::FLTPACK (4 or
  /// 8 bytes), Codec::DICTPACK (4, 8 or 16 bytes), Codec::RUNPACK and Codec::AUTOPACK (1, 2, 4,
  /// 8 or 16 bytes), Codec::CASCADE (1, 2, 4 or 8 bytes), Codec::RANSPLANE (2, 4 or 8 bytes), Codec::PATCHPACK (1, 2, 4 or 8 bytes) and Codec::DECPACK (16 bytes) pack; they take no filter.  The decoder reads the width from each stream, so only the compressing side needs it
  /// -- except for Codec::RANSPLANE, whose decoder is the configured width's own and rejects
  /// streams of another width.
  void set_element_width(std::uint8_t element_width) { element_width_ = element_width; }

  static HipConfiguration Defaults() { return {}; }

 private:
  ChecksumType checksum_type_ = ChecksumType::NONE;
  Filter filter_ = Filter::NONE;
  std::uint8_t element_width_ = 1;
};

}  // namespace bitar
