// runtime.hip -- the C-ABI of libbitar_hip.so (include/bitar_hip.h).
//
// A context = one gfx950 device + N HIP streams (queue pairs) + a sticky device error word.
// Every entry point validates shapes on the host before launching, so a kernel never sees a
// grid or a size it does not assume (one wave per segment, seg <= 65536).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/bitar_hip.h"
#include "../../include/bitar_hip_codecs.h"
#include "../../include/bitar_hip_snappy.h"
#define BITAR_COLUMN_DECLARATIONS_ONLY  // (the kernels are defined in the formats' files)
#include "autopack.hip.h"
#include "kernels.hip.h"
#include "order.hip.h"
#include "zstd_hand.hip.h"
#include "zstd_layout.hip.h"

// Error words: one sticky uint32 per stream (bit0 decode error, bit1 slot overflow, bit2 a
// failed segment handed to pack).  Word 0 serves the NULL stream, word q+1 queue pair q, and
// further words are handed out on first use to foreign streams (e.g. torch's current
// stream), so a failure on one queue pair is never reported by -- or cleared by -- another
// (the reference reports errors per queue pair: device.cc:84-110, 512-520).
constexpr uint32_t kErrWords = 1024;

struct bitar_hip_ctx {
  int device = -1;
  std::vector<hipStream_t> streams;
  uint32_t* d_err = nullptr;  // kErrWords words
  unsigned long long* d_stats = nullptr;  // BITAR_HIP_PATH_COUNT path counters
  // decoder options (bitar_hip_decoder_options), per context
  std::atomic<uint32_t> inflate_lanes{4}, zstd_lanes{16}, zstd_seq{1}, count_paths{0};
  std::atomic<uint32_t> zstd_fork{1};  // Zstd literals beside phase A (decompress_zstd)
  std::atomic<uint32_t> cost_order{1};  // LZ4: dispatch the estimated most expensive segments first
  // priority lanes (order.hip.h): the device's CUs, and the resident workgroups of the fast
  // LZ4 compressor, queried on first use (0: not yet)
  uint32_t cus = 0;
  std::atomic<uint32_t> lane_slots{0};
  std::mutex mu;              // guards `words` and `order_scratch`
  std::vector<std::pair<hipStream_t, uint32_t>> words;  // stream -> error word index
  // cost-ordered dispatch scratch of the context's own streams (and the default stream),
  // cached per (stream, slot) and reused in stream order (a call holds its entry's mutex from
  // the sort's launch to the last launch that reads it); foreign streams get per-call scratch
  struct OrderScratch {
    hipStream_t stream;
    int slot;
    void* p = nullptr;
    uint64_t cap = 0;
    std::mutex m;
    OrderScratch(hipStream_t s, int k) : stream(s), slot(k) {}
  };
  std::list<OrderScratch> order_scratch;
  // host-memory calls (bitar_hip_compress_host / _decompress_host): the copy stream paired
  // with each caller stream, created on first use
  std::vector<std::pair<hipStream_t, hipStream_t>> copy_streams;
  // per caller stream: a stream for kernels forked off it (Zstd literals beside sequences)
  std::vector<std::pair<hipStream_t, hipStream_t>> aux_streams;
};

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(e == hipErrorOutOfMemory ? BITAR_HIP_OUT_OF_MEMORY : BITAR_HIP_UNKNOWN_ERROR,
              std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr, what)                       \
  do {                                            \
    hipError_t _e = (expr);                       \
    if (_e != hipSuccess) return hip_fail(_e, what); \
  } while (0)

int enter(bitar_hip_ctx* ctx) {
  if (!ctx) return fail(BITAR_HIP_INVALID, "null context");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  return 0;
}

// NULL is the HIP default stream (the usual HIP convention); queue-pair streams come from
// bitar_hip_stream().
hipStream_t pick_stream(bitar_hip_ctx*, void* stream) {
  return reinterpret_cast<hipStream_t>(stream);
}

constexpr uint32_t kMaxSeg = BITAR_HIP_MAX_SEG_SIZE;
constexpr uint32_t kMaxZstdFrame = 1u << 30;

// Calls whose kernels need per-segment scratch (dynamic DEFLATE and Zstd compress, Zstd
// decode) run in chunks of at most kChunkSegs segments (2 GiB of 64 KiB segments: every
// chunk still fills the chip many times over) over ONE scratch allocation sized for a chunk,
// so a call's scratch is bounded whatever its size.  Chunks are balanced (a 18059-segment
// call is one chunk, a 65536-segment call two of 32768).
constexpr uint64_t kChunkSegs = 32768;
struct Chunks {
  uint64_t size;
  explicit Chunks(uint64_t nseg, uint64_t most = kChunkSegs) {
    const uint64_t k = (nseg + most - 1) / most;
    size = k ? (nseg + k - 1) / k : 1;
  }
};
// The device pool's cached stream-ordered memory above this is returned to the driver at
// the next synchronisation (a chunk of Zstd compress scratch is ~12 GB; steady-state calls
// stay below this and never touch the driver).
constexpr uint64_t kPoolKeepBytes = 24ull << 30;
// AUTOPACK compress keeps a whole slot per segment and later candidate (up to three of them):
// chunks of at most 8192 segments bound that scratch at 3 * 8192 * 65792 B = 1.6 GB (64 KiB
// segments, element widths 4 and 8), and 8192 one-wave workgroups still cover the chip.
// Decompress keeps 16 bytes per segment (four index lists): 1 MiB per chunk of 65536 segments.
constexpr uint64_t kAutoChunkSegs = 8192;
constexpr uint64_t kAutoDecChunkSegs = 65536;

// index of the error word of `stream`; words run out only after 1000+ distinct foreign
// streams, after which they share the NULL stream's word (still correct, merely coarser)
uint32_t word_index(bitar_hip_ctx* ctx, hipStream_t stream) {
  if (!stream) return 0;
  for (uint32_t q = 0; q < ctx->streams.size(); ++q)
    if (ctx->streams[q] == stream) return q + 1;
  std::lock_guard<std::mutex> g(ctx->mu);
  for (auto& w : ctx->words)
    if (w.first == stream) return w.second;
  const uint32_t next = (uint32_t)(ctx->streams.size() + 1 + ctx->words.size());
  if (next >= kErrWords) return 0;
  ctx->words.emplace_back(stream, next);
  return next;
}

uint32_t* err_word(bitar_hip_ctx* ctx, hipStream_t stream) {
  return ctx->d_err + word_index(ctx, stream);
}

int sync_error(uint32_t err) {
  if (!err) return 0;
  if (err & 2u) return fail(BITAR_HIP_IO_ERROR, "Compress data output is larger than allocated buffer");
  if (err & 4u)
    return fail(BITAR_HIP_IO_ERROR, "pack / join: a segment's size exceeds its slot (failed op)");
  return fail(BITAR_HIP_IO_ERROR, "Some operations have failed");
}

}  // namespace

static void init_options(bitar_hip_ctx* ctx, uint32_t flags);
static void free_order_scratch(bitar_hip_ctx* ctx);

extern "C" {

int bitar_hip_abi_version(void) { return BITAR_HIP_ABI_VERSION; }

const char* bitar_hip_last_error(void) { return g_last_error.c_str(); }

int bitar_hip_device_count(int* count) {
  if (!count) return fail(BITAR_HIP_INVALID, "null count");
  *count = 0;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e == hipErrorNoDevice || n == 0) return 0;
  if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
  int gfx950 = 0;
  for (int d = 0; d < n; ++d) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d) == hipSuccess &&
        std::strncmp(prop.gcnArchName, "gfx950", 6) == 0)
      ++gfx950;
  }
  *count = gfx950;
  return 0;
}

int bitar_hip_open(int device, const bitar_hip_config* cfg, bitar_hip_ctx** out) {
  if (!out) return fail(BITAR_HIP_INVALID, "null out");
  *out = nullptr;
  const uint32_t nstreams = cfg && cfg->num_streams ? cfg->num_streams : 1;
  if (nstreams > 64) return fail(BITAR_HIP_INVALID, "num_streams must be in [1, 64]");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n), "hipGetDeviceCount");
  if (device < 0 || device >= n) return fail(BITAR_HIP_INVALID, "no such device");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(BITAR_HIP_NOT_IMPLEMENTED,
                std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950");
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  auto* ctx = new bitar_hip_ctx();
  ctx->device = device;
  ctx->cus = (uint32_t)prop.multiProcessorCount;
  for (uint32_t q = 0; q < nstreams; ++q) {
    hipStream_t s;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) {
      bitar_hip_close(ctx);
      return hip_fail(e, "hipStreamCreate");
    }
    ctx->streams.push_back(s);
  }
  // stream-ordered scratch (dynamic-Huffman DEFLATE) comes from the device's default pool;
  // keep its memory cached between calls instead of returning it at every sync
  {
    hipMemPool_t pool;
    if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess) {
      uint64_t keep = kPoolKeepBytes;
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
    (void)hipGetLastError();
  }
  init_options(ctx, cfg ? cfg->flags : 0u);
  hipError_t e = hipMalloc(&ctx->d_err, kErrWords * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(ctx->d_err, 0, kErrWords * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&ctx->d_stats, BITAR_HIP_PATH_COUNT * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(ctx->d_stats, 0, BITAR_HIP_PATH_COUNT * sizeof(unsigned long long));
  if (e != hipSuccess) {
    bitar_hip_close(ctx);
    return hip_fail(e, "error word");
  }
  *out = ctx;
  return 0;
}

int bitar_hip_close(bitar_hip_ctx* ctx) {
  if (!ctx) return 0;
  if (hipSetDevice(ctx->device) == hipSuccess) {
    for (auto s : ctx->streams) {
      (void)hipStreamSynchronize(s);
      (void)hipStreamDestroy(s);
    }
    (void)hipDeviceSynchronize();  // (order scratch may sit on foreign streams)
    free_order_scratch(ctx);
    for (auto& cs : ctx->copy_streams) (void)hipStreamDestroy(cs.second);
    ctx->copy_streams.clear();
    for (auto& cs : ctx->aux_streams) (void)hipStreamDestroy(cs.second);
    ctx->aux_streams.clear();
    if (ctx->d_err) (void)hipFree(ctx->d_err);
    if (ctx->d_stats) (void)hipFree(ctx->d_stats);
  }
  delete ctx;
  return 0;
}

int bitar_hip_stream(bitar_hip_ctx* ctx, uint32_t qp, void** stream) {
  if (!ctx || !stream) return fail(BITAR_HIP_INVALID, "null argument");
  if (qp >= ctx->streams.size()) return fail(BITAR_HIP_INVALID, "queue pair out of range");
  *stream = ctx->streams[qp];
  return 0;
}

int bitar_hip_device(bitar_hip_ctx* ctx, int* device) {
  if (!ctx || !device) return fail(BITAR_HIP_INVALID, "null argument");
  *device = ctx->device;
  return 0;
}

extern "C++" {
// The column codecs: a family's ids are base + log2(element width) for the widths it offers
// (`widths`: those widths ORed together, so bit lg stands for 1 << lg bytes), and its streams
// carry `nibble` in the high half of byte 0
// (AUTOPACK has no format of its own).  CASCADE, RANSPLANE, PATCHPACK, RANS, SYMTAB and DECPACK are no
// candidates of AUTOPACK: they have no store-less encoder and no listed decoder, and they come
// after the families that do.  RANS and SYMTAB are byte codecs run by the column kernels: one id
// each, width 1.  Two orders here are load-bearing:
//   Candidate order (AUTOPACK compress): RUNPACK first, into the caller's slot; then INTPACK,
//     DICTPACK, FLTPACK into scratch slabs k = 0, 1, 2.  autopack_select_kernel breaks ties
//     towards the earlier candidate.
//   Listed-decoder order (AUTOPACK decompress): list f belongs to family f of this table, tag
//     nibble 4 + f -- INTPACK, FLTPACK, DICTPACK, RUNPACK -- which is what autopack_route_kernel
//     writes.
enum ColumnFamily : int {
  kIntPack, kFltPack, kDictPack, kRunPack, kAutoPack, kCascade, kRansPlane, kPatchPack, kRans,
  kSymTab, kDecPack, kColumnFamilies
};
struct ColumnRow {
  uint32_t base, nibble, widths;
};
constexpr ColumnRow kColumn[kColumnFamilies] = {
    {BITAR_HIP_CODEC_INTPACK8, 4, 1 | 2 | 4 | 8},            // INTPACK
    {BITAR_HIP_CODEC_FLTPACK32 - 2, 5, 4 | 8},               // FLTPACK
    {BITAR_HIP_CODEC_DICTPACK32 - 2, 6, 4 | 8 | 16},         // DICTPACK
    {BITAR_HIP_CODEC_RUNPACK8, 7, 1 | 2 | 4 | 8 | 16},       // RUNPACK
    {BITAR_HIP_CODEC_AUTOPACK8, 0, 1 | 2 | 4 | 8 | 16},      // AUTOPACK
    {BITAR_HIP_CODEC_CASCADE8, 8, 1 | 2 | 4 | 8},            // CASCADE (no candidate of AUTOPACK)
    {BITAR_HIP_CODEC_RANSPLANE16 - 1, 0xB, 2 | 4 | 8},       // RANSPLANE (likewise)
    {BITAR_HIP_CODEC_PATCHPACK8, 9, 1 | 2 | 4 | 8},          // PATCHPACK (likewise)
    {BITAR_HIP_CODEC_RANS, 0xA, 1},                          // RANS (likewise; bytes)
    {BITAR_HIP_CODEC_SYMTAB, 0xC, 1},                        // SYMTAB (likewise; bytes)
    {BITAR_HIP_CODEC_DECPACK128 - 4, 0xD, 16},               // DECPACK (likewise; bitar_hip_codecs.h)
};
constexpr ColumnFamily kCandidates[] = {kRunPack, kIntPack, kDictPack, kFltPack};
constexpr uint32_t kListedDecoders = 4;
static_assert(kColumn[kIntPack].nibble == 4 && kColumn[kFltPack].nibble == 5 &&
                  kColumn[kDictPack].nibble == 6 && kColumn[kRunPack].nibble == 7,
              "list f is tag nibble 4 + f");

static bool offers(ColumnFamily f, uint32_t lg) { return lg < 5 && (kColumn[f].widths >> lg & 1u); }

// codec -> its family and log2 of its element width; family kColumnFamilies: not a column codec
struct ColumnCodec {
  ColumnFamily family;
  uint32_t lg;
  explicit operator bool() const { return family != kColumnFamilies; }
};
static ColumnCodec column_codec(uint32_t codec) {
  for (int f = 0; f < kColumnFamilies; ++f)
    if (offers((ColumnFamily)f, codec - kColumn[f].base))
      return {(ColumnFamily)f, codec - kColumn[f].base};
  return {kColumnFamilies, 0};
}

// The kernels of a family (not AUTOPACK) at a width it offers: the one place where a run-time
// width becomes a template argument.  Only instantiations the formats' files define are named.
using CompressKernel = void (*)(const uint8_t*, uint64_t, uint32_t, uint8_t*, uint64_t,
                                uint8_t* const*, uint32_t*);
using DecompressKernel = void (*)(const uint8_t* const*, const uint8_t*, uint64_t, const uint32_t*,
                                  uint32_t, uint32_t, uint8_t*, uint32_t*, uint32_t*,
                                  const uint32_t*, const uint32_t*);
template <class F, ColumnFamily FAMILY, bool STORE, uint32_t LG = 0>
static CompressKernel width_kernel(uint32_t lg) {
  if constexpr (LG < 5) {
    if constexpr ((kColumn[FAMILY].widths >> LG & 1u) != 0)
      if (lg == LG) return bitar_hip::column_compress_kernel<F, 1u << LG, STORE>;
    return width_kernel<F, FAMILY, STORE, LG + 1>(lg);
  } else {
    return nullptr;
  }
}
// STORE = false: the store-less form of a later candidate of AUTOPACK (RUNPACK, always the
// first, has none)
template <bool STORE>
static CompressKernel compress_kernel(ColumnFamily f, uint32_t lg) {
  switch (f) {
    case kIntPack: return width_kernel<bitar_hip::IntPack, kIntPack, STORE>(lg);
    case kFltPack: return width_kernel<bitar_hip::FltPack, kFltPack, STORE>(lg);
    case kDictPack: return width_kernel<bitar_hip::DictPack, kDictPack, STORE>(lg);
    case kRunPack: return width_kernel<bitar_hip::RunPack, kRunPack, true>(lg);
    case kCascade: return width_kernel<bitar_hip::Cascade, kCascade, true>(lg);
    case kRansPlane: return width_kernel<bitar_hip::RansPlane, kRansPlane, true>(lg);
    case kPatchPack: return width_kernel<bitar_hip::PatchPack, kPatchPack, true>(lg);
    case kRans: return width_kernel<bitar_hip::Rans, kRans, true>(lg);
    case kSymTab: return width_kernel<bitar_hip::SymTab, kSymTab, true>(lg);
    case kDecPack: return width_kernel<bitar_hip::DecPack, kDecPack, true>(lg);
    default: return nullptr;
  }
}
// The decoder of a family (not AUTOPACK).  A stream's tag carries its width, so the families
// ignore lg, but for RANSPLANE: one decoder per element width (its LDS is the width's), and an id
// decodes its own width alone.  LISTED: AUTOPACK's decoder of one of its candidates' formats; the
// other families have no listed form.
template <bool LISTED>
static DecompressKernel decompress_kernel(uint32_t f, uint32_t lg) {
  using namespace bitar_hip;
  switch (f) {
    case kIntPack: return column_decompress_kernel<IntPack, LISTED>;
    case kFltPack: return column_decompress_kernel<FltPack, LISTED>;
    case kDictPack: return column_decompress_kernel<DictPack, LISTED>;
    case kRunPack: return column_decompress_kernel<RunPack, LISTED>;
  }
  if constexpr (!LISTED) {
    switch (f) {
      case kCascade: return column_decompress_kernel<Cascade, false>;
      case kPatchPack: return column_decompress_kernel<PatchPack, false>;
      case kRans: return column_decompress_kernel<Rans, false>;
      case kSymTab: return column_decompress_kernel<SymTab, false>;
      case kDecPack: return column_decompress_kernel<DecPack, false>;
      case kRansPlane:
        switch (lg) {
          case 1: return column_decompress_kernel<RansPlaneDecoder<2>, false>;
          case 2: return column_decompress_kernel<RansPlaneDecoder<4>, false>;
          default: return column_decompress_kernel<RansPlaneDecoder<8>, false>;
        }
    }
  }
  return nullptr;
}

// What the entry points know about an id: the format it decodes as (its own, or the one two
// parses share; 0: no such codec), the worst-case size of a segment's stream, the largest match
// distance its encoder emits, and its column family if it has one.  kByte has a row per byte
// codec; find_codec() looks there and in kColumn, and nothing else lists the ids that exist.
// The window-scan parse verifies candidates in its LDS input ring, which runs up to 1536 B
// ahead of the scan: a 4 KiB ring (window_parse.hip.h kMaxDist) for the fast parses of LZ4,
// DEFLATE and Zstd, a 16 KiB ring for the wide LZ4 parse (compress.hip, lz4_wide).  A column
// codec's max distance of 0 is "none", it has no matches at all; an unknown id's is "unknown".
struct Codec {
  uint32_t id, format;
  uint64_t (*bound)(uint64_t seg);
  uint32_t max_distance;
  ColumnCodec column = {kColumnFamilies, 0};
  explicit operator bool() const { return format != 0; }
};
constexpr uint64_t column_bound(uint64_t n) { return n + 4u; }  // the stored form: header + the segment
constexpr uint64_t lz4_bound(uint64_t n) { return n + n / 255u + 16u; }  // LZ4_compressBound
constexpr uint64_t snappy_bound(uint64_t n) { return n + 6u; }  // the stored form: varint + tag + segment
constexpr uint64_t deflate_bound(uint64_t n) { return (n * 9 + 7) / 8 + 16u; }  // fixed Huffman, 9 bits/literal
constexpr uint64_t zstd_bound(uint64_t n) { return n + 7u + 3u + 8u + 512u; }  // oracle bo_zstd_bound: one block, raw if larger
constexpr uint32_t kFastReach = 4096u - 1536u, kWideReach = 16384u - 1536u;
constexpr Codec kByte[] = {
    {BITAR_HIP_CODEC_LZ4, BITAR_HIP_CODEC_LZ4, lz4_bound, kFastReach},
    {BITAR_HIP_CODEC_LZ4_WIDE, BITAR_HIP_CODEC_LZ4, lz4_bound, kWideReach},  // same format
    {BITAR_HIP_CODEC_SNAPPY, BITAR_HIP_CODEC_SNAPPY, snappy_bound, kFastReach},  // (the LZ4 codec's parse)
    {BITAR_HIP_CODEC_DEFLATE, BITAR_HIP_CODEC_DEFLATE, deflate_bound, kFastReach},
    {BITAR_HIP_CODEC_DEFLATE_DYNAMIC, BITAR_HIP_CODEC_DEFLATE, deflate_bound, kFastReach},  // same format
    {BITAR_HIP_CODEC_ZSTD, BITAR_HIP_CODEC_ZSTD, zstd_bound, kFastReach},
};
static Codec find_codec(uint32_t id) {
  for (const Codec& r : kByte)
    if (r.id == id) return r;
  if (const ColumnCodec cc = column_codec(id)) return {id, id, column_bound, 0, cc};
  return {};
}
}  // extern "C++"

// AUTOPACK decode: 1 (default) sorts the segments into one index list per format on the device,
// 0 has every format's decoder look at every segment's tag (DESIGN.md 4.21 has both measured).
// Read at every call, so that one process can run both forms alternately.
static bool autopack_lists() {
  const char* e = std::getenv("BITAR_HIP_AUTOPACK_LISTS");
  return !(e && e[0] == '0' && e[1] == 0);
}

// AUTOPACK compress: 1 (default) runs the later candidates in their store-less form, 0 the
// codecs' own kernels (DESIGN.md 4.21 has both measured).  Read at every call.
static bool autopack_storeless() {
  const char* e = std::getenv("BITAR_HIP_AUTOPACK_STORELESS");
  return !(e && e[0] == '0' && e[1] == 0);
}

uint64_t bitar_hip_slot_size(uint32_t codec, uint32_t seg) {
  const Codec c = find_codec(codec);
  return c ? (c.bound(seg) + 255u) & ~(uint64_t)255u : 0;
}

uint32_t bitar_hip_max_distance(uint32_t codec) { return find_codec(codec).max_distance; }

int bitar_hip_alloc(bitar_hip_ctx* ctx, uint64_t bytes, void** ptr) {
  if (int r = enter(ctx)) return r;
  if (!ptr) return fail(BITAR_HIP_INVALID, "null ptr");
  HIP_TRY(hipMalloc(ptr, bytes ? bytes : 1), "hipMalloc");
  return 0;
}

int bitar_hip_free(bitar_hip_ctx* ctx, void* ptr) {
  if (int r = enter(ctx)) return r;
  HIP_TRY(hipFree(ptr), "hipFree");
  return 0;
}

int bitar_hip_host_alloc(bitar_hip_ctx* ctx, uint64_t bytes, void** ptr) {
  if (int r = enter(ctx)) return r;
  if (!ptr) return fail(BITAR_HIP_INVALID, "null ptr");
  HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault), "hipHostMalloc");
  return 0;
}

int bitar_hip_host_free(bitar_hip_ctx* ctx, void* ptr) {
  if (int r = enter(ctx)) return r;
  HIP_TRY(hipHostFree(ptr), "hipHostFree");
  return 0;
}

int bitar_hip_memcpy(bitar_hip_ctx* ctx, void* dst, const void* src, uint64_t bytes,
                     void* stream) {
  if (int r = enter(ctx)) return r;
  if (!bytes) return 0;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, pick_stream(ctx, stream)),
          "hipMemcpyAsync");
  return 0;
}

// Cost-ordered dispatch (util_kernels.hip, seg_order_kernel): a launch of one wave per segment
// ends with a drain of about one segment's duration, longest when expensive segments come
// last.  For calls of at least kOrderMinSegs segments the LZ4 kernels take their segments in
// the order of an estimated cost key, most expensive first.  Measured (1 GiB, kind 1 = 1 MiB
// regions of columns / text / random data): see DESIGN.md 4.1.
extern "C++" {
constexpr uint32_t kOrderMinSegs = 2048;
// An order is an optimisation only: make() cannot fail, and where its scratch cannot be
// allocated (or the call is too small, or ordering is off) the call runs in plain order
// (order == nullptr).
struct SegOrder {
  bitar_hip_ctx::OrderScratch* e = nullptr;
  std::unique_lock<std::mutex> held;
  void* transient = nullptr;  // a foreign stream's scratch (freed by release(), stream-ordered)
  hipStream_t tstream = nullptr;
  uint32_t* order = nullptr;  // null: plain order
  const uint32_t* keys = nullptr;  // the keys the sort read (null: none made, or csizes given)
  // order = argsort of the keys: keys[i] written by `key` (a launch), or -- csizes given --
  // the compressed sizes' key computed by the sort itself (decompress; seg: the segment size).
  // slot: which of the stream's cached scratch areas (a call holding two orders at once
  // uses slots 0 and 1).  The scratch is allocated once per stream and grown on demand, so
  // steady-state calls queue no allocation.
  // cut, slots: the priority lanes (order.hip.h: H = the segments with keys below `cut`, S =
  // slots): the fast lane's entries of the order carry kLaneTag, which only the LZ4 kernels
  // know; slots == 0 for every kernel without lanes.
  template <class F>
  void make(bitar_hip_ctx* ctx, hipStream_t s, uint32_t nseg, const uint32_t* csizes, F key,
            uint32_t seg = 0, int slot = 0, uint32_t cut = 0, uint32_t slots = 0) {
    if (!ctx->cost_order.load(std::memory_order_relaxed) || nseg < kOrderMinSegs) return;
    const uint32_t tile = bitar_hip::order_tile(nseg);
    const uint32_t ntiles = (nseg + tile - 1) / tile;
    const uint64_t need = 8ull * nseg + 4ull * bitar_hip::kOrderBins * ntiles + 64;
    bool own = s == nullptr;
    for (hipStream_t q : ctx->streams) own = own || q == s;
    if (!own) {
      // a foreign stream (e.g. a torch side stream): no cache entry, which would pin HBM for
      // the context's life and be inherited by a later stream reusing the handle -- the
      // scratch is allocated and freed in this stream's order by this call
      if (hipMallocAsync(&transient, need, s) != hipSuccess) {
        (void)hipGetLastError();
        transient = nullptr;
        return;
      }
      tstream = s;
    } else {
      {
        std::lock_guard<std::mutex> g(ctx->mu);
        for (auto& x : ctx->order_scratch)
          if (x.stream == s && x.slot == slot) e = &x;
        if (!e) e = &ctx->order_scratch.emplace_back(s, slot);
      }
      held = std::unique_lock<std::mutex>(e->m);
      if (e->cap < need) {
        if (e->p) (void)hipFreeAsync(e->p, s);
        e->p = nullptr;
        e->cap = 0;
        const uint64_t cap = (need + (1u << 20) - 1) & ~(uint64_t)((1u << 20) - 1);
        if (hipMallocAsync(&e->p, cap, s) != hipSuccess) {
          (void)hipGetLastError();
          e->p = nullptr;
          held.unlock();
          return;
        }
        e->cap = cap;
      }
    }
    order = static_cast<uint32_t*>(transient ? transient : e->p);
    uint32_t* const kbuf = csizes ? nullptr : order + nseg;
    keys = kbuf;
    auto* hist = reinterpret_cast<uint32_t*>(
        (reinterpret_cast<uintptr_t>(order + 2ull * nseg) + 15) & ~(uintptr_t)15);
    if (kbuf) key(kbuf);
    hipLaunchKernelGGL(bitar_hip::order_hist_kernel, dim3(ntiles), dim3(64), 0, s, kbuf, csizes,
                       seg, nseg, tile, hist);
    hipLaunchKernelGGL(bitar_hip::order_scatter_kernel, dim3(ntiles), dim3(64), 0, s, kbuf,
                       csizes, seg, nseg, tile, ntiles, hist, order, cut, slots);
  }
  // after the last launch that reads the order has been queued
  void release() {
    if (held.owns_lock()) held.unlock();
    if (transient) (void)hipFreeAsync(transient, tstream);
    transient = nullptr;
  }
  ~SegOrder() { release(); }
};

// the context's cached order scratch, freed at close (after its streams are idle)
static void free_order_scratch(bitar_hip_ctx* ctx) {
  std::lock_guard<std::mutex> g(ctx->mu);
  for (auto& x : ctx->order_scratch)
    if (x.p) (void)hipFree(x.p);
  ctx->order_scratch.clear();
}

// ---- compress: one function per format, dispatched by compress_impl ------------------------
// What every format's function takes (validated by compress_impl): segment i is min(seg, n -
// i * seg) bytes at in + i * seg, its slot slab + i * stride or dsts[i].  chunk(): the same for
// the segments [c0, c0 + most) of the call -- every per-segment pointer moved up by c0.
struct CompressArgs {
  const uint8_t* in;
  uint64_t n;
  uint32_t seg, nseg;  // nseg = ceil(n / seg)
  uint8_t* slab;
  uint64_t stride;
  uint8_t* const* dsts;
  uint32_t *sizes, *bits;  // bits: DEFLATE's bit lengths (bitar_hip_compress_bits), else null
  CompressArgs chunk(uint64_t c0, uint64_t most) const {
    const uint64_t cn = nseg - c0 < most ? nseg - c0 : most;
    const uint64_t cb = c0 * seg, nb = n - cb < cn * seg ? n - cb : cn * seg;
    return {in + cb, nb, seg, (uint32_t)cn, slab ? slab + c0 * stride : nullptr, stride,
            dsts ? dsts + c0 : nullptr, sizes + c0, bits ? bits + c0 : nullptr};
  }
};

// cost-ordered dispatch of the segments of a call or chunk: key = distinct byte values in a
// 128-byte sample of each segment (incompressible segments, which the parses skip through and
// whose stored form is a copy, show the most)
// (slots != 0: with the priority lanes' tags, heavy = keys below kCheapKey)
static void cost_order(bitar_hip_ctx* ctx, hipStream_t s, SegOrder& o, const CompressArgs& a,
                       uint32_t slots = 0) {
  o.make(ctx, s, a.nseg, nullptr, [&](uint32_t* keys) {
    hipLaunchKernelGGL(bitar_hip::seg_cost_kernel, dim3((a.nseg + 15) / 16), dim3(64), 0, s, a.in,
                       a.n, a.seg, a.nseg, keys);
  }, 0, 0, slots ? bitar_hip::kCheapKey : 0u, slots);
}

// Priority lanes (order.hip.h): the workgroups of `kernel` (one wave, no
// dynamic LDS) that the device holds at once, asked of the runtime once per context and
// kernel.  0 -- lanes compiled out, a call too small for an order, or the query failed --
// means no lanes: every workgroup runs at priority 0.
// Lanes are for a launch that has the device to itself.  Beside another queue pair's launch
// the tail is filled by that launch's waves anyway, and the lanes' priority competes with
// them (the four-stream record batch measured 0.7 % slower with lanes).  A
// context's queue-pair streams exist to run calls side by side, so a call on one of several
// is taken to have siblings and gets no lanes.  This is a convention, not a check of what the
// device is doing: concurrent calls on streams of the caller's own (torch streams, say) are
// not seen and get lanes, the configuration that measured slower.  (Asking the other streams
// with hipStreamQuery instead cost a synchronous call ~15 us of host time and would not see
// foreign streams either.)
static bool alone_by_convention(bitar_hip_ctx* ctx, hipStream_t s) {
  if (ctx->streams.size() < 2) return true;
  for (hipStream_t q : ctx->streams)
    if (q == s) return false;
  return true;
}
template <class K>
static uint32_t lane_slots(bitar_hip_ctx* ctx, hipStream_t s, K kernel, uint32_t nseg) {
  // (a probe build asks too: scripts/launch_timeline.py prints the answer)
  if ((!bitar_hip::kLanePrio && !BITAR_LAUNCH_TIMELINE) || nseg < kOrderMinSegs) return 0;
  if (nseg > bitar_hip::kLaneTag) return 0;  // (the tag is the segment index's top bit)
  if (!ctx->cost_order.load(std::memory_order_relaxed) || !alone_by_convention(ctx, s)) return 0;
  uint32_t v = ctx->lane_slots.load(std::memory_order_relaxed);
  if (!v) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    v = (uint32_t)(per_cu > 0 ? per_cu : 0) * ctx->cus;
    ctx->lane_slots.store(v, std::memory_order_relaxed);
  }
  return v;
}
#if BITAR_LAUNCH_TIMELINE
// probe builds: the slot count the context found for the fast compressor (0: not asked yet)
extern "C" __attribute__((visibility("default"))) uint32_t bitar_hip_timeline_slots(
    bitar_hip_ctx* ctx) {
  return ctx ? ctx->lane_slots.load(std::memory_order_relaxed) : 0u;
}
#endif

// A family's codec: one streaming kernel, the same work for every segment: plain order
// (intpack.hip, fltpack.hip, dictpack.hip, runpack.hip, cascade.hip, ransplane.hip,
// patchpack.hip, decpack.hip, and the byte codecs rans.hip and symtab.hip: one segment's histogram or table,
// and its coder, in one wave).  A segment never fails (the stored form fits every slot).
// AUTOPACK: the smallest of the candidates' streams per segment (autopack.hip): RUNPACK straight
// into the caller's slots, every later candidate that offers the width (kCandidates, kColumn)
// into a stream-ordered scratch slab of its own with its own sizes (store-less: a segment a
// later candidate would store gets its size only, and the select kernel never takes it), then
// the select kernel.  Chunks of <= kAutoChunkSegs segments over one allocation.
static int compress_column(hipStream_t s, ColumnCodec cc, const CompressArgs& a) {
  const uint32_t lg = cc.lg;
  if (cc.family != kAutoPack) {
    hipLaunchKernelGGL(compress_kernel<true>(cc.family, lg), dim3(a.nseg), dim3(64), 0, s, a.in,
                       a.n, a.seg, a.slab, a.stride, a.dsts, a.sizes);
    return 0;
  }
  uint32_t extra = 0;  // the candidates after the first
  for (ColumnFamily f : kCandidates) extra += offers(f, lg) ? 1u : 0u;
  --extra;
  const uint64_t scr_stride = bitar_hip_slot_size(kColumn[kAutoPack].base + lg, a.seg);
  const Chunks ch(a.nseg, kAutoChunkSegs);
  const bool lean = autopack_storeless();
  void* scratch = nullptr;
  HIP_TRY(hipMallocAsync(&scratch, extra * ch.size * (scr_stride + 4u), s), "scratch allocation");
  auto* scr = static_cast<uint8_t*>(scratch);
  auto* ssz = reinterpret_cast<uint32_t*>(scr + extra * ch.size * scr_stride);
  for (uint64_t c0 = 0; c0 < a.nseg; c0 += ch.size) {
    const CompressArgs c = a.chunk(c0, ch.size);
    const uint32_t cn = c.nseg;
    uint32_t k = 0;  // the next scratch candidate
    for (ColumnFamily f : kCandidates) {
      if (!offers(f, lg)) continue;
      if (f == kCandidates[0]) {
        hipLaunchKernelGGL(compress_kernel<true>(f, lg), dim3(cn), dim3(64), 0, s, c.in, c.n,
                           c.seg, c.slab, c.stride, c.dsts, c.sizes);
      } else {
        const CompressKernel kernel =
            lean ? compress_kernel<false>(f, lg) : compress_kernel<true>(f, lg);
        hipLaunchKernelGGL(kernel, dim3(cn), dim3(64), 0, s, c.in, c.n, c.seg,
                           scr + k * ch.size * scr_stride, scr_stride,
                           (uint8_t* const*)nullptr, ssz + k * ch.size);
        ++k;
      }
    }
    hipLaunchKernelGGL(bitar_hip::autopack_select_kernel, dim3((cn + 3) / 4), dim3(256), 0, s,
                       static_cast<const uint8_t*>(scr), scr_stride,
                       static_cast<const uint32_t*>(ssz), (uint32_t)ch.size, extra + 1u, cn,
                       c.slab, c.stride, c.dsts, c.sizes);
  }
  const hipError_t le = hipGetLastError();
  HIP_TRY(hipFreeAsync(scratch, s), "scratch release");
  HIP_TRY(le, "compress launch");
  return 0;
}

// LZ4 blocks from the fast parse (4 KiB ring) or the wide one (16 KiB)
static int compress_lz4(bitar_hip_ctx* ctx, hipStream_t s, bool wide, const CompressArgs& a) {
  const auto kernel = wide ? bitar_hip::lz4_compress_kernel<16384, 12>
                           : bitar_hip::lz4_compress_kernel<4096, 10>;
  SegOrder ord;
  // (lanes for the fast parse only: the wide parse's leg did not gain)
  cost_order(ctx, s, ord, a, wide ? 0u : lane_slots(ctx, s, kernel, a.nseg));
  hipLaunchKernelGGL(kernel, dim3(a.nseg), dim3(64), 0, s, a.in, a.n, a.seg, a.slab, a.stride,
                     a.dsts, a.sizes, err_word(ctx, s), ord.order);
  return 0;
}

// the LZ4 parse with the Snappy emitter (snappy.hip), dispatched as LZ4 is; a segment never
// fails (the stored form fits every slot), so the kernel takes no error word
static int compress_snappy(bitar_hip_ctx* ctx, hipStream_t s, const CompressArgs& a) {
  SegOrder ord;
  cost_order(ctx, s, ord, a);
  hipLaunchKernelGGL(bitar_hip::snappy_compress_kernel, dim3(a.nseg), dim3(64), 0, s, a.in, a.n,
                     a.seg, a.slab, a.stride, a.dsts, a.sizes, ord.order);
  return 0;
}

// fixed-Huffman DEFLATE (compress.hip)
static int compress_deflate(bitar_hip_ctx* ctx, hipStream_t s, const CompressArgs& a) {
  SegOrder ord;
  cost_order(ctx, s, ord, a);
  if (a.bits)  // (a kernel of its own: bitar_hip_compress keeps its code, compress.hip)
    hipLaunchKernelGGL(bitar_hip::deflate_compress_bits_kernel, dim3(a.nseg), dim3(64), 0, s, a.in,
                       a.n, a.seg, a.slab, a.stride, a.dsts, a.sizes, err_word(ctx, s), ord.order,
                       a.bits);
  else
    hipLaunchKernelGGL(bitar_hip::deflate_compress_kernel, dim3(a.nseg), dim3(64), 0, s, a.in, a.n,
                       a.seg, a.slab, a.stride, a.dsts, a.sizes, err_word(ctx, s), ord.order);
  return 0;
}

// pass 1 (parse -> records + histograms) and pass 2 (codes + emit) through a stream-ordered
// scratch per segment (deflate_dyn.hip): 2 KiB plan + the literal stream (<= seg bytes, 16-B
// aligned) + 8-byte match records (<= seg / 4: matches are >= 4 bytes); the per-window form
// (BITAR_DYN_BULK 0) needs 2 KiB + 16 KiB of window masks + 4-byte records, within the same
// stride.  Large calls run in chunks of <= kChunkSegs segments over one scratch allocation, so
// scratch is bounded whatever the call's size.
static int compress_deflate_dynamic(bitar_hip_ctx* ctx, hipStream_t s, const CompressArgs& a) {
  const uint32_t seg = a.seg;
  const uint64_t scr_old = bitar_hip_slot_size(BITAR_HIP_CODEC_DEFLATE, seg) + 2048u + 16384u;
  const uint64_t scr_bulk = 2048u + ((seg + 15u) & ~15ull) + 8u * ((uint64_t)seg / 4u + 64u);
  const uint64_t scr_stride = ((scr_old > scr_bulk ? scr_old : scr_bulk) + 15u) & ~15ull;
  const Chunks ch(a.nseg);
  void* scratch = nullptr;
  HIP_TRY(hipMallocAsync(&scratch, ch.size * scr_stride, s), "scratch allocation");
  auto* scr = static_cast<uint8_t*>(scratch);
  for (uint64_t c0 = 0; c0 < a.nseg; c0 += ch.size) {
    const CompressArgs c = a.chunk(c0, ch.size);
    const uint32_t cn = c.nseg;
    SegOrder ord;
    cost_order(ctx, s, ord, c);
    hipLaunchKernelGGL(bitar_hip::deflate_dyn_parse_kernel, dim3(cn), dim3(64), 0, s, c.in, c.n,
                       seg, scr, scr_stride, err_word(ctx, s), ord.order);
    hipLaunchKernelGGL(bitar_hip::deflate_dyn_emit_kernel, dim3(cn), dim3(64), 0, s, c.in, c.n,
                       seg, static_cast<const uint8_t*>(scr), scr_stride, c.slab, c.stride, c.dsts,
                       c.sizes, err_word(ctx, s), ord.order, c.bits);
  }
  const hipError_t le = hipGetLastError();
  HIP_TRY(hipFreeAsync(scratch, s), "scratch release");
  HIP_TRY(le, "compress launch");
  return 0;
}

// pass 1 (parse -> literals + sequence records) and pass 2 (entropy coding) through a
// stream-ordered scratch: per segment the literal area + records (zstd_compress.hip),
// then {nlit, nseq} per segment
static int compress_zstd(bitar_hip_ctx* ctx, hipStream_t s, const CompressArgs& a) {
  const uint32_t seg = a.seg;
  const uint64_t scr_stride = bitar_hip::zse::scratch_stride(seg);
  // + the chain-walk scratch (zstd_layout.hip.h: a 5000-byte header with the record, the
  // literal codes and the FSE tables, then 10 bytes per sequence and 12 per step of <= 64)
  const uint64_t w_stride = bitar_hip::zse::walk_stride(seg);
  const Chunks ch(a.nseg);
  void* scratch = nullptr;
  HIP_TRY(hipMallocAsync(&scratch, ch.size * (scr_stride + 8u + w_stride), s),
          "scratch allocation");
  auto* scr = static_cast<uint8_t*>(scratch);
  auto* meta = reinterpret_cast<uint2*>(scr + ch.size * scr_stride);
  auto* wscr = scr + ch.size * scr_stride + ch.size * 8u;
  for (uint64_t c0 = 0; c0 < a.nseg; c0 += ch.size) {
    const CompressArgs c = a.chunk(c0, ch.size);
    const uint32_t cn = c.nseg;
    SegOrder ord;
    cost_order(ctx, s, ord, c);
    hipLaunchKernelGGL(bitar_hip::zstd_parse_kernel, dim3(cn), dim3(64), 0, s, c.in, c.n, seg, scr,
                       scr_stride, meta, ord.order);
    hipLaunchKernelGGL(bitar_hip::zstd_entropy_kernel, dim3(cn), dim3(64), 0, s, c.in, c.n, seg,
                       scr, scr_stride, meta, wscr, w_stride, ord.order);
    SegOrder word;  // (the walk's order: sequence counts, most first)
    word.make(ctx, s, cn, nullptr, [&](uint32_t* keys) {
      hipLaunchKernelGGL(bitar_hip::walk_key_kernel, dim3((cn + 63) / 64), dim3(64), 0, s, meta,
                         cn, keys);
    }, 0, 1);
    hipLaunchKernelGGL(bitar_hip::zstd_walk_kernel, dim3((cn + 3) / 4), dim3(64), 0, s, scr,
                       scr_stride, seg, cn, wscr, w_stride, word.order);
    word.release();
    hipLaunchKernelGGL(bitar_hip::zstd_emit_kernel, dim3(cn), dim3(64), 0, s, c.in, c.n, seg, scr,
                       scr_stride, c.slab, c.stride, c.dsts, c.sizes, wscr, w_stride, ord.order);
  }
  const hipError_t le = hipGetLastError();
  HIP_TRY(hipFreeAsync(scratch, s), "scratch release");
  HIP_TRY(le, "compress launch");
  return 0;
}

static int compress_impl(bitar_hip_ctx* ctx, void* stream, uint32_t codec, const void* d_in,
                         uint64_t n, uint32_t seg, void* d_slab, uint64_t slot_stride,
                         void* const* d_dsts, uint32_t* d_sizes, uint32_t* d_bits = nullptr) {
  if (int r = enter(ctx)) return r;
  const Codec c = find_codec(codec);
  if (!c) return fail(BITAR_HIP_NOT_IMPLEMENTED, "unknown codec");
  if (seg == 0 || seg > kMaxSeg) return fail(BITAR_HIP_INVALID, "seg must be in [1, 65536]");
  if (n == 0) return 0;  // empty input -> no segments (reference device.cc:161-164)
  if (!d_in || (!d_slab && !d_dsts) || !d_sizes) return fail(BITAR_HIP_INVALID, "null buffer");
  if (slot_stride < bitar_hip_slot_size(codec, seg))
    return fail(BITAR_HIP_INVALID, "slot size below the worst-case bound");
  if (d_slab && (((uintptr_t)d_slab & 15u) != 0 || (slot_stride & 15u) != 0))
    return fail(BITAR_HIP_INVALID, "d_slab and slot_stride must be 16-B aligned");
  const uint64_t nseg = (n + seg - 1) / seg;
  if (nseg > 0x7FFFFFFFull) return fail(BITAR_HIP_INVALID, "too many segments");
  hipStream_t s = pick_stream(ctx, stream);
  const CompressArgs a{static_cast<const uint8_t*>(d_in), n, seg, (uint32_t)nseg,
                       static_cast<uint8_t*>(d_slab), slot_stride,
                       reinterpret_cast<uint8_t* const*>(d_dsts), d_sizes, d_bits};
  int r;
  if (c.column) r = compress_column(s, c.column, a);
  else switch (codec) {
    case BITAR_HIP_CODEC_LZ4: r = compress_lz4(ctx, s, false, a); break;
    case BITAR_HIP_CODEC_LZ4_WIDE: r = compress_lz4(ctx, s, true, a); break;
    case BITAR_HIP_CODEC_SNAPPY: r = compress_snappy(ctx, s, a); break;
    case BITAR_HIP_CODEC_DEFLATE: r = compress_deflate(ctx, s, a); break;
    case BITAR_HIP_CODEC_DEFLATE_DYNAMIC: r = compress_deflate_dynamic(ctx, s, a); break;
    default: r = compress_zstd(ctx, s, a); break;
  }
  if (r) return r;
  HIP_TRY(hipGetLastError(), "compress launch");
  return 0;
}
}  // extern "C++"

int bitar_hip_compress(bitar_hip_ctx* ctx, void* stream, uint32_t codec, const void* d_in,
                       uint64_t n, uint32_t seg, void* d_slab, uint64_t slot_stride,
                       uint32_t* d_sizes) {
  if (n && !d_slab) return fail(BITAR_HIP_INVALID, "null d_slab");
  return compress_impl(ctx, stream, codec, d_in, n, seg, d_slab, slot_stride, nullptr, d_sizes);
}

int bitar_hip_compress_scattered(bitar_hip_ctx* ctx, void* stream, uint32_t codec,
                                 const void* d_in, uint64_t n, uint32_t seg,
                                 void* const* d_dsts, uint64_t slot_capacity, uint32_t* d_sizes) {
  if (n && !d_dsts) return fail(BITAR_HIP_INVALID, "null d_dsts");
  return compress_impl(ctx, stream, codec, d_in, n, seg, nullptr, slot_capacity, d_dsts,
                       d_sizes);
}

int bitar_hip_compress_bits(bitar_hip_ctx* ctx, void* stream, uint32_t codec, const void* d_in,
                            uint64_t n, uint32_t seg, void* d_slab, uint64_t slot_stride,
                            uint32_t* d_sizes, uint32_t* d_bits) {
  if (codec != BITAR_HIP_CODEC_DEFLATE && codec != BITAR_HIP_CODEC_DEFLATE_DYNAMIC)
    return fail(BITAR_HIP_INVALID, "bit lengths exist for DEFLATE and DEFLATE_DYNAMIC only");
  if (n && !d_slab) return fail(BITAR_HIP_INVALID, "null d_slab");
  return compress_impl(ctx, stream, codec, d_in, n, seg, d_slab, slot_stride, nullptr, d_sizes,
                       d_bits);
}

// The dispatch order of a call, copied out for tests (tests/test_gpu_order.py): built by the
// code the codecs run -- SegOrder::make, through cost_order() for the compress key, with
// lane_slots() of the fast LZ4 compressor for BITAR_HIP_ORDER_SLOTS_CALL -- and read back in
// stream order before the scratch is released.  Nothing here launches the sort itself.
int bitar_hip_debug_order(bitar_hip_ctx* ctx, void* stream, uint32_t mode, const void* d_in,
                          uint64_t n, uint32_t seg, const uint32_t* d_values, uint32_t nseg,
                          uint32_t cut, uint32_t slots, uint32_t* d_order, uint32_t* d_keys,
                          uint32_t* slots_used) {
  if (int r = enter(ctx)) return r;
  if (slots_used) *slots_used = 0;
  if (mode > BITAR_HIP_ORDER_CALLER_KEYS) return fail(BITAR_HIP_INVALID, "unknown order mode");
  if (cut >= bitar_hip::kOrderBins) return fail(BITAR_HIP_INVALID, "cut must be below 256");
  if (nseg > bitar_hip::kLaneTag)
    return fail(BITAR_HIP_INVALID, "too many segments (the lane tag is the index's top bit)");
  if (!d_order) return fail(BITAR_HIP_INVALID, "null d_order");
  const bool compress = mode == BITAR_HIP_ORDER_COMPRESS_KEY;
  if (compress) {
    if (seg == 0 || seg > kMaxSeg) return fail(BITAR_HIP_INVALID, "seg must be in [1, 65536]");
    if (!d_in || !n) return fail(BITAR_HIP_INVALID, "null or empty input");
    if ((n + seg - 1) / seg != nseg) return fail(BITAR_HIP_INVALID, "nseg must be ceil(n / seg)");
  } else {
    if (!d_values) return fail(BITAR_HIP_INVALID, "null d_values");
    if (mode == BITAR_HIP_ORDER_DECOMPRESS_KEY && (seg == 0 || d_keys))
      return fail(BITAR_HIP_INVALID, "the decompress key needs seg and keeps no key array");
  }
  hipStream_t s = pick_stream(ctx, stream);
  if (slots == BITAR_HIP_ORDER_SLOTS_CALL)
    slots = lane_slots(ctx, s, bitar_hip::lz4_compress_kernel<4096, 10>, nseg);
  if (slots_used) *slots_used = slots;
  SegOrder ord;
  if (compress) {
    const CompressArgs a{static_cast<const uint8_t*>(d_in), n, seg, nseg, nullptr, 0, nullptr,
                         nullptr, nullptr};
    cost_order(ctx, s, ord, a, slots);  // (its cut: kCheapKey with slots, else 0)
  } else if (mode == BITAR_HIP_ORDER_DECOMPRESS_KEY) {
    ord.make(ctx, s, nseg, d_values, [](uint32_t*) {}, seg, 0, cut, slots);
  } else {
    ord.make(ctx, s, nseg, nullptr, [&](uint32_t* keys) {
      (void)hipMemcpyAsync(keys, d_values, 4ull * nseg, hipMemcpyDeviceToDevice, s);
    }, 0, 0, cut, slots);
  }
  if (!ord.order) return BITAR_HIP_NO_ORDER;
  HIP_TRY(hipMemcpyAsync(d_order, ord.order, 4ull * nseg, hipMemcpyDeviceToDevice, s),
          "copy of the order");
  if (d_keys)
    HIP_TRY(hipMemcpyAsync(d_keys, ord.keys, 4ull * nseg, hipMemcpyDeviceToDevice, s),
            "copy of the keys");
  HIP_TRY(hipGetLastError(), "order launch");
  return 0;
}

int bitar_hip_deflate_join(bitar_hip_ctx* ctx, void* stream, const void* d_slab,
                           uint64_t slot_stride, const uint32_t* d_sizes, const uint32_t* d_bits,
                           uint32_t nseg, uint64_t* d_starts, void* d_joined, uint64_t capacity) {
  if (int r = enter(ctx)) return r;
  if (!d_starts) return fail(BITAR_HIP_INVALID, "null d_starts");
  if (nseg > 0x7FFFFFFFu) return fail(BITAR_HIP_INVALID, "too many segments");
  // (whole dwords are stored and OR-ed: the last one must lie inside the capacity)
  if (d_joined && (((uintptr_t)d_joined & 3u) != 0 || (capacity & 3u) != 0))
    return fail(BITAR_HIP_INVALID, "d_joined must be 4-B aligned and capacity a multiple of 4");
  if (nseg) {
    if (!d_slab || !d_sizes || !d_bits) return fail(BITAR_HIP_INVALID, "null buffer");
    if (((uintptr_t)d_slab & 15u) != 0 || (slot_stride & 15u) != 0 || slot_stride == 0)
      return fail(BITAR_HIP_INVALID, "d_slab and slot_stride must be 16-B aligned");
  }
  hipStream_t s = pick_stream(ctx, stream);
  // the joined stream is OR-ed into zeros at its segments' shared dwords (deflate_join.hip)
  if (d_joined && capacity) HIP_TRY(hipMemsetAsync(d_joined, 0, capacity, s), "clear joined stream");
  if (nseg == 0) {
    HIP_TRY(hipMemsetAsync(d_starts, 0, sizeof(uint64_t), s), "clear starts");
    return 0;
  }
  const auto* slab = static_cast<const uint8_t*>(d_slab);
  hipLaunchKernelGGL(bitar_hip::join_scan_kernel, dim3(1), dim3(512), 0, s, slab, slot_stride,
                     d_sizes, d_bits, nseg, d_joined ? capacity : ~0ull, d_starts,
                     err_word(ctx, s));
  HIP_TRY(hipGetLastError(), "join scan launch");
  if (d_joined) {
    hipLaunchKernelGGL(bitar_hip::deflate_join_kernel, dim3(nseg), dim3(64), 0, s, slab,
                       slot_stride, d_sizes, d_bits, nseg, d_starts,
                       static_cast<uint32_t*>(d_joined), capacity);
    HIP_TRY(hipGetLastError(), "join launch");
  }
  return 0;
}

int bitar_hip_deflate_split(bitar_hip_ctx* ctx, void* stream, const void* d_joined,
                            uint64_t joined_len, const uint64_t* d_starts,
                            const uint32_t* d_entries, uint32_t nseg, void* d_slab,
                            uint64_t slot_stride, uint32_t* d_sizes) {
  if (int r = enter(ctx)) return r;
  if (nseg == 0) return 0;
  if (nseg > 0x7FFFFFFFu) return fail(BITAR_HIP_INVALID, "too many segments");
  if (!d_joined || !d_starts || !d_entries || !d_slab || !d_sizes)
    return fail(BITAR_HIP_INVALID, "null buffer");
  if (((uintptr_t)d_joined & 3u) != 0) return fail(BITAR_HIP_INVALID, "d_joined must be 4-B aligned");
  if (joined_len >> 60) return fail(BITAR_HIP_INVALID, "joined_len out of range");
  if (((uintptr_t)d_slab & 15u) != 0 || (slot_stride & 15u) != 0 || slot_stride == 0)
    return fail(BITAR_HIP_INVALID, "d_slab and slot_stride must be 16-B aligned");
  hipStream_t s = pick_stream(ctx, stream);
  hipLaunchKernelGGL(bitar_hip::deflate_split_kernel, dim3(nseg), dim3(64), 0, s,
                     static_cast<const uint8_t*>(d_joined), joined_len, d_starts, d_entries, nseg,
                     static_cast<uint8_t*>(d_slab), slot_stride, d_sizes, err_word(ctx, s));
  HIP_TRY(hipGetLastError(), "split launch");
  return 0;
}

int bitar_hip_crc32_combine(bitar_hip_ctx* ctx, void* stream, const uint64_t* d_sums, uint64_t n,
                            uint32_t seg, uint32_t nseg, uint32_t* d_crc) {
  if (int r = enter(ctx)) return r;
  if (seg == 0 || seg > kMaxSeg) return fail(BITAR_HIP_INVALID, "seg must be in [1, 65536]");
  if ((uint64_t)nseg != (n + seg - 1) / seg)
    return fail(BITAR_HIP_INVALID, "nseg must be ceil(n / seg)");
  if (!d_crc || (nseg && !d_sums)) return fail(BITAR_HIP_INVALID, "null buffer");
  hipStream_t s = pick_stream(ctx, stream);
  if (nseg == 0) {  // the CRC-32 of nothing
    HIP_TRY(hipMemsetAsync(d_crc, 0, sizeof(uint32_t), s), "clear crc");
    return 0;
  }
  hipLaunchKernelGGL(bitar_hip::crc32_combine_kernel, dim3(1), dim3(256), 0, s, d_sums, n, seg,
                     nseg, d_crc);
  HIP_TRY(hipGetLastError(), "crc combine launch");
  return 0;
}

int bitar_hip_pointer_info(const void* ptr, int* kind, int* device) {
  if (!kind || !device) return fail(BITAR_HIP_INVALID, "null argument");
  *kind = 0;
  *device = -1;
  if (!ptr) return 0;
  hipPointerAttribute_t a;
  hipError_t e = hipPointerGetAttributes(&a, ptr);
  if (e != hipSuccess) {  // unknown to HIP: ordinary pageable host memory
    (void)hipGetLastError();
    return 0;
  }
  if (a.type == hipMemoryTypeDevice) {
    *kind = 2;
    *device = a.device;
  } else if (a.type == hipMemoryTypeHost && a.devicePointer == ptr) {
    // pinned host memory the device reaches at the same address (hipHostMalloc, torch
    // pin_memory): kernels may read it in place.  Memory pinned by hipHostRegister can have
    // another device address; it is reported as pageable (kind 0), so callers stage it with a
    // copy (hipMemcpyDefault) instead of handing its host address to a kernel.
    *kind = 1;
    *device = a.device;
  }
  return 0;
}

// Decoder options: per context (bitar_hip_decoder_options).  The environment variables
// BITAR_HIP_INFLATE_LANES / BITAR_HIP_ZSTD_LANES / BITAR_HIP_ZSTD_SEQ (tuning runs) set the
// defaults a context starts from; cfg->flags override them at open.
static uint32_t zstd_lanes_from(long x) {
  return x <= 0 ? 0u : x >= 64 ? 64u : x >= 32 ? 32u : x >= 16 ? 16u : 8u;
}
static uint32_t inflate_lanes_from(long x) {
  return x <= 0 ? 0u : x >= 32 ? 32u : x >= 16 ? 16u : x >= 8 ? 8u : 4u;
}
static long env_long(const char* name, long dflt) {
  const char* e = std::getenv(name);
  return e ? std::strtol(e, nullptr, 10) : dflt;
}

// Zstd: zstd_hlit_kernel on a stream of its own, beside zstd_seqdec_kernel (both latency-bound
// with about one wave per SIMD, and independent: the sequences need no literal).  Per
// context: BITAR_HIP_FLAG_ZSTD_SERIAL (or BITAR_HIP_ZSTD_FORK=0) queues them one after the
// other; BITAR_HIP_ZSTD_FORK=2 (timing runs) puts phase A on the side stream instead.
static uint32_t zstd_fork_env() {
  static const uint32_t v = (uint32_t)env_long("BITAR_HIP_ZSTD_FORK", 1);
  return v > 2 ? 1u : v;
}

static void init_options(bitar_hip_ctx* ctx, uint32_t flags) {
  // The lane inflater in front of the wave inflater is off by default since the wave
  // inflater's batches take far matches (round 3): 1 GiB fixed-Huffman decode, wave alone vs
  // 4 lanes per wave in front: kind 1 11.6 / 14.1 ms, kind 2 12.4 / 17.6, kind 5 13.3 / 12.6,
  // kind 6 11.7 / 8.9 (the lanes win long-match data only; splitting segments between the
  // two by compression ratio was slower than either: the launches run one after the other).
  // Dynamic blocks always take the wave inflater.  inflate_lanes = 4 keeps the lane form.
  ctx->inflate_lanes = flags & BITAR_HIP_FLAG_INFLATE_WAVE_ONLY
                           ? 0u : inflate_lanes_from(env_long("BITAR_HIP_INFLATE_LANES", 0));
  ctx->zstd_lanes = flags & BITAR_HIP_FLAG_ZSTD_WAVE_ONLY
                        ? 0u : zstd_lanes_from(env_long("BITAR_HIP_ZSTD_LANES", 16));
  ctx->zstd_seq = flags & BITAR_HIP_FLAG_ZSTD_LANE_EXEC ? 0u : env_long("BITAR_HIP_ZSTD_SEQ", 1) != 0;
  ctx->zstd_fork = flags & BITAR_HIP_FLAG_ZSTD_SERIAL ? 0u : zstd_fork_env();
  ctx->count_paths = (flags & BITAR_HIP_FLAG_COUNT_PATHS) ? 1u : 0u;
  ctx->cost_order = (flags & BITAR_HIP_FLAG_PLAIN_ORDER) ? 0u : env_long("BITAR_HIP_COST_ORDER", 1) != 0;
}

// the counters' device pointer for a launch, null (= not counted) unless count_paths is on
static unsigned long long* stats_of(bitar_hip_ctx* ctx) {
  return ctx->count_paths.load(std::memory_order_relaxed) ? ctx->d_stats : nullptr;
}

extern "C" int bitar_hip_get_decoder_options(bitar_hip_ctx* ctx, bitar_hip_decoder_options* opt) {
  if (!ctx || !opt) return fail(BITAR_HIP_INVALID, "null argument");
  opt->inflate_lanes = ctx->inflate_lanes.load();
  opt->zstd_lanes = ctx->zstd_lanes.load();
  opt->zstd_seq = ctx->zstd_seq.load();
  opt->count_paths = ctx->count_paths.load();
  return 0;
}

extern "C" int bitar_hip_set_decoder_options(bitar_hip_ctx* ctx,
                                             const bitar_hip_decoder_options* opt) {
  if (!ctx || !opt) return fail(BITAR_HIP_INVALID, "null argument");
  ctx->inflate_lanes = inflate_lanes_from((long)opt->inflate_lanes);
  ctx->zstd_lanes = zstd_lanes_from((long)opt->zstd_lanes);
  ctx->zstd_seq = opt->zstd_seq ? 1u : 0u;
  ctx->count_paths = opt->count_paths ? 1u : 0u;
  return 0;
}

extern "C" int bitar_hip_path_counters(bitar_hip_ctx* ctx, uint64_t* out, uint32_t n) {
  if (int r = enter(ctx)) return r;
  if (!out && n) return fail(BITAR_HIP_INVALID, "null out");
  HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
  unsigned long long v[BITAR_HIP_PATH_COUNT];
  HIP_TRY(hipMemcpy(v, ctx->d_stats, sizeof(v), hipMemcpyDeviceToHost), "read path counters");
  HIP_TRY(hipMemset(ctx->d_stats, 0, sizeof(v)), "reset path counters");
  for (uint32_t k = 0; k < n && k < BITAR_HIP_PATH_COUNT; ++k) out[k] = v[k];
  return 0;
}

// segments per wave of zstd_hlit_kernel / zstd_handoff_kernel / zstd_seqdec_kernel (4 / 8 /
// 16): tuning knobs BITAR_HIP_HLIT_SEGS, BITAR_HIP_HANDOFF_LANES, BITAR_HIP_SEQDEC_SEGS, read once
// (decompress_zstd keeps them in function-local statics)
static uint32_t pow2_knob(const char* name) {
  const long x = env_long(name, 16);
  return x >= 16 ? 16u : x >= 8 ? 8u : 4u;
}
// (tuning knob: 1 puts the forked single-block literal kernel on the side stream after the
// multi-block one instead of on the caller's stream after phase A)
#ifndef BITAR_HLIT1_SIDE
#define BITAR_HLIT1_SIDE 0
#endif

// the stream paired with the caller's stream s in `list` (created on first use; null if that
// fails)
static hipStream_t side_stream_for(bitar_hip_ctx* ctx,
                                   std::vector<std::pair<hipStream_t, hipStream_t>>& list,
                                   hipStream_t s) {
  std::lock_guard<std::mutex> g(ctx->mu);
  for (auto& cs : list)
    if (cs.first == s) return cs.second;
  hipStream_t c = nullptr;
  if (hipStreamCreateWithFlags(&c, hipStreamNonBlocking) != hipSuccess) return nullptr;
  list.emplace_back(s, c);
  return c;
}
static int stream_after(hipStream_t b, hipStream_t a);

// ---- decompress: one function per format, dispatched by decompress_impl --------------------
extern "C++" {
// What every format's function takes (validated by decompress_impl): segment i is sizes[i]
// bytes at srcs[i] (or slab + i * stride) and decodes to out + i * seg, its length to
// produced[i].  chunk(): the same for the segments [c0, c0 + most) of the call.
struct DecompressArgs {
  const uint8_t* const* srcs;
  const uint8_t* slab;
  uint64_t stride;
  const uint32_t* sizes;
  uint32_t nseg, seg;
  uint8_t* out;
  uint32_t* produced;
  DecompressArgs chunk(uint64_t c0, uint64_t most) const {
    const uint32_t cn = (uint32_t)(nseg - c0 < most ? nseg - c0 : most);
    return {srcs ? srcs + c0 : nullptr, slab ? slab + c0 * stride : nullptr, stride, sizes + c0,
            cn, seg, out + c0 * seg, produced + c0};
  }
};

// A run-time lane count as a template argument: f(Width<W>{}) for the W of the list that n
// equals, or for the last of the list when n equals none.
template <uint32_t W>
using Width = std::integral_constant<uint32_t, W>;
template <uint32_t W, uint32_t... Rest, class F>
static void with_width(uint32_t n, F&& f) {
  if constexpr (sizeof...(Rest) > 0)
    if (n != W) return with_width<Rest...>(n, f);
  f(Width<W>{});
}

// A family's codec: its decoder over every segment, in plain order (a segment's work is its
// length whatever its coded size).
// AUTOPACK: each segment to the decoder its tag names (autopack.hip): the route kernel rejects the
// segments no format claims and sorts the others into one index list per format, with the
// counts, in a stream-ordered scratch; each format's listed decoder then runs over nseg
// workgroups of which the first count[f] take a segment.  No host round trip.
static int decompress_column(bitar_hip_ctx* ctx, hipStream_t s, ColumnCodec cc,
                             const DecompressArgs& a) {
  if (cc.family != kAutoPack) {
    hipLaunchKernelGGL(decompress_kernel<false>(cc.family, cc.lg), dim3(a.nseg), dim3(64), 0, s,
                       a.srcs, a.slab, a.stride, a.sizes, a.nseg, a.seg, a.out, a.produced,
                       err_word(ctx, s), (const uint32_t*)nullptr, (const uint32_t*)nullptr);
    return 0;
  }
  const bool lists = autopack_lists();
  const Chunks ch(a.nseg, kAutoDecChunkSegs);
  void* scratch = nullptr;
  if (lists) HIP_TRY(hipMallocAsync(&scratch, 16u * ch.size + 16u, s), "scratch allocation");
  auto* counts = static_cast<uint32_t*>(scratch);
  uint32_t* ew = err_word(ctx, s);
  hipError_t me = hipSuccess;
  for (uint64_t c0 = 0; c0 < a.nseg && me == hipSuccess; c0 += ch.size) {
    const DecompressArgs c = a.chunk(c0, ch.size);
    const uint32_t cn = c.nseg;
    uint32_t* cl = lists ? counts + 4 : nullptr;
    if (lists) me = hipMemsetAsync(counts, 0, 16, s);
    if (me != hipSuccess) break;
    hipLaunchKernelGGL(bitar_hip::autopack_route_kernel, dim3((cn + 255) / 256), dim3(256), 0, s,
                       c.srcs, c.slab, c.stride, c.sizes, cn, c.produced, ew, cl, counts);
    for (uint32_t f = 0; f < kListedDecoders; ++f)
      hipLaunchKernelGGL(decompress_kernel<true>(f, 0), dim3(cn), dim3(64), 0, s, c.srcs, c.slab,
                         c.stride, c.sizes, cn, c.seg, c.out, c.produced, ew,
                         lists ? cl + (uint64_t)f * cn : (const uint32_t*)nullptr,
                         lists ? counts + f : (const uint32_t*)nullptr);
  }
  const hipError_t le = hipGetLastError();
  if (scratch) HIP_TRY(hipFreeAsync(scratch, s), "scratch release");
  HIP_TRY(me, "clear counts");
  HIP_TRY(le, "decompress launch");
  return 0;
}

// near-history kernel over every segment, then the far-history kernel over the segments
// it deferred (lz4_decompress.hip)
// cost key: the coded size, largest first; incompressible segments (copies) last
static int decompress_lz4(bitar_hip_ctx* ctx, hipStream_t s, const DecompressArgs& a) {
  unsigned long long* const stats = stats_of(ctx);
  SegOrder ord;
  ord.make(ctx, s, a.nseg, a.sizes, [](uint32_t*) {}, a.seg);
  for (auto kernel : {bitar_hip::lz4_decompress_kernel<false>, bitar_hip::lz4_decompress_kernel<true>})
    hipLaunchKernelGGL(kernel, dim3(a.nseg), dim3(64), 0, s, a.srcs, a.slab, a.stride, a.sizes,
                       a.nseg, a.seg, a.out, a.produced, err_word(ctx, s), stats, ord.order);
  return 0;
}

// one kernel (snappy.hip): far history is read back from HBM inside it.  Cost key: the
// coded size, largest first; stored segments (one literal: copies) last
static int decompress_snappy(bitar_hip_ctx* ctx, hipStream_t s, const DecompressArgs& a) {
  SegOrder ord;
  ord.make(ctx, s, a.nseg, a.sizes, [](uint32_t*) {}, a.seg);
  hipLaunchKernelGGL(bitar_hip::snappy_decompress_kernel<false>, dim3(a.nseg), dim3(64), 0, s,
                     a.srcs, a.slab, a.stride, a.sizes, a.nseg, a.seg, a.out, a.produced,
                     err_word(ctx, s), ord.order);
  return 0;
}

// lane-per-segment decoder for stored / fixed-Huffman streams first; the wave decoder
// then takes the segments it deferred (inflate_lanes.hip).  fixed_hint: the caller's id was
// DEFLATE, not DEFLATE_DYNAMIC, which picks the inflater built for fixed-Huffman streams (9 /
// 8-bit fast tables, more waves per CU; any stream still decodes, inflate_fixed.hip)
static int decompress_deflate(bitar_hip_ctx* ctx, hipStream_t s, bool fixed_hint,
                              const DecompressArgs& a) {
  const uint32_t L = ctx->inflate_lanes.load(std::memory_order_relaxed);
  if (L)
    with_width<32, 16, 8, 4>(L, [&](auto lanes) {
      hipLaunchKernelGGL(bitar_hip::inflate_lanes_kernel<decltype(lanes)::value>,
                         dim3((a.nseg + L - 1) / L), dim3(64), 0, s, a.srcs, a.slab, a.stride,
                         a.sizes, a.nseg, a.seg, a.out, a.produced);
    });
  SegOrder ord;
  ord.make(ctx, s, a.nseg, a.sizes, [](uint32_t*) {}, a.seg);
  hipLaunchKernelGGL(fixed_hint ? bitar_hip::inflate_fixed_kernel : bitar_hip::inflate_kernel,
                     dim3(a.nseg), dim3(64), 0, s, a.srcs, a.slab, a.stride, a.sizes, a.nseg, a.seg,
                     a.out, a.produced, err_word(ctx, s), L ? 1u : 0u, stats_of(ctx), ord.order);
  return 0;
}

// lane-per-segment decoder first; the wave-per-segment decoder then takes the segments it
// deferred (zstd_lanes.hip)
static int decompress_zstd(bitar_hip_ctx* ctx, hipStream_t s, const DecompressArgs& a) {
  unsigned long long* const stats = stats_of(ctx);
  const uint32_t seg = a.seg;
  const uint32_t L = ctx->zstd_lanes.load(std::memory_order_relaxed);
  if (L)
    with_width<64, 32, 16, 8>(L, [&](auto lanes) {
      hipLaunchKernelGGL(bitar_hip::zstd_lanes_kernel<decltype(lanes)::value>,
                         dim3((a.nseg + L - 1) / L), dim3(64), 0, s, a.srcs, a.slab, a.stride,
                         a.sizes, a.nseg, seg, a.out, a.produced);
    });
  // The wave decoder hands the sequence sections of its frames' last blocks over through a
  // stream-ordered scratch (zstd_hand.hip.h: kStride bytes per segment); segments <= 64 KiB
  // then run FSE chains -> records (zstd_seqdec_kernel, rcap 8-byte records per segment)
  // -> output (zstd_exec_kernel), the rest the lane executor.  Both scratch buffers are
  // allocated before any kernel is queued, once, for a chunk of <= kChunkSegs segments.
  const Chunks ch(a.nseg);
  const bool seq = ctx->zstd_seq.load(std::memory_order_relaxed) && seg <= 65536;
  const uint32_t rcap = seg / 3 + 1;  // every valid frame (matches are >= 3 bytes)
  void* hscr = nullptr;
  void* recs = nullptr;
  HIP_TRY(hipMallocAsync(&hscr, ch.size * bitar_hip::zhand::kStride, s), "scratch allocation");
  if (seq) {
    const hipError_t e = hipMallocAsync(&recs, ch.size * rcap * 8, s);
    if (e != hipSuccess) {
      (void)hipFreeAsync(hscr, s);
      return hip_fail(e, "scratch allocation");
    }
  }
  uint8_t* hs = static_cast<uint8_t*>(hscr);
  auto* rp = static_cast<uint64_t*>(recs);
  uint32_t* ew = err_word(ctx, s);
  static const uint32_t hs_n = pow2_knob("BITAR_HIP_HLIT_SEGS"),
                        ho_n = pow2_knob("BITAR_HIP_HANDOFF_LANES"),
                        sd = pow2_knob("BITAR_HIP_SEQDEC_SEGS");
  for (uint64_t c0 = 0; c0 < a.nseg; c0 += ch.size) {
    const DecompressArgs c = a.chunk(c0, ch.size);
    const uint32_t cn = c.nseg;
    SegOrder ord;  // (cost key: the compressed size)
    ord.make(ctx, s, cn, c.sizes, [](uint32_t*) {}, seg);
    // (multi-block hand-offs -- every block of this engine's frames -- need the two-phase
    // sequence path; the lane executor takes last blocks only)
    hipLaunchKernelGGL(bitar_hip::zstd_decompress_kernel, dim3(cn), dim3(64), 0, s, c.srcs, c.slab,
                       c.stride, c.sizes, cn, seg, c.out, c.produced, ew, L ? 1u : 0u, hs, stats,
                       ord.order, seq ? 1u : 0u);
    // N segments per wave and B blocks per segment of the literal and the sequence kernels
    // (the multi-block kernels (B > 1) take units of 4 blocks: 2 cn of them)
    auto launch_hlit = [&](hipStream_t s, auto segs, auto blocks, const uint32_t* order) {
      constexpr uint32_t N = decltype(segs)::value, B = decltype(blocks)::value;
      hipLaunchKernelGGL((bitar_hip::zstd_hlit_kernel<N, B>),
                         dim3(((B > 1 ? 2 : 1) * cn + N - 1) / N), dim3(64), 0, s, c.srcs, c.slab,
                         c.stride, c.sizes, cn, seg, c.out, c.produced, hs, ew, order);
    };
    auto launch_seqdec = [&](hipStream_t s, auto segs, auto blocks, const uint32_t* order) {
      constexpr uint32_t N = decltype(segs)::value, B = decltype(blocks)::value;
      hipLaunchKernelGGL((bitar_hip::zstd_seqdec_kernel<N, B>),
                         dim3(((B > 1 ? 2 : 1) * cn + N - 1) / N), dim3(64), 0, s, c.srcs, c.slab,
                         c.stride, c.sizes, cn, seg, c.produced, hs, rp, rcap, ew, stats, order);
    };
    // the literal streams beside the sequences' phase A: one of the two on the aux stream
    // (zstd_fork 1: the literals there, launched first; 2: phase A there, first)
    // the multi-block lane kernels take their segments most expensive first (by sequences /
    // by literals: the column types of a record batch alternate in runs of segments, and
    // index order would give whole CUs the same kind of segment)
    SegOrder oseq, olit;
    if (seq) {
      oseq.make(ctx, s, 2 * cn, nullptr, [&](uint32_t* keys) {
        hipLaunchKernelGGL(bitar_hip::hand_key_kernel, dim3((2 * cn + 63) / 64), dim3(64), 0, s,
                           c.produced, hs, cn, 0u, keys);
      }, 0, 1);
      olit.make(ctx, s, 2 * cn, nullptr, [&](uint32_t* keys) {
        hipLaunchKernelGGL(bitar_hip::hand_key_kernel, dim3((2 * cn + 63) / 64), dim3(64), 0, s,
                           c.produced, hs, cn, 1u, keys);
      }, 0, 2);
    }
    const uint32_t fork = seq ? ctx->zstd_fork.load(std::memory_order_relaxed) : 0u;
    hipStream_t aux = fork ? side_stream_for(ctx, ctx->aux_streams, s) : nullptr;
    if (aux && stream_after(aux, s)) aux = nullptr;
    // single-block hand-offs (16 segments x 4 streams / chains per wave) and, with the
    // two-phase path, the multi-block ones (4 segments x 4 blocks x 4 per wave).  Forked
    // (fork 1), the single-block literal kernel goes on the caller's stream after phase A:
    // ahead of the multi-block literals on the side stream, its 36 KiB workgroups -- which
    // exit at once on this engine's multi-block frames -- waited for CU room behind phase A,
    // and the multi-block literals behind them (1 GiB kind 2: 1.3 ms on the call's path).
    const bool split = aux && fork == 1;
    auto hlit1 = [&](hipStream_t s) {
      with_width<4, 8, 16>(hs_n, [&](auto segs) { launch_hlit(s, segs, Width<1>{}, nullptr); });
    };
    auto hlit = [&](hipStream_t s) {
      if (!split) hlit1(s);
      if (seq) launch_hlit(s, Width<4>{}, Width<4>{}, olit.order);
      if (split && BITAR_HLIT1_SIDE) hlit1(s);
    };
    auto seqdec = [&](hipStream_t s) {
      with_width<4, 8, 16>(sd, [&](auto segs) { launch_seqdec(s, segs, Width<1>{}, nullptr); });
      launch_seqdec(s, Width<4>{}, Width<4>{}, oseq.order);
    };
    if (aux && fork == 2) {
      seqdec(aux);
      hlit(s);
    } else {
      hlit(aux ? aux : s);
      if (seq) seqdec(s);
      if (split && !BITAR_HLIT1_SIDE) hlit1(s);
    }
    if (seq) {
      if (aux && stream_after(s, aux)) (void)hipStreamSynchronize(aux);  // (join failed: wait here)
      hipLaunchKernelGGL(bitar_hip::zstd_exec_kernel, dim3(cn), dim3(64), 0, s, c.srcs, c.slab,
                         c.stride, cn, seg, c.out, c.produced, hs, rp, rcap, ew, stats, ord.order);
    }
    ord.release();
    oseq.release();
    olit.release();
    with_width<4, 8, 16>(ho_n, [&](auto lanes) {
      constexpr uint32_t N = decltype(lanes)::value;
      hipLaunchKernelGGL(bitar_hip::zstd_handoff_kernel<N>, dim3((cn + N - 1) / N), dim3(64), 0, s,
                         c.srcs, c.slab, c.stride, c.sizes, cn, seg, c.out, c.produced, hs, ew);
    });
  }
  const hipError_t le = hipGetLastError();
  if (recs) (void)hipFreeAsync(recs, s);
  HIP_TRY(hipFreeAsync(hscr, s), "scratch release");
  HIP_TRY(le, "decompress launch");
  return 0;
}

static int decompress_impl(bitar_hip_ctx* ctx, void* stream, uint32_t codec,
                           const void* const* d_srcs, const void* d_slab, uint64_t stride,
                           const uint32_t* d_sizes, uint32_t nseg, uint32_t seg, void* d_out,
                           uint64_t capacity, uint32_t* d_produced) {
  if (int r = enter(ctx)) return r;
  // (DEFLATE_DYNAMIC and LZ4_WIDE decode as DEFLATE and LZ4; a column codec's width is in each
  // stream's tag, and under AUTOPACK the format too)
  const Codec c = find_codec(codec);
  if (!c) return fail(BITAR_HIP_NOT_IMPLEMENTED, "unknown codec");
  if (nseg == 0) return 0;  // reference device.cc:244-246
  // Zstd: a segment may be a whole stock frame of up to kMaxZstdFrame bytes (the wave
  // decoder reads far history from HBM; the Arrow adapter decodes stock IPC bodies so)
  const uint32_t max_seg = c.format == BITAR_HIP_CODEC_ZSTD ? kMaxZstdFrame : kMaxSeg;
  if (seg == 0 || seg > max_seg)
    return fail(BITAR_HIP_INVALID, "seg must be in [1, " + std::to_string(max_seg) + "]");
  if (capacity < (uint64_t)nseg * seg)  // reference device.cc:248-254
    return fail(BITAR_HIP_CAPACITY_ERROR,
                "The decompressed_buffer is required to be >= " +
                    std::to_string((uint64_t)nseg * seg) + " bytes");
  if (!d_sizes || !d_out || !d_produced || (!d_srcs && !d_slab))
    return fail(BITAR_HIP_INVALID, "null buffer");
  if (nseg > 0x7FFFFFFFu) return fail(BITAR_HIP_INVALID, "too many segments");
  hipStream_t s = pick_stream(ctx, stream);
  const DecompressArgs a{reinterpret_cast<const uint8_t* const*>(d_srcs),
                         static_cast<const uint8_t*>(d_slab), stride, d_sizes, nseg, seg,
                         static_cast<uint8_t*>(d_out), d_produced};
  int r;
  if (c.column) r = decompress_column(ctx, s, c.column, a);
  else switch (c.format) {
    case BITAR_HIP_CODEC_LZ4: r = decompress_lz4(ctx, s, a); break;
    case BITAR_HIP_CODEC_SNAPPY: r = decompress_snappy(ctx, s, a); break;
    // (the caller's FIXED hint: DEFLATE itself, not the DEFLATE_DYNAMIC that decodes as it)
    case BITAR_HIP_CODEC_DEFLATE: r = decompress_deflate(ctx, s, codec == c.format, a); break;
    default: r = decompress_zstd(ctx, s, a); break;
  }
  if (r) return r;
  HIP_TRY(hipGetLastError(), "decompress launch");
  return 0;
}
}  // extern "C++"

int bitar_hip_decompress(bitar_hip_ctx* ctx, void* stream, uint32_t codec,
                         const void* const* d_srcs, const uint32_t* d_sizes, uint32_t nseg,
                         uint32_t seg, void* d_out, uint64_t capacity, uint32_t* d_produced) {
  if (nseg && !d_srcs) return fail(BITAR_HIP_INVALID, "null d_srcs");
  return decompress_impl(ctx, stream, codec, d_srcs, nullptr, 0, d_sizes, nseg, seg, d_out,
                         capacity, d_produced);
}

int bitar_hip_decompress_slab(bitar_hip_ctx* ctx, void* stream, uint32_t codec,
                              const void* d_slab, uint64_t slot_stride,
                              const uint32_t* d_sizes, uint32_t nseg, uint32_t seg,
                              void* d_out, uint64_t capacity, uint32_t* d_produced) {
  if (nseg && !d_slab) return fail(BITAR_HIP_INVALID, "null d_slab");
  return decompress_impl(ctx, stream, codec, nullptr, d_slab, slot_stride, d_sizes, nseg, seg,
                         d_out, capacity, d_produced);
}

// ---- host-memory calls: the PCIe link and the kernels overlapped ---------------------------
// The caller's stream s and a copy stream paired with it: the copy stream first waits for
// everything queued on s (the staging area may still be read by an earlier call), then per
// chunk of whole segments one copy + one event, and s waits on each chunk's event before the
// chunk's kernels (compress) -- or the copy stream waits on the chunk's decode before copying
// it out (decompress).  s finally waits on the copy stream, so a sync of s covers the call.
static hipStream_t copy_stream_for(bitar_hip_ctx* ctx, hipStream_t s) {
  return side_stream_for(ctx, ctx->copy_streams, s);
}

// b waits for what is queued on a now
static int stream_after(hipStream_t b, hipStream_t a) {
  hipEvent_t e;
  HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
  hipError_t r = hipEventRecord(e, a);
  if (r == hipSuccess) r = hipStreamWaitEvent(b, e, 0);
  (void)hipEventDestroy(e);  // (released once recorded work completes)
  HIP_TRY(r, "stream ordering");
  return 0;
}

// chunks of whole segments: about 1/8 of the call, at least 32 MiB
static uint64_t host_chunk_segs(uint64_t nseg, uint32_t seg) {
  uint64_t c = (nseg + 7) / 8;
  const uint64_t lo = ((32ull << 20) + seg - 1) / seg;
  return c < lo ? lo : c;
}

int bitar_hip_compress_host(bitar_hip_ctx* ctx, void* stream, uint32_t codec, const void* h_in,
                            uint64_t n, uint32_t seg, void* d_stage, void* d_slab,
                            void* const* d_dsts, uint64_t slot_stride, uint32_t* d_sizes) {
  if (int r = enter(ctx)) return r;
  if (n == 0) return 0;
  if (!h_in || !d_stage || (!d_slab && !d_dsts) || !d_sizes)
    return fail(BITAR_HIP_INVALID, "null buffer");
  if (seg == 0 || seg > kMaxSeg) return fail(BITAR_HIP_INVALID, "seg must be in [1, 65536]");
  const hipStream_t s = pick_stream(ctx, stream);
  const hipStream_t c = copy_stream_for(ctx, s);
  if (!c) return fail(BITAR_HIP_UNKNOWN_ERROR, "copy stream");
  if (int r = stream_after(c, s)) return r;
  const uint64_t nseg = (n + seg - 1) / seg, per = host_chunk_segs(nseg, seg);
  auto* stage = static_cast<uint8_t*>(d_stage);
  const auto* src = static_cast<const uint8_t*>(h_in);
  auto* slab = static_cast<uint8_t*>(d_slab);
  for (uint64_t c0 = 0; c0 < nseg; c0 += per) {
    const uint64_t cn = nseg - c0 < per ? nseg - c0 : per;
    const uint64_t off = c0 * seg, nb = n - off < cn * seg ? n - off : cn * seg;
    HIP_TRY(hipMemcpyAsync(stage + off, src + off, nb, hipMemcpyDefault, c), "stage input");
    if (int r = stream_after(s, c)) return r;
    if (int r = compress_impl(ctx, s, codec, stage + off, nb, seg,
                              slab ? slab + c0 * slot_stride : nullptr, slot_stride,
                              d_dsts ? d_dsts + c0 : nullptr, d_sizes + c0))
      return r;
  }
  return 0;
}

int bitar_hip_decompress_host(bitar_hip_ctx* ctx, void* stream, uint32_t codec,
                              const void* const* d_srcs, const uint32_t* d_sizes, uint32_t nseg,
                              uint32_t seg, void* d_stage, void* h_out, uint64_t capacity,
                              uint32_t* d_produced) {
  if (int r = enter(ctx)) return r;
  if (nseg == 0) return 0;
  if (capacity < (uint64_t)nseg * seg)  // reference device.cc:248-254
    return fail(BITAR_HIP_CAPACITY_ERROR, "The decompressed_buffer is required to be >= " +
                                              std::to_string((uint64_t)nseg * seg) + " bytes");
  if (!d_srcs || !d_sizes || !d_stage || !h_out || !d_produced)
    return fail(BITAR_HIP_INVALID, "null buffer");
  if (seg == 0 || seg > kMaxSeg) return fail(BITAR_HIP_INVALID, "seg must be in [1, 65536]");
  const hipStream_t s = pick_stream(ctx, stream);
  const hipStream_t c = copy_stream_for(ctx, s);
  if (!c) return fail(BITAR_HIP_UNKNOWN_ERROR, "copy stream");
  if (int r = stream_after(c, s)) return r;  // (h_out / d_stage users queued before)
  const uint64_t per = host_chunk_segs(nseg, seg);
  auto* stage = static_cast<uint8_t*>(d_stage);
  auto* out = static_cast<uint8_t*>(h_out);
  for (uint64_t c0 = 0; c0 < nseg; c0 += per) {
    const uint64_t cn = nseg - c0 < per ? nseg - c0 : per;
    if (int r = decompress_impl(ctx, s, codec, d_srcs + c0, nullptr, 0, d_sizes + c0,
                                (uint32_t)cn, seg, stage + c0 * seg, cn * seg, d_produced + c0))
      return r;
    if (int r = stream_after(c, s)) return r;
    HIP_TRY(hipMemcpyAsync(out + c0 * seg, stage + c0 * seg, cn * seg, hipMemcpyDefault, c),
            "output copy");
  }
  return stream_after(s, c);
}

int bitar_hip_sync(bitar_hip_ctx* ctx, void* stream) {
  if (int r = enter(ctx)) return r;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (s) {
    // this stream's word only: read and clear it in stream order, so work queued on other
    // streams (other queue pairs) can neither be reported here nor lose its error
    uint32_t* w = err_word(ctx, s);
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, w, sizeof(err), hipMemcpyDeviceToHost, s), "read error word");
    HIP_TRY(hipMemsetAsync(w, 0, sizeof(err), s), "clear error word");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
    return sync_error(err);
  }
  // NULL: the default stream and this context's queue pairs (not other contexts' or other
  // libraries' streams).  Only their words (0 = the default stream, 1..num_streams) are read
  // and cleared: a foreign stream's word belongs to a sync of that stream, since work still
  // running there could set it after this read and lose its error at the clear.
  HIP_TRY(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
  for (hipStream_t q : ctx->streams) HIP_TRY(hipStreamSynchronize(q), "hipStreamSynchronize");
  const size_t nw = ctx->streams.size() + 1;
  std::vector<uint32_t> words(nw);
  HIP_TRY(hipMemcpy(words.data(), ctx->d_err, nw * sizeof(uint32_t), hipMemcpyDeviceToHost),
          "read error words");
  uint32_t err = 0;
  for (uint32_t x : words) err |= x;
  if (err) HIP_TRY(hipMemset(ctx->d_err, 0, nw * sizeof(uint32_t)), "clear error words");
  return sync_error(err);
}

int bitar_hip_pack(bitar_hip_ctx* ctx, void* stream, const void* d_slab, uint64_t slot_stride,
                   const uint32_t* d_sizes, uint32_t nseg, uint64_t* d_offsets, void* d_frame) {
  if (int r = enter(ctx)) return r;
  if (!d_sizes || !d_offsets) return fail(BITAR_HIP_INVALID, "null buffer");
  if (d_frame && nseg && (!d_slab || slot_stride == 0))
    return fail(BITAR_HIP_INVALID, "null slab or zero slot stride");
  hipStream_t s = pick_stream(ctx, stream);
  // sizes above the slot stride (a failed op's SEGMENT_ERROR) pack as 0 bytes and flag the
  // stream's error word, so the next sync reports IOError instead of copying out of bounds
  const uint64_t limit = slot_stride ? slot_stride : (uint64_t)BITAR_HIP_SEGMENT_ERROR - 1;
  hipLaunchKernelGGL(bitar_hip::scan_sizes_kernel, dim3(1), dim3(1024), 0, s, d_sizes, nseg,
                     limit, d_offsets, err_word(ctx, s));
  HIP_TRY(hipGetLastError(), "scan launch");
  if (d_frame && nseg) {
    hipLaunchKernelGGL(bitar_hip::pack_kernel, dim3(nseg), dim3(64), 0, s,
                       static_cast<const uint8_t*>(d_slab), slot_stride, d_sizes, d_offsets,
                       nseg, static_cast<uint8_t*>(d_frame));
    HIP_TRY(hipGetLastError(), "pack launch");
  }
  return 0;
}

// ---- whole-buffer raw Snappy streams (snappy.hip) ----
constexpr uint32_t kSnappyBlock = 65536;   // a stream decodes as fragments of this many bytes
constexpr uint32_t kSnappyTile = 4096;     // bytes of the stream per tile walk (BITAR_SNAPPY_TILE)
constexpr uint32_t kSnappyRounds = 64;     // default bound of scan rounds
constexpr uint32_t kSnappyRoundGrid = 2048;  // workgroups of a round after the first
// positions in the stream are 32-bit in the scan's records, and a tile's output count (its
// literals, inside the stream, and <= 64 bytes per 2-byte copy) must fit 32 bits as well
constexpr uint64_t kSnappyMaxStream = 0xFFF00000ull;

int bitar_hip_snappy_join(bitar_hip_ctx* ctx, void* stream, const void* d_slab,
                          uint64_t slot_stride, const uint32_t* d_sizes, uint64_t n, uint32_t seg,
                          uint64_t* d_offsets, void* d_joined, uint64_t capacity,
                          uint64_t* d_joined_len) {
  if (int r = enter(ctx)) return r;
  if (seg != kSnappyBlock)
    return fail(BITAR_HIP_INVALID, "a joined Snappy stream is made of 65536-byte segments");
  if (n > 0xFFFFFFFFull) return fail(BITAR_HIP_INVALID, "a Snappy preamble holds 32 bits");
  const uint32_t nseg = (uint32_t)((n + kSnappyBlock - 1) / kSnappyBlock);
  if (!d_offsets || (nseg && (!d_sizes || (d_joined && !d_slab))))
    return fail(BITAR_HIP_INVALID, "null buffer");
  if (nseg && d_joined && slot_stride < bitar_hip_slot_size(BITAR_HIP_CODEC_SNAPPY, seg))
    return fail(BITAR_HIP_INVALID, "slot stride below the Snappy slot size");
  hipStream_t s = pick_stream(ctx, stream);
  void* body = nullptr;
  HIP_TRY(hipMallocAsync(&body, 4ull * nseg + 16, s), "scratch allocation");
  auto* d_body = static_cast<uint32_t*>(body);
  if (nseg)
    hipLaunchKernelGGL(bitar_hip::snappy_join_sizes_kernel, dim3((nseg + 255) / 256), dim3(256), 0,
                       s, d_sizes, nseg, n, d_body);
  hipLaunchKernelGGL(bitar_hip::scan_sizes_kernel, dim3(1), dim3(1024), 0, s, d_body, nseg,
                     (uint64_t)kSnappyBlock + 6, d_offsets, err_word(ctx, s));
  hipLaunchKernelGGL(bitar_hip::snappy_join_kernel, dim3(nseg + 1), dim3(64), 0, s,
                     static_cast<const uint8_t*>(d_slab), slot_stride, d_body, d_offsets, nseg, n,
                     static_cast<uint8_t*>(d_joined), capacity, d_joined_len, err_word(ctx, s));
  const hipError_t le = hipGetLastError();
  HIP_TRY(hipFreeAsync(body, s), "scratch release");
  HIP_TRY(le, "join launch");
  return 0;
}

int bitar_hip_snappy_split(bitar_hip_ctx* ctx, void* stream, const void* d_joined, uint64_t len,
                           uint64_t n, uint32_t max_rounds, uint64_t* d_starts,
                           uint32_t* d_status, uint32_t* d_stats) {
  if (int r = enter(ctx)) return r;
  if (!d_joined || !d_starts || !d_status) return fail(BITAR_HIP_INVALID, "null buffer");
  if (len > kSnappyMaxStream)
    return fail(BITAR_HIP_NOT_IMPLEMENTED, "Snappy streams above 4293918720 bytes");
  if (n > 0xFFFFFFFFull) return fail(BITAR_HIP_INVALID, "a Snappy preamble holds 32 bits");
  const uint64_t nfrag = (n + kSnappyBlock - 1) / kSnappyBlock;
  const bool serial = !(max_rounds & BITAR_HIP_SNAPPY_NO_SERIAL_FINISH);
  uint32_t rounds = max_rounds & ~BITAR_HIP_SNAPPY_NO_SERIAL_FINISH;
  if (rounds == 0) rounds = kSnappyRounds;
  if (rounds > 4096) return fail(BITAR_HIP_INVALID, "max_rounds above 4096");
  const uint32_t ntile = len ? (uint32_t)((len + kSnappyTile - 1) / kSnappyTile) : 1u;
  // an element gives at most 64 bytes for 3 of the stream's: more cannot be a stream's length
  const uint32_t hopeless = n > 64 * len ? 1u : 0u;
  hipStream_t s = pick_stream(ctx, stream);
  const auto* src = static_cast<const uint8_t*>(d_joined);
  const uint32_t len32 = (uint32_t)len;
  // scratch: control words; per tile a record, a chain position, a dirty entry, round 1's result
  void* scratch = nullptr;
  HIP_TRY(hipMallocAsync(&scratch, 64 + 48ull * ntile, s), "scratch allocation");
  auto* ctl = static_cast<uint32_t*>(scratch);
  auto* rec = reinterpret_cast<uint4*>(static_cast<uint8_t*>(scratch) + 64);
  uint4* cur = rec + ntile;
  auto* list = reinterpret_cast<uint2*>(cur + ntile);
  uint2* guess = list + ntile;
  const uint64_t fill = (nfrag + 256) / 256;
  hipLaunchKernelGGL(bitar_hip::snappy_scan_init_kernel, dim3((uint32_t)(fill < 1024 ? fill : 1024)),
                     dim3(256), 0, s, src, len32, nfrag, d_starts, ctl, cur, d_status, hopeless);
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t grid = r == 0 || ntile < kSnappyRoundGrid ? ntile : kSnappyRoundGrid;
    hipLaunchKernelGGL(bitar_hip::snappy_scan_walk_kernel, dim3(grid), dim3(64), 0, s, src, len32,
                       ntile, ctl, rec, guess, r == 0 ? (const uint2*)nullptr : list);
    hipLaunchKernelGGL(bitar_hip::snappy_scan_resolve_kernel, dim3(1), dim3(64), 0, s, src, len32,
                       n, nfrag, ntile, ctl, rec, guess, cur, list, d_starts, d_status);
  }
  hipLaunchKernelGGL(bitar_hip::snappy_scan_serial_kernel, dim3(1), dim3(64), 0, s, src, len32, n,
                     nfrag, ntile, ctl, cur, d_starts, d_status, serial ? 1u : 0u);
  hipLaunchKernelGGL(bitar_hip::snappy_scan_finish_kernel, dim3(ntile), dim3(64), 0, s, src, len32,
                     n, ntile, ctl, rec, cur, d_starts, d_status);
  hipError_t le = hipGetLastError();
  // rounds run, tile walks, tiles, 1 if the serial finish ran (the control words' order)
  if (le == hipSuccess && d_stats) {
    le = hipMemcpyAsync(d_stats, ctl + 3, 8, hipMemcpyDeviceToDevice, s);
    if (le == hipSuccess) le = hipMemcpyAsync(d_stats + 3, ctl + 7, 4, hipMemcpyDeviceToDevice, s);
    if (le == hipSuccess) le = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_stats + 2), (int)ntile, 1, s);
  }
  HIP_TRY(hipFreeAsync(scratch, s), "scratch release");
  HIP_TRY(le, "scan launch");
  return 0;
}

int bitar_hip_snappy_decompress_joined(bitar_hip_ctx* ctx, void* stream, const void* d_joined,
                                       uint64_t len, uint64_t n, const uint64_t* d_starts,
                                       void* d_out, uint64_t capacity, uint32_t* d_produced) {
  if (int r = enter(ctx)) return r;
  if (n == 0) return 0;
  if (len > kSnappyMaxStream)
    return fail(BITAR_HIP_NOT_IMPLEMENTED, "Snappy streams above 4293918720 bytes");
  if (n > 0xFFFFFFFFull) return fail(BITAR_HIP_INVALID, "a Snappy preamble holds 32 bits");
  if (capacity < n)
    return fail(BITAR_HIP_CAPACITY_ERROR, "The decompressed_buffer is required to be >= " +
                                              std::to_string(n) + " bytes");
  if (!d_joined || !d_starts || !d_out || !d_produced) return fail(BITAR_HIP_INVALID, "null buffer");
  const uint32_t nfrag = (uint32_t)((n + kSnappyBlock - 1) / kSnappyBlock);
  hipStream_t s = pick_stream(ctx, stream);
  // cost key: the fragment's coded size, as the slab decode's
  SegOrder ord;
  ord.make(
      ctx, s, nfrag, nullptr,
      [&](uint32_t* keys) {
        hipLaunchKernelGGL(bitar_hip::snappy_joined_key_kernel, dim3((nfrag + 255) / 256),
                           dim3(256), 0, s, d_starts, nfrag, keys);
      },
      kSnappyBlock);
  hipLaunchKernelGGL(bitar_hip::snappy_decompress_kernel<true>, dim3(nfrag), dim3(64), 0, s,
                     reinterpret_cast<const uint8_t* const*>(d_starts),
                     static_cast<const uint8_t*>(d_joined), n, (const uint32_t*)nullptr, nfrag,
                     (uint32_t)len, static_cast<uint8_t*>(d_out), d_produced, err_word(ctx, s),
                     ord.order);
  ord.release();
  HIP_TRY(hipGetLastError(), "decompress launch");
  return 0;
}

int bitar_hip_lz4_chain(bitar_hip_ctx* ctx, void* stream, const void* d_src, uint32_t src_len,
                        const uint32_t* d_blocks, uint32_t nblocks, void* d_out,
                        uint64_t capacity, uint32_t* d_produced) {
  if (int r = enter(ctx)) return r;
  if (!d_src || !d_blocks || !d_out || !d_produced) return fail(BITAR_HIP_INVALID, "null buffer");
  if (capacity > 0xFFFFFFFFull) capacity = 0xFFFFFFFFull;
  hipStream_t s = pick_stream(ctx, stream);
  hipLaunchKernelGGL(bitar_hip::lz4_chain_kernel, dim3(1), dim3(64), 0, s,
                     static_cast<const uint8_t*>(d_src), src_len, d_blocks, nblocks,
                     static_cast<uint8_t*>(d_out), (uint32_t)capacity, d_produced,
                     err_word(ctx, s));
  HIP_TRY(hipGetLastError(), "lz4 chain launch");
  return 0;
}

int bitar_hip_copy_batch(bitar_hip_ctx* ctx, void* stream, const void* const* d_srcs,
                         void* const* d_dsts, const uint32_t* d_sizes, uint32_t n) {
  if (int r = enter(ctx)) return r;
  if (n == 0) return 0;
  if (!d_srcs || !d_dsts || !d_sizes) return fail(BITAR_HIP_INVALID, "null buffer");
  hipStream_t s = pick_stream(ctx, stream);
  hipLaunchKernelGGL(bitar_hip::copy_batch_kernel, dim3(n), dim3(64), 0, s,
                     reinterpret_cast<const uint8_t* const*>(d_srcs),
                     reinterpret_cast<uint8_t* const*>(d_dsts), d_sizes, n);
  HIP_TRY(hipGetLastError(), "copy batch launch");
  return 0;
}

int bitar_hip_pack_lz4f(bitar_hip_ctx* ctx, void* stream, const void* d_in, uint64_t n,
                        uint32_t seg, const void* d_slab, uint64_t slot_stride,
                        const uint32_t* d_sizes, uint32_t* d_framed, uint64_t* d_offsets,
                        void* d_frame) {
  if (int r = enter(ctx)) return r;
  if (seg == 0 || seg > kMaxSeg) return fail(BITAR_HIP_INVALID, "seg must be in [1, 65536]");
  const uint64_t nseg64 = (n + seg - 1) / seg;
  if (nseg64 > 0x7FFFFFFFull) return fail(BITAR_HIP_INVALID, "too many segments");
  const uint32_t nseg = (uint32_t)nseg64;
  if (!d_sizes || !d_framed || !d_offsets) return fail(BITAR_HIP_INVALID, "null buffer");
  hipStream_t s = pick_stream(ctx, stream);
  if (nseg) {
    hipLaunchKernelGGL(bitar_hip::lz4f_sizes_kernel, dim3((nseg + 255) / 256), dim3(256), 0, s,
                       d_sizes, nseg, n, seg, d_framed);
    HIP_TRY(hipGetLastError(), "lz4f sizes launch");
  }
  hipLaunchKernelGGL(bitar_hip::scan_sizes_kernel, dim3(1), dim3(1024), 0, s, d_framed, nseg,
                     (uint64_t)BITAR_HIP_SEGMENT_ERROR - 1, d_offsets, err_word(ctx, s));
  HIP_TRY(hipGetLastError(), "scan launch");
  if (d_frame && nseg) {
    if (!d_slab || !d_in) return fail(BITAR_HIP_INVALID, "null input or slab");
    hipLaunchKernelGGL(bitar_hip::lz4f_pack_kernel, dim3(nseg), dim3(64), 0, s,
                       static_cast<const uint8_t*>(d_in), n, seg,
                       static_cast<const uint8_t*>(d_slab), slot_stride, d_sizes, d_offsets,
                       nseg, static_cast<uint8_t*>(d_frame));
    HIP_TRY(hipGetLastError(), "lz4f pack launch");
  }
  return 0;
}

int bitar_hip_checksum(bitar_hip_ctx* ctx, void* stream, uint32_t kind, const void* d_data,
                       uint64_t n, uint32_t seg, const uint32_t* d_lens, uint32_t nseg,
                       uint64_t* d_sums) {
  if (int r = enter(ctx)) return r;
  if (kind < BITAR_HIP_CHECKSUM_CRC32 || kind > BITAR_HIP_CHECKSUM_CRC32_ADLER32)
    return fail(BITAR_HIP_INVALID, "checksum kind must be CRC32, ADLER32 or CRC32_ADLER32");
  if (seg == 0 || seg > kMaxSeg) return fail(BITAR_HIP_INVALID, "seg must be in [1, 65536]");
  if (!d_lens && nseg != (uint32_t)((n + seg - 1) / seg))
    return fail(BITAR_HIP_INVALID, "nseg must be ceil(n / seg) without a length array");
  if (!nseg) return 0;
  if (!d_data || !d_sums) return fail(BITAR_HIP_INVALID, "null buffer");
  hipLaunchKernelGGL(bitar_hip::checksum_kernel, dim3(nseg), dim3(64), 0, pick_stream(ctx, stream),
                     kind, static_cast<const uint8_t*>(d_data), n, seg, d_lens, nseg, d_sums);
  HIP_TRY(hipGetLastError(), "checksum launch");
  return 0;
}

}  // extern "C"

namespace {

template <uint32_t W>
void launch_filter(bool bits, bool inv, uint32_t nseg, hipStream_t s, const uint8_t* in,
                   uint64_t n, uint32_t seg, const uint32_t* lens, uint8_t* out) {
  using Kernel = void (*)(const uint8_t*, uint64_t, uint32_t, const uint32_t*, uint32_t, uint8_t*);
  const Kernel k = bits ? (inv ? bitar_hip::filter_kernel<W, true, true>
                               : bitar_hip::filter_kernel<W, true, false>)
                        : (inv ? bitar_hip::filter_kernel<W, false, true>
                               : bitar_hip::filter_kernel<W, false, false>);
  hipLaunchKernelGGL(k, dim3(nseg), dim3(256), 0, s, in, n, seg, lens, nseg, out);
}

int filter_impl(bitar_hip_ctx* ctx, void* stream, uint32_t filter, uint32_t width, const void* d_in,
                uint64_t n, uint32_t seg, const uint32_t* d_lens, uint32_t nseg, void* d_out,
                bool inv) {
  if (int r = enter(ctx)) return r;
  if (filter != BITAR_HIP_FILTER_SHUFFLE && filter != BITAR_HIP_FILTER_BITSHUFFLE)
    return fail(BITAR_HIP_INVALID, "filter must be SHUFFLE or BITSHUFFLE");
  if (width != 2 && width != 4 && width != 8 && width != 16)
    return fail(BITAR_HIP_INVALID, "element width must be 2, 4, 8 or 16");
  if (seg == 0 || seg > kMaxSeg) return fail(BITAR_HIP_INVALID, "seg must be in [1, 65536]");
  if (n == 0 || nseg == 0) return 0;
  if (!d_in || !d_out) return fail(BITAR_HIP_INVALID, "null buffer");
  const uintptr_t a = reinterpret_cast<uintptr_t>(d_in), b = reinterpret_cast<uintptr_t>(d_out);
  if (a < b ? b - a < n : a - b < n)
    return fail(BITAR_HIP_INVALID, "filter input and output overlap");
  // segments at or past n move nothing: launch only those that start inside the buffer
  const uint64_t inside = (n + seg - 1) / seg;
  if (inside < nseg) nseg = (uint32_t)inside;
  const bool bits = filter == BITAR_HIP_FILTER_BITSHUFFLE;
  hipStream_t s = pick_stream(ctx, stream);
  const uint8_t* in = static_cast<const uint8_t*>(d_in);
  uint8_t* out = static_cast<uint8_t*>(d_out);
  switch (width) {
    case 2: launch_filter<2>(bits, inv, nseg, s, in, n, seg, d_lens, out); break;
    case 4: launch_filter<4>(bits, inv, nseg, s, in, n, seg, d_lens, out); break;
    case 8: launch_filter<8>(bits, inv, nseg, s, in, n, seg, d_lens, out); break;
    default: launch_filter<16>(bits, inv, nseg, s, in, n, seg, d_lens, out); break;
  }
  HIP_TRY(hipGetLastError(), "filter launch");
  return 0;
}

}  // namespace

extern "C" {

int bitar_hip_filter_apply(bitar_hip_ctx* ctx, void* stream, uint32_t filter, uint32_t width,
                           const void* d_in, uint64_t n, uint32_t seg, const uint32_t* d_lens,
                           uint32_t nseg, void* d_out) {
  return filter_impl(ctx, stream, filter, width, d_in, n, seg, d_lens, nseg, d_out, false);
}

int bitar_hip_filter_invert(bitar_hip_ctx* ctx, void* stream, uint32_t filter, uint32_t width,
                            const void* d_in, uint64_t n, uint32_t seg, const uint32_t* d_lens,
                            uint32_t nseg, void* d_out) {
  return filter_impl(ctx, stream, filter, width, d_in, n, seg, d_lens, nseg, d_out, true);
}

int bitar_hip_fill_at(bitar_hip_ctx* ctx, void* stream, int kind, uint64_t seed,
                      uint64_t offset, void* d_out, uint64_t n) {
  if (int r = enter(ctx)) return r;
  if (offset & 63u) return fail(BITAR_HIP_INVALID, "fill offset must be a multiple of 64");
  if (!n) return 0;
  if (!d_out) return fail(BITAR_HIP_INVALID, "null buffer");
  const uint64_t lines = (n + 63) / 64;
  uint64_t blocks = (lines + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(bitar_hip::fill_kernel, dim3((uint32_t)blocks), dim3(256), 0,
                     pick_stream(ctx, stream), kind, seed, offset,
                     static_cast<uint8_t*>(d_out), n);
  HIP_TRY(hipGetLastError(), "fill launch");
  return 0;
}

int bitar_hip_fill(bitar_hip_ctx* ctx, void* stream, int kind, uint64_t seed, void* d_out,
                   uint64_t n) {
  return bitar_hip_fill_at(ctx, stream, kind, seed, 0, d_out, n);
}

}  // extern "C"
