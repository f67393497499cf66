// dictpack_test.cc -- Codec::DICTPACK through the C++ front-end.
//   cpu            ToString, the ids, and the configurations Initialize refuses (validation runs
//                  before the device is opened, so no device is needed)
//   gpu            CompressDevice round trips of low-cardinality columns -- int64 ids of 40 values
//                  (width 8), floats of 900 values (width 4), 16-byte ids of 500 values (width
//                  16) -- host and HBM buffers, sync and async calls, Recycle, segments of 65536
//                  and 59460 bytes; the CRC32 of the caller's bytes on both sides; the compressed
//                  total against Codec::LZ4 and against what the format's size formula allows;
//                  noise comes out stored
// Built twice (release and debug front-end); run by tests/test_gpu_dictpack_frontend.py.
#include <arrow/buffer.h>
#include <arrow/memory_pool.h>

#include <cstdint>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "bitar/bitar.h"
#include "bitar_hip.h"

namespace {

int g_failures = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::cerr << __FILE__ << ":" << __LINE__ << " CHECK failed: " #cond "\n"; \
      ++g_failures;                                                           \
    }                                                                         \
  } while (0)
#define CHECK_OK(expr)                                                                 \
  do {                                                                                 \
    auto _s = (expr);                                                                  \
    if (!_s.ok()) {                                                                    \
      std::cerr << __FILE__ << ":" << __LINE__ << " not OK: " << _s.ToString() << "\n"; \
      ++g_failures;                                                                    \
    }                                                                                  \
  } while (0)

using Config = bitar::HipConfiguration;
using Device = std::unique_ptr<bitar::HipGfx950CompressDevice>;

std::unique_ptr<Config> MakeConfig(bitar::Codec codec, std::uint32_t seg, std::uint8_t width) {
  auto c = std::make_unique<Config>(Config::Defaults());
  c->set_codec(codec);
  c->set_decompressed_seg_size32(seg);
  c->set_max_preallocate_memzones(64);
  c->set_checksum_type(bitar::ChecksumType::CRC32);
  c->set_element_width(width);
  return c;
}

// a device that has not been opened: Initialize validates the configuration first
Device Unopened() {
  auto d = bitar::DeviceManager::Instance()->Create<bitar::Class_HIP_GFX950>(0, {0});
  CHECK_OK(d.status());
  return d.ok() ? Device(*d) : nullptr;
}

void CpuTests() {
  CHECK(bitar::ToString(bitar::Codec::DICTPACK) == "DICTPACK");
  CHECK(static_cast<int>(bitar::Codec::DICTPACK) == 6);
  CHECK(BITAR_HIP_CODEC_DICTPACK(4) == 26 && BITAR_HIP_CODEC_DICTPACK(8) == 27 &&
        BITAR_HIP_CODEC_DICTPACK(16) == 28);
  Config c;
  c.set_codec(bitar::Codec::DICTPACK);
  c.set_element_width(16);
  CHECK(c.element_width() == 16 && c.filter() == bitar::Filter::NONE);
  CHECK(c.ToString().find("codec: DICTPACK") != std::string::npos);

  // element_width outside {4, 8, 16}
  for (const std::uint8_t width : {std::uint8_t{0}, std::uint8_t{1}, std::uint8_t{2},
                                   std::uint8_t{3}, std::uint8_t{12}, std::uint8_t{32},
                                   std::uint8_t{255}}) {
    auto d = Unopened();
    if (!d) return;
    CHECK(d->Initialize(MakeConfig(bitar::Codec::DICTPACK, 65536, width)).IsInvalid());
  }
  for (const auto filter : {bitar::Filter::SHUFFLE, bitar::Filter::BITSHUFFLE}) {  // no filter
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::DICTPACK, 65536, 8);
    cfg->set_filter(filter, 8);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
  }
  {  // no chained ops
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::DICTPACK, 4096, 4);
    cfg->set_max_sgl_segs(2);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
  }
  for (const std::uint8_t level : {std::uint8_t{0}, std::uint8_t{2}, std::uint8_t{9}}) {  // level 1
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::DICTPACK, 65536, 16);
    cfg->set_level(level);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
  }
  // valid configurations pass the validation (without a device the open itself then fails, but
  // not as Invalid); a window is ignored, whatever it says
  for (const std::uint8_t width : {std::uint8_t{4}, std::uint8_t{8}, std::uint8_t{16}}) {
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::DICTPACK, 59460, width);
    cfg->set_window_size(width == 4 ? 3 : 0);
    CHECK(!d->Initialize(std::move(cfg)).IsInvalid());
  }
  // the other codecs' rules are unchanged: FLTPACK still refuses 16-byte elements, INTPACK
  // still takes 2-byte ones
  {
    auto d = Unopened();
    CHECK(d->Initialize(MakeConfig(bitar::Codec::FLTPACK, 65536, 16)).IsInvalid());
    auto e = Unopened();
    CHECK(!e->Initialize(MakeConfig(bitar::Codec::INTPACK, 65536, 2)).IsInvalid());
  }
}

// zlib's CRC-32, bit by bit
std::uint32_t Crc32(const std::uint8_t* p, std::size_t n) {
  std::uint32_t c = 0xFFFFFFFFu;
  for (std::size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int b = 0; b < 8; ++b) c = c & 1u ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  }
  return ~c;
}

std::uint64_t SplitMix(std::uint64_t* x) {
  *x += 0x9E3779B97F4A7C15ull;
  std::uint64_t z = *x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// `bytes` bytes of elements of `width` bytes drawn from `distinct` values whose bytes are all
// random; cut at an odd byte count
std::vector<std::uint8_t> DrawnColumn(std::size_t bytes, std::size_t width, std::size_t distinct,
                                      std::uint64_t seed) {
  std::uint64_t x = seed;
  std::vector<std::uint8_t> values(distinct * width);
  for (auto& b : values) b = static_cast<std::uint8_t>(SplitMix(&x) >> 56);
  for (std::size_t k = 0; k < distinct; ++k) {  // (distinct for certain)
    values[k * width] = static_cast<std::uint8_t>(k);
    values[k * width + 1] = static_cast<std::uint8_t>(k >> 8);
  }
  std::vector<std::uint8_t> v(bytes + width);
  for (std::size_t i = 0; i + width <= v.size(); i += width)
    std::memcpy(&v[i], &values[(SplitMix(&x) % distinct) * width], width);
  v.resize(bytes);
  return v;
}

// all bytes random: stored
std::vector<std::uint8_t> NoiseColumn(std::size_t bytes) {
  std::vector<std::uint8_t> v(bytes);
  std::uint64_t x = 13;
  for (auto& b : v) b = static_cast<std::uint8_t>(SplitMix(&x) >> 56);
  return v;
}

Device NewDevice() {
  auto* driver = bitar::CompressDriver<bitar::Class_HIP_GFX950>::Instance();
  auto ids = driver->ListAvailableDeviceIds();
  CHECK_OK(ids.status());
  if (!ids.ok() || ids->empty()) return nullptr;
  driver->set_num_workers(1);
  auto devs = driver->GetDevices({(*ids)[0]});
  CHECK_OK(devs.status());
  if (!devs.ok()) return nullptr;
  return std::move((*devs)[0]);
}

void CheckSums(const Device& d, const std::vector<std::uint8_t>& data, std::uint32_t seg) {
  const auto& sums = d->checksums(0);
  const std::size_t nseg = (data.size() + seg - 1) / seg;
  CHECK(sums.size() == nseg);
  for (std::size_t i = 0; i < nseg && i < sums.size(); ++i) {
    const std::size_t len = std::min<std::size_t>(seg, data.size() - i * seg);
    CHECK((sums[i] & 0xFFFFFFFFu) == Crc32(data.data() + i * seg, len));
  }
}

std::size_t Total(const bitar::BufferVector& bufs) {
  std::size_t total = 0;
  for (const auto& b : bufs) total += static_cast<std::size_t>(b->size());
  return total;
}

// host -> slots -> host (sync calls) and HBM -> slots -> HBM (CompressAsync / DecompressAsync) on one device; the
// total of the compressed sizes
std::size_t RoundTrips(const Device& d, const std::vector<std::uint8_t>& data, std::uint32_t seg) {
  const auto n = static_cast<std::int64_t>(data.size());
  const std::size_t nseg = (data.size() + seg - 1) / seg;
  auto host_in = std::make_shared<arrow::Buffer>(data.data(), n);
  auto comp = d->Compress(0, host_in);
  CHECK_OK(comp.status());
  if (!comp.ok()) return 0;
  CHECK(comp->size() == nseg);
  CheckSums(d, data, seg);
  const std::size_t total = Total(*comp);
  auto out = arrow::AllocateResizableBuffer(static_cast<std::int64_t>(nseg * seg));
  CHECK_OK(out.status());
  std::unique_ptr<arrow::ResizableBuffer> host_out = std::move(*out);
  std::memset(host_out->mutable_data(), 0x5A, nseg * seg);
  CHECK_OK(d->Decompress(0, *comp, host_out));
  CHECK(host_out->size() == n);
  CHECK(std::memcmp(host_out->data(), data.data(), data.size()) == 0);
  CheckSums(d, data, seg);
  d->Recycle(*comp);

  auto dev_in = arrow::Buffer::Copy(host_in, bitar::hip_memory_manager(0));
  CHECK_OK(dev_in.status());
  if (!dev_in.ok()) return total;
  // the async pair: the calls run on the queue pair's worker, the callbacks hand the results back
  using Class = bitar::Class_HIP_GFX950;
  arrow::Result<bitar::BufferVector> comp2 = arrow::Status::UnknownError("callback not run");
  const auto on_compressed = [&comp2](std::uint8_t, std::uint16_t,
                                      arrow::Result<bitar::BufferVector>&& result) {
    comp2 = std::move(result);
    return bitar::kAsyncReturnOK;
  };
  const std::shared_ptr<arrow::Buffer> device_input = *dev_in;
  auto cparam = std::make_unique<bitar::CompressParam<Class, decltype(on_compressed)>>(
      d, 0, device_input, on_compressed);
  CHECK(bitar::CompressAsync(cparam) == 0);
  CHECK(bitar::WaitLcore(d->LcoreOf(0)) == bitar::kAsyncReturnOK);
  CHECK_OK(comp2.status());
  if (!comp2.ok()) return total;
  CheckSums(d, data, seg);
  CHECK(Total(*comp2) == total);
  auto dev_out = bitar::AllocateResizableDeviceBuffer(static_cast<std::int64_t>(nseg * seg), 0);
  CHECK_OK(dev_out.status());
  std::unique_ptr<arrow::ResizableBuffer> dout = std::move(*dev_out);
  arrow::Status dstatus = arrow::Status::UnknownError("callback not run");
  const auto on_decompressed = [&dstatus](std::uint8_t, std::uint16_t,
                                          const arrow::Status& status) {
    dstatus = status;
    return bitar::kAsyncReturnOK;
  };
  auto dparam = std::make_unique<bitar::DecompressParam<Class, decltype(on_decompressed)>>(
      d, 0, *comp2, dout, on_decompressed);
  CHECK(bitar::DecompressAsync(dparam) == 0);
  CHECK(bitar::WaitLcore(d->LcoreOf(0)) == bitar::kAsyncReturnOK);
  CHECK_OK(dstatus);
  CHECK(!dout->is_cpu() && dout->size() == n);
  CheckSums(d, data, seg);
  auto back = arrow::Buffer::Copy(std::shared_ptr<arrow::Buffer>(std::move(dout)),
                                  arrow::default_cpu_memory_manager());
  CHECK_OK(back.status());
  if (back.ok()) CHECK(std::memcmp((*back)->data(), data.data(), data.size()) == 0);
  d->Recycle(*comp2);
  return total;
}

// the packed size of a segment of L bytes with d distinct elements (include/bitar_hip.h)
std::size_t PackedSize(std::size_t L, std::size_t w, std::size_t d) {
  std::size_t b = 0;
  while ((std::size_t{1} << b) < d) ++b;
  const std::size_t m = L / w;
  return 6 + d * w + 8 * b * ((m + 63) / 64) + (L - m * w);
}

void GpuTests() {
  struct Case {
    const char* name;
    std::vector<std::uint8_t> data;
    std::uint8_t width;
    std::size_t distinct;
  };
  const Case cases[] = {{"int64 ids, 40 values", DrawnColumn(5 * 65536 + 4099, 8, 40, 7), 8, 40},
                        {"floats, 900 values", DrawnColumn(5 * 65536 + 4099, 4, 900, 11), 4, 900},
                        {"16-byte ids, 500 values", DrawnColumn(5 * 65536 + 4099, 16, 500, 17), 16,
                         500}};
  for (const auto& c : cases) {
    for (const std::uint32_t seg : {65536u, 59460u}) {
      std::size_t lz4 = 0, packed = 0;
      {
        auto d = NewDevice();
        if (!d) return;
        CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::LZ4, seg, 1)));
        lz4 = RoundTrips(d, c.data, seg);
      }
      {
        auto d = NewDevice();
        auto cfg = MakeConfig(bitar::Codec::DICTPACK, seg, c.width);
        cfg->set_window_size(9);  // ignored
        CHECK_OK(d->Initialize(std::move(cfg)));
        CHECK(d->encoder_window() == 0);
        CHECK(d->slot_size() >= seg + 4u);
        packed = RoundTrips(d, c.data, seg);
      }
      std::cout << c.name << " seg " << seg << ": DICTPACK " << packed << " bytes, LZ4 " << lz4
                << " of " << c.data.size() << "\n";
      const std::size_t nseg = (c.data.size() + seg - 1) / seg;
      if (seg % c.width == 0) {
        // every segment packs, at no more than the size that `distinct` entries give
        std::size_t bound = 0;
        for (std::size_t i = 0; i < nseg; ++i)
          bound += PackedSize(std::min<std::size_t>(seg, c.data.size() - i * seg), c.width,
                              c.distinct);
        CHECK(packed > 0 && packed < lz4 && packed <= bound);
      } else {
        // 59460 is no multiple of 8 or 16: a segment that starts inside an element sees the
        // halves of two neighbours as one value, far more than 1024 of them, and is stored;
        // the segments that start on an element pack as above
        CHECK(packed > 0 && packed <= c.data.size() + 4 * nseg);
        CHECK(packed < c.data.size());
      }
    }
  }
  // noise is stored: 4 bytes of header per segment
  {
    auto d = NewDevice();
    CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::DICTPACK, 65536, 8)));
    const auto noise = NoiseColumn(3 * 65536 + 5);
    CHECK(RoundTrips(d, noise, 65536) == noise.size() + 4 * 4);
  }
  // another width still round-trips (it only packs worse, or not at all)
  {
    auto d = NewDevice();
    CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::DICTPACK, 59460, 4)));
    CHECK(RoundTrips(d, cases[0].data, 59460) > 0);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "cpu";
  if (mode == "cpu") CpuTests();
  else if (mode == "gpu") GpuTests();
  else {
    std::cerr << "usage: bitar_dictpack_test cpu|gpu\n";
    return 2;
  }
  if (g_failures) {
    std::cerr << g_failures << " check(s) failed\n";
    return 1;
  }
  std::cout << "dictpack_test " << mode << ": ok\n";
  return 0;
}
