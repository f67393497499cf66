// ransplane_test.cc -- Codec::RANSPLANE through the C++ front-end.
//   cpu            ToString, the ids, and the configurations Initialize refuses (validation runs
//                  before the device is opened, so no device is needed): an element width other
//                  than 2, 4 or 8, a filter, chained operations and a level other than 1
//   gpu            CompressDevice round trips -- host and HBM buffers, sync and async calls,
//                  Recycle, segments of 65536 and 59460 bytes, the CRC32 of the caller's bytes on
//                  both sides -- of bf16-like weights at width 2, a smooth float32 walk at width 4
//                  and N(0,1) float64 at width 8, each against Codec::RANS behind Filter::SHUFFLE
//                  at the same width; noise comes out stored
// Built twice (release and debug front-end); run by tests/test_gpu_ransplane_frontend.py.
#include <arrow/buffer.h>
#include <arrow/memory_pool.h>

#include <cmath>
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

std::unique_ptr<Config> MakeConfig(bitar::Codec codec, std::uint32_t seg,
                                   std::uint8_t width,
                                   bitar::Filter filter = bitar::Filter::NONE) {
  auto c = std::make_unique<Config>(Config::Defaults());
  c->set_codec(codec);
  c->set_decompressed_seg_size32(seg);
  c->set_max_preallocate_memzones(64);
  c->set_checksum_type(bitar::ChecksumType::CRC32);
  if (filter != bitar::Filter::NONE) c->set_filter(filter, width);
  else c->set_element_width(width);
  return c;
}

// a device that has not been opened: Initialize validates the configuration first
Device Unopened() {
  auto d = bitar::DeviceManager::Instance()->Create<bitar::Class_HIP_GFX950>(0, {0});
  CHECK_OK(d.status());
  return d.ok() ? Device(*d) : nullptr;
}

void CpuTests() {
  CHECK(bitar::ToString(bitar::Codec::RANSPLANE) == "RANSPLANE");
  CHECK(static_cast<int>(bitar::Codec::RANSPLANE) == 12);
  CHECK(static_cast<int>(bitar::Codec::CASCADE) == 10 &&
        static_cast<int>(bitar::Codec::RANS) == 11);  // appended: the others keep their values
  CHECK(BITAR_HIP_CODEC_RANSPLANE16 == 81 && BITAR_HIP_CODEC_RANSPLANE32 == 82 &&
        BITAR_HIP_CODEC_RANSPLANE64 == 83);
  CHECK(BITAR_HIP_CODEC_RANSPLANE(2) == 81 && BITAR_HIP_CODEC_RANSPLANE(4) == 82 &&
        BITAR_HIP_CODEC_RANSPLANE(8) == 83);
  Config c;
  c.set_codec(bitar::Codec::RANSPLANE);
  CHECK(c.ToString().find("codec: RANSPLANE") != std::string::npos);

  for (const std::uint8_t width : {std::uint8_t{1}, std::uint8_t{3}, std::uint8_t{16}}) {
    auto d = Unopened();
    if (!d) return;
    const auto st = d->Initialize(MakeConfig(bitar::Codec::RANSPLANE, 65536, width));
    CHECK(st.IsInvalid());
    CHECK(st.ToString().find("element_width (" + std::to_string(width) +
                             ") of RANSPLANE must be 2, 4 or 8") != std::string::npos);
  }
  for (const auto filter : {bitar::Filter::SHUFFLE, bitar::Filter::BITSHUFFLE}) {  // no filter
    auto d = Unopened();
    const auto st = d->Initialize(MakeConfig(bitar::Codec::RANSPLANE, 65536, 4, filter));
    CHECK(st.IsInvalid());
    CHECK(st.ToString().find("RANSPLANE takes no filter") != std::string::npos);
  }
  {  // no chained ops
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::RANSPLANE, 4096, 4);
    cfg->set_max_sgl_segs(2);
    const auto st = d->Initialize(std::move(cfg));
    CHECK(st.IsInvalid());
    CHECK(st.ToString().find("RANSPLANE cannot be combined with chained operations") !=
          std::string::npos);
  }
  for (const std::uint8_t level : {std::uint8_t{0}, std::uint8_t{2}, std::uint8_t{9}}) {  // level 1
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::RANSPLANE, 65536, 4);
    cfg->set_level(level);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
  }
  // valid configurations pass the validation (without a device the open itself then fails, but
  // not as Invalid); a window is ignored whatever it says
  for (const std::uint8_t width : {std::uint8_t{2}, std::uint8_t{4}, std::uint8_t{8}}) {
    for (const std::uint32_t seg : {59460u, 65536u}) {
      auto d = Unopened();
      auto cfg = MakeConfig(bitar::Codec::RANSPLANE, seg, width);
      cfg->set_window_size(width == 4 ? 3 : 0);
      CHECK(!d->Initialize(std::move(cfg)).IsInvalid());
    }
  }
  // the other codecs' rules are unchanged: RANS still takes a filter, CASCADE none
  {
    auto d = Unopened();
    CHECK(!d->Initialize(MakeConfig(bitar::Codec::RANS, 65536, 4, bitar::Filter::SHUFFLE))
               .IsInvalid());
    auto d2 = Unopened();
    CHECK(d2->Initialize(MakeConfig(bitar::Codec::CASCADE, 65536, 4, bitar::Filter::SHUFFLE))
              .IsInvalid());
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

// the sum of twelve uniforms less six: near enough N(0,1)
double Gauss(std::uint64_t* x) {
  double s = -6.0;
  for (int k = 0; k < 12; ++k) s += static_cast<double>(SplitMix(x) >> 11) / 9007199254740992.0;
  return s;
}

// a smooth float32 walk, and N(0,1) float64 values; cut at an odd byte count
std::vector<std::uint8_t> FloatWalk(std::size_t bytes, std::uint64_t seed) {
  std::uint64_t x = seed;
  std::vector<float> f(bytes / 4 + 1);
  double at = 0;
  for (auto& e : f) e = static_cast<float>(at += 0.01 * Gauss(&x));
  std::vector<std::uint8_t> v(f.size() * 4);
  std::memcpy(v.data(), f.data(), v.size());
  v.resize(bytes);
  return v;
}
std::vector<std::uint8_t> Normal64(std::size_t bytes, std::uint64_t seed) {
  std::uint64_t x = seed;
  std::vector<double> f(bytes / 8 + 1);
  for (auto& e : f) e = Gauss(&x);
  std::vector<std::uint8_t> v(f.size() * 8);
  std::memcpy(v.data(), f.data(), v.size());
  v.resize(bytes);
  return v;
}

// float32 values of N(0, 0.02) cut to their high 16 bits: bf16 weights; an odd byte count
std::vector<std::uint8_t> Weights16(std::size_t bytes, std::uint64_t seed) {
  std::uint64_t x = seed;
  std::vector<std::uint16_t> h(bytes / 2 + 1);
  for (auto& e : h) {
    const float f = static_cast<float>(0.02 * Gauss(&x));
    std::uint32_t u;
    std::memcpy(&u, &f, 4);
    e = static_cast<std::uint16_t>(u >> 16);
  }
  std::vector<std::uint8_t> v(h.size() * 2);
  std::memcpy(v.data(), h.data(), v.size());
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

void GpuTests() {
  struct Case {
    const char* name;
    std::vector<std::uint8_t> data;
    std::uint8_t width;
  };
  const Case cases[] = {
      {"bf16 weights, width 2", Weights16(5 * 65536 + 4099, 7), 2},
      {"float32 walk, width 4", FloatWalk(5 * 65536 + 4099, 8), 4},
      {"N(0,1) float64, width 8", Normal64(5 * 65536 + 4099, 9), 8},
  };
  for (const auto& c : cases) {
    for (const std::uint32_t seg : {65536u, 59460u}) {
      std::size_t total[2] = {0, 0};
      for (int k = 0; k < 2; ++k) {
        auto d = NewDevice();
        if (!d) return;
        auto cfg = k == 0 ? MakeConfig(bitar::Codec::RANS, seg, c.width, bitar::Filter::SHUFFLE)
                          : MakeConfig(bitar::Codec::RANSPLANE, seg, c.width);
        if (k == 1) cfg->set_window_size(9);  // ignored
        CHECK_OK(d->Initialize(std::move(cfg)));
        if (k == 1) {
          CHECK(d->encoder_window() == 0);
          CHECK(d->slot_size() >= seg + 4u);
        }
        total[k] = RoundTrips(d, c.data, seg);
      }
      std::cout << c.name << ", seg " << seg << ": RANSPLANE " << total[1]
                << " bytes, shuffle + RANS " << total[0] << " of " << c.data.size() << "\n";
      // the planes' histograms differ in every case: a table a plane is smaller than one table
      // over the shuffled planes (tests/test_ransplane_model.py has the model's margins)
      CHECK(total[1] > 0 && total[1] < c.data.size());
      CHECK(total[1] < total[0]);
    }
  }
  // noise is stored: 4 bytes of header per segment
  for (const std::uint8_t width : {std::uint8_t{2}, std::uint8_t{4}, std::uint8_t{8}}) {
    auto d = NewDevice();
    if (!d) return;
    CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::RANSPLANE, 65536, width)));
    const auto noise = NoiseColumn(3 * 65536 + 5);
    CHECK(RoundTrips(d, noise, 65536) == noise.size() + 4 * 4);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "cpu";
  if (mode == "cpu") CpuTests();
  else if (mode == "gpu") GpuTests();
  else {
    std::cerr << "usage: bitar_ransplane_test cpu|gpu\n";
    return 2;
  }
  if (g_failures) {
    std::cerr << g_failures << " check(s) failed\n";
    return 1;
  }
  std::cout << "ransplane_test " << mode << ": ok\n";
  return 0;
}
