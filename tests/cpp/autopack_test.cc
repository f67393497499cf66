// autopack_test.cc -- Codec::AUTOPACK through the C++ front-end.
//   cpu            ToString, the ids, and the configurations Initialize refuses, each with a
//                  message that names the field (validation runs before the device is opened, so
//                  no device is needed)
//   gpu            CompressDevice round trips of an int64 column whose shape changes every 64 KiB
//                  -- sorted timestamps, 2-decimal prices, ids of 40 values, integers in a range
//                  of 3000, random values -- from host and HBM buffers, sync and async calls,
//                  Recycle, segments of 65536 and 59460 bytes; the CRC32 of the caller's bytes on
//                  both sides; the compressed total against each single codec's on the same
//                  buffer; noise comes out stored
// Built twice (release and debug front-end); run by tests/test_gpu_autopack_frontend.py.
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

bool Refused(arrow::Status st, const char* field) {
  return st.IsInvalid() && st.message().find(field) != std::string::npos;
}

void CpuTests() {
  CHECK(bitar::ToString(bitar::Codec::AUTOPACK) == "AUTOPACK");
  CHECK(static_cast<int>(bitar::Codec::AUTOPACK) == 8);
  CHECK(BITAR_HIP_CODEC_AUTOPACK(1) == 40 && BITAR_HIP_CODEC_AUTOPACK(2) == 41 &&
        BITAR_HIP_CODEC_AUTOPACK(4) == 42 && BITAR_HIP_CODEC_AUTOPACK(8) == 43 &&
        BITAR_HIP_CODEC_AUTOPACK(16) == 44);
  Config c;
  c.set_codec(bitar::Codec::AUTOPACK);
  c.set_element_width(16);
  CHECK(c.element_width() == 16 && c.filter() == bitar::Filter::NONE);
  CHECK(c.ToString().find("codec: AUTOPACK") != std::string::npos);

  // element_width outside {1, 2, 4, 8, 16}
  for (const std::uint8_t width : {std::uint8_t{0}, std::uint8_t{3}, std::uint8_t{5},
                                   std::uint8_t{12}, std::uint8_t{32}, std::uint8_t{255}}) {
    auto d = Unopened();
    if (!d) return;
    CHECK(Refused(d->Initialize(MakeConfig(bitar::Codec::AUTOPACK, 65536, width)), "element_width"));
  }
  for (const auto filter : {bitar::Filter::SHUFFLE, bitar::Filter::BITSHUFFLE}) {  // no filter
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::AUTOPACK, 65536, 8);
    cfg->set_filter(filter, 8);
    CHECK(Refused(d->Initialize(std::move(cfg)), "filter"));
  }
  {  // no chained ops
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::AUTOPACK, 4096, 4);
    cfg->set_max_sgl_segs(2);
    CHECK(Refused(d->Initialize(std::move(cfg)), "max_sgl_segs"));
  }
  for (const std::uint8_t level : {std::uint8_t{0}, std::uint8_t{2}, std::uint8_t{9}}) {  // level 1
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::AUTOPACK, 65536, 16);
    cfg->set_level(level);
    CHECK(Refused(d->Initialize(std::move(cfg)), "level"));
  }
  // valid configurations pass the validation (without a device the open itself then fails, but
  // not as Invalid); a window is ignored, whatever it says
  for (const std::uint8_t width : {std::uint8_t{1}, std::uint8_t{2}, std::uint8_t{4},
                                   std::uint8_t{8}, std::uint8_t{16}}) {
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::AUTOPACK, 59460, width);
    cfg->set_window_size(width == 4 ? 3 : 0);
    CHECK(!d->Initialize(std::move(cfg)).IsInvalid());
  }
  // the four codecs' rules are unchanged
  {
    auto d = Unopened();
    CHECK(d->Initialize(MakeConfig(bitar::Codec::FLTPACK, 65536, 16)).IsInvalid());
    auto e = Unopened();
    CHECK(e->Initialize(MakeConfig(bitar::Codec::INTPACK, 65536, 16)).IsInvalid());
    auto f = Unopened();
    CHECK(f->Initialize(MakeConfig(bitar::Codec::DICTPACK, 65536, 1)).IsInvalid());
    auto g = Unopened();
    CHECK(!g->Initialize(MakeConfig(bitar::Codec::RUNPACK, 65536, 16)).IsInvalid());
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

// int64 elements whose shape changes every 64 KiB: sorted timestamps of 50 values, prices with
// two decimals (doubles), ids drawn from 40 random values, integers in a range of 3000, random
// 63-bit values -- `rounds` times, then cut at an odd byte count
std::vector<std::uint8_t> MixedColumn(std::size_t rounds) {
  const std::size_t m = 65536 / 8;
  std::uint64_t x = 2026;
  std::vector<std::uint64_t> ids(40);
  for (auto& v : ids) v = SplitMix(&x) >> 1;
  std::vector<std::uint64_t> col;
  for (std::size_t r = 0; r < rounds; ++r) {
    for (std::size_t i = 0; i < m; ++i) col.push_back(1700000000000ull + 60000ull * (i * 50 / m));
    for (std::size_t i = 0; i < m; ++i) {
      const double price = static_cast<double>(SplitMix(&x) % 100000) / 100.0;
      std::uint64_t bits;
      std::memcpy(&bits, &price, 8);
      col.push_back(bits);
    }
    for (std::size_t i = 0; i < m; ++i) col.push_back(ids[SplitMix(&x) % 40]);
    for (std::size_t i = 0; i < m; ++i) col.push_back(1000000ull + SplitMix(&x) % 3000);
    for (std::size_t i = 0; i < m; ++i) col.push_back(SplitMix(&x) >> 1);
  }
  std::vector<std::uint8_t> v(col.size() * 8);
  std::memcpy(v.data(), col.data(), v.size());
  v.resize(v.size() - 4099);
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
  const auto data = MixedColumn(2);
  for (const std::uint32_t seg : {65536u, 59460u}) {
    std::size_t packed = 0;
    {
      auto d = NewDevice();
      if (!d) return;
      auto cfg = MakeConfig(bitar::Codec::AUTOPACK, seg, 8);
      cfg->set_window_size(9);  // ignored
      CHECK_OK(d->Initialize(std::move(cfg)));
      CHECK(d->encoder_window() == 0);
      CHECK(d->slot_size() >= seg + 4u);
      packed = RoundTrips(d, data, seg);
    }
    CHECK(packed > 0 && packed < data.size());
    std::cout << "mixed int64 column, seg " << seg << ": AUTOPACK " << packed << " of "
              << data.size() << " bytes;";
    // never above a single candidate's total on the same buffer
    for (const auto codec : {bitar::Codec::RUNPACK, bitar::Codec::INTPACK, bitar::Codec::DICTPACK,
                             bitar::Codec::FLTPACK}) {
      auto d = NewDevice();
      CHECK_OK(d->Initialize(MakeConfig(codec, seg, 8)));
      const std::size_t single = RoundTrips(d, data, seg);
      std::cout << " " << bitar::ToString(codec) << " " << single;
      CHECK(single > 0 && packed <= single);
      if (seg == 65536) CHECK(packed < single);  // (whole-segment shapes: each codec loses some)
    }
    std::cout << "\n";
  }
  // noise is stored: 4 bytes of header per segment
  {
    auto d = NewDevice();
    CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::AUTOPACK, 65536, 8)));
    const auto noise = NoiseColumn(3 * 65536 + 5);
    CHECK(RoundTrips(d, noise, 65536) == noise.size() + 4 * 4);
  }
  // every width round-trips the same bytes; the decoding side needs no width (the default, 1)
  for (const std::uint8_t width : {std::uint8_t{1}, std::uint8_t{2}, std::uint8_t{4},
                                   std::uint8_t{16}}) {
    auto d = NewDevice();
    CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::AUTOPACK, 59460, width)));
    CHECK(RoundTrips(d, data, 59460) > 0);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "cpu";
  if (mode == "cpu") CpuTests();
  else if (mode == "gpu") GpuTests();
  else {
    std::cerr << "usage: bitar_autopack_test cpu|gpu\n";
    return 2;
  }
  if (g_failures) {
    std::cerr << g_failures << " check(s) failed\n";
    return 1;
  }
  std::cout << "autopack_test " << mode << ": ok\n";
  return 0;
}
