// snappy_test.cc -- Codec::SNAPPY through the C++ front-end.
//   cpu            ToString, the ids, and the configurations Initialize refuses or takes
//                  (validation runs before the device is opened, so no device is needed)
//   gpu            CompressDevice round trips of a text-like column, a column of records and
//                  noise -- host and HBM buffers, sync and async calls, Recycle, segments of 65536
//                  and 59460 bytes, chained operations of 4 x 16384 -- with the CRC32 of the
//                  caller's bytes on both sides; Arrow's own Snappy codec decodes every
//                  compressed stream to the input; the totals against Codec::LZ4 (the same parse)
// Built twice (release and debug front-end); run by tests/test_gpu_snappy_frontend.py.
#include <arrow/buffer.h>
#include <arrow/memory_pool.h>
#include <arrow/util/compression.h>

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

std::unique_ptr<Config> MakeConfig(bitar::Codec codec, std::uint32_t seg, std::uint16_t sgl = 1) {
  auto c = std::make_unique<Config>(Config::Defaults());
  c->set_codec(codec);
  c->set_decompressed_seg_size32(seg);
  c->set_max_preallocate_memzones(64);
  c->set_checksum_type(bitar::ChecksumType::CRC32);
  c->set_max_sgl_segs(sgl);
  return c;
}

// a device that has not been opened: Initialize validates the configuration first
Device Unopened() {
  auto d = bitar::DeviceManager::Instance()->Create<bitar::Class_HIP_GFX950>(0, {0});
  CHECK_OK(d.status());
  return d.ok() ? Device(*d) : nullptr;
}

void CpuTests() {
  CHECK(bitar::ToString(bitar::Codec::SNAPPY) == "SNAPPY");
  CHECK(static_cast<int>(bitar::Codec::SNAPPY) == 9);
  CHECK(BITAR_HIP_CODEC_SNAPPY == 6 && BITAR_HIP_ABI_VERSION == 3);
  CHECK(bitar_hip_slot_size(BITAR_HIP_CODEC_SNAPPY, 65536) == 65792);
  CHECK(bitar_hip_max_distance(BITAR_HIP_CODEC_SNAPPY) == 2560);
  CHECK(bitar_hip_slot_size(7, 65536) == 0 && bitar_hip_slot_size(12, 65536) == 0);
  Config c;
  c.set_codec(bitar::Codec::SNAPPY);
  CHECK(c.ToString().find("codec: SNAPPY") != std::string::npos);
  for (const std::uint8_t level : {std::uint8_t{0}, std::uint8_t{2}, std::uint8_t{9}}) {  // level 1
    auto d = Unopened();
    if (!d) return;
    auto cfg = MakeConfig(bitar::Codec::SNAPPY, 65536);
    cfg->set_level(level);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
  }
  // the window: the reach (2560 B -> 2^12) up to the format's 2^16
  for (const std::uint8_t window : {std::uint8_t{11}, std::uint8_t{17}}) {
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::SNAPPY, 65536);
    cfg->set_window_size(window);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
  }
  for (const std::uint8_t window : {std::uint8_t{0}, std::uint8_t{12}, std::uint8_t{16}}) {
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::SNAPPY, 59460);
    cfg->set_window_size(window);
    CHECK(!d->Initialize(std::move(cfg)).IsInvalid());
  }
  {  // chained operations: up to 64 KiB per operation, as for LZ4
    auto d = Unopened();
    CHECK(!d->Initialize(MakeConfig(bitar::Codec::SNAPPY, 16384, 4)).IsInvalid());
    auto e = Unopened();
    CHECK(e->Initialize(MakeConfig(bitar::Codec::SNAPPY, 32768, 4)).IsInvalid());
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

// words drawn from a list of 200, separated by blanks
std::vector<std::uint8_t> TextColumn(std::size_t bytes) {
  std::uint64_t x = 3;
  std::vector<std::string> words(200);
  for (auto& w : words) {
    w.resize(2 + SplitMix(&x) % 9);
    for (auto& ch : w) ch = static_cast<char>('a' + SplitMix(&x) % 26);
  }
  std::vector<std::uint8_t> v;
  while (v.size() < bytes) {
    const auto& w = words[SplitMix(&x) % words.size()];
    v.insert(v.end(), w.begin(), w.end());
    v.push_back(' ');
  }
  v.resize(bytes);
  return v;
}

// 24-byte records: a counter, one of 16 tags, a slowly changing value, noise
std::vector<std::uint8_t> RecordColumn(std::size_t bytes) {
  std::uint64_t x = 5, value = 1000;
  std::vector<std::uint8_t> v(bytes + 24);
  for (std::size_t i = 0; i * 24 < bytes; ++i) {
    const std::uint64_t f[3] = {i, (SplitMix(&x) % 16) * 0x0101010101010101ull,
                                value += SplitMix(&x) % 3};
    std::memcpy(&v[i * 24], f, 24);
    v[i * 24 + 23] = static_cast<std::uint8_t>(SplitMix(&x));
  }
  v.resize(bytes);
  return v;
}

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

// one CRC32 per operation of `op` bytes
void CheckSums(const Device& d, const std::vector<std::uint8_t>& data, std::size_t op) {
  const auto& sums = d->checksums(0);
  const std::size_t nops = (data.size() + op - 1) / op;
  CHECK(sums.size() == nops);
  for (std::size_t i = 0; i < nops && i < sums.size(); ++i) {
    const std::size_t len = std::min<std::size_t>(op, data.size() - i * op);
    CHECK((sums[i] & 0xFFFFFFFFu) == Crc32(data.data() + i * op, len));
  }
}

std::size_t Total(const bitar::BufferVector& bufs) {
  std::size_t total = 0;
  for (const auto& b : bufs) total += static_cast<std::size_t>(b->size());
  return total;
}

// Arrow's Snappy codec on every operation's stream (k buffers each, joined)
void StockDecodes(const bitar::BufferVector& bufs, const std::vector<std::uint8_t>& data,
                  std::size_t op, std::size_t k) {
  auto codec = arrow::util::Codec::Create(arrow::Compression::SNAPPY);
  CHECK_OK(codec.status());
  if (!codec.ok()) return;
  std::vector<std::uint8_t> out(op);
  for (std::size_t j = 0; j * k < bufs.size(); ++j) {
    std::vector<std::uint8_t> stream;
    for (std::size_t i = j * k; i < std::min(bufs.size(), (j + 1) * k); ++i) {
      if (bufs[i]->size() == 0) continue;  // (a chained operation's trailing slots)
      auto view = std::make_shared<arrow::Buffer>(
          reinterpret_cast<const std::uint8_t*>(bufs[i]->address()), bufs[i]->size(),
          bufs[i]->memory_manager());
      auto host = arrow::Buffer::Copy(view, arrow::default_cpu_memory_manager());
      CHECK_OK(host.status());
      if (!host.ok()) return;
      stream.insert(stream.end(), (*host)->data(), (*host)->data() + (*host)->size());
    }
    const std::size_t len = std::min<std::size_t>(op, data.size() - j * op);
    auto got = (*codec)->Decompress(static_cast<std::int64_t>(stream.size()), stream.data(),
                                    static_cast<std::int64_t>(len), out.data());
    CHECK_OK(got.status());
    CHECK(got.ok() && static_cast<std::size_t>(*got) == len &&
          std::memcmp(out.data(), data.data() + j * op, len) == 0);
  }
}

// host -> slots -> host (sync calls) and HBM -> slots -> HBM (CompressAsync / DecompressAsync)
// on one device; the total of the compressed sizes
std::size_t RoundTrips(const Device& d, const std::vector<std::uint8_t>& data, std::uint32_t seg,
                       std::size_t k) {
  const auto n = static_cast<std::int64_t>(data.size());
  const std::size_t nseg = (data.size() + seg - 1) / seg;
  auto host_in = std::make_shared<arrow::Buffer>(data.data(), n);
  auto comp = d->Compress(0, host_in);
  CHECK_OK(comp.status());
  if (!comp.ok()) return 0;
  CHECK(comp->size() == nseg);
  CheckSums(d, data, k * seg);
  StockDecodes(*comp, data, k * seg, k);
  const std::size_t total = Total(*comp);
  auto out = arrow::AllocateResizableBuffer(static_cast<std::int64_t>(nseg * seg));
  CHECK_OK(out.status());
  std::unique_ptr<arrow::ResizableBuffer> host_out = std::move(*out);
  std::memset(host_out->mutable_data(), 0x5A, nseg * seg);
  CHECK_OK(d->Decompress(0, *comp, host_out));
  CHECK(host_out->size() == n);
  CHECK(std::memcmp(host_out->data(), data.data(), data.size()) == 0);
  CheckSums(d, data, k * seg);
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
  CheckSums(d, data, k * seg);
  CHECK(Total(*comp2) == total);
  StockDecodes(*comp2, data, k * seg, k);
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
  CheckSums(d, data, k * seg);
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
  };
  const Case cases[] = {{"text", TextColumn(5 * 65536 + 4099)},
                        {"records", RecordColumn(5 * 65536 + 4099)}};
  struct Shape {
    std::uint32_t seg;
    std::uint16_t sgl;
  };
  for (const auto& c : cases) {
    for (const Shape s : {Shape{65536, 1}, Shape{59460, 1}, Shape{16384, 4}}) {
      std::size_t lz4 = 0, snappy = 0;
      {
        auto d = NewDevice();
        if (!d) return;
        CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::LZ4, s.seg, s.sgl)));
        auto comp = d->Compress(0, std::make_shared<arrow::Buffer>(
                                       c.data.data(), static_cast<std::int64_t>(c.data.size())));
        CHECK_OK(comp.status());
        if (comp.ok()) lz4 = Total(*comp);
      }
      {
        auto d = NewDevice();
        CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::SNAPPY, s.seg, s.sgl)));
        CHECK(d->encoder_window() == 12);
        CHECK(d->slot_size() >= s.seg + 6u);
        snappy = RoundTrips(d, c.data, s.seg, s.sgl);
      }
      std::cout << c.name << " seg " << s.seg << " x " << s.sgl << ": SNAPPY " << snappy
                << " bytes, LZ4 " << lz4 << " of " << c.data.size() << "\n";
      // the same sequences, so the format alone bounds the difference: a sequence costs Snappy
      // at most one byte more than LZ4 (a literal tag and a 3-byte copy against a token and an
      // offset) and LZ4 at least 3 bytes; a match splits into 3-byte copies per 64 bytes where
      // LZ4 spends a length byte per 255; the preamble and the last literal's tag are <= 6
      // bytes per operation
      const std::size_t nops = (c.data.size() + s.seg * s.sgl - 1) / (s.seg * s.sgl);
      CHECK(snappy > 0 && snappy < c.data.size());
      CHECK(snappy <= lz4 + lz4 / 3 + 3 * c.data.size() / 64 + 6 * nops);
    }
  }
  // noise is stored: the preamble and one literal tag, 6 bytes per whole segment
  {
    auto d = NewDevice();
    CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::SNAPPY, 65536)));
    const auto noise = NoiseColumn(3 * 65536 + 5);
    CHECK(RoundTrips(d, noise, 65536, 1) == noise.size() + 3 * 6 + 2);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "cpu";
  if (mode == "cpu") CpuTests();
  else if (mode == "gpu") GpuTests();
  else {
    std::cerr << "usage: bitar_snappy_test cpu|gpu\n";
    return 2;
  }
  if (g_failures) {
    std::cerr << g_failures << " check(s) failed\n";
    return 1;
  }
  std::cout << "snappy_test " << mode << ": ok\n";
  return 0;
}
