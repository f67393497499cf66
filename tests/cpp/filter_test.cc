// filter_test.cc -- the segment filters (bitar::Filter) through the C++ front-end.
//   cpu            the configuration's setters, defaults and ToString (no device)
//   gpu            CompressDevice round trips with a filter for the three codecs, host and HBM
//                  buffers, both filters, widths 8 and 4, segments of 65536 and 59460 bytes; the
//                  compressed total against Filter::NONE; the CRC32 of the caller's bytes on
//                  both sides; the rejected configurations; explicit NONE against the default
// Run by tests/test_gpu_filter_frontend.py.
#include <arrow/buffer.h>
#include <arrow/memory_pool.h>

#include <cstdint>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "bitar/bitar.h"

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

std::unique_ptr<Config> MakeConfig(bitar::Codec codec, std::uint32_t seg) {
  auto c = std::make_unique<Config>(Config::Defaults());
  c->set_codec(codec);
  c->set_decompressed_seg_size32(seg);
  c->set_max_preallocate_memzones(64);
  c->set_checksum_type(bitar::ChecksumType::CRC32);
  return c;
}

void CpuTests() {
  Config c;
  CHECK(c.filter() == bitar::Filter::NONE && c.element_width() == 1);
  CHECK(c.ToString().find("filter: NONE/1") != std::string::npos);
  CHECK(c.ToString().find("level: 1") != std::string::npos);
  CHECK(c.ToString().find("checksum_type: NONE") != std::string::npos);
  c.set_filter(bitar::Filter::BITSHUFFLE, 8);
  CHECK(c.filter() == bitar::Filter::BITSHUFFLE && c.element_width() == 8);
  CHECK(c.ToString().find("filter: BITSHUFFLE/8") != std::string::npos);
  c.set_filter(bitar::Filter::SHUFFLE, 16);
  CHECK(c.ToString().find("filter: SHUFFLE/16") != std::string::npos);
  CHECK(bitar::ToString(bitar::Filter::NONE) == "NONE");
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

// an int64 column of small-range values (SplitMix64), cut at an odd byte count
std::vector<std::uint8_t> Int64Column(std::size_t bytes) {
  std::vector<std::uint8_t> v(bytes + 8);
  std::uint64_t x = 0x9E3779B97F4A7C15ull;
  for (std::size_t i = 0; i + 8 <= v.size(); i += 8) {
    x += 0x9E3779B97F4A7C15ull;
    std::uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const std::int64_t value = 1000000 + static_cast<std::int64_t>(z % 4096);
    std::memcpy(&v[i], &value, 8);
  }
  v.resize(bytes);
  return v;
}

std::vector<std::uint8_t> ToHost(const bitar::BufferVector& bufs) {
  std::vector<std::uint8_t> all;
  for (const auto& b : bufs) {
    auto view = std::make_shared<arrow::Buffer>(reinterpret_cast<const std::uint8_t*>(b->address()),
                                                b->size(), b->memory_manager());
    auto copied = arrow::Buffer::Copy(view, arrow::default_cpu_memory_manager());
    CHECK_OK(copied.status());
    if (!copied.ok()) return all;
    const auto size = static_cast<std::uint32_t>(b->size());
    const auto* s = reinterpret_cast<const std::uint8_t*>(&size);
    all.insert(all.end(), s, s + 4);
    all.insert(all.end(), (*copied)->data(), (*copied)->data() + size);
  }
  return all;
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

// host -> slots -> host and HBM -> slots -> HBM on one device; the total of the compressed sizes
std::size_t RoundTrips(const Device& d, const std::vector<std::uint8_t>& data, std::uint32_t seg,
                       std::vector<std::uint8_t>* slots) {
  const auto n = static_cast<std::int64_t>(data.size());
  const std::size_t nseg = (data.size() + seg - 1) / seg;
  auto host_in = std::make_shared<arrow::Buffer>(data.data(), n);
  auto comp = d->Compress(0, host_in);
  CHECK_OK(comp.status());
  if (!comp.ok()) return 0;
  CHECK(comp->size() == nseg);
  CheckSums(d, data, seg);
  std::size_t total = 0;
  for (const auto& b : *comp) total += static_cast<std::size_t>(b->size());
  if (slots) *slots = ToHost(*comp);
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
  auto comp2 = d->Compress(0, *dev_in);
  CHECK_OK(comp2.status());
  if (!comp2.ok()) return total;
  CheckSums(d, data, seg);
  std::size_t total2 = 0;
  for (const auto& b : *comp2) total2 += static_cast<std::size_t>(b->size());
  CHECK(total2 == total);
  auto dev_out = bitar::AllocateResizableDeviceBuffer(static_cast<std::int64_t>(nseg * seg), 0);
  CHECK_OK(dev_out.status());
  std::unique_ptr<arrow::ResizableBuffer> dout = std::move(*dev_out);
  CHECK_OK(d->Decompress(0, *comp2, dout));
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
  const auto data = Int64Column(5 * 65536 + 4099);
  for (const auto codec : {bitar::Codec::DEFLATE, bitar::Codec::LZ4, bitar::Codec::ZSTD}) {
    for (const std::uint32_t seg : {65536u, 59460u}) {
      // the default configuration, and Filter::NONE set explicitly: the same slots
      std::vector<std::uint8_t> plain_slots, none_slots;
      std::size_t plain = 0;
      {
        auto d = NewDevice();
        if (!d) return;
        CHECK_OK(d->Initialize(MakeConfig(codec, seg)));
        plain = RoundTrips(d, data, seg, &plain_slots);
      }
      {
        auto d = NewDevice();
        auto cfg = MakeConfig(codec, seg);
        cfg->set_filter(bitar::Filter::NONE, 1);
        CHECK_OK(d->Initialize(std::move(cfg)));
        CHECK(RoundTrips(d, data, seg, &none_slots) == plain);
        CHECK(!plain_slots.empty() && none_slots == plain_slots);
      }
      for (const auto filter : {bitar::Filter::SHUFFLE, bitar::Filter::BITSHUFFLE}) {
        for (const std::uint8_t width : {std::uint8_t{8}, std::uint8_t{4}}) {
          auto d = NewDevice();
          auto cfg = MakeConfig(codec, seg);
          cfg->set_filter(filter, width);
          CHECK_OK(d->Initialize(std::move(cfg)));
          std::vector<std::uint8_t> slots;
          const std::size_t total = RoundTrips(d, data, seg, &slots);
          std::cout << "codec " << bitar::ToString(codec) << " seg " << seg << " filter "
                    << bitar::ToString(filter) << "/" << +width << ": " << total << " bytes (plain "
                    << plain << ")\n";
          CHECK(total > 0 && slots != plain_slots);
          // the int64 column at its own width: the filter pays
          if (width == 8) CHECK(total < plain);
        }
      }
    }
  }
  // rejected configurations
  for (const std::uint8_t width : {std::uint8_t{0}, std::uint8_t{1}, std::uint8_t{3},
                                   std::uint8_t{12}, std::uint8_t{32}}) {
    auto d = NewDevice();
    auto cfg = MakeConfig(bitar::Codec::LZ4, 65536);
    cfg->set_filter(bitar::Filter::SHUFFLE, width);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
  }
  {
    auto d = NewDevice();
    auto cfg = MakeConfig(bitar::Codec::LZ4, 4096);
    cfg->set_filter(bitar::Filter::BITSHUFFLE, 8);
    cfg->set_max_sgl_segs(2);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
    // ... and the same chained configuration without a filter is fine
    auto d2 = NewDevice();
    auto cfg2 = MakeConfig(bitar::Codec::LZ4, 4096);
    cfg2->set_filter(bitar::Filter::NONE, 8);
    cfg2->set_max_sgl_segs(2);
    CHECK_OK(d2->Initialize(std::move(cfg2)));
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "cpu";
  if (mode == "cpu") CpuTests();
  else if (mode == "gpu") GpuTests();
  else {
    std::cerr << "usage: bitar_filter_test cpu|gpu\n";
    return 2;
  }
  if (g_failures) {
    std::cerr << g_failures << " check(s) failed\n";
    return 1;
  }
  std::cout << "filter_test " << mode << ": ok\n";
  return 0;
}
