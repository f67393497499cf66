// symtab_test.cc -- Codec::SYMTAB through the C++ front-end.
//   cpu            ToString, the ids, and the configurations Initialize refuses (validation runs
//                  before the device is opened, so no device is needed): chained operations and
//                  a level other than 1; filters and checksums are allowed
//   gpu            CompressDevice round trips -- host and HBM buffers, sync and async calls,
//                  Recycle, segments of 65536 and 59460 bytes, the CRC32 of the caller's bytes on
//                  both sides -- of log lines and of names without a filter (against
//                  Codec::LZ4), a smooth float32 walk behind Filter::SHUFFLE at width 4 and an
//                  int64 counter behind Filter::BITSHUFFLE at width 8; noise comes out stored
// Built twice (release and debug front-end); run by tests/test_gpu_symtab_frontend.py.
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
                                   bitar::Filter filter = bitar::Filter::NONE,
                                   std::uint8_t width = 1) {
  auto c = std::make_unique<Config>(Config::Defaults());
  c->set_codec(codec);
  c->set_decompressed_seg_size32(seg);
  c->set_max_preallocate_memzones(64);
  c->set_checksum_type(bitar::ChecksumType::CRC32);
  if (filter != bitar::Filter::NONE) c->set_filter(filter, width);
  return c;
}

// a device that has not been opened: Initialize validates the configuration first
Device Unopened() {
  auto d = bitar::DeviceManager::Instance()->Create<bitar::Class_HIP_GFX950>(0, {0});
  CHECK_OK(d.status());
  return d.ok() ? Device(*d) : nullptr;
}

void CpuTests() {
  CHECK(bitar::ToString(bitar::Codec::SYMTAB) == "SYMTAB");
  CHECK(static_cast<int>(bitar::Codec::SYMTAB) == 13);
  CHECK(static_cast<int>(bitar::Codec::SNAPPY) == 9 &&
        static_cast<int>(bitar::Codec::CASCADE) == 10);  // appended: the others keep their values
  CHECK(BITAR_HIP_CODEC_SYMTAB == 88);
  Config c;
  c.set_codec(bitar::Codec::SYMTAB);
  CHECK(c.ToString().find("codec: SYMTAB") != std::string::npos);

  {  // no chained ops
    auto d = Unopened();
    if (!d) return;
    auto cfg = MakeConfig(bitar::Codec::SYMTAB, 4096);
    cfg->set_max_sgl_segs(2);
    const auto st = d->Initialize(std::move(cfg));
    CHECK(st.IsInvalid());
    CHECK(st.ToString().find("SYMTAB cannot be combined with chained operations") !=
          std::string::npos);
  }
  for (const std::uint8_t level : {std::uint8_t{0}, std::uint8_t{2}, std::uint8_t{9}}) {  // level 1
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::SYMTAB, 65536);
    cfg->set_level(level);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
  }
  {  // a filter of a width no filter has
    auto d = Unopened();
    CHECK(d->Initialize(MakeConfig(bitar::Codec::SYMTAB, 65536, bitar::Filter::SHUFFLE, 3))
              .IsInvalid());
  }
  // valid configurations pass the validation (without a device the open itself then fails, but
  // not as Invalid): filters and checksums are allowed, a window is ignored whatever it says
  for (const auto filter : {bitar::Filter::NONE, bitar::Filter::SHUFFLE, bitar::Filter::BITSHUFFLE}) {
    for (const std::uint8_t width : {std::uint8_t{2}, std::uint8_t{4}, std::uint8_t{8},
                                     std::uint8_t{16}}) {
      auto d = Unopened();
      auto cfg = MakeConfig(bitar::Codec::SYMTAB, 59460, filter, width);
      cfg->set_window_size(width == 4 ? 3 : 0);
      CHECK(!d->Initialize(std::move(cfg)).IsInvalid());
    }
  }
  // the other codecs' rules are unchanged: CASCADE still takes no filter
  {
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::CASCADE, 65536, bitar::Filter::SHUFFLE, 4);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
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

// log lines of a few words and a number, and names of syllable words
std::vector<std::uint8_t> Lines(std::size_t bytes, std::uint64_t seed, bool names) {
  static const char* const kWords[] = {"GET", "POST", "/api/v1/", "users", "items", "status=",
                                       "200", "404", "INFO", "WARN", "request", "took", "ms",
                                       "host-", "id="};
  static const char* const kSyllables[] = {"an", "ar", "be", "bo", "ca", "chi", "da", "de", "el",
                                           "en", "fa", "fi", "ga", "go", "ha", "hu", "son", "ton",
                                           "lin", "ber", "man", "sen", "ley", "ard", "ett", "ing"};
  std::uint64_t x = seed;
  std::string out;
  while (out.size() < bytes) {
    if (names) {
      for (int word = 0; word < 2; ++word) {
        const int n = 2 + static_cast<int>(SplitMix(&x) % 3);
        for (int k = 0; k < n; ++k) out += kSyllables[SplitMix(&x) % 26];
        out += word ? '\n' : ' ';
      }
    } else {
      for (int k = 0; k < 6; ++k) out += std::string(kWords[SplitMix(&x) % 15]) + " ";
      out += std::to_string(SplitMix(&x) % 100000) + "\n";
    }
  }
  return std::vector<std::uint8_t>(out.begin(), out.begin() + static_cast<std::ptrdiff_t>(bytes));
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
std::vector<std::uint8_t> Counter64(std::size_t bytes, std::uint64_t seed) {
  std::uint64_t x = seed;
  std::vector<std::uint64_t> f(bytes / 8 + 1);
  std::uint64_t at = 1000000;
  for (auto& e : f) e = at += SplitMix(&x) % 3;
  std::vector<std::uint8_t> v(f.size() * 8);
  std::memcpy(v.data(), f.data(), v.size());
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
    bitar::Filter filter;
    std::uint8_t width;
  };
  const Case cases[] = {
      {"log lines", Lines(5 * 65536 + 4099, 7, false), bitar::Filter::NONE, 1},
      {"names", Lines(5 * 65536 + 4099, 7, true), bitar::Filter::NONE, 1},
      {"float32 walk, shuffle 4", FloatWalk(5 * 65536 + 4099, 8), bitar::Filter::SHUFFLE, 4},
      {"int64 counter, bitshuffle 8", Counter64(5 * 65536 + 4099, 9), bitar::Filter::BITSHUFFLE, 8},
  };
  for (const auto& c : cases) {
    for (const std::uint32_t seg : {65536u, 59460u}) {
      std::size_t total[2] = {0, 0};
      const bitar::Codec codecs[2] = {bitar::Codec::LZ4, bitar::Codec::SYMTAB};
      for (int k = 0; k < 2; ++k) {
        auto d = NewDevice();
        if (!d) return;
        auto cfg = MakeConfig(codecs[k], seg, c.filter, c.width);
        if (k == 1) cfg->set_window_size(9);  // ignored
        CHECK_OK(d->Initialize(std::move(cfg)));
        if (k == 1) {
          CHECK(d->encoder_window() == 0);
          CHECK(d->slot_size() >= seg + 4u);
        }
        total[k] = RoundTrips(d, c.data, seg);
      }
      std::cout << c.name << ", seg " << seg << ": SYMTAB " << total[1] << " bytes, LZ4 " << total[0]
                << " of " << c.data.size() << "\n";
      // every case has strings that repeat: the coded form is taken (a stored segment is 4 bytes
      // larger than its input); short strings leave LZ4's four-byte matches little
      CHECK(total[1] > 0 && total[1] < c.data.size());
      if (c.filter == bitar::Filter::NONE) CHECK(total[1] < total[0]);
    }
  }
  // noise is stored: 4 bytes of header per segment
  {
    auto d = NewDevice();
    CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::SYMTAB, 65536)));
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
    std::cerr << "usage: bitar_symtab_test cpu|gpu\n";
    return 2;
  }
  if (g_failures) {
    std::cerr << g_failures << " check(s) failed\n";
    return 1;
  }
  std::cout << "symtab_test " << mode << ": ok\n";
  return 0;
}
