// runpack_test.cc -- Codec::RUNPACK through the C++ front-end.
//   cpu            ToString, the ids, and the configurations Initialize refuses (validation runs
//                  before the device is opened, so no device is needed)
//   gpu            CompressDevice round trips of run-shaped columns -- sorted int64 timestamps of
//                  50 values (width 8), 16-byte ids in runs of about 500 (width 16), flag bytes
//                  in runs of about 200 (width 1), int32 keys in runs of about 20 (width 4) --
//                  host and HBM buffers, sync and async calls, Recycle, segments of 65536 and
//                  59460 bytes; the CRC32 of the caller's bytes on both sides; the compressed
//                  total against Codec::LZ4 and against what the format's size formula allows;
//                  noise comes out stored
// Built twice (release and debug front-end); run by tests/test_gpu_runpack_frontend.py.
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
  CHECK(bitar::ToString(bitar::Codec::RUNPACK) == "RUNPACK");
  CHECK(static_cast<int>(bitar::Codec::RUNPACK) == 7);
  CHECK(BITAR_HIP_CODEC_RUNPACK(1) == 32 && BITAR_HIP_CODEC_RUNPACK(2) == 33 &&
        BITAR_HIP_CODEC_RUNPACK(4) == 34 && BITAR_HIP_CODEC_RUNPACK(8) == 35 &&
        BITAR_HIP_CODEC_RUNPACK(16) == 36);
  Config c;
  c.set_codec(bitar::Codec::RUNPACK);
  c.set_element_width(16);
  CHECK(c.element_width() == 16 && c.filter() == bitar::Filter::NONE);
  CHECK(c.ToString().find("codec: RUNPACK") != std::string::npos);

  // element_width outside {1, 2, 4, 8, 16}
  for (const std::uint8_t width : {std::uint8_t{0}, std::uint8_t{3}, std::uint8_t{5},
                                   std::uint8_t{12}, std::uint8_t{32}, std::uint8_t{255}}) {
    auto d = Unopened();
    if (!d) return;
    CHECK(d->Initialize(MakeConfig(bitar::Codec::RUNPACK, 65536, width)).IsInvalid());
  }
  for (const auto filter : {bitar::Filter::SHUFFLE, bitar::Filter::BITSHUFFLE}) {  // no filter
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::RUNPACK, 65536, 8);
    cfg->set_filter(filter, 8);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
  }
  {  // no chained ops
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::RUNPACK, 4096, 4);
    cfg->set_max_sgl_segs(2);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
  }
  for (const std::uint8_t level : {std::uint8_t{0}, std::uint8_t{2}, std::uint8_t{9}}) {  // level 1
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::RUNPACK, 65536, 16);
    cfg->set_level(level);
    CHECK(d->Initialize(std::move(cfg)).IsInvalid());
  }
  // valid configurations pass the validation (without a device the open itself then fails, but
  // not as Invalid); a window is ignored, whatever it says
  for (const std::uint8_t width : {std::uint8_t{1}, std::uint8_t{2}, std::uint8_t{4},
                                   std::uint8_t{8}, std::uint8_t{16}}) {
    auto d = Unopened();
    auto cfg = MakeConfig(bitar::Codec::RUNPACK, 59460, width);
    cfg->set_window_size(width == 4 ? 3 : 0);
    CHECK(!d->Initialize(std::move(cfg)).IsInvalid());
  }
  // the other codecs' rules are unchanged: FLTPACK and INTPACK still refuse 16-byte elements,
  // the dictionary codec still refuses 1-byte ones and takes 16-byte ones
  {
    auto d = Unopened();
    CHECK(d->Initialize(MakeConfig(bitar::Codec::FLTPACK, 65536, 16)).IsInvalid());
    auto e = Unopened();
    CHECK(e->Initialize(MakeConfig(bitar::Codec::INTPACK, 65536, 16)).IsInvalid());
    auto f = Unopened();
    CHECK(f->Initialize(MakeConfig(bitar::Codec::DICTPACK, 65536, 1)).IsInvalid());
    auto g = Unopened();
    CHECK(!g->Initialize(MakeConfig(bitar::Codec::DICTPACK, 65536, 16)).IsInvalid());
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

// `bytes` bytes of elements of `width` bytes in runs of one of `distinct` values (all bytes
// random).  sorted: the values in order, each in one stretch, as a sorted column has them;
// else a run's length is uniform in [1, 2 * mean - 1] and its value never that of the run
// before.  Cut at an odd byte count.  *runs = the number of runs written.
std::vector<std::uint8_t> RunColumn(std::size_t bytes, std::size_t width, std::size_t distinct,
                                    std::size_t mean, bool sorted, std::uint64_t seed,
                                    std::size_t* runs) {
  std::uint64_t x = seed;
  std::vector<std::uint8_t> values(distinct * width);
  for (auto& b : values) b = static_cast<std::uint8_t>(SplitMix(&x) >> 56);
  for (std::size_t k = 0; k < distinct; ++k) {  // (distinct for certain)
    values[k * width] = static_cast<std::uint8_t>(k);
    if (width > 1) values[k * width + 1] = static_cast<std::uint8_t>(k >> 8);
  }
  const std::size_t m = bytes / width + 1;
  std::vector<std::uint8_t> v(m * width);
  std::size_t at = 0, value = 0;
  *runs = 0;
  while (at < m) {
    std::size_t len = sorted ? (m + distinct - 1) / distinct : 1 + SplitMix(&x) % (2 * mean - 1);
    if (len > m - at) len = m - at;
    if (sorted) value = *runs % distinct;
    else value = (value + 1 + SplitMix(&x) % (distinct - 1)) % distinct;
    for (std::size_t i = 0; i < len; ++i)
      std::memcpy(&v[(at + i) * width], &values[value * width], width);
    at += len;
    ++*runs;
  }
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
    std::uint8_t width;
    std::size_t distinct, mean;
    bool sorted;
    std::vector<std::uint8_t> data;
    std::size_t runs;
  };
  Case cases[] = {{"sorted int64 timestamps, 50 values", 8, 50, 0, true, {}, 0},
                  {"16-byte ids, runs of about 500", 16, 4000, 500, false, {}, 0},
                  {"flag bytes, runs of about 200", 1, 2, 200, false, {}, 0},
                  {"int32 keys, runs of about 20", 4, 1000, 20, false, {}, 0}};
  for (auto& c : cases)
    c.data = RunColumn(5 * 65536 + 4099, c.width, c.distinct, c.mean, c.sorted, 7 + c.width,
                       &c.runs);
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
        auto cfg = MakeConfig(bitar::Codec::RUNPACK, seg, c.width);
        cfg->set_window_size(9);  // ignored
        CHECK_OK(d->Initialize(std::move(cfg)));
        CHECK(d->encoder_window() == 0);
        CHECK(d->slot_size() >= seg + 4u);
        packed = RoundTrips(d, c.data, seg);
      }
      std::cout << c.name << " seg " << seg << ": RUNPACK " << packed << " bytes, LZ4 " << lz4
                << " of " << c.data.size() << "\n";
      // What the size formula allows (include/bitar_hip.h): per segment 6 bytes and a tail below
      // the width; per run a value and a length of at most 2 bytes.  A segment border cuts at
      // most one run in two, and in a segment that starts inside an element (59460 is no
      // multiple of 8 or 16) every run is still one run of the shifted elements, with one
      // element of its own between it and the next.
      const std::size_t nseg = (c.data.size() + seg - 1) / seg;
      const std::size_t shifted = seg % c.width == 0 ? 1 : 2;
      const std::size_t bound =
          nseg * (6 + c.width) + (shifted * c.runs + 2 * nseg) * (c.width + 2);
      CHECK(packed > 0 && packed < lz4 && packed <= bound);
    }
  }
  // noise is stored: 4 bytes of header per segment
  {
    auto d = NewDevice();
    CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::RUNPACK, 65536, 8)));
    const auto noise = NoiseColumn(3 * 65536 + 5);
    CHECK(RoundTrips(d, noise, 65536) == noise.size() + 4 * 4);
  }
  // another width still round-trips (it only packs worse, or not at all)
  {
    auto d = NewDevice();
    CHECK_OK(d->Initialize(MakeConfig(bitar::Codec::RUNPACK, 59460, 2)));
    CHECK(RoundTrips(d, cases[0].data, 59460) > 0);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "cpu";
  if (mode == "cpu") CpuTests();
  else if (mode == "gpu") GpuTests();
  else {
    std::cerr << "usage: bitar_runpack_test cpu|gpu\n";
    return 2;
  }
  if (g_failures) {
    std::cerr << g_failures << " check(s) failed\n";
    return 1;
  }
  std::cout << "runpack_test " << mode << ": ok\n";
  return 0;
}
