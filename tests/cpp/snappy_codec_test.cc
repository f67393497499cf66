// snappy_codec_test -- the SNAPPY codec of the Arrow adapter (bitar::MakeArrowSnappyCodec).
//
//   bitar_snappy_codec_test cpu           what needs no device: the codec is made, its bound is
//                                         stock Snappy's, streaming is NotImplemented; prints
//                                         one "ok ..." or "FAIL ..." line per check
//   bitar_snappy_codec_test gpu SCRIPT    run the commands of SCRIPT, one per line, on device 0
//                                         and print one result line per command:
//       compress IN OUT [CAP]    GPU codec: IN -> one raw Snappy stream at OUT (output buffer of
//                                CAP bytes; default MaxCompressedLen)
//       decompress IN OUT CAP    GPU codec: IN -> OUT, output buffer of CAP bytes
//       hbm_compress IN OUT      the same two with the input and the output buffer in HBM
//       hbm_decompress IN OUT CAP
//       stock IN OUT CAP         Arrow's own Snappy codec decompresses IN
//       stock_compress IN OUT    Arrow's own Snappy codec compresses IN
//     result: "OK <bytes>" or "<StatusCode> <message>"
#include <arrow/util/compression.h>

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "bitar/arrow_codec.h"
#include "bitar_hip.h"

namespace {

bool ReadFile(const std::string& path, std::vector<uint8_t>* out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  out->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return true;
}

bool WriteFile(const std::string& path, const uint8_t* p, size_t n) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(p), static_cast<std::streamsize>(n));
  return static_cast<bool>(f);
}

int g_failed = 0;
void Check(bool ok, const std::string& what) {
  std::printf("%s %s\n", ok ? "ok" : "FAIL", what.c_str());
  if (!ok) ++g_failed;
}

int Cpu() {
  auto made = bitar::MakeArrowSnappyCodec();
  Check(made.ok(), "MakeArrowSnappyCodec: " + made.status().ToString());
  // (the general factory answers for SNAPPY as it always did)
  Check(bitar::MakeArrowCodec(arrow::Compression::SNAPPY).status().IsNotImplemented(),
        "MakeArrowCodec(SNAPPY) is NotImplemented");
  if (!made.ok()) return 1;
  std::unique_ptr<arrow::util::Codec> codec = std::move(*made);
  Check(codec->compression_type() == arrow::Compression::SNAPPY, "compression_type");
  for (int64_t n : {int64_t{0}, int64_t{1}, int64_t{5}, int64_t{6}, int64_t{65536}, int64_t{65537},
                    int64_t{1} << 30, (int64_t{1} << 32) - 1})
    Check(codec->MaxCompressedLen(n, nullptr) == 32 + n + n / 6,
          "MaxCompressedLen(" + std::to_string(n) + ")");
  Check(codec->MakeCompressor().status().IsNotImplemented(), "MakeCompressor is NotImplemented");
  Check(codec->MakeDecompressor().status().IsNotImplemented(),
        "MakeDecompressor is NotImplemented");
  return g_failed ? 1 : 0;
}

void Report(const arrow::Result<int64_t>& r) {
  if (r.ok()) {
    std::printf("OK %lld\n", static_cast<long long>(*r));
  } else {
    std::string msg = r.status().message();
    for (char& c : msg)
      if (c == '\n') c = ' ';
    std::printf("%s %s\n", r.status().CodeAsString().c_str(), msg.c_str());
  }
  std::fflush(stdout);
}

// a buffer in HBM holding `data`, `room` bytes large (C ABI allocations of a context of its own)
struct Hbm {
  bitar_hip_ctx* ctx;
  void* p = nullptr;
  Hbm(bitar_hip_ctx* c, uint64_t room, const std::vector<uint8_t>* data) : ctx(c) {
    if (bitar_hip_alloc(ctx, room + 16, &p) != 0) p = nullptr;
    if (p && data && !data->empty()) {
      bitar_hip_memcpy(ctx, p, data->data(), data->size(), nullptr);
      bitar_hip_sync(ctx, nullptr);
    }
  }
  ~Hbm() {
    if (p) bitar_hip_free(ctx, p);
  }
};

int Gpu(const char* script) {
  auto made = bitar::MakeArrowSnappyCodec();
  if (!made.ok()) {
    std::printf("MakeArrowSnappyCodec: %s\n", made.status().ToString().c_str());
    return 1;
  }
  std::unique_ptr<arrow::util::Codec> gpu = std::move(*made);
  auto stock_made = arrow::util::Codec::Create(arrow::Compression::SNAPPY);
  if (!stock_made.ok()) {
    std::printf("stock codec: %s\n", stock_made.status().ToString().c_str());
    return 1;
  }
  std::unique_ptr<arrow::util::Codec> stock = std::move(*stock_made);
  bitar_hip_config cfg{1, 0};
  bitar_hip_ctx* ctx = nullptr;
  if (bitar_hip_open(0, &cfg, &ctx) != 0) {
    std::printf("bitar_hip_open: %s\n", bitar_hip_last_error());
    return 1;
  }
  std::ifstream f(script);
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream is(line);
    std::string cmd, in, out;
    long long cap = -1;
    is >> cmd >> in >> out >> cap;
    if (cmd.empty()) continue;
    std::vector<uint8_t> data;
    if (!ReadFile(in, &data)) {
      std::printf("IOError cannot read %s\n", in.c_str());
      continue;
    }
    const int64_t n = static_cast<int64_t>(data.size());
    arrow::Result<int64_t> r = arrow::Status::Invalid("unknown command ", cmd);
    std::vector<uint8_t> buf;
    const bool compress = cmd == "compress" || cmd == "hbm_compress" || cmd == "stock_compress";
    if (compress && cap < 0)
      cap = (cmd == "stock_compress" ? stock : gpu)->MaxCompressedLen(n, data.data());
    buf.resize(static_cast<size_t>(cap < 0 ? 0 : cap) + 1);  // (+1: a valid pointer for cap 0)
    if (cmd == "compress") {
      r = gpu->Compress(n, data.data(), cap, buf.data());
    } else if (cmd == "stock_compress") {
      r = stock->Compress(n, data.data(), cap, buf.data());
    } else if (cmd == "decompress") {
      r = gpu->Decompress(n, data.data(), cap, buf.data());
    } else if (cmd == "stock") {
      r = stock->Decompress(n, data.data(), cap, buf.data());
    } else if (cmd == "hbm_compress" || cmd == "hbm_decompress") {
      Hbm src(ctx, data.size(), &data), dst(ctx, static_cast<uint64_t>(cap), nullptr);
      if (!src.p || !dst.p) {
        r = arrow::Status::OutOfMemory("bitar_hip_alloc");
      } else {
        const auto* s = static_cast<const uint8_t*>(src.p);
        auto* d = static_cast<uint8_t*>(dst.p);
        r = compress ? gpu->Compress(n, s, cap, d) : gpu->Decompress(n, s, cap, d);
        if (r.ok() && *r > 0) {
          bitar_hip_memcpy(ctx, buf.data(), dst.p, static_cast<uint64_t>(*r), nullptr);
          if (bitar_hip_sync(ctx, nullptr) != 0) r = arrow::Status::IOError("copy back");
        }
      }
    }
    if (r.ok() && !WriteFile(out, buf.data(), static_cast<size_t>(*r)))
      r = arrow::Status::IOError("cannot write ", out);
    Report(r);
  }
  bitar_hip_close(ctx);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "cpu") return Cpu();
  if (argc == 3 && std::string(argv[1]) == "gpu") return Gpu(argv[2]);
  std::fprintf(stderr, "usage: %s cpu | gpu SCRIPT\n", argv[0]);
  return 2;
}
