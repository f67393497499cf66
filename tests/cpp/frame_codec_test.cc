// frame_codec_test -- the ZSTD and LZ4_FRAME codecs of the Arrow adapter (bitar::MakeArrowCodec)
// on streams a test builds by hand (tests/test_gpu_frame_codec.py).
//
//   bitar_frame_codec_test gpu SCRIPT    run the commands of SCRIPT, one per line, on device 0
//                                        and print one result line per command:
//       decompress zstd|lz4f IN OUT CAP [fresh]      IN -> OUT, output buffer of CAP bytes
//       hbm_decompress zstd|lz4f IN OUT CAP [fresh]  the same with both buffers in HBM
//     `fresh` makes a new codec for that line (its staging buffers only grow: those an earlier,
//     larger stream left behind would hide a reserve that is too small).
//     result: "ok <bytes>" or "<StatusCode> <message>"
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

void Report(const arrow::Result<int64_t>& r) {
  if (r.ok()) {
    std::printf("ok %lld\n", static_cast<long long>(*r));
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
  std::unique_ptr<arrow::util::Codec> codecs[2];
  const arrow::Compression::type types[2] = {arrow::Compression::ZSTD,
                                             arrow::Compression::LZ4_FRAME};
  for (int k = 0; k < 2; ++k) {
    auto made = bitar::MakeArrowCodec(types[k]);
    if (!made.ok()) {
      std::printf("MakeArrowCodec: %s\n", made.status().ToString().c_str());
      return 1;
    }
    codecs[k] = std::move(*made);
  }
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
    std::string cmd, kind, in, out, opt;
    long long cap = -1;
    is >> cmd >> kind >> in >> out >> cap >> opt;
    if (cmd.empty()) continue;
    std::vector<uint8_t> data;
    if (!ReadFile(in, &data)) {
      std::printf("IOError cannot read %s\n", in.c_str());
      continue;
    }
    const bool hbm = cmd == "hbm_decompress";
    if ((cmd != "decompress" && !hbm) || (kind != "zstd" && kind != "lz4f") || cap < 0 ||
        (!opt.empty() && opt != "fresh")) {
      std::printf("Invalid unknown command: %s\n", line.c_str());
      continue;
    }
    const int k = kind == "zstd" ? 0 : 1;
    std::unique_ptr<arrow::util::Codec> own;
    arrow::util::Codec* codec = codecs[k].get();
    if (opt == "fresh") {
      auto made = bitar::MakeArrowCodec(types[k]);
      if (!made.ok()) {
        Report(made.status());
        continue;
      }
      own = std::move(*made);
      codec = own.get();
    }
    const int64_t n = static_cast<int64_t>(data.size());
    // (one byte behind each buffer: a valid pointer for an empty one)
    data.push_back(0);
    std::vector<uint8_t> buf(static_cast<size_t>(cap) + 1);
    arrow::Result<int64_t> r = arrow::Status::Invalid("unknown command ", cmd);
    if (!hbm) {
      r = codec->Decompress(n, data.data(), cap, buf.data());
    } else {
      Hbm src(ctx, data.size(), &data), dst(ctx, static_cast<uint64_t>(cap), nullptr);
      if (!src.p || !dst.p) {
        r = arrow::Status::OutOfMemory("bitar_hip_alloc");
      } else {
        r = codec->Decompress(n, static_cast<const uint8_t*>(src.p), cap,
                              static_cast<uint8_t*>(dst.p));
        if (r.ok() && *r > 0) {
          bitar_hip_memcpy(ctx, buf.data(), dst.p, static_cast<uint64_t>(*r), nullptr);
          if (bitar_hip_sync(ctx, nullptr) != 0) r = arrow::Status::IOError("copy back");
        }
      }
    }
    if (r.ok() && *r > cap) r = arrow::Status::UnknownError("more bytes than the buffer holds");
    if (r.ok() && !WriteFile(out, buf.data(), static_cast<size_t>(*r)))
      r = arrow::Status::IOError("cannot write ", out);
    Report(r);
  }
  bitar_hip_close(ctx);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && std::string(argv[1]) == "gpu") return Gpu(argv[2]);
  std::fprintf(stderr, "usage: %s gpu SCRIPT\n", argv[0]);
  return 2;
}
