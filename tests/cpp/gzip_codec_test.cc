// gzip_codec_test -- the GZIP codec of the Arrow adapter (bitar::MakeArrowCodec(GZIP)).
//
//   bitar_gzip_codec_test cpu FILE...     parse each file with gzip_frame.h and print its member
//                                         table, one JSON line per file (no device needed)
//   bitar_gzip_codec_test gpu SCRIPT      run the commands of SCRIPT, one per line, on device 0
//                                         and print one result line per command:
//       compress IN OUT          GPU codec: IN -> one gzip member at OUT
//       decompress IN OUT CAP    GPU codec: IN -> OUT, output buffer of CAP bytes
//       stock IN OUT CAP         Arrow's own GZIP codec (zlib): IN -> OUT
//     result: "OK <bytes>" or "<StatusCode> <message>"
#include <arrow/util/compression.h>

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "bitar/arrow_codec.h"
#include "gzip_frame.h"

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

template <class T>
void PrintList(const char* name, const std::vector<T>& v) {
  std::printf(",\"%s\":[", name);
  for (size_t i = 0; i < v.size(); ++i)
    std::printf("%s%llu", i ? "," : "", static_cast<unsigned long long>(v[i]));
  std::printf("]");
}

int Cpu(int argc, char** argv) {
  namespace gzf = bitar::gzf;
  for (int a = 2; a < argc; ++a) {
    std::vector<uint8_t> data;
    if (!ReadFile(argv[a], &data)) {
      std::fprintf(stderr, "cannot read %s\n", argv[a]);
      return 2;
    }
    std::vector<gzf::Member> ms;
    const gzf::Status st = gzf::Walk(data.data(), data.size(), &ms);
    if (!st.ok()) {
      std::printf("{\"status\":\"%s\",\"msg\":\"%s\"}\n",
                  st.code == gzf::Code::kInvalid ? "Invalid" : "NotImplemented", st.msg.c_str());
      continue;
    }
    std::printf("{\"status\":\"OK\",\"members\":[");
    for (size_t i = 0; i < ms.size(); ++i) {
      const gzf::Member& m = ms[i];
      std::printf("%s{\"offset\":%llu,\"csize\":%llu,\"deflate_off\":%llu,\"deflate_len\":%llu,"
                  "\"crc\":%u,\"isize\":%u,\"indexed\":%d,\"seg\":%u,\"nseg\":%u",
                  i ? "," : "", (unsigned long long)m.offset, (unsigned long long)m.csize,
                  (unsigned long long)(m.deflate_off - m.offset),
                  (unsigned long long)m.deflate_len, m.crc, m.isize, m.indexed ? 1 : 0,
                  m.indexed ? m.seg : 0u, m.indexed ? m.nseg : 0u);
      PrintList("entries", m.indexed ? m.entries : std::vector<uint32_t>());
      PrintList("starts", m.indexed ? m.starts : std::vector<uint64_t>());
      std::printf("}");
    }
    std::printf("]}\n");
  }
  return 0;
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

int Gpu(const char* script) {
  auto made = bitar::MakeArrowCodec(arrow::Compression::GZIP);
  if (!made.ok()) {
    std::printf("MakeArrowCodec: %s\n", made.status().ToString().c_str());
    return 1;
  }
  std::unique_ptr<arrow::util::Codec> gpu = std::move(*made);
  auto stock_made = arrow::util::Codec::Create(arrow::Compression::GZIP);
  if (!stock_made.ok()) {
    std::printf("stock codec: %s\n", stock_made.status().ToString().c_str());
    return 1;
  }
  std::unique_ptr<arrow::util::Codec> stock = std::move(*stock_made);
  std::ifstream f(script);
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream is(line);
    std::string cmd, in, out;
    long long cap = 0;
    is >> cmd >> in >> out >> cap;
    if (cmd.empty()) continue;
    std::vector<uint8_t> data;
    if (!ReadFile(in, &data)) {
      std::printf("IOError cannot read %s\n", in.c_str());
      continue;
    }
    arrow::Result<int64_t> r = arrow::Status::Invalid("unknown command ", cmd);
    std::vector<uint8_t> buf;
    if (cmd == "compress") {
      buf.resize(static_cast<size_t>(gpu->MaxCompressedLen(data.size(), data.data())));
      r = gpu->Compress(static_cast<int64_t>(data.size()), data.data(),
                        static_cast<int64_t>(buf.size()), buf.data());
    } else if (cmd == "decompress" || cmd == "stock") {
      buf.resize(static_cast<size_t>(cap) + 1);  // (+1: a valid pointer for cap 0)
      r = (cmd == "stock" ? stock : gpu)
              ->Decompress(static_cast<int64_t>(data.size()), data.data(), cap, buf.data());
    }
    if (r.ok() && !WriteFile(out, buf.data(), static_cast<size_t>(*r)))
      r = arrow::Status::IOError("cannot write ", out);
    Report(r);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "cpu") return Cpu(argc, argv);
  if (argc == 3 && std::string(argv[1]) == "gpu") return Gpu(argv[2]);
  std::fprintf(stderr, "usage: %s cpu FILE... | gpu SCRIPT\n", argv[0]);
  return 2;
}
