// gzip_frame_check -- a stand-alone program over gzip_frame.h alone (host code, no device, no
// Arrow), meant to be built with -fsanitize=address,undefined: it walks every file given, every
// truncation of it and single-byte changes of its header and trailer bytes, each from a heap
// copy of exactly the variant's size, so a read past the input is a sanitizer report.  It also
// checks that WriteHeader / WriteEmptyMember and Walk agree.  Prints one line per file:
//   <file> <OK|Invalid|NotImplemented> members=<n> variants=<n>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "gzip_frame.h"

namespace gzf = bitar::gzf;

static const char* Name(gzf::Code c) {
  return c == gzf::Code::kOk ? "OK" : c == gzf::Code::kInvalid ? "Invalid" : "NotImplemented";
}

// walk an exact-size heap copy; members that parse must lie inside the input
static gzf::Status WalkCopy(const uint8_t* p, size_t n, std::vector<gzf::Member>* ms) {
  std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(copy.get(), p, n);
  const gzf::Status st = gzf::Walk(copy.get(), n, ms);
  if (st.ok()) {
    uint64_t at = 0;
    for (const gzf::Member& m : *ms) {
      if (m.offset != at || m.csize == 0 || m.csize > n - m.offset ||
          m.deflate_off < m.offset || m.deflate_len > m.csize ||
          m.deflate_off - m.offset + m.deflate_len + gzf::kTrailerLen > m.csize ||
          (m.indexed && (m.entries.size() != m.nseg || m.starts.size() != m.nseg + 1ull))) {
        std::fprintf(stderr, "member outside its input\n");
        std::abort();
      }
      at += m.csize;
    }
    if (at != n) {
      std::fprintf(stderr, "members do not cover the input\n");
      std::abort();
    }
  }
  return st;
}

static void SelfCheck() {
  std::vector<uint32_t> entries = {138, 139 | 0, (8 * 69) | gzf::kStoredBit, 141};
  std::vector<uint64_t> starts;
  gzf::IndexStarts(entries, &starts);
  const uint64_t body = (starts.back() + 7) / 8;
  std::vector<uint8_t> m(gzf::HeaderLen(entries.size()) + body + gzf::kTrailerLen, 0);
  gzf::WriteHeader(64, (uint32_t)entries.size(), entries.data(), m.data());
  gzf::Wr32(m.data() + m.size() - 4, 3 * 64 + 5);
  std::vector<gzf::Member> ms;
  gzf::Status st = WalkCopy(m.data(), m.size(), &ms);
  if (!st.ok() || ms.size() != 1 || !ms[0].indexed || ms[0].entries != entries ||
      ms[0].starts != starts || ms[0].deflate_len != body) {
    std::fprintf(stderr, "header round trip: %s\n", st.msg.c_str());
    std::abort();
  }
  std::vector<uint8_t> e(gzf::EmptyMemberLen());
  gzf::WriteEmptyMember(e.data());
  st = WalkCopy(e.data(), e.size(), &ms);
  if (!st.ok() || ms.size() != 1 || ms[0].nseg != 0 || ms[0].isize != 0) {
    std::fprintf(stderr, "empty member: %s\n", st.msg.c_str());
    std::abort();
  }
}

int main(int argc, char** argv) {
  SelfCheck();
  for (int a = 1; a < argc; ++a) {
    std::ifstream f(argv[a], std::ios::binary);
    if (!f) {
      std::fprintf(stderr, "cannot read %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<gzf::Member> ms, tmp;
    const gzf::Status st = WalkCopy(d.data(), d.size(), &ms);
    size_t variants = 0;
    // truncations: every length near the ends and through the header, then strides
    for (size_t n = 0; n < d.size(); n += (n < 300 || d.size() - n < 40) ? 1 : 997) {
      WalkCopy(d.data(), n, &tmp);
      ++variants;
    }
    // single-byte changes in the header (and index) and in the trailer
    std::vector<uint8_t> v = d;
    for (size_t i = 0; i < d.size(); i += (i < 200 || d.size() - i < 16) ? 1 : 4099) {
      for (uint8_t x : {uint8_t(0x00), uint8_t(0xFF), uint8_t(d[i] ^ 0x04), uint8_t(d[i] + 1)}) {
        v[i] = x;
        WalkCopy(v.data(), v.size(), &tmp);
        ++variants;
      }
      v[i] = d[i];
    }
    std::printf("%s %s members=%zu variants=%zu\n", argv[a], Name(st.code), ms.size(), variants);
  }
  return 0;
}
