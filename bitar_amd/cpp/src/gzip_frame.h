// gzip_frame.h -- the host side of the GZIP codec's frame (RFC 1952): build the member
// header, walk the members of a stream, validate the segment index, and turn an index into
// bit positions.  Header-only, no Arrow and no HIP includes, so a stand-alone program can
// exercise it (tests/cpp/gzip_frame_check.cc).
//
// Layout written by the codec (one member per buffer):
//   1f 8b 08 04 | MTIME 0 (4) | XFL 0 | OS 255 | XLEN (2) | FEXTRA | raw DEFLATE | CRC-32 | ISIZE
// FEXTRA holds one subfield 'B','T':
//   LE32 segment size | LE32 nseg | nseg x LE24 entry (bits 0..19: the segment's length in
//   bits, bit 23: stored; bits 20..22 zero)
// The raw DEFLATE stream is the join of the segments' streams (csrc/deflate_join.hip); the
// index locates every segment in it by the same model, restated in IndexStarts below, so a
// reader can split the stream and inflate the segments in parallel.  Stock readers skip the
// subfield and see an ordinary gzip member.  An empty buffer is the header with nseg = 0, the
// two bytes 03 00 (an empty final fixed block) and a zero trailer.
//
// Accepted on decode: members with a valid 'BT' index; members whose ISIZE is <= 65536 (any
// stock gzip of a small buffer: one segment); concatenated members when each one's length is
// known, from 'BT' or from the BGZF subfield 'B','C' (BSIZE) -- the last member may run to the
// end of the input.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace bitar {
namespace gzf {

constexpr uint32_t kMaxSeg = 65536;
constexpr uint32_t kStoredBit = 1u << 23, kBitsMask = (1u << 20) - 1, kReservedBits = 7u << 20;
// XLEN is 16 bits: 4 (subfield header) + 8 + 3 * nseg <= 65535
constexpr uint32_t kMaxIndexSegs = (65535 - 12) / 3;

enum class Code { kOk, kInvalid, kNotImplemented };
struct Status {
  Code code = Code::kOk;
  std::string msg;
  bool ok() const { return code == Code::kOk; }
};
inline Status Invalid(std::string m) { return {Code::kInvalid, std::move(m)}; }
inline Status NotImplemented(std::string m) { return {Code::kNotImplemented, std::move(m)}; }

// worst-case bytes of one DEFLATE segment (the engine's slot size: bitar_hip_slot_size for
// the DEFLATE codecs, restated; arrow_codec.cc checks the two agree)
inline uint64_t SlotSize(uint32_t seg) {
  return (((uint64_t)seg * 9 + 7) / 8 + 16 + 255) & ~(uint64_t)255;
}

inline uint32_t Rd16(const uint8_t* p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8; }
inline uint32_t Rd24(const uint8_t* p) { return Rd16(p) | uint32_t(p[2]) << 16; }
inline uint32_t Rd32(const uint8_t* p) { return Rd16(p) | Rd16(p + 2) << 16; }
inline void Wr16(uint8_t* p, uint32_t v) { p[0] = uint8_t(v); p[1] = uint8_t(v >> 8); }
inline void Wr32(uint8_t* p, uint32_t v) { Wr16(p, v); Wr16(p + 2, v >> 16); }

// CRC-32 of header bytes (FHCRC is its low 16 bits); payload CRCs are the device's
inline uint32_t Crc32(const uint8_t* p, uint64_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint64_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int b = 0; b < 8; ++b) c = c & 1u ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  }
  return ~c;
}

// bit position of every segment in the joined stream, and of its end (nseg + 1 values):
//   coded:  pos += bits
//   stored: 3 header bits, then byte-aligned bytes 1..size-1 of the segment's stored blocks
inline void IndexStarts(const std::vector<uint32_t>& entries, std::vector<uint64_t>* starts) {
  starts->resize(entries.size() + 1);
  uint64_t pos = 0;
  for (size_t i = 0; i < entries.size(); ++i) {
    (*starts)[i] = pos;
    const uint64_t bits = entries[i] & kBitsMask;
    if (entries[i] & kStoredBit) pos = ((pos + 3 + 7) & ~7ull) + (bits >= 8 ? bits - 8 : 0);
    else pos += bits;
  }
  (*starts)[entries.size()] = pos;
}

inline uint64_t HeaderLen(uint64_t nseg) { return 10 + 2 + 4 + 8 + 3 * nseg; }
constexpr uint64_t kTrailerLen = 8;
inline uint64_t EmptyMemberLen() { return HeaderLen(0) + 2 + kTrailerLen; }

// the member header for nseg segments of `seg` bytes; entries[i] = bits | stored << 23
// (nseg <= kMaxIndexSegs); out has room for HeaderLen(nseg) bytes
inline void WriteHeader(uint32_t seg, uint32_t nseg, const uint32_t* entries, uint8_t* out) {
  static const uint8_t kFixed[10] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 255};
  std::memcpy(out, kFixed, 10);
  Wr16(out + 10, 4 + 8 + 3 * nseg);
  out[12] = 'B';
  out[13] = 'T';
  Wr16(out + 14, 8 + 3 * nseg);
  Wr32(out + 16, seg);
  Wr32(out + 20, nseg);
  for (uint32_t i = 0; i < nseg; ++i) {
    out[24 + 3 * i] = uint8_t(entries[i]);
    out[25 + 3 * i] = uint8_t(entries[i] >> 8);
    out[26 + 3 * i] = uint8_t(entries[i] >> 16);
  }
}
inline void WriteEmptyMember(uint8_t* out) {
  WriteHeader(kMaxSeg, 0, nullptr, out);
  out[HeaderLen(0)] = 0x03;
  out[HeaderLen(0) + 1] = 0x00;
  std::memset(out + HeaderLen(0) + 2, 0, kTrailerLen);
}

struct Member {
  uint64_t offset = 0, csize = 0;            // the whole member in the input
  uint64_t deflate_off = 0, deflate_len = 0;  // its raw DEFLATE stream
  uint32_t crc = 0, isize = 0;                // trailer
  bool indexed = false;                       // has a valid 'BT' index
  uint32_t seg = 0, nseg = 0;                 // indexed: segment size and count
  std::vector<uint32_t> entries;              // indexed: bits | stored << 23
  std::vector<uint64_t> starts;               // indexed: IndexStarts(entries)
};

// Walk the members of p[0, n).  Every length comes from the (untrusted) input and is checked
// against n before it is used.
inline Status Walk(const uint8_t* p, uint64_t n, std::vector<Member>* out) {
  out->clear();
  uint64_t pos = 0;
  while (pos < n) {
    Member m;
    m.offset = pos;
    if (n - pos < 10) return Invalid("truncated gzip header");
    if (p[pos] != 0x1f || p[pos + 1] != 0x8b) return Invalid("not a gzip member");
    if (p[pos + 2] != 8) return NotImplemented("gzip compression method other than DEFLATE");
    const uint32_t flg = p[pos + 3];
    if (flg & 0xE0u) return Invalid("reserved gzip FLG bits set");
    pos += 10;
    bool has_bt = false, has_bc = false;
    uint64_t bsize = 0;
    if (flg & 4u) {  // FEXTRA
      if (n - pos < 2) return Invalid("truncated gzip header (XLEN)");
      const uint64_t xlen = Rd16(p + pos);
      pos += 2;
      if (n - pos < xlen) return Invalid("gzip XLEN past the end of the input");
      const uint64_t xend = pos + xlen;
      while (pos < xend) {
        if (xend - pos < 4) return Invalid("truncated gzip extra subfield");
        const uint8_t s1 = p[pos], s2 = p[pos + 1];
        const uint64_t len = Rd16(p + pos + 2);
        pos += 4;
        if (xend - pos < len) return Invalid("gzip extra subfield past XLEN");
        if (s1 == 'B' && s2 == 'T') {
          if (has_bt) return Invalid("two BT subfields");
          if (len < 8) return Invalid("BT subfield too short");
          m.seg = Rd32(p + pos);
          m.nseg = Rd32(p + pos + 4);
          if ((len - 8) % 3 != 0 || (len - 8) / 3 != m.nseg)
            return Invalid("BT subfield: nseg does not match its length");
          m.entries.resize(m.nseg);
          for (uint32_t i = 0; i < m.nseg; ++i) m.entries[i] = Rd24(p + pos + 8 + 3 * i);
          has_bt = true;
        } else if (s1 == 'B' && s2 == 'C' && len == 2) {
          bsize = (uint64_t)Rd16(p + pos) + 1;
          has_bc = true;
        }
        pos += len;
      }
    }
    for (uint32_t bit : {8u, 16u}) {  // FNAME, FCOMMENT: zero-terminated
      if (!(flg & bit)) continue;
      const void* z = std::memchr(p + pos, 0, n - pos);
      if (!z) return Invalid("unterminated gzip name or comment");
      pos = (uint64_t)(static_cast<const uint8_t*>(z) - p) + 1;
    }
    if (flg & 2u) {  // FHCRC
      if (n - pos < 2) return Invalid("truncated gzip header (FHCRC)");
      if ((Crc32(p + m.offset, pos - m.offset) & 0xFFFFu) != Rd16(p + pos))
        return Invalid("gzip header CRC mismatch");
      pos += 2;
    }
    m.deflate_off = pos;
    uint64_t end;  // of the member
    if (has_bt) {
      // the index is validated before anything is sized by it
      if (m.seg == 0 || m.seg > kMaxSeg) return Invalid("BT subfield: segment size");
      const uint64_t slot_bits = 8 * SlotSize(m.seg);
      for (uint32_t e : m.entries) {
        const uint32_t bits = e & kBitsMask;
        if ((e & kReservedBits) || bits == 0 || bits > slot_bits)
          return Invalid("BT subfield: entry out of range");
        if ((e & kStoredBit) && ((bits & 7u) || bits < 8 * 5))
          return Invalid("BT subfield: stored entry");
      }
      IndexStarts(m.entries, &m.starts);
      m.deflate_len = m.nseg ? (m.starts[m.nseg] + 7) / 8 : 2;
      if (n - pos < m.deflate_len || n - pos - m.deflate_len < kTrailerLen)
        return Invalid("truncated gzip member (index reaches past the input)");
      end = pos + m.deflate_len + kTrailerLen;
      if (has_bc && bsize != end - m.offset) return Invalid("BT and BC subfields disagree");
      m.indexed = true;
    } else if (has_bc) {
      if (bsize > n - m.offset) return Invalid("BGZF block size past the end of the input");
      end = m.offset + bsize;
      if (end < pos || end - pos < kTrailerLen) return Invalid("BGZF block size too small");
      m.deflate_len = end - pos - kTrailerLen;
    } else {
      if (n - pos < kTrailerLen) return Invalid("truncated gzip trailer");
      end = n;  // the last member runs to the end of the input
      m.deflate_len = end - pos - kTrailerLen;
    }
    m.crc = Rd32(p + end - 8);
    m.isize = Rd32(p + end - 4);
    m.csize = end - m.offset;
    if (m.indexed) {
      if ((uint64_t)m.nseg != ((uint64_t)m.isize + m.seg - 1) / m.seg)
        return Invalid("BT subfield: nseg does not match ISIZE");
      if (m.nseg == 0 && (p[pos] != 0x03 || p[pos + 1] != 0x00))
        return Invalid("empty member: not an empty final block");
    } else if (m.isize > kMaxSeg) {
      return NotImplemented(
          "gzip member above 64 KiB without a BT index (decoded in parallel only with one)");
    }
    out->push_back(std::move(m));
    pos = end;
  }
  return {};
}

}  // namespace gzf
}  // namespace bitar
