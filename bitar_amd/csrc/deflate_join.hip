// deflate_join.hip -- ONE raw DEFLATE stream (RFC 1951) from the per-segment streams of the two
// DEFLATE compressors, its inverse, and the CRC-32 of a buffer from its segments' CRC-32s: what
// a gzip member (RFC 1952) needs on top of the segment codec (gfx950).
//
// What the compressors guarantee (compress.hip deflate_compress_kernel, deflate_dyn.hip
// deflate_dyn_emit_kernel; bits[] is their optional output):
//   a CODED segment is exactly one block, BFINAL at bit 0 of byte 0, bits[i] bits long up to
//   and including its end-of-block code;
//   a STORED segment is ceil(n / 65535) byte-aligned stored blocks (n <= 65536: one or two),
//   bits[i] = 8 * sizes[i]; its header bytes are 0 except the last block's, which is 1.
// BTYPE (bits 1..2 of byte 0) tells the two apart: 00 is stored.
//
// The join, stated sequentially:
//   pos = 0
//   for i in 0..nseg-1:
//     starts[i] = pos
//     coded:  copy bits[i] bits to pos, bit 0 cleared unless i is last;      pos += bits[i]
//     stored: 3 header bits at pos (BFINAL = i is last and the segment is one block, BTYPE 00);
//             pos = align8(pos + 3); copy bytes 1..size-1 there (a second block's header byte:
//             1 only if i is last);                                           pos += 8*(size-1)
//   starts[nseg] = pos; the stream is ceil(pos / 8) bytes, padding bits zero
// A segment moves pos by an amount that depends on pos & 7 only, so the scan composes
// 8-entry tables (join_scan_kernel); the copies then run one wave per segment.
//
// Output dwords are written in two ways only: a dword that a segment covers completely is
// stored plainly by that segment's wave, every other dword (the first and last of a coded
// segment, the head and tail of a stored body, a stored header bit) is merged with atomicOr
// into the output the caller's memset zeroed.  So a dword is either owned by one wave or
// touched by atomics alone, however many segments share it.
#include "kernels.hip.h"
#include "crc32.hip.h"
#include "wave.hip.h"

namespace bitar_hip {

namespace dj {

constexpr uint32_t kScanTile = 512;
constexpr uint32_t kStoredFlag = 1u << 23;  // split entries: bits | stored << 23
constexpr uint32_t kBitsMask = kStoredFlag - 1;
// a stored slot of more than 5 + 65535 bytes holds two blocks; the second header starts here
constexpr uint32_t kSecondHdr = 65540;

struct Seg {
  uint32_t size, bits;
  bool ok, stored;
};

// segment i as the compressors left it; anything else (a failed op's SEGMENT_ERROR, a size
// above the slot, sizes[] and bits[] that disagree) is not ok and joins as nothing
__device__ __forceinline__ Seg classify(const uint8_t* __restrict__ slab, uint64_t stride,
                                        const uint32_t* __restrict__ sizes,
                                        const uint32_t* __restrict__ bits, uint32_t i) {
  Seg s;
  s.size = sizes[i];
  s.bits = bits[i];
  s.ok = s.size != 0 && (uint64_t)s.size <= stride && s.bits != 0 &&
         ((uint64_t)s.bits + 7) >> 3 == s.size;
  s.stored = false;
  if (s.ok) {
    s.stored = (slab[(uint64_t)i * stride] & 6u) == 0;
    if (s.stored && (s.bits != s.size * 8u || s.size < 5)) s.ok = false;
  }
  return s;
}

// bits segment s adds to a stream that stands at phase p = pos & 7
__device__ __forceinline__ uint32_t advance(const Seg& s, uint32_t p) {
  if (!s.ok) return 0;
  if (!s.stored) return s.bits;
  return (((p + 3u + 7u) & ~7u) - p) + 8u * (s.size - 1);
}

}  // namespace dj

// starts[i] = bit position of segment i in the joined stream, starts[nseg] = its length.
// One workgroup; tiles of kScanTile segments, the position carried from tile to tile.  Inside
// a tile an inclusive Hillis-Steele scan composes the segments' tables f[p] = bits added when
// entered at phase p: (A then B)[p] = A[p] + B[(p + A[p]) & 7].
__global__ __launch_bounds__(dj::kScanTile) void join_scan_kernel(
    const uint8_t* __restrict__ slab, uint64_t stride, const uint32_t* __restrict__ sizes,
    const uint32_t* __restrict__ bits, uint32_t nseg, uint64_t capacity,
    uint64_t* __restrict__ starts, uint32_t* __restrict__ err) {
  using namespace dj;
  __shared__ uint32_t f[2][8][kScanTile];
  __shared__ uint64_t carry;
  const uint32_t t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nseg; base += kScanTile) {
    const uint32_t idx = base + t;
    Seg s{0u, 0u, false, false};
    if (idx < nseg) {
      s = classify(slab, stride, sizes, bits, idx);
      if (!s.ok) atomicOr(err, 4u);
    }
#pragma unroll
    for (uint32_t p = 0; p < 8; ++p) f[0][p][t] = advance(s, p);
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t d = 1; d < kScanTile; d <<= 1) {
#pragma unroll
      for (uint32_t p = 0; p < 8; ++p) {
        uint32_t v;
        if (t >= d) {
          const uint32_t a = f[cur][p][t - d];
          v = a + f[cur][(p + a) & 7u][t];
        } else {
          v = f[cur][p][t];
        }
        f[cur ^ 1][p][t] = v;
      }
      __syncthreads();
      cur ^= 1;
    }
    const uint64_t c = carry;
    const uint32_t ph = (uint32_t)c & 7u;
    if (idx < nseg) starts[idx] = c + (t ? f[cur][ph][t - 1] : 0u);
    __syncthreads();
    if (t == kScanTile - 1) carry = c + f[cur][ph][t];
    __syncthreads();
  }
  if (t == 0) {
    starts[nseg] = carry;
    if ((carry + 7) >> 3 > capacity) atomicOr(err, 2u);
  }
}

namespace dj {

// len bytes from s to byte offset at of the zeroed output: the bytes of the first and last
// partial dwords by atomicOr, the dword-aligned middle by a plain wave copy
__device__ __forceinline__ void put_bytes(uint32_t* out, uint64_t at, const GMEM uint8_t* s,
                                          uint32_t len) {
  const uint32_t lane = lane_id();
  uint32_t head = (uint32_t)((4u - (at & 3u)) & 3u);
  if (head > len) head = len;
  if (lane < head) {
    const uint64_t b = at + lane;
    atomicOr(out + (b >> 2), (uint32_t)s[lane] << (8u * ((uint32_t)b & 3u)));
  }
  const uint32_t tail = (len - head) & 3u, mid = len - head - tail;
  if (mid)
    wave_copy_global(global_ptr(reinterpret_cast<uint8_t*>(out)) + at + head, s + head, mid);
  if (lane < tail) {
    const uint64_t b = at + head + mid + lane;
    atomicOr(out + (b >> 2), (uint32_t)s[head + mid + lane] << (8u * ((uint32_t)b & 3u)));
  }
}

}  // namespace dj

// one wave per segment: segment i's bits to starts[i] of the zeroed output (`out`, 4-B
// aligned).  A segment that would end past `capacity` bytes is not written at all (the scan
// has flagged the call).
__global__ __launch_bounds__(64) void deflate_join_kernel(
    const uint8_t* __restrict__ slab, uint64_t stride, const uint32_t* __restrict__ sizes,
    const uint32_t* __restrict__ bits, uint32_t nseg, const uint64_t* __restrict__ starts,
    uint32_t* __restrict__ out, uint64_t capacity) {
  using namespace dj;
  const uint32_t i = blockIdx.x;
  if (i >= nseg) return;
  const uint32_t lane = lane_id();
  const Seg s = classify(slab, stride, sizes, bits, i);
  if (!s.ok) return;
  const uint64_t pos = starts[i];
  if ((starts[i + 1] + 7) >> 3 > capacity) return;
  const bool last = i + 1 == nseg;
  const GMEM uint8_t* slot = global_ptr(slab + (uint64_t)i * stride);
  if (s.stored) {
    const bool two = s.size > kSecondHdr;
    if (last && !two && lane == 0) atomicOr(out + (pos >> 5), 1u << ((uint32_t)pos & 31u));
    const uint64_t at = (pos + 3 + 7) >> 3;
    if (!two) {
      put_bytes(out, at, slot + 1, s.size - 1);
    } else {
      put_bytes(out, at, slot + 1, kSecondHdr - 1);
      if (last && lane == 0) {
        const uint64_t b = at + kSecondHdr - 1;
        atomicOr(out + (b >> 2), 1u << (8u * ((uint32_t)b & 3u)));
      }
      put_bytes(out, at + kSecondHdr, slot + kSecondHdr + 1, s.size - kSecondHdr - 1);
    }
    return;
  }
  // coded: output dword w0 + k = source dwords k-1 and k funnelled by pos & 31
  const GMEM uint32_t* src = reinterpret_cast<const GMEM uint32_t*>(slot);
  const uint32_t nb = s.bits, sh = (uint32_t)pos & 31u;
  const uint64_t w0 = pos >> 5;
  const uint32_t nw = (uint32_t)(((pos + nb - 1) >> 5) - w0) + 1;
  const uint32_t nsrc = (nb + 31) >> 5;
  auto get = [&](uint32_t j) -> uint32_t {  // source dword j, limited to the block's bits
    if (j >= nsrc) return 0u;               // (j = k - 1 wraps for k = 0)
    uint32_t x = src[j];
    if (j == nsrc - 1 && (nb & 31u)) x &= (1u << (nb & 31u)) - 1u;
    if (j == 0 && !last) x &= ~1u;          // BFINAL
    return x;
  };
  for (uint32_t k = lane; k < nw; k += kWave) {
    uint32_t v = get(k) << sh;
    if (sh) v |= get(k - 1) >> (32u - sh);
    if (k == 0 || k == nw - 1) atomicOr(out + w0 + k, v);
    else out[w0 + k] = v;
  }
}

namespace dj {

// dword w of the joined stream (len bytes, 4-B aligned base); bytes past len read as 0 and
// are never loaded
__device__ __forceinline__ uint32_t load_dword(const GMEM uint8_t* j, uint64_t w, uint64_t len) {
  const uint64_t b = w * 4;
  if (b + 4 <= len) return reinterpret_cast<const GMEM uint32_t*>(j)[w];
  uint32_t v = 0;
  for (uint32_t k = 0; k < 4; ++k)
    if (b + k < len) v |= (uint32_t)j[b + k] << (8u * k);
  return v;
}

}  // namespace dj

// The inverse: slot i = the segment at starts[i] of the joined stream, as the compressors
// wrote it (BFINAL set again), sizes[i] its bytes.  entries[i] = bits | stored << 23 with
// bits = 8 * size for a stored segment.  starts[] and entries[] are untrusted: an entry that
// reaches past 8 * joined_len bits or whose size exceeds the slot marks sizes[i] with
// BITAR_HIP_SEGMENT_ERROR and sets the error word; nothing is read or written for it.
__global__ __launch_bounds__(64) void deflate_split_kernel(
    const uint8_t* __restrict__ joined, uint64_t joined_len, const uint64_t* __restrict__ starts,
    const uint32_t* __restrict__ entries, uint32_t nseg, uint8_t* __restrict__ slab,
    uint64_t stride, uint32_t* __restrict__ sizes, uint32_t* __restrict__ err) {
  using namespace dj;
  const uint32_t i = blockIdx.x;
  if (i >= nseg) return;
  const uint32_t lane = lane_id();
  const uint64_t pos = starts[i], total = joined_len * 8;
  const uint32_t e = entries[i], nb = e & kBitsMask;
  const bool stored = (e & kStoredFlag) != 0;
  const uint32_t size = (nb + 7) >> 3;
  const GMEM uint8_t* j = global_ptr(joined);
  GMEM uint8_t* slot = global_ptr(slab + (uint64_t)i * stride);
  bool ok = (e >> 24) == 0 && nb != 0 && (uint64_t)size <= stride && pos <= total;
  uint64_t at = 0;
  if (ok && stored) {
    at = (pos + 3 + 7) >> 3;  // (pos <= total < 2^63: no wrap)
    ok = (nb & 7u) == 0 && size >= 5 && at <= joined_len && size - 1 <= joined_len - at;
  } else if (ok) {
    ok = nb <= total - pos;
  }
  if (!ok) {
    if (lane == 0) {
      sizes[i] = 0xFFFFFFFFu;
      atomicOr(err, 1u);
    }
    return;
  }
  if (stored) {
    const bool two = size > kSecondHdr;
    if (lane == 0) slot[0] = two ? 0 : 1;
    if (!two) {
      wave_copy_global(slot + 1, j + at, size - 1);
    } else {
      wave_copy_global(slot + 1, j + at, kSecondHdr - 1);
      if (lane == 0) slot[kSecondHdr] = 1;
      wave_copy_global(slot + kSecondHdr + 1, j + at + kSecondHdr, size - kSecondHdr - 1);
    }
  } else {
    GMEM uint32_t* dst = reinterpret_cast<GMEM uint32_t*>(slot);
    const uint32_t sh = (uint32_t)pos & 31u, ndst = (nb + 31) >> 5;
    const uint64_t w0 = pos >> 5;
    for (uint32_t k = lane; k < ndst; k += kWave) {
      uint32_t v = load_dword(j, w0 + k, joined_len) >> sh;
      if (sh) v |= load_dword(j, w0 + k + 1, joined_len) << (32u - sh);
      if (k == ndst - 1 && (nb & 31u)) v &= (1u << (nb & 31u)) - 1u;
      if (k == 0) v |= 1u;  // BFINAL
      dst[k] = v;           // (whole dwords: the slot is 16-B aligned and a multiple of 16 B)
    }
  }
  if (lane == 0) sizes[i] = size;
}

// crc[0] = CRC-32 of n bytes from the CRC-32s of their nseg = ceil(n / seg) segments (the low
// words of sums[], as checksum_kernel writes them): XOR over segments of
// x^(8 * bytes after the segment) * crc(segment) mod P.  One workgroup; thread t takes segments
// t, t + 256, ... from the back, so its factor grows by the constant x^(8 * 256 * seg) per
// step (x has order 2^32 - 1 at most: exponents reduce modulo that).
__global__ __launch_bounds__(256) void crc32_combine_kernel(const uint64_t* __restrict__ sums,
                                                            uint64_t n, uint32_t seg,
                                                            uint32_t nseg,
                                                            uint32_t* __restrict__ crc) {
  using namespace cks;
  __shared__ uint32_t part[256 / kWave];
  const uint32_t t = threadIdx.x;
  uint32_t acc = 0;
  if (t < nseg) {
    const uint32_t step = x8nmodp((uint32_t)((256ull * seg) % 0xFFFFFFFFull));
    uint32_t pw = 0;
    bool fresh = true;
    for (int64_t i = t + (uint64_t)((nseg - 1 - t) / 256u) * 256u; i >= 0; i -= 256) {
      const uint64_t end = (uint64_t)(i + 1) * seg < n ? (uint64_t)(i + 1) * seg : n;
      if (fresh) pw = x8nmodp((uint32_t)((n - end) % 0xFFFFFFFFull));
      else pw = multmodp(pw, step);
      fresh = (uint32_t)i == nseg - 1;  // the last segment may be short: no constant step from it
      acc ^= multmodp(pw, (uint32_t)sums[i]);
    }
  }
  for (uint32_t d = 1; d < 64; d <<= 1) acc ^= (uint32_t)__shfl_xor((int)acc, (int)d, 64);
  if ((t & 63u) == 0) part[t >> 6] = acc;
  __syncthreads();
  if (t == 0) crc[0] = part[0] ^ part[1] ^ part[2] ^ part[3];
}

}  // namespace bitar_hip
