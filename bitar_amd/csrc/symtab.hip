// symtab.hip -- SYMTAB: a per-segment static symbol table for string data (names, URLs, log
// lines, keys), in the style of FSST: up to 255 byte strings of 1..8 bytes, the text written as
// one-byte codes, anything else escaped; both directions (gfx950).  No reference counterpart.
//
// Stream of a segment of L bytes (tests/symtab_model.py restates it in Python):
//   byte 0      0xC0 | mode                     mode 0 coded, 1 stored
//   byte 1      nsym, 1..255                    (0 in the stored form)
//   bytes 2..3  LE16(L - 1)
//   stored:     L raw bytes                                                  size = 4 + L
//   coded:      LE16 nc   lens[nsym]   syms   codes[nc]   lits[nx]
//               size = 6 + nsym + sum(lens) + nc + nx
// A code c < nsym is symbol c, 255 is the next unread byte of lits.  The coded form is taken when
// its size is strictly below 4 + L.
//
// The encoder's rule (normative): five generations over a sample of 256-byte
// chunks, a lane a chunk; in each the chunks are parsed greedily against the table, items and
// adjacent pairs are counted (pairs in 4096 hashed slots, the smallest key of a slot alone), and
// the 255 candidates of the largest gain, ties in index order, are the next table.  Then one
// greedy parse of the whole segment, 64 positions a step.  No float and no race decides a byte.
//
// One wavefront per segment, one launch each way, no scratch in HBM.  The kernels are the column
// codecs' (autopack.hip.h) with this format's traits: the element width is always 1.
#include "../../include/bitar_hip.h"
#include "rans.hip.h"

namespace bitar_hip {

namespace symtab {

using rans::lanes_below;
using rans::ld16;
using rans::wave_sum;

constexpr uint32_t kEsc = 255;
constexpr uint32_t kMaxSyms = 255;
constexpr uint32_t kChunk = 256;                   // bytes of a sample chunk
constexpr uint32_t kSampleAll = 16384;             // segments up to this length are sampled whole
constexpr uint32_t kGenerations = 5;
constexpr uint32_t kStride = kChunk / 4 + 1;       // dwords between two chunks in LDS: lane t's
                                                   // dword k lies in bank (t + k) % 32
constexpr uint32_t kSlots = 4096;                  // pair slots
constexpr uint32_t kCand = 512 + kSlots;           // candidate indices: items, then slots
constexpr uint32_t kPerLane = kCand / kWave;       // 72 candidates a lane, contiguous
constexpr uint32_t kEmpty = 0xFFFFFFFFu;           // a slot no pair fell into
constexpr uint32_t kCountBits = 14;                // slot word: key << 14 | count (a sample has
                                                   // at most 64 * 255 pairs)
constexpr uint32_t kHashMul = 0x9E3779B1u;
constexpr uint32_t kBuckets = 512;                 // of the lookup, by a symbol's first two bytes
constexpr uint32_t kBlock = 1024;                  // bytes of text staged for the final parse
constexpr uint32_t kTextDwords = 5 * kWave;        // a block, the 8 bytes past it, the misalignment

// bytes [a, a + 8) of a little-endian byte string kept in dwords
__device__ __forceinline__ uint64_t window(const uint32_t* buf, uint32_t a) {
  const uint32_t i = a >> 2;
  const uint32_t w0 = buf[i], w1 = buf[i + 1], w2 = buf[i + 2];
  return funnel(w0, w1, a) | (uint64_t)funnel(w1, w2, a) << 32;
}

// ---- encoder --------------------------------------------------------------------------------
struct EncShared {
  union {
    struct {
      uint32_t sample[64 * kStride + 4];  // chunk t at dword t * kStride (the generations)
      __attribute__((aligned(16))) uint32_t slots[kSlots];  // key << 14 | count, or kEmpty
    } gen;
    uint32_t text[kTextDwords];           // the final parse's block
  } a;
  union {
    // a candidate's gain, 0 = no candidate (a gain is at most 2 * 16384)
    __attribute__((aligned(16))) uint16_t gain[kCand];
    struct {
      // the table's symbols of two bytes and more, ordered by the bucket of their first two
      // bytes: .x, .y the symbol, .z = length | code << 8
      __attribute__((aligned(16))) uint4 ent[256 + 4];  // (read four at a time)
      uint16_t start[kBuckets + 8];       // entries of bucket h: [start[h], start[h + 1])
      uint8_t single[256];                // byte -> 1 + the code of the one-byte symbol, or 0
    } look;
  } b;
  __attribute__((aligned(16))) uint32_t c1[512];  // item counts (and the lookup's counters)
  __attribute__((aligned(8))) uint2 sym[2][256];  // the table and the next one, bytes past the length 0
  uint8_t len[2][256];
};

__device__ __forceinline__ void store_segment(const GMEM uint8_t* src, uint32_t L, GMEM uint8_t* dst,
                                              uint32_t* size_out) {
  if (lane_id() == 0) {
    dst[0] = 0xC1;
    dst[1] = 0;
    dst[2] = (uint8_t)(L - 1);
    dst[3] = (uint8_t)((L - 1) >> 8);
    *size_out = 4u + L;
  }
  wave_copy_global(dst + 4, src, L);
}

__device__ __forceinline__ uint32_t bucket(uint32_t two_bytes) {
  return ((two_bytes & 0xFFFFu) * kHashMul) >> 23;
}

// The longest-match lookup of table `cur`: the one-byte symbols by their byte, the others ordered
// by the bucket of their first two bytes.  The order inside a bucket is whatever the atomics
// gave: a table holds no string twice, so the longest match is one entry whatever the order.
__device__ __forceinline__ void build_lookup(EncShared& sh, uint32_t cur, uint32_t nsym) {
  const uint32_t lane = lane_id();
  for (uint32_t k = lane; k < kBuckets; k += kWave) sh.c1[k] = 0;
  reinterpret_cast<uint32_t*>(sh.b.look.single)[lane] = 0;
  lds_order();
  for (uint32_t c = lane; c < nsym; c += kWave) {
    const uint32_t first = sh.sym[cur][c].x;
    if (sh.len[cur][c] == 1) sh.b.look.single[first & 255u] = (uint8_t)(c + 1u);
    else atomicAdd(&sh.c1[bucket(first)], 1u);
  }
  lds_order();
  {
    const uint4 u = reinterpret_cast<const uint4*>(sh.c1)[2 * lane];  // buckets 8 lane .. + 7
    const uint4 v = reinterpret_cast<const uint4*>(sh.c1)[2 * lane + 1];
    const uint32_t n[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) s += n[k];
    const uint32_t incl = wave_incl_sum(s);
    uint32_t at = incl - s;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      sh.b.look.start[8 * lane + k] = (uint16_t)at;
      at += n[k];
    }
    if (lane == kWave - 1) sh.b.look.start[kBuckets] = (uint16_t)incl;
  }
  lds_order();
  for (uint32_t c = lane; c < nsym; c += kWave) {
    const uint2 s = sh.sym[cur][c];
    const uint32_t l = sh.len[cur][c];
    if (l == 1) continue;
    const uint32_t h = bucket(s.x);
    // (a bucket fills from its end: the count is its own cursor)
    const uint32_t at = sh.b.look.start[h] + atomicSub(&sh.c1[h], 1u) - 1u;
    sh.b.look.ent[at] = make_uint4(s.x, s.y, l | c << 8, 0);
  }
  lds_order();
}

// the longest symbol that matches the window w within `rem` bytes, else the single byte
__device__ __forceinline__ void longest(const EncShared& sh, uint64_t w, uint32_t rem,
                                        uint32_t& item, uint32_t& len) {
  const uint32_t b0 = (uint32_t)w & 255u;
  const uint32_t h = bucket((uint32_t)w);
  const uint32_t one = sh.b.look.single[b0];
  const uint32_t e = sh.b.look.start[h + 1];
  item = one ? 255u + one : b0;
  len = 0;
  // four entries a trip: a trip waits for LDS once
  for (uint32_t k = sh.b.look.start[h]; k < e; k += 4) {
    uint4 en[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) en[j] = sh.b.look.ent[k + j];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t l = en[j].z & 255u;
      const uint64_t s = en[j].x | (uint64_t)en[j].y << 32;
      if (k + j < e && l <= rem && l > len && ((w ^ s) << ((64u - 8u * l) & 63u)) == 0) {
        len = l;
        item = 256u + (en[j].z >> 8);
      }
    }
  }
  if (len == 0) len = 1;
}

// One parse of this lane's sample chunk (clen bytes at dword `at` of the sample).  COUNT: items
// into c1, every short pair's key into its slot by minimum.  Otherwise: the pairs whose key is
// their slot's are counted.
template <bool COUNT>
__device__ __forceinline__ void parse_chunk(EncShared& sh, uint32_t at, uint32_t clen) {
  uint32_t pos = 0, prev = 0, prev_len = 0;
  while (pos < clen) {
    uint32_t item, len;
    longest(sh, window(sh.a.gen.sample, 4u * at + pos), clen - pos, item, len);
    if (COUNT) atomicAdd(&sh.c1[item], 1u);
    if (prev_len && prev_len + len <= 8u) {
      const uint32_t key = prev * 512u + item;
      uint32_t* slot = &sh.a.gen.slots[(key * kHashMul) >> 20];
      if (COUNT) {
        atomicMin(slot, key << kCountBits);
      } else if ((*slot >> kCountBits) == key) {
        atomicAdd(slot, 1u);
      }
    }
    prev = item;
    prev_len = len;
    pos += len;
  }
}

__device__ __forceinline__ uint32_t item_len(const EncShared& sh, uint32_t cur, uint32_t x) {
  return x < 256u ? 1u : sh.len[cur][x - 256u];
}
__device__ __forceinline__ uint64_t item_bytes(const EncShared& sh, uint32_t cur, uint32_t x) {
  if (x < 256u) return x;
  const uint2 s = sh.sym[cur][x - 256u];
  return s.x | (uint64_t)s.y << 32;
}

// this lane's candidates with a gain of at least t (g: its 72 gains, two a dword)
__device__ __forceinline__ uint32_t at_least(const uint32_t (&g)[kPerLane / 2], uint32_t t) {
  uint32_t n = 0;
#pragma unroll
  for (uint32_t k = 0; k < kPerLane / 2; ++k) n += ((g[k] & 0xFFFFu) >= t) + ((g[k] >> 16) >= t);
  return n;
}

// One generation: table `cur` (nsym symbols) -> table cur ^ 1; returns its size.
__device__ __forceinline__ uint32_t generation(EncShared& sh, uint32_t cur, uint32_t nsym,
                                               uint32_t at, uint32_t clen) {
  const uint32_t lane = lane_id();
  build_lookup(sh, cur, nsym);
  for (uint32_t k = lane; k < 512; k += kWave) sh.c1[k] = 0;
  for (uint32_t k = lane; k < kSlots / 4; k += kWave)
    reinterpret_cast<uint4*>(sh.a.gen.slots)[k] = make_uint4(kEmpty, kEmpty, kEmpty, kEmpty);
  lds_order();
  parse_chunk<true>(sh, at, clen);
  lds_order();
  parse_chunk<false>(sh, at, clen);
  lds_order();

  // ---- gains (the lookup's LDS is the gains' from here on) ----------------------------------
  for (uint32_t i = lane; i < 512; i += kWave) {
    const uint32_t c = sh.c1[i];
    sh.b.gain[i] = (uint16_t)(c ? c * item_len(sh, cur, i) : 0u);
  }
  for (uint32_t s = lane; s < kSlots; s += kWave) {
    const uint32_t v = sh.a.gen.slots[s];
    uint32_t g = 0;
    if (v != kEmpty) {
      const uint32_t key = v >> kCountBits;
      g = (v & ((1u << kCountBits) - 1u)) * (item_len(sh, cur, key >> 9) + item_len(sh, cur, key & 511u));
    }
    sh.b.gain[512 + s] = (uint16_t)g;
  }
  lds_order();

  // ---- the threshold: lane t has the candidates 72 t .. 72 t + 71 ---------------------------
  uint32_t g[kPerLane / 2];
#pragma unroll
  for (uint32_t k = 0; k < kPerLane / 8; ++k) {
    const uint4 v = reinterpret_cast<const uint4*>(sh.b.gain)[lane * (kPerLane / 8) + k];
    g[4 * k] = v.x;
    g[4 * k + 1] = v.y;
    g[4 * k + 2] = v.z;
    g[4 * k + 3] = v.w;
  }
  uint32_t thr = 0, room = 0;
  if (wave_sum(at_least(g, 1)) > kMaxSyms) {
    // the 255th largest gain: the largest t that at least 255 candidates reach
    uint32_t lo = 1, hi = 2u * kSampleAll;
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (wave_sum(at_least(g, mid)) >= kMaxSyms) lo = mid; else hi = mid - 1;
    }
    thr = lo;
    room = kMaxSyms - wave_sum(at_least(g, thr + 1));
  }
  // candidates above thr, and the first `room` of those at thr in index order
  const uint32_t above = at_least(g, thr + 1);
  const uint32_t equal = thr ? at_least(g, thr) - above : 0u;
  uint32_t eq_rank = wave_incl_sum(equal) - equal;
  const uint32_t eq_take = eq_rank >= room ? 0u : min(equal, room - eq_rank);
  const uint32_t take = above + eq_take;
  const uint32_t take_incl = wave_incl_sum(take);
  uint32_t out = take_incl - take;
  for (uint32_t j = 0; j < kPerLane; ++j) {
    const uint32_t i = lane * kPerLane + j;
    const uint32_t gi = sh.b.gain[i];
    bool taken = gi > thr;
    if (thr && gi == thr) taken = eq_rank++ < room;
    if (!taken) continue;
    uint64_t s;
    uint32_t l;
    if (i < 512u) {
      s = item_bytes(sh, cur, i);
      l = item_len(sh, cur, i);
    } else {
      const uint32_t key = sh.a.gen.slots[i - 512u] >> kCountBits;
      const uint32_t lx = item_len(sh, cur, key >> 9);
      s = item_bytes(sh, cur, key >> 9) | item_bytes(sh, cur, key & 511u) << (8u * lx);
      l = lx + item_len(sh, cur, key & 511u);
    }
    sh.sym[cur ^ 1u][out] = make_uint2((uint32_t)s, (uint32_t)(s >> 32));
    sh.len[cur ^ 1u][out] = (uint8_t)l;
    ++out;
  }
  lds_order();
  return readlane(take_incl, 63);
}

// r: the lanes on the chain that starts at this lane, as a 64-bit mask, where lane t's successor
// is lane next (itself: none).  Pointer doubling: after round k a lane has its next 2^k - 1
// successors; a step of 64 positions has at most 64 links, so six rounds.
__device__ __forceinline__ void reach(uint32_t next, uint32_t& r_lo, uint32_t& r_hi) {
  const uint32_t lane = lane_id();
  auto bit = [](uint32_t l, uint32_t& lo, uint32_t& hi) {
    lo = l < 32u ? 1u << l : 0u;
    hi = l < 32u ? 0u : 1u << (l - 32u);
  };
  bit(lane, r_lo, r_hi);
  uint32_t j4 = next << 2;  // (ds_bpermute takes a byte address)
#pragma unroll
  for (uint32_t r = 0; r < 6; ++r) {
    uint32_t a, b;
    if (r == 0) {
      bit(next, a, b);
    } else {
      a = (uint32_t)__builtin_amdgcn_ds_bpermute((int)j4, (int)r_lo);
      b = (uint32_t)__builtin_amdgcn_ds_bpermute((int)j4, (int)r_hi);
    }
    if (r < 5) j4 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)j4, (int)j4);
    r_lo |= a;
    r_hi |= b;
  }
}

__device__ __forceinline__ void compress_segment(const GMEM uint8_t* src, uint32_t L,
                                                 GMEM uint8_t* dst, uint32_t* size_out,
                                                 EncShared& sh) {
  const uint32_t lane = lane_id();
  // (no coded form is smaller than one symbol of one byte and one code)
  if (9u >= 4u + L) return store_segment(src, L, dst, size_out);

  // ---- the sample: lane t's chunk is chunk t (or 4 t) of the segment ------------------------
  const uint32_t every = L <= kSampleAll ? 1u : 4u;
  const uint32_t nchunks = (L + kChunk - 1u) / kChunk;
  const uint32_t nsample = (nchunks + every - 1u) / every;
  for (uint32_t t = 0; t < nsample; ++t) {
    const uint32_t lo = t * every * kChunk;
    const uint32_t n = min(kChunk, L - lo);
    uint32_t v = 0;
    if (4u * lane + 4u <= n) {
      __builtin_memcpy(&v, src + lo + 4u * lane, 4);
    } else {
      for (uint32_t k = 0; 4u * lane + k < n; ++k) v |= (uint32_t)src[lo + 4u * lane + k] << (8u * k);
    }
    sh.a.gen.sample[t * kStride + lane] = v;
  }
  lds_order();
  const uint32_t at = lane * kStride;
  const uint32_t clen = lane < nsample ? min(kChunk, L - lane * every * kChunk) : 0u;

  uint32_t cur = 0, nsym = 0;
  for (uint32_t gen = 0; gen < kGenerations; ++gen) {
    nsym = generation(sh, cur, nsym, at, clen);
    cur ^= 1u;
  }
  build_lookup(sh, cur, nsym);

  // ---- header, lens and symbols: lane t has the symbols 4t .. 4t + 3 ------------------------
  uint32_t l4[4], ls = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    l4[k] = 4 * lane + k < nsym ? sh.len[cur][4 * lane + k] : 0u;
    ls += l4[k];
  }
  const uint32_t ls_incl = wave_incl_sum(ls);
  const uint32_t codes_at = 6u + nsym + readlane(ls_incl, 63);
  const uint32_t limit = 4u + L;  // the coded form must stay strictly below
  if (codes_at + 1u >= limit) return store_segment(src, L, dst, size_out);
  {
    uint32_t o = 6u + nsym + ls_incl - ls;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      if (l4[k] == 0) continue;
      dst[6u + 4 * lane + k] = (uint8_t)l4[k];
      const uint2 s = sh.sym[cur][4 * lane + k];
      const uint64_t v = s.x | (uint64_t)s.y << 32;
      for (uint32_t j = 0; j < l4[k]; ++j) dst[o + j] = (uint8_t)(v >> (8u * j));
      o += l4[k];
    }
  }

  // ---- the parse: 64 positions a step, the text staged a block of 16 steps at a time --------
  // text dword k of block b is the aligned dword 256 b + k of the segment's memory: byte p of
  // the segment is byte mis + p - 1024 b of the block
  const uint32_t mis = (uint32_t)((uintptr_t)src & 3u);
  const GMEM uint32_t* words = reinterpret_cast<const GMEM uint32_t*>(src - mis);
  const uint32_t nd = (mis + L + 3u) >> 2;
  auto load_block = [&](uint32_t b, uint32_t (&v)[kTextDwords / kWave]) {
#pragma unroll
    for (uint32_t j = 0; j < kTextDwords / kWave; ++j) {
      const uint32_t d = b * (kBlock / 4) + j * kWave + lane;
      v[j] = d < nd ? words[d] : 0u;
    }
  };
  uint32_t tv[kTextDwords / kWave];
  load_block(0, tv);
  GMEM uint8_t* cp = dst + codes_at;
  uint32_t nc = 0, nx = 0, carry = 0;  // carry: the step's first position the chain starts at
  for (uint32_t b = 0; b * kBlock < L; ++b) {
    lds_order();
#pragma unroll
    for (uint32_t j = 0; j < kTextDwords / kWave; ++j) sh.a.text[j * kWave + lane] = tv[j];
    lds_order();
    if ((b + 1u) * kBlock < L) load_block(b + 1u, tv);
    for (uint32_t t = 0; t < kBlock / kWave; ++t) {
      const uint32_t p0 = b * kBlock + t * kWave;
      if (p0 >= L) break;
      const uint32_t p = p0 + lane;
      uint32_t item = 0, len = 1;
      if (p < L) longest(sh, window(sh.a.text, mis + t * kWave + lane), L - p, item, len);
      // the greedy chain through the step's positions: every lane's reach, the start's taken
      const uint32_t end = min((uint32_t)kWave, L - p0);
      uint64_t chain = 0;
      if (carry < end) {
        uint32_t r_lo, r_hi;
        reach(lane + len < end ? lane + len : lane, r_lo, r_hi);
        chain = readlane(r_lo, carry) | (uint64_t)readlane(r_hi, carry) << 32;
        const uint32_t last = 63u - (uint32_t)__builtin_clzll(chain);
        carry = last + readlane(len, last);
      }
      carry -= end;  // (0 at the segment's end: no match passes it)
      const uint64_t esc = chain & ballot(item < 256u);
      const uint32_t n = (uint32_t)__builtin_popcountll(chain);
      nx += (uint32_t)__builtin_popcountll(esc);
      if (BITAR_RARE(codes_at + nc + n + nx >= limit)) return store_segment(src, L, dst, size_out);
      if (chain >> lane & 1u) cp[nc + lanes_below(chain)] = (uint8_t)(item < 256u ? kEsc : item - 256u);
      nc += n;
    }
  }

  // ---- lits: the escapes' bytes, found again from the codes' lengths -------------------------
  if (nx) {
    global_fence_wave();  // (the codes are this wave's own stores)
    GMEM uint8_t* lits = cp + nc;
    uint32_t pos = 0, xq = 0;
    for (uint32_t i0 = 0; i0 < nc; i0 += kWave) {
      const uint32_t i = i0 + lane;
      const uint32_t c = i < nc ? cp[i] : 0u;
      const uint32_t len = i < nc ? (c == kEsc ? 1u : sh.len[cur][c]) : 0u;
      const uint32_t incl = wave_incl_sum(len);
      const uint64_t esc = ballot(i < nc && c == kEsc);
      if (esc) {
        if (esc >> lane & 1u) lits[xq + lanes_below(esc)] = src[pos + incl - len];
        xq += (uint32_t)__builtin_popcountll(esc);
      }
      pos += readlane(incl, 63);
    }
  }
  if (lane == 0) {
    dst[0] = 0xC0;
    dst[1] = (uint8_t)nsym;
    dst[2] = (uint8_t)(L - 1);
    dst[3] = (uint8_t)((L - 1) >> 8);
    dst[4] = (uint8_t)nc;
    dst[5] = (uint8_t)(nc >> 8);
    *size_out = codes_at + nc + nx;
  }
}

// ---- decoder --------------------------------------------------------------------------------
constexpr uint32_t kOutRing = 2048;  // output bytes staged in LDS, at their address mod 2048
constexpr uint32_t kGroup = 8;       // steps whose codes are loaded together, a group ahead

struct DecShared {
  __attribute__((aligned(16))) uint8_t ring[kOutRing];
  __attribute__((aligned(8))) uint2 sym[256];
  uint8_t lut[256];  // code -> output bytes; 0: no code of this stream
};

// out[flushed, upto) from the ring to the segment: whole aligned 16-byte blocks unless `final`
__device__ __forceinline__ void flush(GMEM uint8_t* dst, const uint8_t* ring, uint32_t& flushed,
                                      uint32_t upto, bool final) {
  const uint32_t lane = lane_id();
  const uint32_t base = (uint32_t)(uintptr_t)dst;
  uint32_t f = flushed;
  lds_order();
  uint32_t head = (16u - ((base + f) & 15u)) & 15u;
  if (head > upto - f) head = upto - f;
  if (head) {
    if (lane < head) dst[f + lane] = ring[(base + f + lane) & (kOutRing - 1u)];
    f += head;
  }
  const uint32_t nb = (upto - f) >> 4;
  for (uint32_t b = lane; b < nb; b += kWave) {
    const uint32_t k = f + 16u * b;
    *reinterpret_cast<GMEM uint4*>(dst + k) =
        *reinterpret_cast<const uint4*>(ring + ((base + k) & (kOutRing - 1u)));
  }
  f += nb << 4;
  if (final && f < upto) {
    if (lane < upto - f) dst[f + lane] = ring[(base + f + lane) & (kOutRing - 1u)];
    f = upto;
  }
  flushed = f;
  lds_order();
}

__device__ __forceinline__ bool decompress_coded(const GMEM uint8_t* src, uint32_t csize,
                                                 uint32_t nsym, uint32_t L, GMEM uint8_t* dst,
                                                 DecShared& sh) {
  const uint32_t lane = lane_id();
  if (nsym == 0 || csize < 6u + nsym) return false;
  const uint32_t nc = ld16(src + 4);
  if (nc == 0) return false;
  // ---- the table: lane t has the symbols 4t .. 4t + 3 ---------------------------------------
  uint32_t l4[4], ls = 0, bad = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t c = 4 * lane + k;
    l4[k] = c < nsym ? src[6u + c] : 0u;
    bad |= c < nsym && (l4[k] < 1u || l4[k] > 8u);
    ls += l4[k];
  }
  if (ballot(bad != 0)) return false;
  const uint32_t ls_incl = wave_incl_sum(ls);
  const uint32_t codes_at = 6u + nsym + readlane(ls_incl, 63);
  if (csize < codes_at + nc) return false;
  {
    uint32_t o = 6u + nsym + ls_incl - ls;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t c = 4 * lane + k;
      uint64_t v = 0;
      for (uint32_t j = 0; j < l4[k]; ++j) v |= (uint64_t)src[o + j] << (8u * j);
      o += l4[k];
      sh.sym[c] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
      sh.lut[c] = (uint8_t)(c < nsym ? l4[k] : c == kEsc ? 1u : 0u);
    }
  }
  lds_order();

  // ---- the codes once, before any store: their escapes, their range, their output length -----
  const GMEM uint8_t* cp = src + codes_at;
  uint32_t nx;
  {
    const uint32_t mis = (uint32_t)((uintptr_t)cp & 3u);
    const GMEM uint32_t* words = reinterpret_cast<const GMEM uint32_t*>(cp - mis);
    const uint32_t nd = (mis + nc + 3u) >> 2;
    uint32_t total = 0, escapes = 0, none = 0;
    for (uint32_t base = 0; base < nd; base += 4 * kWave) {
      uint32_t v[4];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t d = base + j * kWave + lane;
        v[j] = d < nd ? words[d] : 0u;
      }
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t i = 4u * (base + j * kWave + lane) - mis;  // (past nc where d >= nd)
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
          if (i + k >= nc) continue;  // (a byte in front of the codes wraps past nc too)
          const uint32_t c = v[j] >> (8 * k) & 255u;
          const uint32_t n = sh.lut[c];
          total += n;
          none |= n == 0;
          escapes += c == kEsc;
        }
      }
    }
    if (ballot(none != 0)) return false;
    nx = wave_sum(escapes);
    if (wave_sum(total) != L || csize != codes_at + nc + nx) return false;
  }

  // ---- the codes again: a lane a code, 64 a step, the output staged in the ring --------------
  const GMEM uint8_t* lits = cp + nc;
  const uint32_t base = (uint32_t)(uintptr_t)dst;
  const uint32_t T = (nc + kWave - 1) / kWave;
  auto load_group = [&](uint32_t g, uint32_t (&cd)[kGroup]) {
#pragma unroll
    for (uint32_t j = 0; j < kGroup; ++j) {
      const uint32_t i = (g * kGroup + j) * kWave + lane;
      cd[j] = i < nc ? cp[i] : 0u;
    }
  };
  uint32_t cur[kGroup], nxt[kGroup];
  load_group(0, cur);
  uint32_t op = 0, flushed = 0, xq = 0;
  const uint32_t G = (T + kGroup - 1) / kGroup;
  for (uint32_t g = 0; g < G; ++g) {
    if (g + 1 < G) load_group(g + 1, nxt);
#pragma unroll
    for (uint32_t j = 0; j < kGroup; ++j) {
      const uint32_t t = g * kGroup + j;
      if (t >= T) continue;  // (the last group alone)
      const bool act = t * kWave + lane < nc;
      const uint32_t c = cur[j];
      const uint32_t len = act ? sh.lut[c] : 0u;
      uint2 v = sh.sym[c];
      const uint32_t incl = wave_incl_sum(len);
      const uint64_t esc = ballot(act && c == kEsc);
      if (esc) {
        if (esc >> lane & 1u) v.x = lits[xq + lanes_below(esc)];
        xq += (uint32_t)__builtin_popcountll(esc);
      }
      const uint32_t o = base + op + incl - len;
#pragma unroll
      for (uint32_t k = 0; k < 8; ++k)
        if (k < len) sh.ring[(o + k) & (kOutRing - 1u)] = (uint8_t)((k < 4 ? v.x : v.y) >> (8 * (k & 3)));
      op += readlane(incl, 63);
      // (a step stages at most 512 bytes; at most 15 stay behind a flush)
      if (BITAR_RARE(op - flushed >= kOutRing / 2)) flush(dst, sh.ring, flushed, op, false);
    }
#pragma unroll
    for (uint32_t j = 0; j < kGroup; ++j) cur[j] = nxt[j];
  }
  flush(dst, sh.ring, flushed, op, true);
  return true;
}

}  // namespace symtab

// The codec as the column kernels see it: one "width", the storing form alone.  The encoder
// writes nothing past the stream it reports (at most 4 + L bytes of its slot); the decoder
// validates the whole stream before its first store and writes the segment's L bytes alone.
struct SymTab {
  static constexpr uint32_t kNibble = 0xC;
  template <uint32_t W> using EncShared = symtab::EncShared;
  using DecShared = symtab::DecShared;

  template <uint32_t W, bool STORE>
  static constexpr auto compress_segment = &symtab::compress_segment;

  static __device__ __forceinline__ bool decode_stream(const GMEM uint8_t* src, uint32_t csize,
                                                       uint32_t tag, uint32_t byte1, uint32_t L,
                                                       uint32_t seg, GMEM uint8_t* dst,
                                                       DecShared& sh) {
    if ((tag >> 4) != kNibble || (tag & 15u) > 1u || L > seg) return false;
    if (tag & 1u) return byte1 == 0 && decode_stored(src, csize, L, dst);
    return symtab::decompress_coded(src, csize, byte1, L, dst, sh);
  }
};

BITAR_COLUMN_COMPRESS(SymTab, 1, true);
BITAR_COLUMN_DECOMPRESS(SymTab, false);

}  // namespace bitar_hip
