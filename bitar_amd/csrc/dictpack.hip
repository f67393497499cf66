// dictpack.hip -- DICTPACK: a per-segment dictionary of the distinct elements plus bit-packed
// indices, for columns of wide values with few distinct ones (hash ids, UUIDs, decimal128,
// floats that take a few hundred values), both directions (gfx950).  No reference counterpart.
//
// Stream of a segment of L bytes, element width W in {4, 8, 16}, m = L / W elements compared as
// byte patterns:
//   byte 0      0x60 | mode << 3 | log2(W)     mode 0 packed, 1 stored
//   byte 1      0
//   bytes 2..3  LE16(L - 1)
//   stored:     L raw bytes                                                  size = 4 + L
//   packed:     LE16(d - 1)  dict[d] (W bytes each, in order of first occurrence)  payload  tail
//               payload = ceil(m / 64) miniblocks of 8 * b bytes, b = bit_length(d - 1), element
//               t's index at bits [t*b, (t+1)*b) of the little-endian bit string (bitpack.hip.h)
//               size = 6 + d*W + 8*b*nmb + (L - m*W)
// Packed when d <= 1024 and the packed size is below 4 + L (the two differ by 2 mod 4: never
// equal).
//
// One wavefront per segment, lane t = element t of the current miniblock.  The encoder reads its
// segment twice (build, then emit; the second read comes from L2 / Infinity Cache).  Its hash
// table lives in LDS and holds element POSITIONS, so one table serves all three widths: keys are
// compared by re-reading the input.  First-occurrence order makes the bytes independent of the
// hash and of the order in which lanes win a slot.  Element and stream addresses have any
// alignment (bitpack.hip.h; the 16-byte load and store are here).
#include "../../include/bitar_hip.h"
#include "autopack.hip.h"
#include "bitpack.hip.h"

namespace bitar_hip {

namespace dpk {

using ipk::kMini;

constexpr uint32_t kMaxDict = 1024;         // entries of a dictionary
constexpr uint32_t kSlots = 2 * kMaxDict;   // hash slots: the build stops past kMaxDict claims
                                            // (at most kMaxDict + 64 slots are ever taken)
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kPosBits = 14;           // a position is < 65536 / 4
constexpr uint32_t kMapWords = 65536 / 4 / 32;

template <uint32_t W> struct Key { using T = typename ipk::Elem<W>::U; };
template <> struct Key<16> { using T = uint4; };

// the W-byte element at p (any alignment): only aligned dwords that hold one of its bytes are
// loaded
template <uint32_t W>
__device__ __forceinline__ typename Key<W>::T load_key(const GMEM uint8_t* p) {
  if constexpr (W == 16) {
    const uint32_t a = (uint32_t)(uintptr_t)p;
    if ((a & 15u) == 0) return *reinterpret_cast<const GMEM uint4*>(p);
    const GMEM uint32_t* q = reinterpret_cast<const GMEM uint32_t*>(p - (a & 3u));
    uint4 v = make_uint4(q[0], q[1], q[2], q[3]);
    if ((a & 3u) != 0) {
      const uint32_t top = q[4];
      v.x = funnel(v.x, v.y, a);
      v.y = funnel(v.y, v.z, a);
      v.z = funnel(v.z, v.w, a);
      v.w = funnel(v.w, top, a);
    }
    return v;
  } else {
    return ipk::load_elem<W>(p);
  }
}

__device__ __forceinline__ void key_words(uint32_t v, uint32_t* w) { w[0] = v; }
__device__ __forceinline__ void key_words(uint64_t v, uint32_t* w) {
  w[0] = (uint32_t)v;
  w[1] = (uint32_t)(v >> 32);
}
__device__ __forceinline__ void key_words(uint4 v, uint32_t* w) {
  w[0] = v.x;
  w[1] = v.y;
  w[2] = v.z;
  w[3] = v.w;
}

// (a dictionary starts 6 bytes into a 16-B aligned slot: its entries sit at 2 mod 4, which gets
// halfword and dword stores instead of W byte stores)
template <uint32_t W>
__device__ __forceinline__ void store_key(GMEM uint8_t* p, typename Key<W>::T v) {
  constexpr uint32_t N = W / 4;
  const uint32_t a = (uint32_t)(uintptr_t)p;
  uint32_t w[N];
  key_words(v, w);
  if constexpr (W == 16) {
    if ((a & 15u) == 0) {
      *reinterpret_cast<GMEM uint4*>(p) = v;
      return;
    }
  }
  if ((a & 3u) == 0) {
    GMEM uint32_t* q = reinterpret_cast<GMEM uint32_t*>(p);
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) q[k] = w[k];
  } else if ((a & 3u) == 2) {
    *reinterpret_cast<GMEM uint16_t*>(p) = (uint16_t)w[0];
    GMEM uint32_t* q = reinterpret_cast<GMEM uint32_t*>(p + 2);
#pragma unroll
    for (uint32_t k = 0; k + 1 < N; ++k) q[k] = w[k] >> 16 | w[k + 1] << 16;
    *reinterpret_cast<GMEM uint16_t*>(p + W - 2) = (uint16_t)(w[N - 1] >> 16);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < W; ++k) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3u)));
  }
}

__device__ __forceinline__ bool key_eq(uint32_t a, uint32_t b) { return a == b; }
__device__ __forceinline__ bool key_eq(uint64_t a, uint64_t b) { return a == b; }
__device__ __forceinline__ bool key_eq(uint4 a, uint4 b) {
  return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0;
}

// the slot a key starts at.  Every dword of the key goes through a multiply and an xor-shift,
// so every byte of it reaches the bits that are kept (keys that differ in one byte only, or
// that are multiples of a power of two, spread over the table)
__device__ __forceinline__ uint32_t mix(uint32_t acc, uint32_t word) {
  acc = (acc ^ word) * 0x9E3779B1u;
  return acc ^ (acc >> 15);
}
__device__ __forceinline__ uint32_t fold(uint32_t acc) { return (acc * 0x85EBCA6Bu) >> (32 - 11); }
__device__ __forceinline__ uint32_t key_slot(uint32_t k) { return fold(mix(0, k)); }
__device__ __forceinline__ uint32_t key_slot(uint64_t k) {
  return fold(mix(mix(0, (uint32_t)k), (uint32_t)(k >> 32)));
}
__device__ __forceinline__ uint32_t key_slot(uint4 k) {
  return fold(mix(mix(mix(mix(0, k.x), k.y), k.z), k.w));
}
static_assert(kSlots == 1u << 11, "fold() keeps 11 bits");

struct Shared {
  uint32_t slot[kSlots];         // build: the first position of a key; then position | rank << 14
  uint32_t map[kMapWords];       // bit p: position p is the first occurrence of its value
  uint16_t before[kMapWords];    // set bits in the words below
  uint32_t stage[ipk::kStageDwords];  // one miniblock's bit string
};

__device__ __forceinline__ void store_header(GMEM uint8_t* dst, uint32_t mode, uint32_t lg,
                                             uint32_t L) {
  // (slots are 16-B aligned)
  *reinterpret_cast<GMEM uint32_t*>(dst) = 0x60u | mode << 3 | lg | (L - 1) << 16;
}

// STORE = false is AUTOPACK's candidate form (autopack.hip): a segment that takes the stored form
// writes its size alone -- a later candidate's stored form is never selected, it ties with
// RUNPACK's at best -- and every other segment is written as ever.
template <uint32_t W, bool STORE = true>
__device__ __forceinline__ void compress_segment(const GMEM uint8_t* src, uint32_t L,
                                                 GMEM uint8_t* dst, uint32_t* size_out,
                                                 Shared& sh) {
  using K = typename Key<W>::T;
  constexpr uint32_t kLog = W == 4 ? 2 : W == 8 ? 3 : 4;
  const uint32_t lane = lane_id();
  const uint32_t m = L / W, tail = L - m * W;
  const uint32_t nmb = (m + kMini - 1) / kMini;

  // ---- build: one slot per distinct value, holding its smallest position --------------------
  for (uint32_t s = lane; s < kSlots; s += kWave) sh.slot[s] = kEmpty;
  lds_order();
  uint32_t d = 0;
  for (uint32_t k = 0; k < nmb && d <= kMaxDict; ++k) {
    const uint32_t idx = k * kMini + lane;
    K key = {};
    if (idx < m) key = load_key<W>(src + (uint64_t)idx * W);
    uint32_t h = key_slot(key);
    uint32_t pending = idx < m ? 1u : 0u, claimed = 0;
    // Lanes with equal keys start at the same slot and move in step, so they always meet in one
    // slot: a value never takes two.  At most kMaxDict + 64 of the kSlots slots are taken, so a
    // lane finds its value or an empty slot within that many steps; the count bounds the loop
    // by construction all the same.
    for (uint32_t step = 0; step < kSlots; ++step) {
      if (pending) {
        const uint32_t old = atomicCAS(&sh.slot[h], kEmpty, idx);
        if (old == kEmpty) {
          claimed = 1;
          pending = 0;
        } else if (key_eq(key, load_key<W>(src + (uint64_t)old * W))) {
          atomicMin(&sh.slot[h], idx);  // (several lanes of this miniblock may hold the value)
          pending = 0;
        } else {
          h = (h + 1) & (kSlots - 1);
        }
      }
      if (ballot(pending != 0) == 0) break;
    }
    d += (uint32_t)__popcll(ballot(claimed != 0));
  }
  lds_order();

  // ---- form: packed only with at most kMaxDict values and a size below the stored one ---------
  const uint32_t b = ipk::bit_length(d - 1);
  const uint32_t total = 6u + d * W + 8u * b * nmb + tail;
  if (m == 0 || d > kMaxDict || !(total < 4u + L)) {
    if (lane == 0) {
      if constexpr (STORE) store_header(dst, 1, kLog, L);
      *size_out = 4u + L;
    }
    if constexpr (STORE) wave_copy_global(dst + 4, src, L);
    return;
  }

  // ---- order: a value's index is the rank of its first position -----------------------------
  const uint32_t nw = (m + 31) / 32;
  for (uint32_t j = lane; j < nw; j += kWave) sh.map[j] = 0;
  lds_order();
  for (uint32_t s = lane; s < kSlots; s += kWave) {
    const uint32_t p = sh.slot[s];
    if (p != kEmpty) atomicOr(&sh.map[p >> 5], 1u << (p & 31u));
  }
  lds_order();
  uint32_t run = 0;
  for (uint32_t j0 = 0; j0 < nw; j0 += kWave) {
    const uint32_t j = j0 + lane;
    const uint32_t c = j < nw ? (uint32_t)__popc(sh.map[j]) : 0u;
    const uint32_t incl = wave_incl_sum(c);
    if (j < nw) sh.before[j] = (uint16_t)(run + incl - c);
    run += readlane(incl, 63);
  }
  lds_order();
  if (lane == 0) {
    store_header(dst, 0, kLog, L);
    *reinterpret_cast<GMEM uint16_t*>(dst + 4) = (uint16_t)(d - 1);
    *size_out = total;
  }
  GMEM uint8_t* dict = dst + 6;
  for (uint32_t s = lane; s < kSlots; s += kWave) {
    const uint32_t p = sh.slot[s];
    if (p != kEmpty) {
      const uint32_t rank = sh.before[p >> 5] + (uint32_t)__popc(sh.map[p >> 5] & ((1u << (p & 31u)) - 1u));
      sh.slot[s] = p | rank << kPosBits;
      store_key<W>(dict + rank * W, load_key<W>(src + (uint64_t)p * W));
    }
  }
  lds_order();

  // ---- emit: every element's rank as aligned dwords (bitpack.hip.h) ---------------------------
  GMEM uint8_t* pay = dict + d * W;
  uint32_t off = 0;
  if (b) {
    ipk::PayloadEmitter<4> emit(pay, sh.stage);
    for (uint32_t k = 0; k < nmb; ++k) {
      const uint32_t idx = k * kMini + lane;
      uint32_t rank = 0;
      if (idx < m) {
        const K key = load_key<W>(src + (uint64_t)idx * W);
        uint32_t h = key_slot(key);
        for (uint32_t step = 0; step < kSlots; ++step) {  // (the value is in the table)
          const uint32_t v = sh.slot[h];
          const uint32_t p = v & ((1u << kPosBits) - 1u);
          if (v == kEmpty) break;
          if (p == idx || key_eq(key, load_key<W>(src + (uint64_t)p * W))) {
            rank = v >> kPosBits;
            break;
          }
          h = (h + 1) & (kSlots - 1);
        }
      }
      emit.put(rank, b);
    }
    off = emit.finish();
  }
  if (lane < tail) pay[off + lane] = src[m * W + lane];
}

struct DecShared {
  __attribute__((aligned(16))) uint32_t dict[kMaxDict * 4];  // the dictionary, W bytes an entry
};

// the packed form: src holds csize >= 4 bytes, the header is valid and L <= seg.  Returns false
// for a stream that must be rejected: for its sizes before anything is written, for an index
// that is no entry of the dictionary at the miniblock that holds it (the elements of the
// miniblocks before it are written then, nothing else).
template <uint32_t W>
__device__ __forceinline__ bool decompress_packed(const GMEM uint8_t* src, uint32_t csize,
                                                  uint32_t L, GMEM uint8_t* dst, DecShared& sh) {
  using K = typename Key<W>::T;
  const uint32_t lane = lane_id();
  const uint32_t m = L / W, tail = L - m * W;
  const uint32_t nmb = (m + kMini - 1) / kMini;
  if (csize < 6) return false;
  const uint32_t d = 1u + src[4] + ((uint32_t)src[5] << 8);
  if (d > m || d > kMaxDict) return false;
  const uint32_t b = ipk::bit_length(d - 1);
  const uint32_t pay_at = 6u + d * W, bytes = 8u * b * nmb;
  if (pay_at + bytes + tail != csize) return false;

  for (uint32_t j = lane; j < d * (W / 4); j += kWave)
    sh.dict[j] = ipk::load_elem<4>(src + 6 + 4 * j);
  lds_order();
  const GMEM uint8_t* pay = src + pay_at;
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t idx = k * kMini + lane;
    uint32_t j = 0;
    if (b) j = ipk::extract_field<4>(pay + k * 8 * b, b);
    const bool live = idx < m;
    if (ballot(live & (j >= d)) != 0) return false;
    if (live)
      store_key<W>(dst + (uint64_t)idx * W, *reinterpret_cast<const K*>(&sh.dict[j * (W / 4)]));
  }
  if (lane < tail) dst[m * W + lane] = pay[bytes + lane];
  return true;
}

}  // namespace dpk

// DICTPACK as the shared kernels see it (autopack.hip.h).  Nothing outside the segment's first L
// bytes is written.
struct DictPack {
  static constexpr uint32_t kNibble = 6;
  template <uint32_t W> using EncShared = dpk::Shared;
  using DecShared = dpk::DecShared;

  template <uint32_t W, bool STORE>
  static constexpr auto compress_segment = &dpk::compress_segment<W, STORE>;

  static __device__ __forceinline__ bool decode_stream(const GMEM uint8_t* src, uint32_t csize,
                                                       uint32_t tag, uint32_t rsv, uint32_t L,
                                                       uint32_t seg, GMEM uint8_t* dst,
                                                       DecShared& sh) {
    const uint32_t lg = tag & 7u;
    bool ok = (tag >> 4) == kNibble && lg >= 2u && lg <= 4u && rsv == 0 && L <= seg;
    if (ok && (tag & 8u)) {
      ok = decode_stored(src, csize, L, dst);
    } else if (ok) {
      switch (lg) {
        case 2: ok = dpk::decompress_packed<4>(src, csize, L, dst, sh); break;
        case 3: ok = dpk::decompress_packed<8>(src, csize, L, dst, sh); break;
        default: ok = dpk::decompress_packed<16>(src, csize, L, dst, sh); break;
      }
    }
    return ok;
  }
};

BITAR_COLUMN_COMPRESS(DictPack, 4, true);
BITAR_COLUMN_COMPRESS(DictPack, 8, true);
BITAR_COLUMN_COMPRESS(DictPack, 16, true);
BITAR_COLUMN_COMPRESS(DictPack, 4, false);
BITAR_COLUMN_COMPRESS(DictPack, 8, false);
BITAR_COLUMN_COMPRESS(DictPack, 16, false);
BITAR_COLUMN_DECOMPRESS(DictPack, false);
BITAR_COLUMN_DECOMPRESS(DictPack, true);

}  // namespace bitar_hip
