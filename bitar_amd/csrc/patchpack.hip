// patchpack.hip -- PATCHPACK: INTPACK's frame-of-reference bit packing with per-miniblock
// exceptions, per segment, both directions (gfx950).  No reference counterpart.  INTPACK gives a
// miniblock of 64 elements the bit length of its largest residual, so one outlier widens 64
// slots; here a miniblock takes the width at which its payload plus its exceptions (2 + W bytes
// each, kept raw behind the payload with their positions, as FLTPACK keeps its own) is smallest.
// A third mode packs the complements, for columns whose outliers lie below the rest.
//
// Stream of a segment of L bytes, element width W, m = L / W elements:
//   byte 0      0x90 | mode << 2 | log2(W)     mode 0 plain, 1 delta, 2 stored, 3 complement
//   byte 1      0
//   bytes 2..3  LE16(L - 1)
//   stored:     L raw bytes
//   packed:     LE16 nx  [mode 1: element 0]  widths[nmb]  refs[nblk] (W bytes each)  payload
//               pos[nx] (LE16)  val[nx] (W bytes each)  tail
//
// The width rule, in a miniblock whose residuals have the bit lengths l_t, B the largest:
// cost(b) = 8 b + (2 + W) * #{t : l_t > b} for b = 0..B, and the width is the LARGEST b of minimal
// cost.  #{l_t > b} only changes where b passes one of the l_t, and between two of them 8 b grows,
// so only b = 0, b = one of the l_t, and b = B can be minimal: the wave ORs 1 << l_t into a mask
// of the lengths that occur (one DPP ladder) and walks its set bits from the top down, one ballot
// and one population count each, all on the scalar unit.  The count grows on the way down, and the
// walk ends where (2 + W) * count alone reaches the best cost so far: after one or two steps on a
// miniblock without outliers, after the outliers' lengths and two more on one with.
//
// One wavefront per segment, lane t = element t of the current miniblock.  The encoder plans,
// then emits (the second read of the segment comes from L2 / Infinity Cache, as INTPACK's); the
// plan keeps the references, widths and exception counts of all three modes in LDS.  The decoder
// is INTPACK's walk with FLTPACK's merge before the single store: the validated position list
// gives each miniblock its number of exceptions, the lanes read that many positions and tell
// the lanes they name, through 64 words of LDS, where in val[] their x lies; such a lane takes it
// in place of the unpacked one -- before the prefix add in mode 1, before the complement in
// mode 3 -- and every element is stored once.
// (Loads, stores, plan_block, the payload emitter, the width scan and the exception lists'
// rank and position check: bitpack.hip.h.)
#include "../../include/bitar_hip.h"
#include "autopack.hip.h"
#include "bitpack.hip.h"

namespace bitar_hip {

namespace ppk {

using namespace ipk;

constexpr uint32_t kModes = 3;  // the packed modes 0, 1 and 3 in slots 0, 1 and 2, the order
__device__ constexpr uint32_t mode_of(uint32_t md) { return md == 2 ? 3u : md; }  // of ties

// (a 64 KiB segment has 1024 / W miniblocks and 256 / W blocks: 256 bytes of references)
template <uint32_t W>
struct Shared {
  uint8_t wid[kModes][kMaxMini / W];                         // widths per mode slot
  uint8_t xcnt[kModes][kMaxMini / W];                        // exceptions per miniblock
  __attribute__((aligned(8))) uint8_t ref[kModes][kMaxBlk];  // references, W bytes each
  uint32_t stage[kStageDwords];                              // one miniblock's bit string
};

// The width rule on one miniblock: len = this lane's l_t (0 at or past m), B = the largest.
// Returns the width; cnt = the number of exceptions at it.  Wave-uniform.
template <uint32_t W>
__device__ __forceinline__ uint32_t patch_width(uint32_t len, uint32_t B, uint32_t& cnt) {
  using U = typename Elem<W>::U;
  cnt = 0;
  if (B == 0) return 0;
  // the lengths below B that occur, and 0 (bit l: some l_t = l; B <= 8 W bits, so l < B fits)
  U seen = wave_or<U>(len < B ? (U)1 << (len & (8 * sizeof(U) - 1)) : (U)0) | (U)1;
  uint32_t best = 8 * B, width = B;
  while (seen) {
    const uint32_t b = bit_length(seen) - 1;
    seen &= ~((U)1 << b);
    const uint32_t n = (uint32_t)__popcll(ballot(len > b));
    if ((2 + W) * n >= best) break;  // (and so is every cost further down)
    const uint32_t cost = 8 * b + (2 + W) * n;
    if (cost < best) {  // (a tie stays with the larger width)
      best = cost;
      width = b;
      cnt = n;
    }
  }
  return width;
}

// the x of mode slot md from load_values' two
template <uint32_t W>
__device__ __forceinline__ typename Elem<W>::U pick_x(uint32_t md, typename Elem<W>::U plain,
                                                      typename Elem<W>::U delta) {
  using U = typename Elem<W>::U;
  constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
  return md == 0 ? plain : md == 1 ? delta : (U)(~plain & mask);
}

template <uint32_t W, bool STORE = true>
__device__ __forceinline__ void compress_segment(const GMEM uint8_t* src, uint32_t L,
                                                 GMEM uint8_t* dst, uint32_t* size_out,
                                                 Shared<W>& sh) {
  using U = typename Elem<W>::U;
  using S = typename Elem<W>::S;
  constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
  constexpr uint32_t kLog = W == 1 ? 0 : W == 2 ? 1 : W == 4 ? 2 : 3;
  const uint32_t lane = lane_id();
  const uint32_t m = L / W, tail = L - m * W;
  const uint32_t nmb = (m + kMini - 1) / kMini, nblk = (nmb + 3) / 4;
  const GlobalElems<W> elems{src};

  // ---- plan: every mode's references, widths and exception counts in one sweep ----------------
  uint32_t sum[kModes] = {0, 0, 0}, nxs[kModes] = {0, 0, 0};
  for (uint32_t blk = 0; blk < nblk; ++blk) {
    BlockPlan<W> p;  // modes 0 and 1: x, references, INTPACK's widths (bitpack.hip.h)
    plan_block<W>(elems, blk, m, p);
    // mode 3: the complements; their signed minimum is the complement of the signed maximum
    S lo = (S)(~(U)0 >> 1);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t idx = (blk * 4 + j) * kMini + lane;
      if (idx < m) lo = imin(lo, as_signed<W>((U)(~p.x[0][j] & mask)));
    }
    const U ref3 = (U)wave_min<S, U>(lo) & mask;
#pragma unroll
    for (uint32_t md = 0; md < kModes; ++md) {
      const U ref = md == 2 ? ref3 : p.ref[md];
      if (lane == 0) set_lds_ref<W>(sh.ref[md], blk, ref);
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t k = blk * 4 + j;
        const uint32_t idx = k * kMini + lane;
        U r;
        uint32_t B;
        if (md == 2) {
          r = idx < m ? (U)(((U)~p.x[0][j] - ref) & mask) : (U)0;
          B = wave_width<W>(r);
        } else {
          r = p.residual(md, j, idx < m);
          B = p.b[md][j];
        }
        uint32_t cnt;
        const uint32_t b = patch_width<W>(bit_length(r), B, cnt);
        if (k < nmb) {
          if (lane == 0) {
            sh.wid[md][k] = (uint8_t)b;
            sh.xcnt[md][k] = (uint8_t)cnt;  // (below 64: 64 exceptions cost more than 8 B)
          }
          sum[md] += 8u * b;
          nxs[md] += cnt;
        }
      }
    }
  }
  lds_order();

  // ---- mode: the smallest packed size, a tie to plain, then delta, then complement; stored ----
  // ---- when nothing is gained (m = 0 included) -------------------------------------------------
  const uint32_t fixed = 6u + nmb + nblk * W + tail;
  uint32_t md = 0, paysum = sum[0], nx = nxs[0], total = fixed + sum[0] + nxs[0] * (2u + W);
  {
    const uint32_t size1 = fixed + W + sum[1] + nxs[1] * (2u + W);
    const uint32_t size3 = fixed + sum[2] + nxs[2] * (2u + W);
    if (size1 < total) {
      md = 1, paysum = sum[1], nx = nxs[1], total = size1;
    }
    if (size3 < total) {
      md = 2, paysum = sum[2], nx = nxs[2], total = size3;
    }
  }
  if (!(total < 4u + L)) {
    const uint32_t h = 0x90u | 2u << 2 | kLog | (L - 1) << 16;
    if (lane == 0) *size_out = 4u + L;
    if constexpr (STORE) {
      if (lane < 4) dst[lane] = (uint8_t)(h >> (8 * lane));
      wave_copy_global(dst + 4, src, L);
    }
    return;
  }
  // (nx < m <= 65536: it fits LE16)
  const uint64_t h = 0x90u | mode_of(md) << 2 | kLog | (L - 1) << 16 | (uint64_t)nx << 32;
  if (lane < 6) dst[lane] = (uint8_t)(h >> (8 * lane));
  if (lane == 0) *size_out = total;
  uint32_t at = 6;
  if (md == 1) {
    if (lane < W) dst[at + lane] = src[lane];
    at += W;
  }
  for (uint32_t k = lane; k < nmb; k += kWave) dst[at + k] = sh.wid[md][k];
  at += nmb;
  for (uint32_t k = lane; k < nblk * W; k += kWave) dst[at + k] = sh.ref[md][k];
  at += nblk * W;

  // ---- emit: the payload as aligned dwords (bitpack.hip.h); the exceptions in position order, -
  // ---- a lane's slot = the exceptions of earlier miniblocks + those of lower lanes            -
  PayloadEmitter<W> emit(dst + at, sh.stage);
  GMEM uint8_t* pos_out = dst + at + paysum;
  GMEM uint8_t* val_out = pos_out + 2 * nx;
  uint32_t xbase = 0;
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t b = sh.wid[md][k], c = sh.xcnt[md][k];
    if (b == 0 && c == 0) continue;
    const uint32_t idx = k * kMini + lane;
    U xs[2];
    load_values<W>(elems, idx, m, xs[0], xs[1]);
    const U x = pick_x<W>(md, xs[0], xs[1]);
    const U ref = lds_ref<W>(sh.ref[md], k / 4);
    U r = idx < m ? (U)((x - ref) & mask) : (U)0;
    if (c) {
      const uint64_t out = ballot(bit_length(r) > b);  // (never a lane at or past m: r = 0)
      if ((out >> lane) & 1u) {
        const uint32_t i = xbase + rank_in(out);  // < nx
        pos_out[2 * i] = (uint8_t)idx;
        pos_out[2 * i + 1] = (uint8_t)(idx >> 8);
        store_elem<W>(val_out + i * W, x);
        r = 0;
      }
      xbase += c;
    }
    if (b) emit.put(r, b);
  }
  emit.finish();
  if (lane < tail) val_out[nx * W + lane] = src[m * W + lane];
}

// The decoder keeps no bitmap of the exceptions (8 KiB at W = 1, which with the widths' offsets
// left three waves a SIMD and measured 1.8 ms/GiB on a column without a single exception): the
// position check counts the exceptions of every miniblock, a byte each, and since the list is
// sorted, miniblock k's are the next cnt[k] entries of pos[] and val[].
struct DecShared {
  uint8_t wid[kMaxMini];
  uint32_t cnt[kMaxMini / 4];  // byte k: the exceptions of miniblock k (at most 64)
  uint32_t slot[kMini];        // lane t: 1 + the index in val[] of element t's exception, or 0
};

// the packed form: src holds csize >= 4 bytes, the header's first four bytes are valid and
// L <= seg.  Returns false for a stream that must be rejected (checked before anything is
// written).
template <uint32_t W>
__device__ __forceinline__ bool decompress_packed(const GMEM uint8_t* src, uint32_t csize,
                                                  uint32_t L, uint32_t mode, GMEM uint8_t* dst,
                                                  DecShared& sh) {
  using U = typename Elem<W>::U;
  constexpr U mask = (U)(~(U)0 >> (8 * sizeof(U) - 8 * W));
  const uint32_t lane = lane_id();
  if (csize < 6) return false;
  const uint32_t nx = src[4] | (uint32_t)src[5] << 8;
  // INTPACK's layout, two bytes further in; what follows the payload counts as its tail while
  // the widths are scanned, so that the size check is the whole formula
  Layout<W> lay(L, mode);
  const uint32_t m = lay.m, tail = lay.tail, nmb = lay.nmb;
  if (nx > m) return false;
  lay.wid_at += 2;
  lay.ref_at += 2;
  lay.pay_at += 2;
  lay.tail += nx * (2u + W);

  // widths; the stream's size must be exactly what they and nx add up to (the walk below adds
  // the offsets up again as it goes)
  uint32_t run;
  if (!scan_widths<W>(src, csize, lay, run, [&](uint32_t k, uint32_t b, uint32_t) {
        sh.wid[k] = (uint8_t)b;
        if ((k & 3u) == 0) sh.cnt[k >> 2] = 0;
      }))
    return false;
  lds_order();

  // positions: each below m and above the one before -> counts per miniblock.  (A list that is
  // rejected may have let a byte run over into its neighbour: nothing is decoded then.  A valid
  // one has at most 64 positions in a miniblock.)
  const uint32_t pos_at = lay.pay_at + run, val_at = pos_at + 2 * nx;
  if (!check_positions(src + pos_at, nx, m, [&](uint32_t p) {
        atomicAdd(&sh.cnt[p >> 8], 1u << (8u * ((p >> 6) & 3u)));
      }))
    return false;
  lds_order();

  const GMEM uint8_t* pay = src + lay.pay_at;
  U base = 0, carry = 0, ref = 0;
  if (mode == 1 && m) base = load_elem<W>(src + 6);
  uint32_t xi = 0;   // exceptions of the miniblocks before this one
  uint32_t off = 0;  // payload bytes of the miniblocks before this one
  for (uint32_t k = 0; k < nmb; ++k) {
    const uint32_t b = sh.wid[k];
    const uint32_t c = uniform(sh.cnt[k >> 2] >> (8u * (k & 3u)) & 255u);
    const uint32_t idx = k * kMini + lane;
    // (the block's reference once, and ahead of the field's loads, which wait in a branch of
    // their own: the two latencies overlap)
    if ((k & 3u) == 0) ref = load_elem<W>(src + lay.ref_at + (k / 4) * W);
    U r = 0;
    if (b) r = extract_field<W>(pay + off, b);
    off += 8u * b;
    U x = (r + ref) & mask;
    if (c) {  // (whatever an exception's slot holds is ignored)
      uint32_t t = 0;
      if (lane < c) t = load_elem<2>(src + pos_at + 2 * (xi + lane)) & (kMini - 1);
      sh.slot[lane] = 0;
      lds_order();
      if (lane < c) sh.slot[t] = xi + lane + 1;
      lds_order();
      const uint32_t at = sh.slot[lane];
      lds_order();
      if (at) x = load_elem<W>(src + val_at + (at - 1) * W);
      xi += c;
    }
    if (mode == 1) {  // element 0 is the base, whatever slot 0 or an exception there says
      if (idx == 0) x = base;
      x = wave_incl_add<U>(x) + carry;
      carry = lane63(x);
    }
    if (mode == 3) x = ~x;
    if (idx < m) store_elem<W>(dst + (uint64_t)idx * W, (U)(x & mask));
  }
  if (lane < tail) dst[m * W + lane] = src[val_at + nx * W + lane];
  return true;
}

}  // namespace ppk

// PATCHPACK as the shared kernels see it (autopack.hip.h).  Slots have any alignment.
struct PatchPack {
  static constexpr uint32_t kNibble = 9;
  template <uint32_t W> using EncShared = ppk::Shared<W>;
  using DecShared = ppk::DecShared;

  template <uint32_t W, bool STORE>
  static constexpr auto compress_segment = &ppk::compress_segment<W, STORE>;

  static __device__ __forceinline__ bool decode_stream(const GMEM uint8_t* src, uint32_t csize,
                                                       uint32_t tag, uint32_t rsv, uint32_t L,
                                                       uint32_t seg, GMEM uint8_t* dst,
                                                       DecShared& sh) {
    const uint32_t mode = (tag >> 2) & 3u;
    bool ok = (tag >> 4) == kNibble && rsv == 0 && L <= seg;
    if (ok && mode == 2) {
      ok = decode_stored(src, csize, L, dst);
    } else if (ok) {
      switch (tag & 3u) {
        case 0: ok = ppk::decompress_packed<1>(src, csize, L, mode, dst, sh); break;
        case 1: ok = ppk::decompress_packed<2>(src, csize, L, mode, dst, sh); break;
        case 2: ok = ppk::decompress_packed<4>(src, csize, L, mode, dst, sh); break;
        default: ok = ppk::decompress_packed<8>(src, csize, L, mode, dst, sh); break;
      }
    }
    return ok;
  }
};

BITAR_COLUMN_COMPRESS(PatchPack, 1, true);
BITAR_COLUMN_COMPRESS(PatchPack, 2, true);
BITAR_COLUMN_COMPRESS(PatchPack, 4, true);
BITAR_COLUMN_COMPRESS(PatchPack, 8, true);
BITAR_COLUMN_DECOMPRESS(PatchPack, false);

}  // namespace bitar_hip
