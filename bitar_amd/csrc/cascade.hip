// cascade.hip -- CASCADE: RUNPACK's runs with their values and lengths packed by INTPACK, per
// segment, both directions (gfx950): the "RLE -> delta -> bit-pack" scheme, for sorted keys,
// coarse timestamps, clustered status codes and flag bytes, whose run values are sorted or lie in
// a small range and whose run lengths are small numbers.  No reference counterpart.
//
// Stream of a segment of L bytes, element width W in {1, 2, 4, 8}, m = L / W elements compared
// as byte patterns:
//   byte 0      0x80 | mode << 3 | log2(W)     mode 0 cascade, 1 stored
//   byte 1      0
//   bytes 2..3  LE16(L - 1)
//   stored:     L raw bytes                                                  size = 4 + L
//   cascade:    LE16(r - 1)  LE16(vsize - 1)  values  lengths  tail
//               values   an INTPACK stream of width W of the r*W bytes of the runs' values
//               lengths  an INTPACK stream of width 2 of the 2r bytes LE16(run length - 1)
//               size = 8 + vsize + lsize + (L - m*W)
// Runs are maximal, the sub-streams are what INTPACK writes for those bytes, and the cascade form
// is taken when r <= 32768 and its size is strictly below 4 + L (a tie is stored).
//
// One wavefront per segment, one launch each way, nothing but the stream and the segment in
// global memory.  The encoder reads its segment with RUNPACK's head scan (runs.hip.h); the heads
// go into an LDS staging area of one INTPACK block (256 runs), and every full block is planned
// there with INTPACK's own plan (bitpack.hip.h): pass one adds up both sub-streams' sizes in both
// modes, which settles the modes, the sizes and where the lengths start; pass two scans again,
// plans each block once more and feeds two payload emitters, each block's widths, reference and
// payload going straight to their places in the stream.  A segment of at most 256 runs is
// written from the block pass one left in LDS and read once.  The
// decoder checks both sub-streams and sums the lengths first, then RUNPACK's window expansion
// takes its runs from an LDS ring that a sequential reader fills a miniblock (64 runs) at a time.
#include "../../include/bitar_hip.h"
#include "autopack.hip.h"
#include "bitpack.hip.h"
#include "runs.hip.h"

namespace bitar_hip {

namespace csc {

using ipk::Elem;
using ipk::kMini;
constexpr uint32_t kBlk = 4 * kMini;   // runs per INTPACK block
constexpr uint32_t kMaxRuns = 32768;   // (r - 1 and both sub-streams' L - 1 fit 16 bits)

template <uint32_t W>
__device__ __forceinline__ typename Elem<W>::U as_elem(const uint4& v) {
  if constexpr (W == 8) return ((uint64_t)v.y << 32) | v.x;
  else return v.x;
}

// The block of runs being filled: run base + i has its value in val[i] and starts at pos[i];
// pos[count] is where the run after the block's last starts (positions mod 2^16: m can be 65536).
template <uint32_t W>
struct EncShared {
  __attribute__((aligned(8))) uint8_t val[kBlk * W];
  uint16_t pos[kBlk + 2];
  uint32_t stage[ipk::kStageDwords];  // one miniblock's bit string

  __device__ __forceinline__ void put(uint32_t i, typename Elem<W>::U v) { ipk::set_lds_ref<W>(val, i, v); }
  __device__ __forceinline__ typename Elem<W>::U value(uint32_t i) const { return ipk::lds_ref<W>(val, i); }
  __device__ __forceinline__ uint32_t length(uint32_t i) const {  // run length - 1
    return ((uint32_t)pos[i + 1] - (uint32_t)pos[i] - 1u) & 0xFFFFu;
  }
};

// the block as sources of INTPACK elements: run idx >= base from LDS, run base - 1 (the delta of
// the block's first run needs it) from a register
template <uint32_t W>
struct ValueSource {
  static constexpr bool kKeepShift = true;
  const EncShared<W>& sh;
  uint32_t base;
  typename Elem<W>::U before;
  __device__ __forceinline__ typename Elem<W>::U operator()(uint32_t idx) const {
    return idx < base ? before : sh.value(idx - base);
  }
};
template <uint32_t W>
struct LengthSource {
  static constexpr bool kKeepShift = true;
  const EncShared<W>& sh;
  uint32_t base, before;
  __device__ __forceinline__ uint32_t operator()(uint32_t idx) const {
    return idx < base ? before : sh.length(idx - base);
  }
};

// One pass over the segment: block(base, count, values, lengths) for the runs base .. base +
// count - 1, every block of kBlk runs and the last, shorter one.  Returns the number of runs,
// or leaves early with a number above `limit`.
template <uint32_t W, class BLOCK>
__device__ __forceinline__ uint32_t scan_blocks(const GMEM uint8_t* src, uint32_t L, uint32_t m,
                                                EncShared<W>& sh, uint32_t limit, BLOCK&& block) {
  using U = typename Elem<W>::U;
  constexpr uint32_t E = 16 / W;
  const uint32_t lane = lane_id();
  const uint32_t nch = (m * W + 15u) / 16u;
  rpk::HeadScan<W> hs(src, L, m);
  uint32_t done = 0, base = 0;
  U val_before = 0;
  uint32_t len_before = 0;
  for (uint32_t c0 = 0; c0 < nch; c0 += kWave) {
    const uint32_t c = c0 + lane;
    if (!hs.step(c)) continue;
    const uint32_t cnt = (uint32_t)__popc(hs.mask);
    const uint32_t incl = wave_incl_sum(cnt);
    const uint32_t k0 = done + incl - cnt;  // this lane's first head is run k0
    done += readlane(incl, 63);
    if (done > limit) return done;
    for (;;) {
      // the heads that belong to the block, and the one after it for its last run's length
      uint32_t k = k0;
      for (uint32_t mk = hs.mask; mk; mk &= mk - 1u, ++k) {
        const uint32_t j = (uint32_t)__builtin_ctz(mk);
        const uint32_t i = k - base;  // (wraps for a head of a block already done)
        if (i <= kBlk) sh.pos[i] = (uint16_t)(c * E + j);
        if (i < kBlk) sh.put(i, as_elem<W>(rpk::element<W>(hs.ch, j)));
      }
      if (done <= base + kBlk) break;  // the block's last run has not ended yet
      lds_order();
      block(base, kBlk, ValueSource<W>{sh, base, val_before}, LengthSource<W>{sh, base, len_before});
      val_before = sh.value(kBlk - 1u);
      len_before = sh.length(kBlk - 1u);
      lds_order();
      base += kBlk;
    }
  }
  const uint32_t count = done - base;  // 1 .. kBlk
  if (lane == 0) sh.pos[count] = (uint16_t)m;
  lds_order();
  block(base, count, ValueSource<W>{sh, base, val_before}, LengthSource<W>{sh, base, len_before});
  lds_order();
  return done;
}

// One sub-stream while it is written: an INTPACK stream of width W of r elements at `sub`.
template <uint32_t W>
struct SubWriter {
  using U = typename Elem<W>::U;
  GMEM uint8_t* sub;
  uint32_t mode, r;
  ipk::Layout<W> lay;
  ipk::PayloadEmitter<W> emit;

  __device__ __forceinline__ SubWriter(GMEM uint8_t* sub_, uint32_t mode_, uint32_t r_, uint32_t* stage)
      : sub(sub_), mode(mode_), r(r_), lay(r_ * W, mode_), emit(sub_ + lay.pay_at, stage) {
    const uint32_t lane = lane_id();
    const uint32_t head = ipk::stream_head<W>(mode, r * W);
    if (lane < 4) sub[lane] = (uint8_t)(head >> (8 * lane));
  }
  // the runs base .. base + count - 1 (base a multiple of kBlk)
  template <class SRC>
  __device__ __forceinline__ void block(uint32_t base, uint32_t count, const SRC& src) {
    const uint32_t lane = lane_id();
    if (mode == 2) {
      for (uint32_t i = lane; i < count; i += kWave)
        ipk::store_elem<W>(sub + 4 + (uint64_t)(base + i) * W, src(base + i));
      return;
    }
    const uint32_t blk = base / kBlk;
    ipk::BlockPlan<W> p;
    ipk::plan_block<W>(src, blk, r, p);
    const uint32_t md = mode;
    if (lane == 0) {
      if (md && base == 0) ipk::store_elem<W>(sub + lay.base_at, src(0));
      ipk::store_elem<W>(sub + lay.ref_at + blk * W, md ? p.ref[1] : p.ref[0]);
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t k = blk * 4 + j;
      if (k >= lay.nmb) break;
      const uint32_t b = md ? p.b[1][j] : p.b[0][j];
      if (lane == 0) sub[lay.wid_at + k] = (uint8_t)b;
      if (b == 0) continue;
      const bool in = k * kMini + lane < r;
      emit.put(md ? p.residual(1, j, in) : p.residual(0, j, in), b);
    }
  }
  __device__ __forceinline__ void finish() {
    if (mode != 2) emit.finish();
  }
};

template <uint32_t W>
__device__ __forceinline__ void store_segment(const GMEM uint8_t* src, uint32_t L, GMEM uint8_t* dst,
                                              uint32_t* size_out) {
  constexpr uint32_t kLog = W == 1 ? 0 : W == 2 ? 1 : W == 4 ? 2 : 3;
  if (lane_id() == 0) {
    // (slots are 16-B aligned)
    *reinterpret_cast<GMEM uint32_t*>(dst) = 0x80u | 1u << 3 | kLog | (L - 1) << 16;
    *size_out = 4u + L;
  }
  wave_copy_global(dst + 4, src, L);
}

template <uint32_t W>
__device__ __forceinline__ void compress_segment(const GMEM uint8_t* src, uint32_t L,
                                                 GMEM uint8_t* dst, uint32_t* size_out,
                                                 EncShared<W>& sh) {
  constexpr uint32_t kLog = W == 1 ? 0 : W == 2 ? 1 : W == 4 ? 2 : 3;
  const uint32_t lane = lane_id();
  const uint32_t m = L / W, tail = L - m * W;
  if (m == 0) return store_segment<W>(src, L, dst, size_out);

  // ---- pass one: the runs, and what both sub-streams cost in either mode ---------------------
  uint32_t vsum[2] = {0, 0}, lsum[2] = {0, 0};
  const uint32_t r = scan_blocks<W>(
      src, L, m, sh, kMaxRuns,
      [&](uint32_t base, uint32_t count, const ValueSource<W>& values, const LengthSource<W>& lengths) {
        const uint32_t blk = base / kBlk;
        ipk::BlockPlan<W> pv;
        ipk::plan_block<W>(values, blk, base + count, pv);
        ipk::BlockPlan<2> pl;
        ipk::plan_block<2>(lengths, blk, base + count, pl);
#pragma unroll
        for (uint32_t md = 0; md < 2; ++md)
#pragma unroll
          for (uint32_t j = 0; j < 4; ++j) {  // (a miniblock past the last has width 0)
            vsum[md] += 8u * pv.b[md][j];
            lsum[md] += 8u * pl.b[md][j];
          }
      });
  if (r > kMaxRuns) return store_segment<W>(src, L, dst, size_out);
  uint32_t vsize, lsize;
  const uint32_t vmode = ipk::choose_mode<W>(r * W, vsum, vsize);
  const uint32_t lmode = ipk::choose_mode<2>(r * 2u, lsum, lsize);
  const uint32_t total = 8u + vsize + lsize + tail;
  if (!(total < 4u + L)) return store_segment<W>(src, L, dst, size_out);  // a tie is stored

  // ---- pass two: the same blocks again, each into its place in the two sub-streams -----------
  if (lane == 0) {
    GMEM uint32_t* head = reinterpret_cast<GMEM uint32_t*>(dst);  // (slots are 16-B aligned)
    head[0] = 0x80u | kLog | (L - 1) << 16;
    head[1] = (r - 1u) | (vsize - 1u) << 16;
    *size_out = total;
  }
  SubWriter<W> vw(dst + 8, vmode, r, sh.stage);
  SubWriter<2> lw(dst + 8 + vsize, lmode, r, sh.stage);
  if (r <= kBlk) {
    // the only block is still in LDS: the segment is read once (at 1 GiB the second read comes
    // from HBM, as in RUNPACK's encoder)
    vw.block(0, r, ValueSource<W>{sh, 0, 0});
    lw.block(0, r, LengthSource<W>{sh, 0, 0});
  } else {
    scan_blocks<W>(
        src, L, m, sh, 0xFFFFFFFFu,
        [&](uint32_t base, uint32_t count, const ValueSource<W>& values, const LengthSource<W>& lengths) {
          vw.block(base, count, values);
          lw.block(base, count, lengths);
        });
  }
  vw.finish();
  lw.finish();
  if (lane < tail) dst[8u + vsize + lsize + lane] = src[m * W + lane];
}

// One sub-stream while it is read, a miniblock after the other: an INTPACK stream of width W
// whose segment is n elements.
template <uint32_t W>
struct SubReader {
  using U = typename Elem<W>::U;
  const GMEM uint8_t* sub;
  uint32_t mode = 0, n = 0, off = 0, widths = 0;
  U carry = 0;

  // false for a sub-stream of `size` bytes that must be rejected
  __device__ __forceinline__ bool open(const GMEM uint8_t* sub_, uint32_t size, uint32_t n_) {
    constexpr uint32_t kLog = W == 1 ? 0 : W == 2 ? 1 : W == 4 ? 2 : 3;
    sub = sub_;
    n = n_;
    if (size < 4) return false;
    const uint32_t tag = sub[0];
    mode = (tag >> 2) & 3u;
    if (!ipk::valid_head(tag, sub[1]) || (tag & 3u) != kLog) return false;
    if (1u + sub[2] + ((uint32_t)sub[3] << 8) != n * W) return false;
    if (mode == 2) return size == 4u + n * W;
    uint32_t run;
    return ipk::scan_widths<W>(sub, size, ipk::Layout<W>(n * W, mode), run,
                               [](uint32_t, uint32_t, uint32_t) {});
  }
  __device__ __forceinline__ void rewind() {
    off = 0;
    carry = 0;
  }
  // this lane's element of miniblock k (arbitrary at or past n); k = 0, 1, 2, ...
  __device__ __forceinline__ U next(uint32_t k) {
    const uint32_t lane = lane_id();
    const uint32_t idx = k * kMini + lane;
    if (mode == 2) return idx < n ? ipk::load_elem<W>(sub + 4 + (uint64_t)idx * W) : (U)0;
    const ipk::Layout<W> lay(n * W, mode);
    if ((k & 63u) == 0) widths = k + lane < lay.nmb ? sub[lay.wid_at + k + lane] : 0u;  // 64 at once
    const uint32_t b = readlane(widths, k & 63u);
    const U v = ipk::unpack_miniblock<W>(sub, lay, mode, k, b, sub + lay.pay_at + off, carry);
    off += 8u * b;
    return v;
  }
};

// The runs of a window come out of two rings: the expansion (runs.hip.h) looks at most 64 E
// runs past the window's first for values and 64 runs further for lengths, and a miniblock of 64
// is decoded at a time, so 64 E + 127 values and 128 lengths are live at most.
constexpr uint32_t kValueRing = 4096;  // bytes: 512 values of 8 bytes (>= 255), 4096 of 1 (>= 1151)
constexpr uint32_t kLengthRing = 256;
struct DecShared {
  __attribute__((aligned(16))) uint32_t vals[kValueRing / 4];
  uint16_t lens[kLengthRing];  // run length - 1
  uint32_t map[32];            // bit e: a run starts at element e of the window
};

template <uint32_t W>
struct RingRuns {
  static constexpr uint32_t kRing = kValueRing / W;  // values
  DecShared& sh;
  SubReader<W>& vr;
  SubReader<2>& lr;
  uint32_t r, cur = 0, decoded = 0;

  // the runs below `upto` (and below r) are in the rings
  __device__ __forceinline__ void ensure(uint32_t upto) {
    if (decoded >= upto || decoded >= r) return;
    const uint32_t lane = lane_id();
    lds_order();
    while (decoded < upto && decoded < r) {
      const uint32_t k = decoded / kMini;
      const typename Elem<W>::U v = vr.next(k);
      const uint32_t l = lr.next(k);
      ipk::set_lds_ref<W>(reinterpret_cast<uint8_t*>(sh.vals), (decoded + lane) & (kRing - 1u), v);
      sh.lens[(decoded + lane) & (kLengthRing - 1u)] = (uint16_t)l;
      decoded += kMini;
    }
    lds_order();
  }
  __device__ __forceinline__ uint32_t length_of(uint32_t k) {
    ensure(k + 1u);
    return 1u + sh.lens[k & (kLengthRing - 1u)];
  }
  __device__ __forceinline__ uint32_t lengths_from(uint32_t s) {
    ensure(s + kMini);
    const uint32_t k = s + lane_id();
    return k < r ? 1u + sh.lens[k & (kLengthRing - 1u)] : 0u;
  }
  __device__ __forceinline__ uint4 repeated(uint32_t k) {
    ensure(k + 1u);
    const typename Elem<W>::U v = ipk::lds_ref<W>(reinterpret_cast<const uint8_t*>(sh.vals), k & (kRing - 1u));
    if constexpr (W == 8) {
      return make_uint4((uint32_t)v, (uint32_t)(v >> 32), (uint32_t)v, (uint32_t)(v >> 32));
    } else {
      const uint32_t x = W == 1 ? (uint32_t)v * 0x01010101u : W == 2 ? (uint32_t)v * 0x00010001u : (uint32_t)v;
      return make_uint4(x, x, x, x);
    }
  }
  __device__ __forceinline__ void stage(uint32_t cur_, uint32_t) { cur = cur_; }
  __device__ __forceinline__ const uint32_t* values() const { return sh.vals; }
  __device__ __forceinline__ uint32_t slot(uint32_t i) const { return (cur + i) & (kRing - 1u); }
};

// The cascade form: src holds csize >= 4 bytes, the header's tag is valid and L <= seg.  Returns
// false, having written nothing, for a stream that must be rejected.
template <uint32_t W>
__device__ __forceinline__ bool decompress_cascade(const GMEM uint8_t* src, uint32_t csize, uint32_t L,
                                                   GMEM uint8_t* dst, DecShared& sh) {
  const uint32_t lane = lane_id();
  const uint32_t m = L / W, tail = L - m * W;
  if (csize < 8) return false;
  const uint32_t r = 1u + src[4] + ((uint32_t)src[5] << 8);
  const uint32_t vsize = 1u + src[6] + ((uint32_t)src[7] << 8);
  if (r > m || r > kMaxRuns) return false;
  if (csize < 8u + vsize + 4u + tail) return false;  // room for the lengths' header and the tail
  const uint32_t lsize = csize - 8u - vsize - tail;
  SubReader<W> vr;
  SubReader<2> lr;
  if (!vr.open(src + 8, vsize, r) || !lr.open(src + 8 + vsize, lsize, r)) return false;

  // ---- the run lengths must add up to m (at most 32768 of at most 65536: no overflow) ---------
  uint32_t part = 0;
  for (uint32_t k = 0; k * kMini < r; ++k) {
    const uint32_t l = lr.next(k) & 0xFFFFu;
    if (k * kMini + lane < r) part += 1u + l;
  }
  if (readlane(wave_incl_sum(part), 63) != m) return false;
  lr.rewind();

  RingRuns<W> runs{sh, vr, lr, r};
  rpk::expand_runs<W>(runs, r, m, dst, sh.map);
  if (lane < tail) dst[m * W + lane] = src[csize - tail + lane];
  return true;
}

}  // namespace csc

// CASCADE as the shared kernels see it (autopack.hip.h).  The encoder writes nothing at or past
// the stream's size in its slot; the decoder leaves a rejected segment's output range untouched
// and writes nothing outside the segment's first L bytes.
struct Cascade {
  static constexpr uint32_t kNibble = 8;
  template <uint32_t W> using EncShared = csc::EncShared<W>;
  using DecShared = csc::DecShared;

  template <uint32_t W, bool STORE>
  static constexpr auto compress_segment = &csc::compress_segment<W>;  // (STORE alone)

  static __device__ __forceinline__ bool decode_stream(const GMEM uint8_t* src, uint32_t csize,
                                                       uint32_t tag, uint32_t rsv, uint32_t L,
                                                       uint32_t seg, GMEM uint8_t* dst,
                                                       DecShared& sh) {
    const uint32_t lg = tag & 7u;
    bool ok = (tag >> 4) == kNibble && lg <= 3u && rsv == 0 && L <= seg;
    if (ok && (tag & 8u)) {
      ok = decode_stored(src, csize, L, dst);
    } else if (ok) {
      switch (lg) {
        case 0: ok = csc::decompress_cascade<1>(src, csize, L, dst, sh); break;
        case 1: ok = csc::decompress_cascade<2>(src, csize, L, dst, sh); break;
        case 2: ok = csc::decompress_cascade<4>(src, csize, L, dst, sh); break;
        default: ok = csc::decompress_cascade<8>(src, csize, L, dst, sh); break;
      }
    }
    return ok;
  }
};

BITAR_COLUMN_COMPRESS(Cascade, 1, true);
BITAR_COLUMN_COMPRESS(Cascade, 2, true);
BITAR_COLUMN_COMPRESS(Cascade, 4, true);
BITAR_COLUMN_COMPRESS(Cascade, 8, true);
BITAR_COLUMN_DECOMPRESS(Cascade, false);

}  // namespace bitar_hip
