// snappy.hip -- raw Snappy segments, one wavefront per segment (gfx950):
//   snappy_compress_kernel    the LZ4 codec's window-scan parse (window_parse.hip.h: SKIP, 4 KiB
//                             ring, 1024-entry table, distance cap 2560, LZ4 end rules) with a
//                             Snappy emitter; the stream is the LZ4 block's sequences re-emitted
//                             as Snappy elements (tests/snappy_model.py), or the stored form
//   snappy_decompress_kernel  any raw Snappy stream of <= 64 KiB (stock streams included), on
//                             the decoders' stream window + history ring (stream_ring.hip.h);
//                             <true>: a fragment of a whole-buffer stream, without a preamble
//   snappy_join_* / snappy_scan_*  one whole-buffer stream from the segments' streams, and the
//                             boundary scan that finds its 64 KiB fragments again (further down)
//
// Format (include/bitar_hip.h, BITAR_HIP_CODEC_SNAPPY): the segment's length as a varint, then
// elements -- a literal (tag (len-1) << 2, or 60 << 2 / 61 << 2 with 1 / 2 length bytes), a
// copy-1 (2 bytes: 4 <= len <= 11, offset < 2048) or a copy-2 (3 bytes: len <= 64, 16-bit
// offset).  A literal and the copy after it are separate elements, so a sequence costs two
// chain steps in the decoder where LZ4 has one token.
#include "kernels.hip.h"
#include "order.hip.h"
#include "stream_ring.hip.h"
#include "window_parse.hip.h"

namespace bitar_hip {

namespace snp {

// m's bit for this lane ? a : b (m an SGPR pair used directly as the lane mask)
__device__ __forceinline__ uint32_t lane_sel(uint64_t m, uint32_t a, uint32_t b) {
  uint32_t r;
  __asm__("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
  return r;
}

// header bytes of a literal element of len bytes (len >= 1)
__device__ __forceinline__ uint32_t lit_hdr(uint32_t len) {
  return len <= 60u ? 1u : len <= 256u ? 2u : 3u;
}

}  // namespace snp

namespace cmp {

// ---- Snappy emitter: the LZ4 emitter's two paths (compress.hip, Lz4Out) with Snappy headers ---
// `bulk` takes records of <= 64 ordinary sequences: literal run <= 256 bytes inside the input
// ring (a tag of 1 or 2 bytes), match of 4..64 bytes (ONE copy element of 2 or 3 bytes).  The
// record lane stores its sequence's header bytes itself -- literal tag, literal length byte,
// copy tag, offset low, offset high: five byte stores for the wave, as LZ4's token, length byte,
// offset, length byte -- and the literal bytes are gathered 64 per step.  Everything else -- a
// longer literal run, a run below the input ring, a match of >= 65 bytes, which Snappy splits
// into several copy elements -- takes `one`, a sequence at a time; its 64-byte copy pieces are
// written 21 per step.
constexpr uint32_t kSnapObuf = 512;   // output ring (flushed to HBM in 16-B blocks)
constexpr uint32_t kSnapSeqCap = 64;  // records per flush (a window adds <= 16)
constexpr uint32_t kSnapBulkLit = 256, kSnapBulkMatch = 64;
struct SnapLds {
  uint8_t ring[kSnapObuf + 16];    // + one trash byte (padded)
  uint2 seqs[kSnapSeqCap + 1];     // + a trash record
  uint32_t marks[kWave + 1];       // literal run starts of the current step; + trash
};

struct SnapOut : ByteOutT<kSnapObuf> {
  SnapLds* L;
  uint32_t nseq;      // pending records
  uint32_t last_end;  // end of the last match emitted (the next literal run's start)
  bool matched;       // a match was emitted (else the stream is the stored form already)

  __device__ __forceinline__ void init(SnapLds* lds, GMEM uint8_t* d, uint64_t c) {
    L = lds;
    ring = lds->ring;
    dst = d;
    cap = c;
    op = flushed = 0;
    overflow = false;
    nseq = 0;
    last_end = 0;
    matched = false;
    lds->marks[lane_id()] = 0;
    lds_order();
  }
  // the segment's length as a minimal varint (n <= 65536: <= 3 bytes)
  __device__ __forceinline__ void preamble(uint32_t n) {
    const uint32_t nb = n < 128u ? 1u : n < 16384u ? 2u : 3u;
    const uint32_t lane = lane_id();
    const uint32_t v = lane == 0 ? (n & 127u) | (nb > 1 ? 128u : 0u)
                       : lane == 1 ? ((n >> 7) & 127u) | (nb > 2 ? 128u : 0u) : n >> 14;
    if (!room(nb)) return;
    put(v, nb);
  }
  // one copy element
  __device__ __forceinline__ void piece(uint32_t off, uint32_t len) {
    const uint32_t lane = lane_id();
    if (len <= 11u && off < 2048u) {
      if (!room(2)) return;
      put(lane ? off & 0xFFu : 1u | ((len - 4u) << 2) | ((off >> 8) << 5), 2);
    } else {
      if (!room(3)) return;
      put(lane == 0 ? 2u | ((len - 1u) << 2) : lane == 1 ? off & 0xFFu : off >> 8, 3);
    }
  }
  // One sequence, general path: any literal run (long runs HBM -> HBM), any match length.
  __device__ __forceinline__ void one(const GMEM uint8_t* in, const InRing& I, uint32_t lit_start,
                                      uint32_t lit_len, uint32_t off, uint32_t mlen) {
    if (overflow) return;
    const uint32_t lane = lane_id();
    if (lit_len) {
      const uint32_t nh = snp::lit_hdr(lit_len), m = lit_len - 1u;
      if (!room(nh)) return;
      put(lane == 0 ? (nh == 1 ? m << 2 : (58u + nh) << 2) : lane == 1 ? m & 0xFFu : m >> 8, nh);
      if ((uint64_t)op + lit_len > cap) { overflow = true; return; }
      if (lit_len <= 256 && lit_start >= I.lo) {
        for (uint32_t k = 0; k < lit_len; k += kWave) {
          const uint32_t step = lit_len - k < kWave ? lit_len - k : kWave;
          room(step);
          lds_order();
          const uint32_t b = I.byte(lit_start + k + (lane < step ? lane : 0u));
          put(b, step);
        }
      } else {
        // long run (or not in the input ring): drain the ring, then HBM -> HBM
        flush(op, true);
        wave_copy_global(dst + op, in + lit_start, lit_len);
        op += lit_len;
        flushed = op;
      }
    }
    if (!mlen) return;
    // stock Snappy's split: while len >= 68 a piece of 64, a piece of 60 if len > 64, the rest
    uint32_t rem = mlen;
    if (rem >= 68u) {
      const uint32_t n64 = (rem - 68u) / 64u + 1u;
      const uint32_t t = lane % 3u;
      const uint32_t v = t == 0 ? 2u | (63u << 2) : t == 1 ? off & 0xFFu : off >> 8;
      for (uint32_t k = 0; k < 3u * n64; k += 63u) {  // 21 pieces of 3 bytes per step
        const uint32_t step = 3u * n64 - k < 63u ? 3u * n64 - k : 63u;
        if (!room(step)) return;
        put(v, step);
      }
      rem -= 64u * n64;
    }
    if (rem > 64u) {
      piece(off, 60u);
      rem -= 60u;
    }
    if (overflow) return;
    piece(off, rem);
  }

  // records of lanes [lo, hi) (all ordinary) as Snappy elements; false (nothing written) if
  // they would overrun the slot.  Lz4Out::bulk (compress.hip) with other header bytes:
  //  * one scan of e | lit_len << 16 (e = the sequence's size: literal tag bytes + literals +
  //    copy bytes, <= 2 + 256 + 3) gives each sequence's output offset a and its literal prefix
  //    lp (both < 2^16);
  //  * the range is cut into chunks of consecutive records whose output fits the staging
  //    ring's room; room is made once per chunk;
  //  * per literal step the non-empty runs starting in the step mark their first literal, one
  //    compare gives the start mask, a v_mbcnt pair the run's rank among the non-empty runs, and
  //    one ds_bpermute fetches the run's packed word (input-ring index - u | output-ring index
  //    - u << 16); lanes past the chunk's last literal store to the trash byte.
  __device__ __forceinline__ bool bulk(const InRing& I, uint32_t lo, uint32_t hi, uint32_t q,
                                       uint32_t lit_start, uint32_t off, uint32_t mlen) {
    constexpr uint32_t kTrash = kSnapObuf, kLim = kSnapObuf - 64;
    const uint32_t lane = lane_id();
    const bool in = (lane >= lo) & (lane < hi);
    const uint32_t lit_len = q - lit_start;
    const uint32_t nlt = lit_len == 0u ? 0u : lit_len <= 60u ? 1u : 2u;
    const bool c1 = (mlen <= 11u) & (off < 2048u);
    const uint32_t ncp = c1 ? 2u : 3u;
    const uint32_t e = in ? (nlt + ncp + lit_len) | (lit_len << 16) : 0u;
    const uint32_t incl = wave_incl_sum(e);
    const uint32_t total = readlane(incl, kWave - 1) & 0xFFFFu;
    if ((uint64_t)op + total > cap) return false;
    const uint32_t excl = incl - e;
    const uint32_t a = excl & 0xFFFFu, lp = excl >> 16;  // output offset, literals before
    const uint32_t iend = incl & 0xFFFFu;
    // the header bytes and their ring indices (per byte: the ring wraps)
    const uint32_t h0 = nlt == 1u ? (lit_len - 1u) << 2 : 60u << 2;
    const uint32_t t0 = c1 ? 1u | ((mlen - 4u) << 2) | ((off >> 8) << 5) : 2u | ((mlen - 1u) << 2);
    const uint32_t tA = (uint32_t)(uintptr_t)dst + op + a;
    const uint32_t tO = tA + nlt + lit_len;
    const uint32_t x0 = tA & kMask, x1 = (tA + 1u) & kMask;
    const uint32_t x2 = tO & kMask, x3 = (tO + 1u) & kMask, x4 = (tO + 2u) & kMask;
    const uint64_t l1m = ballot(nlt != 0u), l2m = ballot(nlt == 2u), c3m = ballot(ncp == 3u);
    // the non-empty literal runs: ring indices less u, compacted by rank (ds_permute; the
    // other lanes' words go to lane 63, which no rank reaches unless all 64 runs are non-empty)
    const bool ne = in & (lit_len != 0u);
    const uint64_t nem = ballot(ne);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(nem >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)nem, 0u));
    const uint32_t Din = I.in_lo + lit_start - lp - 1u;
    const uint32_t Dout = tA + nlt - lp - 1u;
    const uint32_t Pc = (uint32_t)__builtin_amdgcn_ds_permute(
        (int)((ne ? rank : kWave - 1) << 2), (int)((Din & 0xFFFFu) | (Dout << 16)));
    const uint32_t lp4 = ne ? lp << 2 : 0x7FFFFF00u;  // mark slot x4 (others: the trash slot)
    const uint32_t mark = lp + 1u;
    const uint32_t zero = 0;
    uint32_t u = lane + 1u;
    uint32_t before = 0;          // non-empty runs starting before the step
    uint32_t c0 = lo, ba = 0, bl = 0;  // the chunk's first record, its a and lp
    do {
      // the chunk: records [c0, c1) end within kLim bytes of its start (one always does)
      const uint64_t over = ballot(iend > ba + kLim);
      uint32_t c1r = over ? (uint32_t)__builtin_ctzll(over) : kWave;
      c1r = c1r < hi ? c1r : hi;
      c1r = c1r > c0 ? c1r : c0 + 1u;  // (a sequence is <= 261 bytes: never taken)
      const uint32_t end = readlane(incl, c1r - 1);
      const uint32_t ea = end & 0xFFFFu, el = end >> 16;
      // (the slot's capacity was checked for the whole range: only the staging ring's room)
      if (op + (ea - ba) - flushed > kLim) flush(op, false);
      lds_order();
      const uint64_t cm = ((c1r < kWave ? 1ull << c1r : 0ull) - 1ull) & ~((1ull << c0) - 1ull);
      ring[snp::lane_sel(cm & l1m, x0, kTrash)] = (uint8_t)h0;
      ring[snp::lane_sel(cm & l2m, x1, kTrash)] = (uint8_t)(lit_len - 1u);
      ring[snp::lane_sel(cm, x2, kTrash)] = (uint8_t)t0;
      ring[snp::lane_sel(cm, x3, kTrash)] = (uint8_t)off;
      ring[snp::lane_sel(cm & c3m, x4, kTrash)] = (uint8_t)(off >> 8);
      for (uint32_t R = bl; R < el; R += kWave) {
        const uint32_t nb = el - R < kWave ? el - R : kWave;
        const uint64_t vm = nb < kWave ? (1ull << nb) - 1ull : ~0ull;
        lds_order();
        const uint32_t slot = min(lp4 - (R << 2), (uint32_t)kWave << 2);
        *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(L->marks) + slot) = mark;
        lds_order();
        const uint32_t mk = L->marks[lane];
        L->marks[lane] = zero;
        // (a run starting past the chunk's last literal belongs to the next chunk)
        const uint64_t S = ballot(mk == u) & vm;
        const uint32_t base = before - 1u + (uint32_t)(S & 1u);
        const uint64_t S1 = S >> 1;
        const uint32_t k = __builtin_amdgcn_mbcnt_hi((uint32_t)(S1 >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)S1, 0u));
        before += (uint32_t)__builtin_popcountll(S);
        const uint32_t p = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((k << 2) + (base << 2)),
                                                                  (int)Pc);
        const uint32_t b = I.ring[(p + u) & I.mask];
        ring[snp::lane_sel(vm, ((p >> 16) + u) & kMask, kTrash)] = (uint8_t)b;
        u += nb;
      }
      lds_order();
      op += ea - ba;
      ba = ea;
      bl = el;
      c0 = c1r;
    } while (c0 < hi);
    return true;
  }

  // every pending record as Snappy elements
  __device__ __forceinline__ void flush_seqs(const GMEM uint8_t* in, const InRing& I) {
    const uint32_t cnt = nseq;
    nseq = 0;
    if (!cnt || overflow) return;
    matched = true;
    const uint32_t lane = lane_id();
    lds_order();
    const uint2 rec = L->seqs[lane < cnt ? lane : kSnapSeqCap];
    const uint32_t q = rec.x & 0xFFFFu, off = (rec.x >> 16) + 1u, mlen = rec.y;
    const uint32_t end = q + mlen;
    const uint32_t prev = wave_shr1(end);
    const uint32_t lit_start = lane == 0 ? last_end : prev;
    const uint32_t lit_len = q - lit_start;
    last_end = readlane(end, cnt - 1);
    // rare sequences (and a flush that would overrun the slot) take the general path
    const uint64_t live = cnt < kWave ? (1ull << cnt) - 1 : ~0ull;
    uint64_t special = (ballot(lit_len > kSnapBulkLit) | ballot(mlen > kSnapBulkMatch) |
                        ballot(lit_start < I.lo)) & live;
    uint32_t lo = 0;
    for (;;) {
      const uint32_t k = special ? (uint32_t)__builtin_ctzll(special) : cnt;
      if (k > lo && !bulk(I, lo, k, q, lit_start, off, mlen)) {
        for (uint32_t j = lo; j < k && !overflow; ++j)  // (the slot's end: exact checks)
          one(in, I, readlane(lit_start, j), readlane(lit_len, j), readlane(off, j),
              readlane(mlen, j));
      }
      if (k >= cnt || overflow) break;
      one(in, I, readlane(lit_start, k), readlane(lit_len, k), readlane(off, k),
          readlane(mlen, k));
      special &= special - 1;
      lo = k + 1;
    }
  }

  // the tail literals (and whatever is pending before them)
  __device__ __forceinline__ void sequence(const GMEM uint8_t* in, const InRing& I,
                                           uint32_t lit_start, uint32_t lit_len, uint32_t off,
                                           uint32_t mlen) {
    flush_seqs(in, I);
    one(in, I, lit_start, lit_len, off, mlen);
  }
  // the tail sequence starts at the last match's end
  __device__ __forceinline__ uint32_t pending_from(uint32_t anchor, uint32_t) const { return anchor; }

  // between windows: flush the records once the next window could overfill the list
  __device__ __forceinline__ void between(const GMEM uint8_t* in, const InRing& I) {
    if (BITAR_RARE(nseq > kSnapSeqCap - 16)) flush_seqs(in, I);
  }
  // One window: its matches appended as records (<= 16: matches are >= 4 bytes)
  __device__ __forceinline__ void window(const GMEM uint8_t*, const InRing&, const Window& W,
                                         uint32_t, uint32_t) {
    if (!W.chain) return;
    const uint64_t chain = W.chain;
    const uint32_t idx = __builtin_amdgcn_mbcnt_hi((uint32_t)(chain >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)chain, nseq));
    const uint32_t lane = lane_id();
    lds_order();
    L->seqs[snp::lane_sel(chain, idx, kSnapSeqCap)] =
        make_uint2((W.x + lane) | (W.dm1 << 16), W.mlen);
    lds_order();
    nseq += (uint32_t)__builtin_popcountll(chain);
  }
};

}  // namespace cmp

__global__ __launch_bounds__(64) void snappy_compress_kernel(
    const uint8_t* __restrict__ input, uint64_t n_total, uint32_t seg,
    uint8_t* __restrict__ slab, uint64_t slot_stride, uint8_t* const* __restrict__ dsts,
    uint32_t* __restrict__ sizes, const uint32_t* __restrict__ order) {
  using namespace cmp;
  // (+ one trash entry: probe lanes past the segment insert there, see parse)
  __shared__ __attribute__((aligned(16))) uint16_t table[(1u << kHashLog) + 8];
  __shared__ __attribute__((aligned(16))) uint8_t inring[kIn + kInPad];
  __shared__ __attribute__((aligned(16))) SnapLds olds;
  // cost-ordered dispatch (seg_order_kernel): workgroup b compresses segment order[b]
  const uint32_t i_seg = order ? order[blockIdx.x] : blockIdx.x;
  const uint64_t seg_off = (uint64_t)i_seg * seg;
  if (seg_off >= n_total) return;
  const uint32_t n = (uint32_t)((n_total - seg_off) < seg ? (n_total - seg_off) : seg);
  const GMEM uint8_t* in = global_ptr(input + seg_off);
  SnapOut o;
  o.init(&olds, global_ptr(dsts ? dsts[i_seg] : slab + (uint64_t)i_seg * slot_stride), slot_stride);
  o.preamble(n);
  parse<SnapOut, false, true, kIn, kHashLog, BITAR_CMP_CHAIN>(in, n, global_ptr(input + n_total),
                                                              table, inring, kIn - 1536u,
                                                              0xFFFFFFFFu, o);
  o.flush(o.op, true);
  // the stored form -- the preamble and one literal element with the whole segment -- unless
  // the stream is smaller (an overrun of the slot is the same case: the slot holds the stored
  // form, bitar_hip_slot_size).  A stream without a match -- incompressible input -- is the
  // stored form as it stands, and is not written twice.
  const uint32_t nb = n < 128u ? 1u : n < 16384u ? 2u : 3u;
  const uint32_t nh = snp::lit_hdr(n);
  const uint32_t stored = nb + nh + n;
  uint32_t size = o.op;
  if (o.overflow || (size >= stored && o.matched)) {
    global_fence_wave();  // the stores above to this range land first
    const uint32_t lane = lane_id(), m = n - 1u;
    const uint32_t pv = lane == 0 ? (n & 127u) | (nb > 1 ? 128u : 0u)
                        : lane == 1 ? ((n >> 7) & 127u) | (nb > 2 ? 128u : 0u) : n >> 14;
    const uint32_t t = lane - nb;
    const uint32_t hv = t == 0 ? (nh == 1 ? m << 2 : (58u + nh) << 2) : t == 1 ? m & 0xFFu : m >> 8;
    if (lane < nb + nh) o.dst[lane] = (uint8_t)(lane < nb ? pv : hv);
    wave_copy_global(o.dst + nb + nh, in, n);
    size = stored;
  }
  if (lane_id() == 0) sizes[i_seg] = size;
}

// ---- decoder --------------------------------------------------------------------------------
// Per step of the fast path ("a batch"):
//   1. every lane parses "an element at stream position ip + lane" from the stream window:
//      class, length, offset, where its literal bytes are, where the next element starts;
//   2. a scalar walk follows the real chain from lane 0 over the parsed window while the
//      elements are eligible (a literal of <= 64 bytes with its length inline or in one byte; a
//      copy-1 or copy-2 with an offset), each element one chain step -- a
//      literal and the copy after it are two.  (The pair as one record, as an LZ4 token is, was
//      not built: stock streams have copies after copies and literals after literals, and the
//      pair form needs a second record shape for them.)
//   3. one prefix sum over the chain lanes places the elements; the declared length and every
//      copy's offset (against the bytes produced before that element) are checked there, once
//      per batch, exactly;
//   4. the output is gathered 64 bytes per step: the elements starting in the step mark their
//      first byte (LDS), a prefix max hands every byte its element's lane, two ds_bpermute its
//      record; a byte is a window literal, a ring history byte, or -- a copy reaching into the
//      step -- another byte of the step, resolved by pointer doubling.  A copy from beyond the
//      ring's reach (stock streams: up to 65535 back) reads its bytes back from HBM, behind a
//      wave-scope fence placed when such a source was stored after the last one: one ballot per
//      step says whether any byte does, and this engine's own streams (offsets <= 2560) never do.
// Everything else takes the general path, an element at a time: long literals (>= 1 KiB HBM ->
// HBM), copy-4, literal length codes 61..63 and the stream's last kBatchIn bytes (a far copy
// there goes through stream_ring.hip.h's match_copy, with the same fence).
namespace snd {

using namespace sr;

// a whole-buffer stream decodes as fragments of kJoinBlock output bytes; a fragment's elements
// take at most 5 stream bytes per output byte (a copy-4 of one byte)
constexpr uint32_t kJoinBlock = 65536;
constexpr uint64_t kJoinMaxFragment = 5ull * kJoinBlock;

// stream bytes a batch may touch past ip: 64 candidate elements, the last a literal with a
// length byte and 64 bytes, or a copy-4's five bytes
constexpr uint32_t kBatchIn = 144;
// walk word: the next element's lane (<= 63 + 2 + 64) | kNextStop if that lane is not an
// eligible element, so the walk goes on exactly while the word is < 64
constexpr uint32_t kNextStop = 256;

// The chain walk (lz4_decompress.hip, walk_chain): from lane 0 (eligible: the caller's test),
// set every chain lane in `chain`; one v_readlane (the word read is the next lane select), one
// s_bitset1, one compare and one branch per element.  Returns the word that ended the walk.
#define BITAR_SN_LINK                       \
  "s_bitset1_b64 %[ch], %[l]\n"             \
  "v_readlane_b32 %[l], %[nx], %[l]\n"      \
  "s_nop 0\n"
#define BITAR_SN_STEP BITAR_SN_LINK "s_cmp_gt_u32 %[l], 63\n" "s_cbranch_scc1 L_so_%=\n"
#define BITAR_SN_STEP4 BITAR_SN_STEP BITAR_SN_STEP BITAR_SN_STEP BITAR_SN_STEP
__device__ __forceinline__ uint32_t walk_chain(uint32_t nx, uint64_t& chain) {
  uint32_t l = 0;
  __asm__ volatile(
      "L_sc_%=:\n"
      BITAR_SN_STEP4 BITAR_SN_STEP4 BITAR_SN_STEP4 BITAR_SN_STEP BITAR_SN_STEP BITAR_SN_STEP
      BITAR_SN_LINK
      "s_cmp_lt_u32 %[l], 64\n"
      "s_cbranch_scc1 L_sc_%=\n"
      "L_so_%=:\n"
      : [l] "+s"(l), [ch] "+s"(chain)
      : [nx] "v"(nx)
      : "scc");
  return l;
}

}  // namespace snd

// JOINED: fragment i of ONE whole-buffer stream (bitar_hip_snappy_decompress_joined, DESIGN.md
// 4.23) instead of segment i of a slab.  The stream is at `slab`, its fragment starts (uint64,
// nseg + 1 of them, as snappy_scan_* wrote them) at `srcs`, its declared length in `slot_stride`
// and its size in bytes in `seg` (the block is kJoinBlock); `csizes` is not read.  A fragment
// has no preamble: its length is the block, or what is left of the declared length.
template <bool JOINED>
__global__ __launch_bounds__(64) void snappy_decompress_kernel(
    const uint8_t* const* __restrict__ srcs, const uint8_t* __restrict__ slab,
    uint64_t slot_stride, const uint32_t* __restrict__ csizes, uint32_t nseg, uint32_t seg,
    uint8_t* __restrict__ out, uint32_t* __restrict__ produced, uint32_t* __restrict__ err,
    const uint32_t* __restrict__ order) {
  using namespace snd;
  // the ring at LDS address 0: a history source is then (address & mask)
  __shared__ __attribute__((aligned(16))) uint8_t lds[kRing + kWin];
  __shared__ uint32_t marks[kWave + 1];  // element starts of the current step; + trash
  uint8_t* ring = lds;
  uint8_t* win = lds + kRing;
  if (blockIdx.x >= nseg) return;
  // cost-ordered dispatch (seg_order_kernel): workgroup b decodes segment order[b]
  const uint32_t i = order ? order[blockIdx.x] : blockIdx.x;

  State s;
  bool ok = false;
  uint32_t dlen = 0;
  if constexpr (JOINED) {
    // starts the scan did not write are all ones: such a fragment reads nothing and rejects
    const uint64_t* starts = reinterpret_cast<const uint64_t*>(srcs);
    const uint64_t s0 = starts[i], s1 = starts[i + 1];
    ok = (s0 <= s1) & (s1 <= (uint64_t)seg) & (s1 - s0 <= kJoinMaxFragment);
    const uint64_t left = slot_stride - (uint64_t)i * kJoinBlock;
    dlen = left < kJoinBlock ? (uint32_t)left : kJoinBlock;
    s.src = global_ptr(slab + (ok ? s0 : 0ull));
    s.csize = ok ? (uint32_t)(s1 - s0) : 0u;
    s.dst = global_ptr(out + (uint64_t)i * kJoinBlock);
  } else {
    s.src = global_ptr(srcs ? srcs[i] : slab + (uint64_t)i * slot_stride);
    s.csize = csizes[i];
    s.dst = global_ptr(out + (uint64_t)i * seg);
  }
  s.cap = seg;
  s.ip = 0;
  s.op = 0;
  s.flushed = 0;
  s.fenced = 0;
  s.wb = ~0ull;  // nothing staged
  s.wlen = 0;
  const uint32_t lane = lane_id();
  const uint32_t base = (uint32_t)(uintptr_t)s.dst;  // ring index = absolute address & mask
  marks[lane] = 0;
  lds_order();

  // the preamble: a varint of <= 5 bytes whose fifth is below 16 (need not be minimal); a
  // declared length above the segment's capacity fails the segment
  if constexpr (!JOINED) {
    for (uint32_t k = 0; k < 5 && s.ip < s.csize; ++k) {
      const uint32_t c = byte_u(s, win, s.ip);
      s.ip += 1;
      if (k == 4 && c >= 16u) break;
      dlen |= (c & 127u) << (7 * k);
      if (c < 128u) { ok = true; break; }
    }
    if (dlen > seg) ok = false;
  }
  s.cap = ok ? dlen : 0u;  // every store below is bounded by the declared length <= seg

  while (ok && s.ip < s.csize) {
    if (s.ip + kBatchIn <= s.csize) {
      // ---- the batch -------------------------------------------------------------------
      const uint32_t wrel = win_at(s, win, s.ip, kBatchIn);
      lds_order();
      const uint32_t wc = wrel + lane;
      const uint32_t tag = win[wc], b1 = win[wc + 1], b2 = win[wc + 2];
      const uint32_t kind = tag & 3u, code = tag >> 2;
      const bool lit = kind == 0u;
      const uint32_t lhdr = code < 60u ? 1u : 2u;
      const uint32_t llen = code < 60u ? code + 1u : b1 + 1u;
      const bool c1 = kind == 1u;
      const uint32_t clen = c1 ? 4u + (code & 7u) : code + 1u;
      const uint32_t coff = c1 ? ((tag >> 5) << 8) | b1 : b1 | (b2 << 8);
      // bitwise on the compares: short-circuit forms compile to exec-mask branches
      const bool lit_ok = lit & (code <= 60u) & (llen <= kWave);
      const bool cp_ok = (c1 | (kind == 2u)) & (coff != 0u);
      const uint32_t len = lit ? llen : clen;
      const uint32_t nxt = lane + (lit ? lhdr + llen : c1 ? 2u : 3u);
      const uint64_t E = ballot(lit_ok | cp_ok);
      if (E & 1ull) {
        const uint32_t inel = (uint32_t)(~E >> (nxt & 63u)) & 1u;
        uint64_t chain = 0;
        const uint32_t stop = walk_chain(nxt | (inel * kNextStop), chain);
        const uint32_t adv = stop & (kNextStop - 1u);
        const bool in = (chain >> lane) & 1ull;
        const uint32_t e = in ? len : 0u;
        const uint32_t incl = wave_incl_sum(e);
        const uint32_t total = readlane(incl, kWave - 1);
        const uint32_t os = incl - e;  // the element's first byte, against the batch's
        // the declared length, and every copy against the bytes produced before it
        if (total > s.cap - s.op) { ok = false; break; }
        if (ballot(in & !lit & (coff > s.op + os))) { ok = false; break; }
        // per element: offset | first byte << 16 | copy << 31; LDS address of its literals
        // less its first byte (so a byte's literal is at w1 + q)
        const uint32_t w0 = coff | (os << 16) | (lit ? 0u : 0x80000000u);
        const uint32_t w1 = kRing + wc + lhdr - os;
        const uint32_t op0 = s.op;
        // does any copy of the batch reach beyond the ring?  (one ballot per batch: the steps
        // of a batch that has none -- every batch of this engine's own streams -- skip the far
        // source's marking and its test)
        const uint64_t anyfar = ballot(in & !lit & (coff > kNearOff));
        const uint32_t rb0 = base + op0;  // ring index of byte q = (rb0 + q) & mask
        const uint32_t mark = lane + 1u;
        uint32_t carry = 0;  // lane + 1 of the last element starting before the step
        for (uint32_t R = 0; R < total; R += kWave) {
          if (s.op + kWave - s.flushed > kFlushAt) flush(s, ring, s.op, false);
          // whose byte: the elements starting in the step mark their first byte's lane
          const uint32_t d = os - R;
          lds_order();
          marks[(in & (d < kWave)) ? d : kWave] = mark;
          lds_order();
          const uint32_t mk = marks[lane];
          marks[lane] = 0;
          lds_order();
          const uint32_t key = max(wave_incl_max(mk), carry);  // >= 1: byte 0 starts an element
          carry = readlane(key, kWave - 1);
          const int from = (int)((key - 1u) << 2);
          const uint32_t r0 = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)w0);
          const uint32_t r1 = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)w1);
          const uint32_t q = R + lane;
          const uint32_t ros = (r0 >> 16) & 0xFFFu, roff = r0 & 0xFFFFu;
          // a copy's source q - off; overlapping (inside the element itself): folded into the
          // first period, ros + (m mod off) - off with m = q - ros (exact in fp32: both < 64)
          int32_t srel = (int32_t)q - (int32_t)roff;
          if (ballot(srel >= (int32_t)ros)) {
            const uint32_t m = (q - ros) & 63u;
            const float qf = floorf(((float)m + 0.5f) *
                                    __builtin_amdgcn_rcpf((float)(roff > 1u ? roff : 1u)));
            const int32_t sf = (int32_t)(ros + m - (uint32_t)qf * roff) - (int32_t)roff;
            srel = srel >= (int32_t)ros ? sf : srel;
          }
          // a window literal, ring history, or an earlier byte of this step (bit 31 | lane)
          uint32_t st = srel >= (int32_t)R ? ((uint32_t)srel - R) | 0x80000000u
                                           : (rb0 + (uint32_t)srel) & kRingMask;
          st = (r0 >> 31) ? st : r1 + q;
          // a source beyond the ring's reach: bit 30 | its output position (< 2^16), which a
          // byte aliasing this one inherits through the pointer doubling
          if (BITAR_RARE(anyfar != 0)) {
            const bool farsrc = ((r0 >> 31) != 0u) & (roff > kNearOff);
            st = farsrc ? 0x40000000u | (op0 + (uint32_t)srel) : st;
          }
          st = q < total ? st : 0u;
          // pointer doubling: every alias chain strictly descends, so <= 6 rounds
          for (uint32_t n = 0; n < 7 && ballot((int32_t)st < 0); ++n) {
            const uint32_t o = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(st << 2), (int)st);
            st = (int32_t)st < 0 ? o : st;
          }
          lds_order();
          uint32_t g = lds[min(st, kRing + kWin - 1u)];  // (resolved: the min is a guard)
          if (BITAR_RARE(anyfar != 0)) {
            const bool far = (st >> 30) == 1u;
            // history only in HBM (> kNearOff behind this step: flushed long ago; at or past
            // position 0 by the offset check above): make the flushed stores visible first
            const uint32_t fsrc = st & 0xFFFFu;
            if (ballot(far & (fsrc >= s.fenced))) {
              global_fence_wave();
              s.fenced = s.flushed;
            }
            if (far) g = s.dst[fsrc];
          }
          if (q < total) ring[(rb0 + q) & kRingMask] = (uint8_t)g;
          lds_order();
          s.op += total - R < kWave ? total - R : kWave;
        }
        s.ip += adv;
        if (adv >= kWave) continue;  // the chain left the parsed window: parse on
      }
    }
    if (s.ip >= s.csize) break;
    // ---- general path: one element, any shape ---------------------------------------------
    const uint32_t tag = byte_u(s, win, s.ip);
    const uint32_t kind = tag & 3u, code = tag >> 2;
    if (kind == 0u) {
      const uint32_t nx = code < 60u ? 0u : code - 59u;
      if (s.ip + 1u + nx > s.csize) { ok = false; break; }
      uint64_t v = code;
      if (nx) {
        v = 0;
        for (uint32_t k = 0; k < nx; ++k) v |= (uint64_t)byte_u(s, win, s.ip + 1u + k) << (8 * k);
      }
      s.ip += 1u + nx;
      const uint64_t len = v + 1u;
      if (s.ip + len > s.csize || s.op + len > s.cap) { ok = false; break; }
      if (len >= kLongLit) literals_long(s, win, ring, (uint32_t)len);
      else literals_short(s, win, ring, (uint32_t)len);
    } else {
      const uint32_t nx = kind == 1u ? 1u : kind == 2u ? 2u : 4u;
      if (s.ip + 1u + nx > s.csize) { ok = false; break; }
      uint32_t v = 0;
      for (uint32_t k = 0; k < nx; ++k) v |= byte_u(s, win, s.ip + 1u + k) << (8 * k);
      s.ip += 1u + nx;
      const uint32_t len = kind == 1u ? 4u + (code & 7u) : code + 1u;
      const uint32_t off = kind == 1u ? ((tag >> 5) << 8) | v : v;
      if (off - 1u >= s.op || len > s.cap - s.op) { ok = false; break; }  // (off 0 wraps)
      match_copy(s, ring, off, len);
    }
  }
  // the elements consumed the input exactly (the loop's condition); the length must be met too
  if (ok && s.op != dlen) ok = false;
  if (ok) {
    flush(s, ring, s.op, true);
    if (lane == 0) produced[i] = s.op;
  } else if (lane == 0) {
    produced[i] = 0xFFFFFFFFu;
    atomicOr(err, 1u);
  }
}

template __global__ void snappy_decompress_kernel<false>(const uint8_t* const*, const uint8_t*,
                                                        uint64_t, const uint32_t*, uint32_t,
                                                        uint32_t, uint8_t*, uint32_t*, uint32_t*,
                                                        const uint32_t*);
template __global__ void snappy_decompress_kernel<true>(const uint8_t* const*, const uint8_t*,
                                                       uint64_t, const uint32_t*, uint32_t,
                                                       uint32_t, uint8_t*, uint32_t*, uint32_t*,
                                                       const uint32_t*);

// the cost key of fragment i of a joined stream: the slab decode's key of its coded size
// (util_kernels.hip order_key: the largest first, stored fragments last)
__global__ __launch_bounds__(256) void snappy_joined_key_kernel(const uint64_t* __restrict__ starts,
                                                                uint32_t nfrag,
                                                                uint32_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nfrag) return;
  const uint64_t s0 = starts[i], s1 = starts[i + 1];
  const uint64_t c = s1 >= s0 ? s1 - s0 : 0;
  keys[i] = c >= snd::kJoinBlock
                ? kOrderBins - 1u
                : kOrderBins - 2u - (uint32_t)(c * (kOrderBins - 2u) / snd::kJoinBlock);
}

// ---- whole-buffer streams: the join and the boundary scan -------------------
// snappy_join_sizes_kernel + scan_sizes_kernel + snappy_join_kernel write ONE raw stream from
// the slots of a compress at 64 KiB segments: varint(n), then every segment's stream less its
// own (minimal) preamble.  Stock readers decode it, and output position k * 65536 begins at an
// element start in it.  The snappy_scan_* kernels find those starts in ANY raw stream (stock
// writers cut at 64 KiB of input too) without a serial walk of the buffer:
//   * the stream is cut into tiles of kTile bytes, a wave per tile.  A tile walk is the
//     decoder's parse of "an element at position ip + lane" with walk_chain, without the output
//     gather: from an entry e inside the tile it gives x, the first chain position at or past
//     the tile's end (kInf when an element reads past the stream), and o, the output bytes of
//     the elements that started in the tile;
//   * round 1 walks every tile from a guess (tile 0 from the byte after the preamble, tile j
//     from j * kTile); a wrong chain usually merges with the true one inside the tile;
//   * the resolve (one wave) carries the true chain position c over the tiles' latest x; a
//     tile whose entry is not c is dirty -- unless the first few elements from c leave the tile
//     by themselves, whose end and output are then the tile's record (incompressible data: long
//     literals from mid-tile to mid-tile) -- and the next round walks the dirty tiles only.
//     Past a dirty tile the resolve goes on with the x of the tile's round-1 walk, not with
//     the latest: a walk from a wrong entry that did not merge ends on a wrong chain, and in
//     periodic data (columns) a wrong chain can hold for many tiles; the guesses start afresh
//     at every tile;
//   * at the fixpoint every active tile's (entry, x, o) is one walk's and entry[j + 1] == x[j]
//     from the preamble on: the true chain.  Every round makes the first dirty tile final, and
//     after the caller's bound of rounds one wave walks from the first unsettled tile to the end;
//   * the finish: a tile whose output range holds a multiple of 65536 walks once more with
//     the running count, writes starts[k] where an element starts at k * 65536 and reports an
//     element that straddles one.
// No workgroup waits for another: the order is the kernels' on the stream.  A record is written
// whole by one wave (the tile's walk, or the resolve for a tile it settles itself).
namespace sns {

using snd::kJoinBlock;
using snd::kNextStop;
using snd::walk_chain;

#ifndef BITAR_SNAPPY_TILE
#define BITAR_SNAPPY_TILE 4096
#endif
constexpr uint32_t kTile = BITAR_SNAPPY_TILE;
constexpr uint32_t kStage = kTile + 80;  // a walk parses 64 positions of up to 5 header bytes
constexpr uint32_t kInf = 0xFFFFFFFFu;
// The resolve follows the chain itself from a new entry for up to kFollow elements, as long as
// they average kFollowBytes of the stream from the second on: where the chain is sparse -- long
// literals with a copy between them, each landing mid-tile -- a tile walk from a wrong entry
// rarely meets it, and every landing would cost a round.  Dense chains are the tile walks'.
constexpr uint32_t kFollow = 16, kFollowBytes = 64;
static_assert(kStage % 16 == 0 && kTile % 64 == 0, "tiles are staged in 16-byte blocks");

// status values (include/bitar_hip.h): a worse one replaces a better one (atomicMax)
constexpr uint32_t kOk = 0, kUnsupported = 1, kInvalid = 2, kIncomplete = 3;

// control words of one scan
enum : uint32_t { cNDirty, cFirst, cDone, cRounds, cWalks, cSettled, cP0, cSerial, cWords };

struct El {
  uint32_t next;  // position of the next element; kInf: this one reads past the stream
  uint32_t out;   // its output bytes
};

// the element at pos from its tag and the four bytes behind it (whatever lies past the stream
// is never used: an element whose header or literal leaves [0, len) is kInf)
__device__ __forceinline__ El parse_el(uint32_t tag, uint32_t b1, uint32_t b2, uint32_t b3,
                                       uint32_t b4, uint32_t pos, uint32_t len) {
  const uint32_t kind = tag & 3u, code = tag >> 2;
  const bool lit = kind == 0u;
  const uint32_t nx = code < 60u ? 0u : code - 59u;  // a literal's length bytes
  const uint32_t ext = b1 | (b2 << 8) | (b3 << 16) | (b4 << 24);
  const uint32_t m = nx == 0u ? code : nx == 4u ? ext : ext & ((1u << (8u * nx)) - 1u);
  const uint32_t hdr = lit ? 1u + nx : kind == 1u ? 2u : kind == 2u ? 3u : 5u;
  const uint32_t rem = len - pos;
  // bitwise: the compares stay vector compares
  const bool bad = (pos >= len) | (hdr > rem) | (lit & (m >= rem - hdr));
  El e;
  e.next = bad ? kInf : pos + hdr + (lit ? m + 1u : 0u);
  e.out = lit ? m + 1u : kind == 1u ? 4u + (code & 7u) : code + 1u;
  return e;
}

// the element at the wave-uniform position pos, read from HBM (inside [0, len) only)
__device__ __forceinline__ El parse_at(const GMEM uint8_t* src, uint32_t pos, uint32_t len) {
  uint32_t b[5];
#pragma unroll
  for (uint32_t k = 0; k < 5; ++k) b[k] = (pos < len && k < len - pos) ? src[pos + k] : 0u;
  return parse_el(b[0], b[1], b[2], b[3], b[4], pos, len);
}

// stream bytes [tb, tb + kStage) into buf, zeros past the stream's end
__device__ __forceinline__ void stage_tile(uint8_t* buf, const GMEM uint8_t* src, uint32_t tb,
                                           uint32_t len) {
  lds_order();
  for (uint32_t i = 16u * lane_id(); i < kStage; i += 16u * kWave) {
    const uint64_t a = (uint64_t)tb + i;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (a + 16 <= len) {
      __builtin_memcpy(&v, (const void*)(src + a), 16);
    } else if (a < len) {
      uint32_t w[4] = {0, 0, 0, 0};
      for (uint32_t k = 0; k < (uint32_t)(len - a); ++k) w[k >> 2] |= (uint32_t)src[a + k] << (8u * (k & 3u));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(buf + i) = v;
  }
  lds_order();
}

// The tile walk over a staged tile [tb, end): from e (tb <= e, e < end or nothing to do) to x
// and o.  FIN: with the running output count `base` at e, the block starts among the elements
// are written and a straddling element is reported.  At most kTile / 2 steps (an element is at
// least 2 bytes); a step parses 64 positions and follows the chain through them.
template <bool FIN>
__device__ __forceinline__ void tile_walk(const uint8_t* buf, uint32_t tb, uint32_t end,
                                          uint32_t len, uint32_t e, uint32_t& x, uint32_t& o,
                                          uint64_t base, uint64_t n, uint64_t* __restrict__ starts,
                                          bool& straddle) {
  const uint32_t lane = lane_id();
  uint32_t ip = e, sum = 0;
  for (uint32_t it = 0; it < kTile && ip < end; ++it) {
    const uint32_t r = ip - tb + lane;
    const uint32_t pos = ip + lane;
    const El el = parse_el(buf[r], buf[r + 1], buf[r + 2], buf[r + 3], buf[r + 4], pos, len);
    const uint64_t E = ballot(el.next != kInf) & ballot(pos < end);
    if (!(E & 1ull)) {  // (ip < end: the element at ip reads past the stream)
      x = kInf;
      o = sum;
      return;
    }
    const uint32_t esz = el.next - pos;
    const uint32_t nl = lane + (esz < kWave ? esz : kWave);  // < 128
    const uint32_t inel = (uint32_t)(~E >> (nl & 63u)) & 1u;
    uint64_t chain = 0;
    walk_chain(nl | (inel * kNextStop), chain);
    const bool in = (chain >> lane) & 1ull;
    const uint32_t eo = in ? el.out : 0u;
    const uint32_t incl = wave_incl_sum(eo);
    if constexpr (FIN) {
      const uint64_t a = base + sum + (incl - eo);
      if (in & ((a & (kJoinBlock - 1u)) == 0u) & (a < n)) starts[a >> 16] = pos;
      const uint64_t above = (a | (kJoinBlock - 1u)) + 1u;
      if (ballot(in & (above < a + eo) & (above < n))) straddle = true;
    }
    sum += readlane(incl, kWave - 1);
    ip = readlane(el.next, 63u - (uint32_t)__builtin_clzll(chain));
  }
  x = ip;
  o = sum;
}

}  // namespace sns

// body size of segment i: its stream less its minimal preamble; a failed segment
// (BITAR_HIP_SEGMENT_ERROR) or a size no segment of this length can have stays as it is and
// is clamped to 0 by the scan that follows (bit 2 of the error word)
__global__ __launch_bounds__(256) void snappy_join_sizes_kernel(const uint32_t* __restrict__ sizes,
                                                                uint32_t nseg, uint64_t n,
                                                                uint32_t* __restrict__ body) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nseg) return;
  const uint64_t left = n - (uint64_t)i * sns::kJoinBlock;
  const uint32_t len = left < sns::kJoinBlock ? (uint32_t)left : sns::kJoinBlock;
  const uint32_t nb = len < 128u ? 1u : len < 16384u ? 2u : 3u;
  const uint32_t sz = sizes[i];
  body[i] = (sz < nb || sz > len + 6u) ? 0xFFFFFFFFu : sz - nb;
}

// workgroup 0: varint(n) at the stream's head, its length at *joined_len; workgroup i + 1: the
// body of segment i at pre + offsets[i] (offsets: the exclusive prefix sum of the body sizes).
// A stream above `capacity` is not written at all (bit 1 of the error word).
__global__ __launch_bounds__(64) void snappy_join_kernel(
    const uint8_t* __restrict__ slab, uint64_t stride, const uint32_t* __restrict__ body,
    uint64_t* __restrict__ offsets, uint32_t nseg, uint64_t n, uint8_t* __restrict__ joined,
    uint64_t capacity, uint64_t* __restrict__ joined_len, uint32_t* __restrict__ err) {
  const uint32_t lane = lane_id();
  uint32_t pre = 1;
  for (uint64_t v = n >> 7; v; v >>= 7) ++pre;  // <= 10 bytes
  const uint64_t total = pre + offsets[nseg];
  const bool fits = joined != nullptr && total <= capacity;
  if (blockIdx.x == 0) {
    if (lane == 0) {
      if (joined_len != nullptr) *joined_len = total;
      if (joined != nullptr && total > capacity) atomicOr(err, 2u);
    }
    if (fits && lane < pre)
      joined[lane] = (uint8_t)(((n >> (7u * lane)) & 127u) | (lane + 1u < pre ? 128u : 0u));
    return;
  }
  const uint32_t i = blockIdx.x - 1u;
  if (i >= nseg || !fits) return;
  const uint32_t b = body[i];
  if (b == 0xFFFFFFFFu) return;  // (a failed segment joins as nothing)
  const uint64_t left = n - (uint64_t)i * sns::kJoinBlock;
  const uint32_t len = left < sns::kJoinBlock ? (uint32_t)left : sns::kJoinBlock;
  const uint32_t nb = len < 128u ? 1u : len < 16384u ? 2u : 3u;
  wave_copy_global(global_ptr(joined + pre + offsets[i]),
                   global_ptr(slab + (uint64_t)i * stride + nb), b);
}

// starts[0, nfrag] = all ones (what no walk writes stays a reject for the fragment decoder);
// thread 0 reads the preamble (<= 5 bytes, the fifth below 16, need not be minimal) and sets
// the scan's control words.  status: kOk, or kInvalid without a preamble (then nothing else runs).
__global__ __launch_bounds__(256) void snappy_scan_init_kernel(
    const uint8_t* __restrict__ src, uint32_t len, uint64_t nfrag, uint64_t* __restrict__ starts,
    uint32_t* __restrict__ ctl, uint4* __restrict__ cur, uint32_t* __restrict__ status,
    uint32_t hopeless) {
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k <= nfrag; k += 256ull * gridDim.x)
    starts[k] = ~0ull;
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t p0 = 0;
  bool ok = false;
  for (uint32_t k = 0; k < 5 && k < len; ++k) {
    const uint32_t c = src[k];
    if (k == 4 && c >= 16u) break;
    if (c < 128u) {
      ok = true;
      p0 = k + 1;
      break;
    }
  }
  ok = ok && !hopeless;
  for (uint32_t k = 0; k < sns::cWords; ++k) ctl[k] = 0;
  ctl[sns::cP0] = p0;
  ctl[sns::cDone] = ok ? 0u : 1u;
  cur[0] = make_uint4(p0, 0u, 0u, 0u);
  *status = ok ? sns::kOk : sns::kInvalid;
}

// The walks of one round: round 1 (list == nullptr) every tile from its guess, later rounds
// the tiles of the dirty list from their new entries.  A workgroup takes tiles blockIdx.x,
// + gridDim.x, ...: at most ntile of them.
__global__ __launch_bounds__(64) void snappy_scan_walk_kernel(
    const uint8_t* __restrict__ src, uint32_t len, uint32_t ntile, const uint32_t* __restrict__ ctl,
    uint4* __restrict__ rec, uint2* __restrict__ guess, const uint2* __restrict__ list) {
  using namespace sns;
  __shared__ __attribute__((aligned(16))) uint8_t buf[kStage];
  if (ctl[cDone]) return;
  const uint32_t count = list ? min(ctl[cNDirty], ntile) : ntile;
  const uint32_t p0 = ctl[cP0];
  const GMEM uint8_t* s = global_ptr(src);
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    uint32_t j = i, e = i == 0 ? p0 : i * kTile;
    if (list) {
      const uint2 d = list[i];
      j = uniform(d.x);
      e = uniform(d.y);
    }
    if (j >= ntile) continue;  // (the list is the resolve's: never taken)
    const uint32_t tb = j * kTile;
    const uint64_t te = (uint64_t)tb + kTile;
    const uint32_t end = te < len ? (uint32_t)te : len;
    stage_tile(buf, s, tb, len);
    uint32_t x, o;
    bool unused = false;
    tile_walk<false>(buf, tb, end, len, e, x, o, 0, 0, nullptr, unused);
    if (lane_id() == 0) {
      rec[j] = make_uint4(e, x, o, 0u);
      if (!list) guess[j] = make_uint2(x, o);  // round 1's result stays (the resolve's estimate)
    }
  }
}

// The resolve, one wave: from the first tile that is not final, 64 tiles per step.  The tiles
// of a step whose entries already continue the chain (entry == the x before it) are taken in
// one go, with a prefix sum of their o; the rest one by one, c and the output count in scalars.
// For those the element at the likely c (the x before the tile) is parsed by the tile's lane
// ahead of the scalar loop, so the loop waits for a load of its own only after a jump.
__global__ __launch_bounds__(64) void snappy_scan_resolve_kernel(
    const uint8_t* __restrict__ src, uint32_t len, uint64_t n, uint64_t nfrag, uint32_t ntile,
    uint32_t* __restrict__ ctl, uint4* __restrict__ rec, const uint2* __restrict__ guess,
    uint4* __restrict__ cur, uint2* __restrict__ list, uint64_t* __restrict__ starts,
    uint32_t* __restrict__ status) {
  using namespace sns;
  if (ctl[cDone]) return;
  const uint32_t lane = lane_id();
  const GMEM uint8_t* s = global_ptr(src);
  const uint32_t first = uniform(ctl[cFirst]);
  const uint32_t walked = ctl[cRounds] ? ctl[cNDirty] : ntile;
  const uint4 c0 = cur[first];
  uint32_t c = uniform(c0.x);
  uint64_t acc = uniform64((uint64_t)c0.z | ((uint64_t)c0.w << 32));
  uint32_t ndirty = 0, newfirst = ntile;
  for (uint32_t j0 = first; j0 < ntile; j0 += kWave) {
    const uint32_t j = j0 + lane;
    const bool live = j < ntile;
    const uint32_t cnt = ntile - j0 < kWave ? ntile - j0 : kWave;
    const uint4 r = live ? rec[j] : make_uint4(0, 0, 0, 0);
    const uint2 g = live ? guess[j] : make_uint2(0, 0);
    const uint32_t entry = r.x, x = r.y, o = r.z;
    const uint64_t te = ((uint64_t)j + 1u) * kTile;
    const uint32_t end = te < len ? (uint32_t)te : len;
    const uint32_t before = wave_shr1(x);
    const uint32_t prevx = lane == 0 ? c : before;
    // the step's leading tiles that continue the chain as they are
    const uint64_t cons = ballot(entry == prevx) & ballot(live);
    const uint32_t K = ~cons ? (uint32_t)__builtin_ctzll(~cons) : kWave;
    const uint32_t slo = wave_incl_sum(o & 0xFFFFu), shi = wave_incl_sum(o >> 16);
    const uint64_t incl = (uint64_t)slo + ((uint64_t)shi << 16);
    uint32_t curc = entry;
    uint64_t curb = acc + incl - o;
    if (K) {
      c = readlane(x, K - 1);
      acc += uniform64(((uint64_t)readlane(shi, K - 1) << 16) + readlane(slo, K - 1));
    }
    uint32_t nentry = 0, nx = 0, no = 0, dentry = 0;
    bool isnew = false, isdirty = false;
    if (K < cnt) {
      // the others: the element at x of the tile before, if that lies in this tile
      const bool want = live & (lane >= K) & (prevx < end) & (prevx >= j * kTile) & (prevx != entry);
      El cand, cand2;
      cand.next = cand2.next = kInf;
      cand.out = cand2.out = 0;
      if (want) {
        cand = parse_at(s, prevx, len);
        if (cand.next < end) cand2 = parse_at(s, cand.next, len);
      }
      const uint64_t parsed = ballot(want);
      for (uint32_t l = K; l < cnt; ++l) {
        uint32_t xl = readlane(x, l), ol = readlane(o, l);
        const uint32_t el = readlane(entry, l), endl = readlane(end, l);
        if (c >= endl) {
          // a long literal jumps over the tile, and over every tile up to the one that holds c
          const uint32_t to = c / kTile - j0;  // (c >= endl: past l; kInf: past every tile)
          const uint32_t stop = max(l + 1u, to < cnt ? to : cnt);  // (c == len in the last tile)
          const bool over = (lane >= l) & (lane < stop);
          curc = over ? c : curc;
          curb = over ? acc : curb;
          l = stop - 1u;
          continue;
        }
        const bool me = lane == l;
        curc = me ? c : curc;
        curb = me ? acc : curb;
        {
          if (el != c) {
            // follow the chain from c while it is sparse (see kFollow); the first two elements
            // are the lane's own parse where c is the x before the tile
            const bool spec = readlane(prevx, l) == c && ((parsed >> l) & 1ull);
            uint32_t q = c, osum = 0, nxt = 0;
            bool left = false;
            for (uint32_t k = 0; k < kFollow; ++k) {
              El p;
              if (spec && k < 2u) {
                p.next = readlane(k ? cand2.next : cand.next, l);
                p.out = readlane(k ? cand2.out : cand.out, l);
              } else {
                p = parse_at(s, q, len);
                p.next = uniform(p.next);
                p.out = uniform(p.out);
              }
              nxt = p.next;
              if (p.next >= endl) {  // the chain leaves the tile (or an element is cut)
                osum += p.next != kInf ? p.out : 0u;
                left = true;
                break;
              }
              osum += p.out;
              q = p.next;
              if (k >= 1u && q - c < kFollowBytes * (k + 1u)) break;
            }
            if (left) {
              nentry = me ? c : nentry;
              nx = me ? nxt : nx;
              no = me ? osum : no;
              isnew = isnew | me;
              xl = nxt;
              ol = osum;
            } else {
              // dirty: go on with the walk from the tile's guess, which no wrong entry made
              dentry = me ? c : dentry;
              isdirty = isdirty | me;
              // (a guess that ran into a garbage literal "past the stream" is no estimate: the
              // next tile's own guess entry is)
              xl = readlane(g.x, l);
              ol = readlane(g.y, l);
              xl = (xl == kInf && endl < len) ? endl : xl;
            }
          }
          c = xl;
          acc += ol;
        }
      }
    }
    if (live) cur[j] = make_uint4(curc, 0u, (uint32_t)curb, (uint32_t)(curb >> 32));
    if (isnew) rec[j] = make_uint4(nentry, nx, no, 0u);
    const uint64_t dm = ballot(isdirty);
    if (dm) {
      const uint32_t at = ndirty + __builtin_amdgcn_mbcnt_hi((uint32_t)(dm >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)dm, 0u));
      if (isdirty) list[at] = make_uint2(j, dentry);
      if (newfirst == ntile) newfirst = j0 + (uint32_t)__builtin_ctzll(dm);
      ndirty += (uint32_t)__builtin_popcountll(dm);
    }
  }
  if (lane != 0) return;
  ctl[cRounds] += 1u;
  ctl[cWalks] += walked;
  ctl[cNDirty] = ndirty;
  ctl[cFirst] = newfirst;
  ctl[cSettled] = newfirst;  // (ntile when nothing is dirty)
  if (ndirty == 0) {
    ctl[cDone] = 1u;
    if (c != len || acc != n) atomicMax(status, kInvalid);
    else starts[nfrag] = len;
  }
}

// After the last round: nothing to do when the resolve found no dirty tile.  Else one wave
// walks from the first unsettled tile (its c and output count are final) to the stream's end
// with the running count -- at most ntile tile walks -- or, where the caller forbade it, the
// status is kIncomplete.
__global__ __launch_bounds__(64) void snappy_scan_serial_kernel(
    const uint8_t* __restrict__ src, uint32_t len, uint64_t n, uint64_t nfrag, uint32_t ntile,
    uint32_t* __restrict__ ctl, const uint4* __restrict__ cur, uint64_t* __restrict__ starts,
    uint32_t* __restrict__ status, uint32_t allowed) {
  using namespace sns;
  __shared__ __attribute__((aligned(16))) uint8_t buf[kStage];
  if (ctl[cDone]) return;
  const uint32_t lane = lane_id();
  if (!allowed) {
    if (lane == 0) atomicMax(status, kIncomplete);
    return;
  }
  const GMEM uint8_t* s = global_ptr(src);
  const uint32_t f = uniform(ctl[cSettled]);
  const uint4 c0 = cur[f < ntile ? f : 0u];
  uint32_t c = uniform(c0.x);
  uint64_t acc = uniform64((uint64_t)c0.z | ((uint64_t)c0.w << 32));
  bool straddle = false;
  for (uint32_t it = 0; it < ntile && c < len; ++it) {
    const uint32_t tb = c / kTile * kTile;
    const uint64_t te = (uint64_t)tb + kTile;
    const uint32_t end = te < len ? (uint32_t)te : len;
    stage_tile(buf, s, tb, len);
    uint32_t x, o;
    tile_walk<true>(buf, tb, end, len, c, x, o, acc, n, starts, straddle);
    c = x;
    acc += o;
  }
  if (lane != 0) return;
  ctl[cSerial] = 1u;
  if (c != len || acc != n) atomicMax(status, kInvalid);
  else starts[nfrag] = len;
  if (straddle) atomicMax(status, kUnsupported);
}

// The finish, a wave per settled tile: an active tile whose output range [base, base + o)
// holds a multiple of 65536 walks once more with the running count.
__global__ __launch_bounds__(64) void snappy_scan_finish_kernel(
    const uint8_t* __restrict__ src, uint32_t len, uint64_t n, uint32_t ntile,
    const uint32_t* __restrict__ ctl, const uint4* __restrict__ rec, const uint4* __restrict__ cur,
    uint64_t* __restrict__ starts, uint32_t* __restrict__ status) {
  using namespace sns;
  __shared__ __attribute__((aligned(16))) uint8_t buf[kStage];
  const uint32_t j = blockIdx.x;
  if (j >= ntile || j >= ctl[cSettled]) return;
  const uint4 cu = cur[j];
  const uint4 r = rec[j];
  const uint32_t tb = j * kTile;
  const uint64_t te = (uint64_t)tb + kTile;
  const uint32_t end = te < len ? (uint32_t)te : len;
  const uint32_t c = uniform(cu.x);
  const uint64_t base = uniform64((uint64_t)cu.z | ((uint64_t)cu.w << 32));
  const uint32_t o = uniform(r.z);
  if (c >= end || c != uniform(r.x)) return;  // jumped over (a settled tile's entry is its c)
  const uint64_t border = (base + (kJoinBlock - 1u)) & ~(uint64_t)(kJoinBlock - 1u);
  if (border >= base + o || border >= n) return;
  stage_tile(buf, global_ptr(src), tb, len);
  uint32_t x, o2;
  bool straddle = false;
  tile_walk<true>(buf, tb, end, len, c, x, o2, base, n, starts, straddle);
  if (straddle && lane_id() == 0) atomicMax(status, kUnsupported);
}

}  // namespace bitar_hip
