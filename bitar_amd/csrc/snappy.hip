// snappy.hip -- raw Snappy segments, one wavefront per segment (gfx950):
//   snappy_compress_kernel    the LZ4 codec's window-scan parse (window_parse.hip.h: SKIP, 4 KiB
//                             ring, 1024-entry table, distance cap 2560, LZ4 end rules) with a
//                             Snappy emitter; the stream is the LZ4 block's sequences re-emitted
//                             as Snappy elements (tests/snappy_model.py), or the stored form
//   snappy_decompress_kernel  any raw Snappy stream of <= 64 KiB (stock streams included), on
//                             the decoders' stream window + history ring (stream_ring.hip.h)
//
// Format (include/bitar_hip.h, BITAR_HIP_CODEC_SNAPPY): the segment's length as a varint, then
// elements -- a literal (tag (len-1) << 2, or 60 << 2 / 61 << 2 with 1 / 2 length bytes), a
// copy-1 (2 bytes: 4 <= len <= 11, offset < 2048) or a copy-2 (3 bytes: len <= 64, 16-bit
// offset).  A literal and the copy after it are separate elements, so a sequence costs two
// chain steps in the decoder where LZ4 has one token.
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
  s.src = global_ptr(srcs ? srcs[i] : slab + (uint64_t)i * slot_stride);
  s.csize = csizes[i];
  s.dst = global_ptr(out + (uint64_t)i * seg);
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
  bool ok = false;
  uint32_t dlen = 0;
  for (uint32_t k = 0; k < 5 && s.ip < s.csize; ++k) {
    const uint32_t c = byte_u(s, win, s.ip);
    s.ip += 1;
    if (k == 4 && c >= 16u) break;
    dlen |= (c & 127u) << (7 * k);
    if (c < 128u) { ok = true; break; }
  }
  if (dlen > seg) ok = false;
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

}  // namespace bitar_hip
