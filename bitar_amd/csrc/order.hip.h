// order.hip.h -- cost-ordered dispatch: the key range and the tiling of the counting sort
// (util_kernels.hip order_hist_kernel / order_scatter_kernel; runtime.hip SegOrder), and the
// priority lanes of the fast LZ4 compressor.
#pragma once
#include <stdint.h>

namespace bitar_hip {

constexpr uint32_t kOrderBins = 256;  // sort keys are < kOrderBins (lowest first)
constexpr uint32_t kOrderMaxTiles = 64;

// segments per tile: a multiple of 1024 (16 per lane), at most kOrderMaxTiles tiles
__host__ __device__ inline uint32_t order_tile(uint32_t nseg) {
  const uint32_t t = (nseg + kOrderMaxTiles - 1) / kOrderMaxTiles;
  return ((t < 1024u ? 1024u : t) + 1023u) & ~1023u;
}

// ---- priority lanes ------------------------------------------------------------------------
// A launch of H equally heavy segments over S resident workgroups runs q = H / S full rounds
// and one round of f = H - q S left-over segments: f slots run q + 1 heavy segments, the
// others q, and the launch ends with those f slots running nearly alone.  The workgroups of
// the q + 1 slots take a higher issue priority (s_setprio), so that they run faster beside
// the others and all slots end together.  The heavy segments are dispatched first (cost
// order), dispatch index b goes to slot b % S while every slot's segments take equally long,
// and a slot freed early is refilled by the next index of the same residue: the test holds
// for all q + 1 segments of a fast slot.
#ifndef BITAR_LANE_PRIO
#define BITAR_LANE_PRIO 1  // the fast lane's priority (1-3); 0 = no lanes, the kernels as before
#endif
constexpr uint32_t kLanePrio = BITAR_LANE_PRIO;
static_assert(kLanePrio <= 3, "s_setprio takes 0-3");

// The compress key (seg_cost_kernel: distinct byte values in a 128-byte sample) below which a
// segment counts as heavy.  The key is bimodal on mixed input (64 KiB segments of the
// generator's kinds 0, 1, 2, 5, 6): integer columns show 16-21, dictionary indices and log
// text 22-44, random bytes and the doubles of kind 2, which the parse skips through, 82-112;
// nothing lies between 44 and 82, and the cut sits in the middle of that gap.
constexpr uint32_t kCheapKey = 64;

// order_scatter_kernel, which holds every bin's total and so H, applies the rule and sets
// kLaneTag on the fast lane's entries of the order (the orders of lz4_compress_kernel<4096,
// 10> only, which strips it; the wide compressor and the LZ4 decoder were measured with lanes
// and lost more than they gained).  The kernel then needs no load and no
// division of its own: with H and S in front of the order and the rule in the kernels, the
// two-stream headline measured 0.9 % slower than the parent with the lanes off.
constexpr uint32_t kLaneTag = 0x80000000u;

// the priority of dispatch index b: H heavy segments, dispatched first; S resident workgroups
// of the kernel on the device (0: no lanes)
__host__ __device__ constexpr uint32_t lane_prio(uint32_t b, uint32_t H, uint32_t S) {
  if (S == 0 || b >= H) return 0;
  const uint32_t q = H / S, f = H - q * S;
  return q >= 1 && f > 0 && b % S < f ? kLanePrio : 0u;
}

namespace lane_rule_checks {
constexpr uint32_t S = 5120, P = kLanePrio;
// H = 0, and no slot count
static_assert(lane_prio(0, 0, S) == 0 && lane_prio(S, 0, S) == 0 && lane_prio(0, 100, 0) == 0);
// H < S: one partial round, nobody runs more than one heavy segment
static_assert(lane_prio(0, S - 1, S) == 0 && lane_prio(S - 2, S - 1, S) == 0);
static_assert(lane_prio(0, 1, S) == 0);
// H = k S: every slot runs k
static_assert(lane_prio(0, S, S) == 0 && lane_prio(S - 1, S, S) == 0);
static_assert(lane_prio(0, 3 * S, S) == 0 && lane_prio(2 * S, 3 * S, S) == 0 &&
              lane_prio(3 * S - 1, 3 * S, S) == 0);
// H = k S + 1: slot 0 alone runs k + 1, in every round
static_assert(lane_prio(0, S + 1, S) == P && lane_prio(1, S + 1, S) == 0 &&
              lane_prio(S, S + 1, S) == P && lane_prio(S - 1, S + 1, S) == 0);
static_assert(lane_prio(0, 2 * S + 1, S) == P && lane_prio(S, 2 * S + 1, S) == P &&
              lane_prio(2 * S, 2 * S + 1, S) == P && lane_prio(2 * S - 1, 2 * S + 1, S) == 0 &&
              lane_prio(S + 1, 2 * S + 1, S) == 0);
// the headline's compress (1 GiB of kind 1 on 256 CUs, measured): H = 10928 = 2 S + 688,
// every lane boundary; past H nothing
static_assert(lane_prio(687, 10928, S) == P && lane_prio(688, 10928, S) == 0 &&
              lane_prio(S - 1, 10928, S) == 0 && lane_prio(S, 10928, S) == P &&
              lane_prio(S + 687, 10928, S) == P && lane_prio(S + 688, 10928, S) == 0 &&
              lane_prio(2 * S, 10928, S) == P && lane_prio(10927, 10928, S) == P &&
              lane_prio(10928, 10928, S) == 0 && lane_prio(16383, 10928, S) == 0);
// H = nseg (homogeneous input): 16384 = 3 S + 1024
static_assert(lane_prio(0, 16384, S) == P && lane_prio(1023, 16384, S) == P &&
              lane_prio(1024, 16384, S) == 0 && lane_prio(3 * S, 16384, S) == P &&
              lane_prio(16383, 16384, S) == P && lane_prio(3 * S - 1, 16384, S) == 0);
// another slot count (6144): 10928 = S + 4784, 12288 = 2 S
static_assert(lane_prio(4783, 10928, 6144) == P && lane_prio(4784, 10928, 6144) == 0 &&
              lane_prio(6144, 10928, 6144) == P && lane_prio(6143, 10928, 6144) == 0 &&
              lane_prio(0, 12288, 6144) == 0 && lane_prio(6144, 12288, 6144) == 0);
}  // namespace lane_rule_checks

// ---- launch timeline (probe builds only: scripts/launch_timeline.py) -----------------------
// BITAR_LAUNCH_TIMELINE=1 makes the LZ4 kernels record, per workgroup, its dispatch index and
// segment and the device's wall clock (100 MHz) at entry and before exit: three 64-bit words
// at buf + 3 b, written by lane 0.  The buffer comes through a symbol of the probe build, set
// by an exported function, so that the kernels keep their argument lists.
#ifndef BITAR_LAUNCH_TIMELINE
#define BITAR_LAUNCH_TIMELINE 0
#endif
#if BITAR_LAUNCH_TIMELINE && defined(__HIPCC__)
#define BITAR_TIMELINE_BUFFER(symbol, setter)                                              \
  __device__ unsigned long long* symbol;                                                   \
  extern "C" __attribute__((visibility("default"))) int setter(void* buf) {                \
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(symbol), &buf, sizeof(buf));                  \
  }
__device__ __forceinline__ void timeline_record(unsigned long long* buf, uint32_t b,
                                                uint32_t segment, unsigned long long t0) {
  if (buf && threadIdx.x == 0) {
    buf[3ull * b] = (unsigned long long)b << 32 | segment;
    buf[3ull * b + 1] = t0;
    buf[3ull * b + 2] = wall_clock64();
  }
}
#endif

}  // namespace bitar_hip
