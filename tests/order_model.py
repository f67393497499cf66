"""numpy model of the cost-ordered dispatch (bitar_amd/csrc/order.hip.h, util_kernels.hip
seg_cost_kernel / order_key / order_scatter_kernel, runtime.hip SegOrder):
the tiling of the counting sort, the two cost keys, the priority lanes' rule, and check_order(),
what every order must satisfy whatever the sort does inside a key.  Test infrastructure only;
tests/test_order_model.py checks the model itself, tests/test_gpu_order.py the device's orders
(bitar_hip_debug_order) against it.
"""
import numpy as np

ORDER_BINS = 256      # kOrderBins: keys are clamped to ORDER_BINS - 1
ORDER_MAX_TILES = 64  # kOrderMaxTiles
ORDER_MIN_SEGS = 2048  # kOrderMinSegs: smaller calls run in plain order
CHEAP_KEY = 64        # kCheapKey: a compress key below it is a heavy segment
LANE_TAG = 0x80000000  # kLaneTag
WAVE = 64


def order_tile(nseg):
    """segments per tile of the counting sort: a multiple of 1024, at most 64 tiles"""
    t = (nseg + ORDER_MAX_TILES - 1) // ORDER_MAX_TILES
    return (max(t, 1024) + 1023) & ~1023


def lane_prio(b, H, S):
    """1 where dispatch index b (array or int) runs in a fast lane: H heavy segments dispatched
    first over S resident workgroups, q = H // S full rounds and f = H - q S left over; the f
    slots that run q + 1 heavy segments are the fast ones, in every round"""
    b = np.asarray(b, dtype=np.int64)
    if S == 0:
        return np.zeros(b.shape, dtype=np.int64)
    q, f = divmod(H, S)
    return ((b < H) & (q >= 1) & (f > 0) & (b % S < f)).astype(np.int64)


def tagged_count(H, S):
    """how many entries of an order carry the tag"""
    if S == 0 or H <= S:
        return 0
    q, f = divmod(H, S)
    return (q + 1) * f if q >= 1 and f > 0 else 0


def decompress_key(csize, seg):
    """order_key without caller keys: stored segments (csize >= seg) last, the others by coded
    size, the largest first"""
    c = np.asarray(csize).astype(np.uint64)
    coded = (ORDER_BINS - 2) - c * np.uint64(ORDER_BINS - 2) // np.uint64(seg)
    return np.where(c >= seg, ORDER_BINS - 1, coded).astype(np.int64)


def _sample_offsets(length):
    """the byte offsets seg_cost_kernel reads in a segment of `length` bytes: four samples at
    length * q / 4, 32 bytes each from 128 bytes up, min(32, length - start) below"""
    out = []
    for q in range(4):
        at = length * q // 4
        cnt = 32 if length >= 128 else min(32, length - at)
        out.append(at + np.arange(cnt, dtype=np.int64))
    return np.concatenate(out)


def _distinct(rows):
    """distinct values per row of a 2-D array with at least one column"""
    s = np.sort(rows, axis=1)
    return 1 + (s[:, 1:] != s[:, :-1]).sum(axis=1)


def cost_key(data, seg):
    """seg_cost_kernel: per segment of `data` (the last may be short) the number of distinct
    byte values among its sampled bytes"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    nseg = (n + seg - 1) // seg
    keys = np.zeros(nseg, dtype=np.int64)
    nfull = n // seg
    if nfull:
        keys[:nfull] = _distinct(data[:nfull * seg].reshape(nfull, seg)[:, _sample_offsets(seg)])
    if nfull < nseg:
        tail = data[nfull * seg:]
        keys[nfull] = _distinct(tail[_sample_offsets(tail.size)][None, :])[0]
    return keys


def check_order(order, keys, cut, slots):
    """what a dispatch order of nseg segments must satisfy: order (uint32, tags left in), keys
    (as written, before the clamp), and the lanes' cut and slot count it was built with.  The
    order inside a key is free, so nothing here compares against one fixed argsort."""
    order = np.asarray(order).astype(np.int64) & 0xFFFFFFFF
    keys = np.asarray(keys).astype(np.int64) & 0xFFFFFFFF
    nseg = keys.size
    assert order.shape == (nseg,)
    tag = (order & LANE_TAG) != 0
    idx = order & ~LANE_TAG
    # a permutation of 0..nseg-1
    assert idx.max() < nseg, f"entry {int(idx.argmax())} = {int(idx.max())} is no segment of {nseg}"
    seen = np.bincount(idx, minlength=nseg)
    assert (seen == 1).all(), (f"segment {int(np.flatnonzero(seen != 1)[0])} is dispatched "
                               f"{int(seen[np.flatnonzero(seen != 1)[0]])} times")
    # keys, clamped, never decrease along the order
    clamped = np.minimum(keys, ORDER_BINS - 1)
    k = clamped[idx]
    down = np.flatnonzero(k[1:] < k[:-1])
    assert down.size == 0, (f"dispatch index {int(down[0]) + 1}: key {int(k[down[0] + 1])} "
                            f"after key {int(k[down[0]])}")
    # tags: exactly the fast lanes' entries
    H = int((clamped < cut).sum())
    want = (lane_prio(np.arange(nseg), H, slots) != 0) if slots != 0 and H > slots else \
        np.zeros(nseg, dtype=bool)
    bad = np.flatnonzero(tag != want)
    assert bad.size == 0, (f"dispatch index {int(bad[0])}: tag {bool(tag[bad[0]])}, H = {H}, "
                           f"S = {slots}; {int(tag.sum())} tags for {int(want.sum())}")
    return H
