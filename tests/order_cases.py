"""Inputs shared by the dispatch-order tests (tests/test_order_model.py, tests/test_gpu_order.py)
and the priority-lane test (tests/test_gpu_priority_lanes.py): the lane test's segment size,
pools and heavy masks, and the key patterns of the counting sort.  Test infrastructure only."""
import numpy as np

import oracle_lib as O
import order_model as M

SEG = 4099  # the lane test's segments: odd, no multiple of any tile
LZ4C_WAVES_PER_CU = 20  # lz4_compress_kernel<4096,10>: 5 waves per SIMD


def big_nseg(cus):
    """the pools' size, and the tagged case's: one round of the fast compressor's resident
    workgroups on a device of `cus` CUs, and 2303 more"""
    return LZ4C_WAVES_PER_CU * cus + 2303


def masks(nseg):
    """name -> heavy[i]"""
    i = np.arange(nseg)
    one = i == nseg // 3
    return {
        "H0": np.zeros(nseg, bool),
        "H1": one,
        "Hn-1": ~one,
        "Hn": np.ones(nseg, bool),
        "half_heavy_first": i < nseg // 2,
        "half_heavy_last": i >= nseg // 2,
        "half_interleaved": (i & 1) == 0,
    }


def lane_pools(nmax):
    """(text, random) as (nmax, SEG) arrays: kind 1's log text (kind 6 is that region alone)
    for heavy segments, kind-0 random bytes for cheap ones"""
    text = O.fill(6, 7, nmax * SEG)
    rand = O.fill(0, 7, nmax * SEG)
    return text.reshape(nmax, SEG), rand.reshape(nmax, SEG)


def key_patterns(nseg):
    """name -> uint32 keys[nseg] for the counting sort: what order_runs' merging of equal
    neighbours (16 keys per batch, tile / 64 segments per lane), the clamp to 255 and the prefix
    over the tiles can get wrong"""
    tile = M.order_tile(nseg)
    per = tile // M.WAVE
    i = np.arange(nseg, dtype=np.int64)
    rng = np.random.default_rng(nseg)
    last_tile = i >= (nseg - 1) // tile * tile
    out = {
        "equal": np.full(nseg, 7),
        "run1": i % 256,
        "bins_0_255": rng.choice([0, 255], nseg),
        # 254 and 255 are keys of their own; 256 and above sort with 255
        "clamped": rng.choice([3, 254, 255, 256, 1000, 0xFFFFFFFF], nseg),
        "ascending": i * 256 // nseg,
        "descending": 255 - i * 256 // nseg,
        # the first tiles hold key 255 alone: every small key's position is a sum over them
        "small_in_last_tile": np.where(last_tile, i % 8, 255),
        "random": rng.integers(0, 256, nseg),
    }
    # runs that end one before, at and one after a 16-key batch and a lane's share of the tile
    for name, run in [("run15", 15), ("run16", 16), ("run17", 17), ("run_per-1", per - 1),
                      ("run_per", per), ("run_per+1", per + 1)]:
        out[name] = i // run % 256
    return {name: k.astype(np.uint32) for name, k in out.items()}


def keys_with_heavy(nseg, H, cut, seed=0):
    """uint32 keys[nseg], exactly H of them below `cut`, at scattered segments"""
    rng = np.random.default_rng(seed)
    keys = np.empty(nseg, dtype=np.uint32)
    where = rng.permutation(nseg)
    keys[where[:H]] = rng.integers(0, cut, H)
    keys[where[H:]] = rng.integers(cut, 300, nseg - H)
    return keys
