"""CPU tests of tests/order_model.py, the numpy model the device's dispatch orders are checked
against (tests/test_gpu_order.py): the model restates order.hip.h's own compile-time table, the
tiling, and the compress key's bimodality that kCheapKey = 64 rests on; and check_order()
rejects the orders it is there to reject."""
import numpy as np
import pytest

import oracle_lib as O
import order_cases as C
import order_model as M

# order.hip.h lane_rule_checks, transcribed: (b, H, S, 1 where the static_assert says P)
S = 5120
LANE_TABLE = [
    # H = 0, and no slot count
    (0, 0, S, 0), (S, 0, S, 0), (0, 100, 0, 0),
    # H < S
    (0, S - 1, S, 0), (S - 2, S - 1, S, 0), (0, 1, S, 0),
    # H = k S
    (0, S, S, 0), (S - 1, S, S, 0), (0, 3 * S, S, 0), (2 * S, 3 * S, S, 0), (3 * S - 1, 3 * S, S, 0),
    # H = k S + 1
    (0, S + 1, S, 1), (1, S + 1, S, 0), (S, S + 1, S, 1), (S - 1, S + 1, S, 0),
    (0, 2 * S + 1, S, 1), (S, 2 * S + 1, S, 1), (2 * S, 2 * S + 1, S, 1),
    (2 * S - 1, 2 * S + 1, S, 0), (S + 1, 2 * S + 1, S, 0),
    # H = 10928 = 2 S + 688
    (687, 10928, S, 1), (688, 10928, S, 0), (S - 1, 10928, S, 0), (S, 10928, S, 1),
    (S + 687, 10928, S, 1), (S + 688, 10928, S, 0), (2 * S, 10928, S, 1), (10927, 10928, S, 1),
    (10928, 10928, S, 0), (16383, 10928, S, 0),
    # H = nseg = 16384 = 3 S + 1024
    (0, 16384, S, 1), (1023, 16384, S, 1), (1024, 16384, S, 0), (3 * S, 16384, S, 1),
    (16383, 16384, S, 1), (3 * S - 1, 16384, S, 0),
    # S = 6144
    (4783, 10928, 6144, 1), (4784, 10928, 6144, 0), (6144, 10928, 6144, 1),
    (6143, 10928, 6144, 0), (0, 12288, 6144, 0), (6144, 12288, 6144, 0),
]


@pytest.mark.parametrize("b,H,slots,want", LANE_TABLE)
def test_lane_prio_is_the_headers_table(b, H, slots, want):
    assert int(M.lane_prio(b, H, slots)) == want
    assert int(M.lane_prio(np.array([b]), H, slots)[0]) == want


@pytest.mark.parametrize("H,slots", [(0, S), (S - 1, S), (S, S), (S + 1, S), (10928, S),
                                     (16384, S), (10928, 6144), (12288, 6144), (100, 0)])
def test_tagged_count_is_the_sum_of_the_rule(H, slots):
    n = 16384
    want = int(M.lane_prio(np.arange(n), H, slots).sum()) if slots and H > slots else 0
    assert M.tagged_count(H, slots) == want


def test_order_tile():
    """1024 up to 65536 segments (64 tiles of 1024), then the next multiple of 1024 that keeps
    the tiles at 64 or fewer"""
    assert [M.order_tile(n) for n in (2048, 65536, 65537, 131072, 131073)] == \
        [1024, 1024, 2048, 2048, 3072]
    for n in (2048, 65536, 65537, 131072, 131073, 1 << 31):
        t = M.order_tile(n)
        assert t % 1024 == 0 and (n + t - 1) // t <= M.ORDER_MAX_TILES


def test_decompress_key():
    seg = 4099
    c = np.array([0, 1, seg // 2, seg - 1, seg, seg + 1, 0xFFFFFFFF], dtype=np.uint32)
    assert M.decompress_key(c, seg).tolist() == [254, 254, 254 - (seg // 2) * 254 // seg, 1, 255,
                                                 255, 255]
    assert M.decompress_key(np.array([12, 13], dtype=np.uint32), 13).tolist() == [20, 255]


def scalar_cost_key(segment):
    """seg_cost_kernel for one segment, byte by byte"""
    n = len(segment)
    seen = set()
    for q in range(4):
        at = n * q // 4
        cnt = 32 if n >= 128 else min(32, n - at)
        seen.update(segment[at:at + cnt].tolist())
    return len(seen)


@pytest.mark.parametrize("seg", [1, 3, 4, 33, 127, 128, 131, 4099])
def test_cost_key_both_branches(seg):
    rng = np.random.default_rng(seg)
    for r in {0, 1, seg - 1}:
        n = 9 * seg - r
        data = rng.integers(0, 256, n, dtype=np.uint8)
        data[2 * seg:4 * seg] //= 32  # (a few distinct values)
        want = [scalar_cost_key(data[i:i + seg]) for i in range(0, n, seg)]
        assert M.cost_key(data, seg).tolist() == want
    assert M.cost_key(np.full(3 * seg, 9, np.uint8), seg).tolist() == [1, 1, 1]


GAP = range(45, 82)  # order.hip.h: no key of the mixed kinds lies here, kCheapKey in the middle


@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("kind", [0, 1, 2, 5, 6])
def test_compress_key_is_bimodal_on_the_generator_kinds(kind, seed):
    """512 segments of 64 KiB: nothing between 44 and 82, text and integer columns below the
    cut, random bytes above it, the mixed kinds on both sides"""
    keys = M.cost_key(O.fill(kind, seed, 512 * 65536), 65536)
    assert not np.isin(keys, GAP).any(), sorted(set(keys[np.isin(keys, GAP)].tolist()))
    assert GAP[0] <= M.CHEAP_KEY <= GAP[-1]
    low, high = (keys < M.CHEAP_KEY).any(), (keys >= M.CHEAP_KEY).any()
    assert (low, high) == {0: (False, True), 1: (True, True), 2: (True, True),
                           5: (True, False), 6: (True, False)}[kind]


def test_compress_key_splits_the_lane_tests_pools():
    """4099-byte segments of the priority-lane test (the pools of a 256-CU device): every
    text segment is heavy, every random one is not, none in the gap"""
    text, rand = C.lane_pools(C.big_nseg(256))
    kt, kr = M.cost_key(text.reshape(-1), C.SEG), M.cost_key(rand.reshape(-1), C.SEG)
    assert not np.isin(kt, GAP).any() and not np.isin(kr, GAP).any()
    assert (kt < M.CHEAP_KEY).all() and (kr >= M.CHEAP_KEY).all()


# ---- check_order rejects what it is there to reject ----
def good_order(keys, cut, slots):
    keys = np.asarray(keys, dtype=np.uint32)
    order = np.argsort(np.minimum(keys, 255), kind="stable").astype(np.uint32)
    H = int((np.minimum(keys, 255) < cut).sum())
    if slots and H > slots:
        order |= (M.lane_prio(np.arange(keys.size), H, slots) * M.LANE_TAG).astype(np.uint32)
    return order


def test_check_order_accepts_any_order_inside_a_key():
    keys = C.keys_with_heavy(3000, 1500, 64)
    order = good_order(keys, 64, 700)
    assert M.check_order(order, keys, 64, 700) == 1500
    assert (order & M.LANE_TAG != 0).sum() == M.tagged_count(1500, 700) == 300
    # reversed inside every key, the tags staying with their dispatch indices
    k = np.minimum(keys, 255)[order & ~np.uint32(M.LANE_TAG)]
    rev = order.copy()
    for v in np.unique(k):
        w = np.flatnonzero(k == v)
        rev[w] = (order[w[::-1]] & ~np.uint32(M.LANE_TAG)) | (order[w] & np.uint32(M.LANE_TAG))
    M.check_order(rev, keys, 64, 700)
    M.check_order(good_order(keys, 0, 0), keys, 0, 0)


def bad_orders():
    keys = C.keys_with_heavy(3000, 1500, 64)
    order = good_order(keys, 64, 700)
    tagged = np.flatnonzero(order & M.LANE_TAG)
    dup = order.copy()
    dup[10] = dup[11]
    yield "duplicate", dup, keys, "dispatched"
    out = order.copy()
    out[5] = 3000
    yield "out_of_range", out, keys, "no segment"
    swap = order.copy()
    k = np.minimum(keys, 255)[order & ~np.uint32(M.LANE_TAG)]
    j = int(np.flatnonzero(k[1:] != k[:-1])[3])  # the last of one key, the first of the next
    i0, i1 = swap[j] & ~np.uint32(M.LANE_TAG), swap[j + 1] & ~np.uint32(M.LANE_TAG)
    swap[j] = i1 | (swap[j] & np.uint32(M.LANE_TAG))
    swap[j + 1] = i0 | (swap[j + 1] & np.uint32(M.LANE_TAG))
    yield "swapped_pair_across_keys", swap, keys, "after key"
    miss = order.copy()
    miss[tagged[7]] &= ~np.uint32(M.LANE_TAG)
    yield "missing_tag", miss, keys, "tag False"
    past = order.copy()
    past[1500] |= np.uint32(M.LANE_TAG)  # (1500 % 700 = 100, a fast slot: only b >= H forbids it)
    yield "tag_past_H", past, keys, "tag True"
    plain = order & ~np.uint32(M.LANE_TAG)
    yield "no_tags_at_all", plain, keys, "0 tags for 300"


@pytest.mark.parametrize("case", list(bad_orders()), ids=lambda c: c[0])
def test_check_order_rejects(case):
    _, order, keys, text = case
    with pytest.raises(AssertionError, match=text):
        M.check_order(order, keys, 64, 700)


def test_check_order_rejects_tags_without_lanes():
    keys = C.keys_with_heavy(3000, 600, 64)
    order = good_order(keys, 64, 0)
    order[0] |= np.uint32(M.LANE_TAG)
    for slots in (0, 700):  # no slot count; H under one round
        with pytest.raises(AssertionError, match="tag True"):
            M.check_order(order, keys, 64, slots)
