"""The cost-ordered dispatch, read back (bitar_hip_debug_order).

Calls of 2048 segments and more run segment order[b] as workgroup b.  The entry builds an
order with the code the codecs run (SegOrder::make, cost_order(), lane_slots()) and copies it
out with its lane tags; tests/order_model.py says what it must be: a permutation, keys that
never decrease along it (the order inside a key is free), and the tag on exactly the dispatch
indices the lane rule selects for H = the keys below the cut and S slots.  A wrong order costs
speed only, so no round trip can see it.

Not reachable here: the keys walk_key_kernel, hand_key_kernel and snappy_joined_key_kernel
compute from runtime-internal scratch.  Their orders run through the same sort, which the
caller-keys mode covers.

The slot count the fast LZ4 compressor's calls get on an MI355X (256 CUs): S = 5120, S / CUs =
20, DESIGN.md 4.29's figure (5 waves per SIMD); the test asserts S > 0 and S % CUs == 0 only,
the occupancy query being no sound reference.
"""
import ctypes

import numpy as np
import pytest

import gpu_canary as G
import gpu_parity as P
import oracle_lib as O
import order_cases as C
import order_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NSEGS = [2048, 2049, 3071, 3072, 3073, 65536, 65537, 131073]
PATTERNS = list(C.key_patterns(2048))


@pytest.fixture(scope="module")
def engines():
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0)
    p = bitar_amd.Engine(0, flags=bitar_amd.FLAG_PLAIN_ORDER)
    yield e, p
    e.close()
    p.close()


@pytest.fixture(scope="module")
def eng(engines):
    return engines[0]


def up(a):
    """uint32 host array -> int32 device tensor"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def caller_order(eng, keys, cut=0, slots=0):
    import bitar_amd as B
    order, kout, used = eng.debug_order(B.ORDER_CALLER_KEYS, keys.size, values=up(keys), cut=cut,
                                        slots=slots, keys=True)
    assert order is not None and used == slots
    assert np.array_equal(down(kout), keys)  # (as written: the clamp is the sort's)
    return down(order)


# ---- the sort ----
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nseg", NSEGS)
def test_sort_of_caller_keys(eng, nseg, pattern):
    keys = C.key_patterns(nseg)[pattern]
    order = caller_order(eng, keys)
    assert M.check_order(order, keys, 0, 0) == 0


# ---- the tags ----
@pytest.mark.parametrize("cut", [1, 64, 255])
@pytest.mark.parametrize("slots", [1, 7, 64, 1000])
def test_tags_of_the_fast_lanes(eng, slots, cut):
    """explicit slot counts, so independent of the device's occupancy: H on both sides of one
    round, of two rounds, the whole call and nothing; 3073 segments are three full tiles and
    one segment, so tagged dispatch indices lie in every tile's share"""
    nseg = 3073
    for H in sorted({slots - 1, slots, slots + 1, 2 * slots, 2 * slots + 1, nseg, 0}):
        keys = C.keys_with_heavy(nseg, H, cut, seed=H)
        order = caller_order(eng, keys, cut, slots)
        assert M.check_order(order, keys, cut, slots) == H
        q, f = divmod(H, slots)
        want = (q + 1) * f if q >= 1 and f > 0 else 0
        assert int((order & M.LANE_TAG != 0).sum()) == want, (H, slots)


def test_arguments_the_entry_refuses(eng):
    import bitar_amd as B
    keys = up(np.zeros(2048, np.uint32))
    for kw in (dict(cut=256), dict(cut=0xFFFFFFFF), dict(mode=3)):
        with pytest.raises(B.BitarError) as e:
            eng.debug_order(kw.pop("mode", B.ORDER_CALLER_KEYS), 2048, values=keys, **kw)
        assert e.value.code == -4
    # nseg above the lane tag (checked before any buffer is read), null buffers, a compress
    # call whose nseg is not its input's
    out = keys
    L, u = B.lib(), ctypes.c_uint32(0)
    st = eng._stream(None)
    assert L.bitar_hip_debug_order(eng.ctx, st, B.ORDER_CALLER_KEYS, None, 0, 0, B._ptr(keys),
                                   0x80000001, 0, 0, B._ptr(out), None, ctypes.byref(u)) == -4
    assert L.bitar_hip_debug_order(eng.ctx, st, B.ORDER_CALLER_KEYS, None, 0, 0, None, 2048, 0,
                                   0, B._ptr(out), None, None) == -4
    assert L.bitar_hip_debug_order(eng.ctx, st, B.ORDER_CALLER_KEYS, None, 0, 0, B._ptr(keys),
                                   2048, 0, 0, None, None, None) == -4
    assert L.bitar_hip_debug_order(eng.ctx, st, B.ORDER_COMPRESS_KEY, B._ptr(keys), 8192, 4,
                                   None, 2047, 0, 0, B._ptr(out), None, None) == -4
    assert L.bitar_hip_debug_order(eng.ctx, st, B.ORDER_DECOMPRESS_KEY, None, 0, 64,
                                   B._ptr(keys), 2048, 0, 0, B._ptr(out), B._ptr(out), None) == -4
    eng.sync()


# ---- the decompress key ----
@pytest.mark.parametrize("nseg", [2048, 3073])
@pytest.mark.parametrize("seg", [13, 4099, 65536])
def test_decompress_key_orders_by_coded_size(eng, seg, nseg):
    import bitar_amd as B
    rng = np.random.default_rng(seg + nseg)
    edge = [0, 1, seg - 1, seg, seg + 1, B.slot_size(B.CODEC_LZ4, seg), 0xFFFFFFFF]
    csize = np.concatenate([rng.integers(0, seg, nseg // 2),
                            rng.integers(0, 2 * seg + 2, nseg - nseg // 2 - 3 * len(edge)),
                            np.repeat(edge, 3)]).astype(np.uint32)
    csize = csize[rng.permutation(nseg)]
    order, kout, used = eng.debug_order(B.ORDER_DECOMPRESS_KEY, nseg, seg=seg, values=up(csize))
    assert kout is None and used == 0
    order = down(order)
    M.check_order(order, M.decompress_key(csize, seg), 0, 0)
    # stored segments (copies) last, and among the coded ones no smaller size class first
    stored = int((csize >= seg).sum())
    assert 3 * 4 <= stored < nseg
    assert (csize[order[nseg - stored:]] >= seg).all() and (csize[order[:nseg - stored]] < seg).all()
    cls = csize[order[:nseg - stored]].astype(np.uint64) * 254 // seg
    assert (cls[1:] <= cls[:-1]).all()


# ---- the compress key ----
@pytest.fixture(scope="module")
def key_pools():
    """2049 segments of 4099 bytes of random bytes and of log text"""
    return O.fill(0, 7, 2049 * 4099), O.fill(6, 7, 2049 * 4099)


def mixed_segments(key_pools, nseg, seg):
    """nseg * seg bytes: segment i is random bytes, log text or one repeated byte; the last
    two are repeated bytes other than the guard's, so that any byte sampled past the input's
    end adds a value to the last segment's key"""
    rand, text = key_pools
    kind = np.random.default_rng(seg).integers(0, 3, nseg)
    kind[-2:] = 2
    const = np.repeat((np.arange(nseg) * 37 % 160).astype(np.uint8)[:, None], seg, axis=1)
    assert G.GUARD_BYTE not in const[-2:]
    r, t = rand[:nseg * seg].reshape(nseg, seg), text[:nseg * seg].reshape(nseg, seg)
    return np.where((kind == 0)[:, None], r, np.where((kind == 1)[:, None], t, const)).reshape(-1)


@pytest.mark.parametrize("short", ["0", "1", "seg-1"])
@pytest.mark.parametrize("nseg", [2048, 2049])
@pytest.mark.parametrize("seg", [4, 33, 127, 128, 131, 4099])
def test_compress_key_is_the_models(eng, key_pools, seg, nseg, short):
    """both branches of seg_cost_kernel (segments under and from 128 bytes) and a last segment
    that is whole, one byte short and one byte long; the input ends where its guarded
    buffer's payload ends, at an odd address"""
    import bitar_amd as B
    n = nseg * seg - {"0": 0, "1": 1, "seg-1": seg - 1}[short]
    host = mixed_segments(key_pools, nseg, seg)[:n]
    buf = G.GuardedBytes(n, residue=(16 - n % 16 + 5) % 16, device="cuda", name="input")
    buf.load(host)
    assert (buf.ptr + n) % 16 == 5
    order, keys, used = eng.debug_order(B.ORDER_COMPRESS_KEY, nseg, data=buf.ptr, n=n, seg=seg,
                                        slots=B.ORDER_SLOTS_CALL, keys=True)
    assert order is not None and used > 0
    keys = down(keys)
    want = M.cost_key(host, seg)
    assert np.array_equal(keys, want), np.flatnonzero(keys != want)[:8]
    M.check_order(down(order), keys, M.CHEAP_KEY, used)
    whole = buf.host()
    buf.check(whole)
    assert np.array_equal(buf.payload(whole), host)


@pytest.mark.parametrize("big", [False, True])
def test_heavy_count_of_the_lane_tests_cases(eng, big):
    """the pools and masks of tests/test_gpu_priority_lanes.py: the H the sort derives from
    the compress keys is the number of text segments, in every case -- at big_nseg() segments
    with the device's own slot count, so that "Hn-1" carries real tags"""
    import bitar_amd as B
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nseg = C.big_nseg(cus) if big else 2049
    text, rand = C.lane_pools(nseg)
    tagged = {}
    for name, heavy in C.masks(nseg).items():
        host = np.where(heavy[:, None], text, rand).reshape(-1)
        data = torch.from_numpy(host).cuda()
        order, keys, used = eng.debug_order(B.ORDER_COMPRESS_KEY, nseg, data=data, n=host.size,
                                            seg=C.SEG, slots=B.ORDER_SLOTS_CALL, keys=True)
        assert order is not None and used > 0
        keys, order = down(keys), down(order)
        assert np.array_equal(keys < M.CHEAP_KEY, heavy)
        assert M.check_order(order, keys, M.CHEAP_KEY, used) == int(heavy.sum())
        # the heavy segments are the first H of the dispatch
        H = int(heavy.sum())
        assert heavy[order[:H] & ~np.uint32(M.LANE_TAG)].all()
        tagged[name] = int((order & M.LANE_TAG != 0).sum())
        assert tagged[name] == M.tagged_count(H, used)
    if big and used == C.LZ4C_WAVES_PER_CU * cus:
        assert tagged["Hn-1"] == 2 * 2302 and tagged["Hn"] == 2 * 2303


# ---- the slot count and the queue-pair convention ----
def test_slot_count_and_queue_pair_convention(engines):
    """Engine(0), one stream: S > 0, a multiple of the CUs (see the module's docstring for
    the value seen).  A context of two queue pairs: none on its own streams (a call there is
    taken to have siblings), S again on a stream that is not the context's.  No order under
    FLAG_PLAIN_ORDER, and none below 2048 segments on any context."""
    import bitar_amd as B
    eng, plain = engines
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    keys = up(np.arange(2048, dtype=np.uint32) % 256)

    def ask(e, nseg=2048, stream=None):
        torch.cuda.synchronize()
        order, _, used = e.debug_order(B.ORDER_CALLER_KEYS, nseg, values=keys, cut=64,
                                       slots=B.ORDER_SLOTS_CALL, stream=stream)
        e.sync(stream)
        return order, used

    order, S = ask(eng)
    print(f"lane slots: S = {S}, CUs = {cus}, S / CUs = {S / cus}")
    assert order is not None and S > 0 and S % cus == 0
    two = B.Engine(0, num_streams=2)
    try:
        for qp in (0, 1):
            order, used = ask(two, stream=two.queue_pair_stream(qp))
            assert order is not None and used == 0
        side = torch.cuda.Stream()
        order, used = ask(two, stream=side)
        assert order is not None and used == S
        assert ask(two, 2047, stream=side) == (None, 0)
        assert ask(two, 2047, stream=two.queue_pair_stream(0)) == (None, 0)
    finally:
        two.close()
    assert ask(plain) == (None, 0)
    assert ask(plain, 2047) == (None, 0)
    assert ask(eng, 2047) == (None, 0)


def test_no_order_leaves_the_outputs_alone(engines):
    import bitar_amd as B
    eng, plain = engines
    keys = up(np.arange(2048, dtype=np.uint32) % 256)
    for e, nseg in ((eng, 2047), (plain, 2048)):
        order = G.GuardedWords(nseg, device="cuda", name="order")
        kout = G.GuardedWords(nseg, device="cuda", name="keys")
        used = ctypes.c_uint32(99)
        rc = B.lib().bitar_hip_debug_order(e.ctx, e._stream(None), B.ORDER_CALLER_KEYS, None, 0,
                                           0, B._ptr(keys), nseg, 64, 7, order.ptr, kout.ptr,
                                           ctypes.byref(used))
        e.sync()
        assert rc == B.NO_ORDER
        for w in (order, kout):
            w.check()
            assert (w.values() == G.FILL_WORD).all()


# ---- calls above 65536 segments, where the tiles grow ----
@pytest.fixture(scope="module")
def small_segments():
    """131073 segments of 64 bytes (the last one 1 byte): random bytes, log text and repeated
    bytes in runs of 1 to 300 segments"""
    n = 131072 * 64 + 1
    rng = np.random.default_rng(64)
    runs = rng.integers(1, 300, 4096)
    kind = np.repeat(rng.integers(0, 3, runs.size), runs)[:131073]
    assert kind.size == 131073
    per_byte = np.repeat(kind, 64)[:n]
    host = np.where(per_byte == 0, O.fill(0, 3, n),
                    np.where(per_byte == 1, O.fill(6, 3, n), np.uint8(0x5A)))
    return torch.from_numpy(host.astype(np.uint8)).cuda()


@pytest.mark.parametrize("nseg", [65537, 131073])
@pytest.mark.parametrize("codec_name", ["LZ4", "LZ4_WIDE", "DEFLATE", "ZSTD", "SNAPPY"])
def test_calls_above_65536_segments(engines, small_segments, codec_name, nseg):
    """tiles of 2048 and 3072 segments, the last holding one: against a plain-order context,
    and the order such a call takes is a real one (several keys)"""
    import bitar_amd as B
    eng, plain = engines
    seg = 64
    data = small_segments[:(nseg - 1) * seg + 1]
    codec = getattr(B, "CODEC_" + codec_name)
    dcodec = B.CODEC_LZ4 if codec_name == "LZ4_WIDE" else codec
    order, keys, used = eng.debug_order(B.ORDER_COMPRESS_KEY, nseg, data=data, n=data.numel(),
                                        seg=seg, keys=True)
    keys = down(keys)
    assert np.unique(keys).size > 8
    M.check_order(down(order), keys, 0, 0)
    P.assert_same_as_plain_order(eng, plain, codec, dcodec, data, seg)
