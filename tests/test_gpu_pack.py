"""GPU tests of frame assembly through the C ABI: bitar_hip_pack and bitar_hip_pack_lz4f
(scan_sizes_kernel, pack_kernel, lz4f_sizes_kernel, lz4f_pack_kernel in csrc/util_kernels.hip)
against tests/pack_model.py, byte for byte, with guards (tests/gpu_canary.py) around every
buffer a call touches.

The scan is one 1024-thread workgroup that walks the sizes in tiles of 1024 with a carried
64-bit base, so the shapes are the segment counts at which it can go wrong: one short of, at
and one past a wave (63, 64, 65), a tile (1023, 1024, 1025) and two tiles (2047, 2048, 2049),
five tiles with a ragged end (5000), sizes whose sum passes 2^32 inside the first wave, and
failed sizes on both sides of a tile border.  Slots and inputs are synthetic (the kernels only
move bytes), so every case is a few hundred KiB at the most; one end-to-end case packs the
engine's own LZ4 blocks of 2 MiB of mixed data and hands the frame to pyarrow."""
import numpy as np
import pytest

import gpu_canary as G
import pack_model as P
from test_gpu_lz4 import down, eng  # noqa: F401  (fixture reuse)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
ERR = P.SEGMENT_ERROR
NSEGS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 5000)
FILL64 = G.FILL_WORD | G.FILL_WORD << 32
SLACK = 300  # frame bytes behind the packed ones, which no call may write


class Longs:
    """n uint64 entries (offsets[]) with guard words on both sides, FILL64 before a call"""

    def __init__(self, n, name="offsets"):
        self.w = G.GuardedWords(2 * n, DEV, name)
        assert self.w.ptr % 8 == 0
        self.ptr = self.w.ptr

    def values(self):
        self.w.check()
        return self.w.values().copy().view(np.uint64)


def words(values, name="sizes"):
    w = G.GuardedWords(max(len(values), 1), DEV, name)
    w.load(values)
    return w


def same_words(w, values):
    """a call's uint32 input after it: guards and every entry"""
    w.check()
    assert np.array_equal(w.values()[:len(values)], np.asarray(values, np.uint32)), \
        f"{w.name} was written"


def sync_code(eng, stream=None):
    """0, or the code the sync raises"""
    import bitar_amd
    try:
        eng.sync(stream)
        return 0
    except bitar_amd.BitarError as ex:
        return ex.code


# ---- bitar_hip_pack, offsets only ------------------------------------------------------------

def offsets_only(eng, sizes, launch=True):
    """pack(frame=None, stride 0) of sizes -> the guarded sizes and offsets, not yet
    synchronized (launch=False: the buffers alone)"""
    sizes = np.asarray(sizes, np.uint32)
    d_sizes, d_off = words(sizes), Longs(sizes.size + 1)
    if launch:
        eng.pack(None, 0, d_sizes.ptr, sizes.size, d_off.ptr, None)
    return d_sizes, d_off


def size_sets(nseg):
    rng = np.random.default_rng(1000 + nseg)
    rnd = rng.integers(1, 70000, nseg).astype(np.uint32)
    rnd[rng.random(nseg) < 0.125] = 0
    return (("random", rnd), ("ramp", np.arange(1, nseg + 1, dtype=np.uint32)))


@pytest.mark.parametrize("nseg", NSEGS)
def test_offsets_are_the_model(eng, nseg):
    for name, sizes in size_sets(nseg):
        want, flagged = P.offsets(sizes, P.NO_STRIDE_LIMIT)
        assert not flagged
        d_sizes, d_off = offsets_only(eng, sizes)
        assert sync_code(eng) == 0, name
        got = d_off.values()
        assert got.size == nseg + 1 and np.array_equal(got, want), \
            (name, np.flatnonzero(got != want)[:4].tolist())
        same_words(d_sizes, sizes)
    if nseg == 0:
        assert got.tolist() == [0]  # written: the entry held FILL64


def carry_sizes():
    rng = np.random.default_rng(64)
    return rng.integers(1 << 31, (1 << 32) - 1, 1500).astype(np.uint32)  # <= 2^32 - 2


def test_offsets_carry_64_bits_across_a_tile(eng):
    sizes = carry_sizes()
    assert sizes.min() >= 1 << 31 and sizes.max() <= ERR - 1
    want, flagged = P.offsets(sizes, P.NO_STRIDE_LIMIT)
    assert not flagged and int(want[2]) >= 1 << 32 and int(want[-1]) > 1500 << 31
    d_sizes, d_off = offsets_only(eng, sizes)
    assert sync_code(eng) == 0
    assert np.array_equal(d_off.values(), want)
    same_words(d_sizes, sizes)


def test_failed_sizes_count_nothing_and_flag_once(eng):
    sizes = carry_sizes()
    for at in (0, 1023, 1024, sizes.size - 1):
        sizes[at] = ERR
    want, flagged = P.offsets(sizes, P.NO_STRIDE_LIMIT)
    assert flagged
    for at in (0, 1023, 1024, sizes.size - 1):
        assert want[at + 1] == want[at]
    d_sizes, d_off = offsets_only(eng, sizes)
    assert sync_code(eng) == -5
    assert sync_code(eng) == 0
    assert np.array_equal(d_off.values(), want)
    same_words(d_sizes, sizes)


# ---- bitar_hip_pack with a frame ---------------------------------------------------------------

STRIDE = 256
SLOT_SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256)


def slot_pattern(nseg, stride):
    """every slot filled over its whole stride with bytes of its own"""
    i = np.arange(nseg, dtype=np.uint32)[:, None]
    j = np.arange(stride, dtype=np.uint32)[None, :]
    return ((i * 131 + j * 7 + (i >> 8) + 1) % 251).astype(np.uint8).reshape(-1)


def pack_guarded(eng, slab_host, stride, sizes, residue):
    """one pack into a guarded frame of total + SLACK bytes; everything checked against the
    model but the sync's verdict, which is returned"""
    sizes = np.asarray(sizes, np.uint32)
    nseg = sizes.size
    want_off, flagged = P.offsets(sizes, stride)
    want = P.pack(slab_host, stride, sizes)
    total = int(want_off[-1])
    assert want.size == total
    slab = G.GuardedBytes(slab_host.size, 1, DEV, "slab")
    slab.load(slab_host)
    d_sizes, d_off = words(sizes), Longs(nseg + 1)
    frame = G.GuardedBytes(total + SLACK, residue, DEV, "frame")
    eng.pack(slab.ptr, stride, d_sizes.ptr, nseg, d_off.ptr, frame.ptr)
    code = sync_code(eng)
    assert code == (-5 if flagged else 0)
    assert np.array_equal(d_off.values(), want_off)
    whole = frame.host()
    frame.check(whole)
    got = frame.payload(whole)[:total]
    assert np.array_equal(got, want), (residue, np.flatnonzero(got != want)[:4].tolist())
    frame.check_fill(total, total + SLACK, "behind the frame", whole)
    same_words(d_sizes, sizes)
    whole = slab.host()
    slab.check(whole)
    assert np.array_equal(slab.payload(whole), slab_host), "the slab was written"
    return code


@pytest.mark.parametrize("nseg", (1, 65, 1024, 1025, 2049))
def test_pack_is_the_model(eng, nseg):
    slab = slot_pattern(nseg, STRIDE)
    for residue in G.RESIDUES:
        rng = np.random.default_rng(7 * nseg + residue)
        sizes = rng.choice(SLOT_SIZES, nseg).astype(np.uint32)
        if nseg > 1:
            sizes[-1] = 17  # a short last slot: an over-copy of it lands in the slack
        assert pack_guarded(eng, slab, STRIDE, sizes, residue) == 0


def test_pack_skips_a_failed_slot_past_the_first_tile(eng):
    nseg = 2049
    rng = np.random.default_rng(5)
    sizes = rng.choice(SLOT_SIZES, nseg).astype(np.uint32)
    sizes[1024] = STRIDE + 1
    assert pack_guarded(eng, slot_pattern(nseg, STRIDE), STRIDE, sizes, 5) == -5
    assert sync_code(eng) == 0


# ---- bitar_hip_pack_lz4f with synthetic slots ---------------------------------------------------

def lz4f_sizes(n, seg, shift):
    """a size per block, in turn from entry `shift`: below its length, at it, one above it,
    SEGMENT_ERROR, 1 and half of it; a 1-byte block gets 1 (its length: raw)"""
    nseg = (n + seg - 1) // seg
    sizes = np.zeros(nseg, np.uint32)
    for i in range(nseg):
        length = min(seg, n - i * seg)
        sizes[i] = (length - 1, length, length + 1, ERR, 1, length // 2)[(i + shift) % 6]
        if length == 1:
            sizes[i] = 1
    return sizes


class Lz4fCase:
    def __init__(self, n, seg, shift=0):
        rng = np.random.default_rng(100 * seg + n % 9973 + shift)
        self.n, self.seg = n, seg
        self.nseg = (n + seg - 1) // seg
        self.stride = seg + 3  # an odd slot pitch: slots at every address residue
        self.data = rng.integers(0, 256, n, dtype=np.uint8)
        self.slab = rng.integers(0, 256, max(self.nseg, 1) * self.stride, dtype=np.uint8)
        self.sizes = lz4f_sizes(n, seg, shift)
        self.want = P.lz4f_blocks(self.data, seg, self.slab, self.stride, self.sizes)
        self.d_data = G.GuardedBytes(max(n, 1), 5, DEV, "input")
        self.d_data.load(self.data)
        self.d_slab = G.GuardedBytes(self.slab.size, 1, DEV, "slab")
        self.d_slab.load(self.slab)
        self.d_sizes = words(self.sizes)

    def inputs_unchanged(self):
        same_words(self.d_sizes, self.sizes)
        for buf, host in ((self.d_data, self.data), (self.d_slab, self.slab)):
            whole = buf.host()
            buf.check(whole)
            assert np.array_equal(buf.payload(whole)[:host.size], host), f"{buf.name} was written"


def lz4f_shapes():
    out = []
    for seg in (64, 13, 65536):
        out += [(seg, seg), (seg, 2 * seg + 1)]
        if seg < 65536:
            out += [(seg, 1025 * seg + 1), (seg, 1), (seg, seg - 1)]
    return out


@pytest.mark.parametrize("shift", (0, 2))  # (two blocks: below and at, one above and failed)
@pytest.mark.parametrize("seg,n", lz4f_shapes())
def test_lz4f_blocks_are_the_model(eng, seg, n, shift):
    c = Lz4fCase(n, seg, shift)
    framed, off, body = c.want
    forms = {"raw" if body[int(o) + 3] >> 7 else "packed" for o in off[:-1]}
    assert forms == {"raw", "packed"} or c.nseg < 6
    for residue in (0, 5):
        d_framed, d_off = G.GuardedWords(c.nseg, DEV, "framed"), Longs(c.nseg + 1)
        frame = G.GuardedBytes(len(body) + SLACK, residue, DEV, "frame")
        eng.pack_lz4f(c.d_data.ptr, n, seg, c.d_slab.ptr, c.stride, c.d_sizes.ptr, d_framed.ptr,
                      d_off.ptr, frame.ptr)
        assert sync_code(eng) == 0  # (a failed segment ships raw: no error of the pack's)
        d_framed.check()
        assert np.array_equal(d_framed.values(), framed)
        assert np.array_equal(d_off.values(), off)
        whole = frame.host()
        frame.check(whole)
        got = frame.payload(whole)[:len(body)]
        want = np.frombuffer(body, np.uint8)
        assert np.array_equal(got, want), (residue, np.flatnonzero(got != want)[:4].tolist())
        frame.check_fill(len(body), len(body) + SLACK, "behind the blocks", whole)
        c.inputs_unchanged()
    # sizing mode: no frame, and neither the input nor the slab is looked at
    d_framed, d_off = G.GuardedWords(c.nseg, DEV, "framed"), Longs(c.nseg + 1)
    eng.pack_lz4f(None, n, seg, None, c.stride, c.d_sizes.ptr, d_framed.ptr, d_off.ptr, None)
    assert sync_code(eng) == 0
    d_framed.check()
    assert np.array_equal(d_framed.values(), framed)
    assert np.array_equal(d_off.values(), off)


def test_lz4f_of_nothing_writes_one_offset(eng):
    d_sizes, d_framed, d_off = words([]), G.GuardedWords(1, DEV, "framed"), Longs(2)
    frame = G.GuardedBytes(SLACK, 0, DEV, "frame")
    eng.pack_lz4f(None, 0, 64, None, 67, d_sizes.ptr, d_framed.ptr, d_off.ptr, frame.ptr)
    assert sync_code(eng) == 0
    assert d_off.values().tolist() == [0, FILL64]
    d_framed.check()
    assert d_framed.values().tolist() == [G.FILL_WORD]
    frame.check()
    frame.check_fill(0, SLACK, "an empty frame")
    d_sizes.check()
    assert d_sizes.values().tolist() == [G.FILL_WORD]


def test_lz4f_refusals(eng):
    import bitar_amd
    c = Lz4fCase(2 * 64 + 1, 64)
    framed, off, body = c.want
    d_framed, d_off = G.GuardedWords(c.nseg, DEV, "framed"), Longs(c.nseg + 1)
    frame = G.GuardedBytes(len(body) + SLACK, 0, DEV, "frame")
    args = (c.d_slab.ptr, c.stride, c.d_sizes.ptr, d_framed.ptr, d_off.ptr, frame.ptr)
    # a frame to fill and no input to take raw blocks from
    with pytest.raises(bitar_amd.BitarError) as ex:
        eng.pack_lz4f(None, c.n, c.seg, *args)
    assert ex.value.code == -4
    assert sync_code(eng) == 0
    frame.check()
    frame.check_fill(0, frame.n, "a refused call's frame")
    for seg in (0, 65537):
        with pytest.raises(bitar_amd.BitarError) as ex:
            eng.pack_lz4f(c.d_data.ptr, c.n, seg, *args)
        assert ex.value.code == -4
    # the engine goes on
    eng.pack_lz4f(c.d_data.ptr, c.n, c.seg, *args)
    assert sync_code(eng) == 0
    assert np.array_equal(d_off.values(), off)
    assert frame.payload()[:len(body)].tobytes() == body


# ---- bitar_hip_pack_lz4f on the engine's own blocks ---------------------------------------------

def test_lz4f_end_to_end_decodes_with_pyarrow(eng):
    """kind 1 at 2048-byte segments, 1025 of them and a 1-byte tail, from the middle of a text
    region through a random one into a column region (regions are 1 MiB): runs of compressed
    and of raw blocks in one call"""
    pa = pytest.importorskip("pyarrow")
    import bitar_amd
    seg = 2048
    n = 1025 * seg + 1
    nseg = 1026
    data = eng.empty(n)
    eng.fill(1, 21, data, offset=3 << 19)
    slab, stride, sizes = eng.compress(bitar_amd.CODEC_LZ4, data, seg)
    d_framed, d_off = G.GuardedWords(nseg, DEV, "framed"), Longs(nseg + 1)
    cap = nseg * (4 + seg)
    frame = G.GuardedBytes(cap, 5, DEV, "frame")
    eng.pack_lz4f(data, n, seg, slab, stride, sizes, d_framed.ptr, d_off.ptr, frame.ptr)
    assert sync_code(eng) == 0
    host = down(data)
    h_sizes = down(sizes).astype(np.uint32)
    framed, off, body = P.lz4f_blocks(host, seg, down(slab), stride, h_sizes)
    raw = int((h_sizes >= np.minimum(seg, n - seg * np.arange(nseg))).sum())
    assert 100 < raw < nseg - 100  # both forms, in runs (the regions)
    d_framed.check()
    assert np.array_equal(d_framed.values(), framed)
    assert np.array_equal(d_off.values(), off)
    whole = frame.host()
    frame.check(whole)
    assert frame.payload(whole)[:len(body)].tobytes() == body
    frame.check_fill(len(body), cap, "behind the blocks", whole)
    back = pa.Codec("lz4").decompress(P.lz4f_frame(body), decompressed_size=n)
    assert back.to_pybytes() == host.tobytes()


# ---- two queue pairs ----------------------------------------------------------------------------

def test_pack_errors_are_per_stream():
    """a pack of 2049 sizes on queue pair 0 beside one with a failed size on queue pair 1: both
    index arrays exact, and only queue pair 1's sync reports it (the scan takes the error word
    of its stream)"""
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0, num_streams=2)
    try:
        s0, s1 = e.queue_pair_stream(0), e.queue_pair_stream(1)
        good = size_sets(2049)[0][1]
        bad = size_sets(2049)[1][1].copy()
        bad[1024] = ERR
        ds1, do1 = offsets_only(e, bad, launch=False)
        ds0, do0 = offsets_only(e, good, launch=False)
        torch.cuda.synchronize()  # the inputs were written on torch's stream
        e.pack(None, 0, ds1.ptr, bad.size, do1.ptr, None, stream=s1)
        e.pack(None, 0, ds0.ptr, good.size, do0.ptr, None, stream=s0)
        assert sync_code(e, s0) == 0  # neither sees nor clears queue pair 1's failure
        assert sync_code(e, s1) == -5
        assert sync_code(e, s1) == 0
        assert np.array_equal(do0.values(), P.offsets(good, P.NO_STRIDE_LIMIT)[0])
        assert np.array_equal(do1.values(), P.offsets(bad, P.NO_STRIDE_LIMIT)[0])
        same_words(ds0, good)
        same_words(ds1, bad)
    finally:
        e.close()
