"""GPU tests of the INTPACK codec (csrc/intpack.hip) through the C ABI: the slots and sizes of
a compress equal the numpy model's streams (intpack_model.py) byte for byte, the decoder
returns the input, and on mutated streams its verdict is the model's, with canaries around
every buffer a call writes.

Shapes: segments of 65536 (16-B aligned everywhere), 59460 (the reference's segment: elements
of 8 bytes straddle every other segment's start), 4096, 1000 / 999 (odd bases: every element
unaligned), 72 and 7 (one partial miniblock, shorter than an int64); lengths that end on and
next to an element, a miniblock (64 elements) and a block (256 elements)."""
import numpy as np
import pytest

import intpack_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEGS = (65536, 59460, 4096, 1000, 999, 72, 7)
CANARY = 0xA5
CANARY32 = np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]
PAD = 256
ERR = np.array([0xFFFFFFFF], np.uint32).view(np.int32)[0]


@pytest.fixture(scope="module")
def eng():
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0)
    yield e
    e.close()


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def column(n, w, seed):
    """n bytes whose segments take every form: small-range noise (mode 0), sorted runs (mode 1,
    with wrap-around for narrow widths), a constant run (widths 0), a block that spans the whole
    signed range (width 8w), negative small values, and random bytes (stored)"""
    rng = np.random.default_rng(seed)
    m = n // w + 1
    U, S = M._U[w], M._S[w]
    v = rng.integers(0, 1 << min(8 * w - 1, 10), m).astype(U)
    q = m // 8
    step = rng.integers(0, 1 << min(4 * w, 6), q).astype(np.uint64)
    v[q:2 * q] = (np.cumsum(step) + np.uint64(12345)).astype(U)
    v[2 * q:2 * q + q // 2] = 7
    info = np.iinfo(S)
    wide = np.array([info.min, info.max, 0], S)[rng.integers(0, 3, min(256, q))]
    v[3 * q:3 * q + wide.size] = wide.view(U)
    v[3 * q + wide.size:4 * q] = 0
    v[4 * q:5 * q] = rng.integers(-5, 6, q).astype(S).view(U)
    out = v.view(np.uint8)[:n].copy()
    a = 5 * q * w  # (the last three eighths: whole segments of it are stored)
    out[a:] = rnd(n - a, seed + 1)
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


class Buffers:
    """device buffers of one compress + decompress with canaries on both sides of each"""

    def __init__(self, nseg, stride, seg):
        self.nseg, self.stride, self.seg = nseg, stride, seg
        self.slab = torch.full((PAD + nseg * stride + PAD,), CANARY, dtype=torch.uint8,
                               device="cuda")
        self.sizes = torch.full((nseg + 16,), int(CANARY32), dtype=torch.int32, device="cuda")
        self.out = torch.full((PAD + nseg * seg + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        self.prod = torch.full((nseg + 16,), int(CANARY32), dtype=torch.int32, device="cuda")

    slab_ptr = property(lambda self: self.slab.data_ptr() + PAD)
    sizes_ptr = property(lambda self: self.sizes.data_ptr() + 32)
    out_ptr = property(lambda self: self.out.data_ptr() + PAD)
    prod_ptr = property(lambda self: self.prod.data_ptr() + 32)

    def check_streams(self, streams):
        """slots and sizes against the model's streams; whatever a stream does not cover is
        still the canary"""
        sizes = self.sizes.cpu().numpy()
        assert np.all(sizes[:8] == CANARY32) and np.all(sizes[8 + self.nseg:] == CANARY32)
        got = sizes[8:8 + self.nseg].view(np.uint32)
        assert got.tolist() == [len(s) for s in streams]
        slab = self.slab.cpu().numpy()
        assert np.all(slab[:PAD] == CANARY) and np.all(slab[-PAD:] == CANARY)
        for i, s in enumerate(streams):
            slot = slab[PAD + i * self.stride:PAD + (i + 1) * self.stride]
            want = np.frombuffer(s, np.uint8)
            assert np.array_equal(slot[:want.size], want), \
                (i, s[0], np.flatnonzero(slot[:want.size] != want)[:8].tolist())
            assert np.all(slot[want.size:] == CANARY), i

    def check_output(self, data):
        n = data.size
        prod = self.prod.cpu().numpy()
        assert np.all(prod[:8] == CANARY32) and np.all(prod[8 + self.nseg:] == CANARY32)
        want = [min(self.seg, n - i * self.seg) for i in range(self.nseg)]
        assert prod[8:8 + self.nseg].tolist() == want
        out = self.out.cpu().numpy()
        assert np.all(out[:PAD] == CANARY) and np.all(out[PAD + n:] == CANARY)
        assert np.array_equal(out[PAD:PAD + n], data), np.flatnonzero(out[PAD:PAD + n] != data)[:8]


def check_case(eng, w, seg, data, in_off=0):
    import bitar_amd as B
    codec = B.codec_intpack(w)
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec, seg)
    src = torch.zeros(in_off + n + PAD, dtype=torch.uint8, device="cuda")
    src[in_off:in_off + n] = dev(data)
    buf = Buffers(nseg, stride, seg)
    eng.compress_into(codec, src.data_ptr() + in_off, seg, buf.slab_ptr, stride, buf.sizes_ptr, n=n)
    eng.decompress_slab_into(codec, buf.slab_ptr, stride, buf.sizes_ptr, nseg, seg, buf.out_ptr,
                             buf.prod_ptr, capacity=nseg * seg)
    eng.sync()
    streams = M.encode(data, w, seg)
    buf.check_streams(streams)
    buf.check_output(data)
    return streams


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_exact_bytes_and_round_trip(eng, w, seg):
    forms = set()
    tails = (0, 256 * w + 3) if seg > 4096 else \
        sorted({0, 1, w - 1, w, 63 * w, 64 * w, 64 * w + 1, 256 * w + 3})
    for r in tails:
        for s in check_case(eng, w, seg, column(3 * seg + r, w, seg * 31 + r + w)):
            forms.add((s[0] >> 2) & 3)
    if seg >= 1000:
        assert forms >= {0, 2}  # (packed and stored segments; mode 1 has its own test below)
    if seg == 72:
        for n in range(1, w):  # shorter than an element
            check_case(eng, w, seg, rnd(n, n))


def sorted_column(n, w, seed):
    """n bytes of a sorted column with small steps (wrapping around for narrow widths)"""
    rng = np.random.default_rng(seed)
    step = rng.integers(0, 3 if w == 1 else 1 << 6, n // w + 1).astype(np.uint64)
    return (np.cumsum(step) + np.uint64(99)).astype(M._U[w]).view(np.uint8)[:n].copy()


@pytest.mark.parametrize("w", M.WIDTHS)
def test_sorted_columns_take_the_delta_form(eng, w):
    for seg in (65536, 59460, 999):
        streams = check_case(eng, w, seg, sorted_column(2 * seg + 64 * w + 1, w, seg + w))
        assert [(s[0] >> 2) & 3 for s in streams] == [1, 1, 1]


@pytest.mark.parametrize("w", M.WIDTHS)
def test_input_at_every_alignment(eng, w):
    for seg in (59460, 4096):
        for in_off in (0, 1, 3, 4, 15):
            check_case(eng, w, seg, column(2 * seg + 64 * w + 1, w, in_off + w), in_off=in_off)


def test_empty_input_launches_nothing(eng):
    import bitar_amd as B
    buf = Buffers(1, 4352, 4096)
    src = torch.zeros(PAD, dtype=torch.uint8, device="cuda")
    for w in M.WIDTHS:
        eng.compress_into(B.codec_intpack(w), src, 4096, buf.slab_ptr, 4352, buf.sizes_ptr, n=0)
        eng.decompress_slab_into(B.codec_intpack(w), buf.slab_ptr, 4352, buf.sizes_ptr, 0, 4096,
                                 buf.out_ptr, buf.prod_ptr, capacity=0)
    eng.sync()
    for t in (buf.slab, buf.out):
        assert bool((t == CANARY).all())
    for t in (buf.sizes, buf.prod):
        assert bool((t == int(CANARY32)).all())


@pytest.mark.parametrize("w", M.WIDTHS)
def test_scattered_pointer_list_and_host_paths(eng, w):
    """one shape per width through bitar_hip_compress_scattered, bitar_hip_decompress with the
    streams at odd addresses, and the host-overlapped pair"""
    import bitar_amd as B
    codec = B.codec_intpack(w)
    seg = 59460
    data = column(3 * seg + 64 * w + 1, w, 77 + w)
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec, seg)
    streams = M.encode(data, w, seg)
    src = dev(data)

    # scattered: slot i of the call is slot perm[i] of the slab
    buf = Buffers(nseg, stride, seg)
    perm = [2, 0, 3, 1]
    assert nseg == len(perm)
    dsts = dev(np.array([buf.slab_ptr + p * stride for p in perm], np.int64))
    B.check(B.lib().bitar_hip_compress_scattered(eng.ctx, eng._stream(None), codec,
                                                 src.data_ptr(), n, seg, dsts.data_ptr(), stride,
                                                 buf.sizes_ptr))
    eng.sync()
    sizes = buf.sizes.cpu().numpy()[8:8 + nseg].view(np.uint32)
    assert sizes.tolist() == [len(s) for s in streams]
    by_slot = [None] * nseg
    for i, p in enumerate(perm):
        by_slot[p] = streams[i]
    buf.sizes[8:8 + nseg] = dev(np.array([len(s) for s in by_slot], np.int32))
    buf.check_streams(by_slot)

    # pointer list: stream i at an odd address (1, 3, 5, 7 past a 16-B boundary)
    room = (max(len(s) for s in streams) + 32) & ~15
    packed = np.full(nseg * room + 16, CANARY, np.uint8)
    ptrs = []
    for i, s in enumerate(streams):
        o = i * room + 2 * i + 1
        packed[o:o + len(s)] = np.frombuffer(s, np.uint8)
        ptrs.append(o)
    d_packed = dev(packed)
    d_ptrs = dev(np.array(ptrs, np.int64) + d_packed.data_ptr())
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    buf = Buffers(nseg, stride, seg)
    eng.decompress_into(codec, d_ptrs, d_sizes, nseg, seg, buf.out_ptr, buf.prod_ptr,
                        capacity=nseg * seg)
    eng.sync()
    buf.check_output(data)

    # host-overlapped: compress from host memory, decompress into host memory
    buf = Buffers(nseg, stride, seg)
    host = torch.from_numpy(data.copy())
    stage = torch.zeros(nseg * seg, dtype=torch.uint8, device="cuda")
    eng.compress_host_into(codec, host, n, seg, stage, buf.slab_ptr, stride, buf.sizes_ptr)
    eng.sync()
    buf.check_streams(streams)
    d_ptrs = dev(np.array([buf.slab_ptr + i * stride for i in range(nseg)], np.int64))
    back = torch.full((nseg * seg,), CANARY, dtype=torch.uint8)
    eng.decompress_host_into(codec, d_ptrs, buf.sizes_ptr, nseg, seg, stage, back, buf.prod_ptr)
    eng.sync()
    assert np.array_equal(back.numpy()[:n], data)
    assert buf.prod.cpu().numpy()[8:8 + nseg].tolist() == [min(seg, n - i * seg) for i in range(nseg)]


def base_streams(w, seg):
    """a mode 0, a mode 1 and a stored stream of full segments of `seg` bytes"""
    rng = np.random.default_rng(seg + w)
    m = seg // w
    noise = rng.integers(0, 1 << min(8 * w - 1, 7), m).astype(M._U[w])
    step = rng.integers(0, 1 << min(4 * w, 6), m).astype(np.uint64)
    # (sorted with steps wider than the noise's range would not beat mode 0 for 1-byte elements)
    sorted_ = (np.cumsum(step if w > 1 else step % 3) + np.uint64(99)).astype(M._U[w])
    out = []
    for form, body in ((0, noise.view(np.uint8)), (1, sorted_.view(np.uint8)), (2, rnd(seg, seg))):
        data = np.concatenate([body, np.zeros(seg - body.size, np.uint8)])[:seg]
        (s,) = M.encode(data, w, seg)
        assert (s[0] >> 2) & 3 == form, (w, seg, form)
        out.append(s)
    return out


def mutants(s, w):
    """deterministic mutations of the stream s -> [(bytes, size given to the decoder)]"""
    out = [(s, len(s))]

    def poke(at, value):
        if s[at] != value & 255:
            t = bytearray(s)
            t[at] = value & 255
            out.append((bytes(t), len(s)))

    for bit in range(8):  # each header byte, bit by bit; then some whole values
        for at in range(4):
            poke(at, s[at] ^ (1 << bit))
    for at in range(4):
        for value in (0, 1, 0x7F, 0xFF, s[at] + 1, s[at] - 1):
            poke(at, value)
    for lg in range(4):  # the tag's width, the tag's mode
        poke(0, (s[0] & ~3) | lg)
        poke(0, (s[0] & ~0x0C) | lg << 2)
    out += [(s, len(s) + 1), (s, len(s) - 1), (s, 3), (s, 0)]
    mode = (s[0] >> 2) & 3
    if mode != 2:
        L = 1 + s[2] + (s[3] << 8)
        p = 4 + (w if mode == 1 else 0)
        for k in range((L // w + 63) // 64):  # every widths[] byte
            poke(p + k, 8 * w + 1)
            poke(p + k, 255)
        poke(p, s[p] - 1 if s[p] else 1)  # a valid width, but the size no longer adds up
    return out


@pytest.mark.parametrize("seg", (4096, 65536))
@pytest.mark.parametrize("w", M.WIDTHS)
def test_hostile_streams_get_the_model_verdict(eng, w, seg):
    """every mutant is accepted with the model's bytes or rejected with SEGMENT_ERROR, the sync
    reports IOError exactly when one was rejected, nothing outside the output is written and
    the engine works afterwards"""
    import bitar_amd as B
    codec = B.codec_intpack(w)
    stride = B.slot_size(codec, seg)
    for base in base_streams(w, seg):
        muts = mutants(base, w)
        nseg = len(muts)
        slab = np.full((nseg, stride), 0x5A, np.uint8)
        for i, (t, _) in enumerate(muts):
            slab[i, :len(t)] = np.frombuffer(t, np.uint8)
        verdicts = [M.decode(slab[i, :size].tobytes(), seg) for i, (_, size) in enumerate(muts)]
        assert verdicts[0] is not None and any(v is None for v in verdicts)
        d_slab = dev(slab.reshape(-1))
        d_sizes = dev(np.array([size for _, size in muts], np.int32))
        out = torch.full((PAD + nseg * seg + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        prod = torch.full((nseg + 16,), int(CANARY32), dtype=torch.int32, device="cuda")
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, nseg, seg, out.data_ptr() + PAD,
                                 prod.data_ptr() + 32, capacity=nseg * seg)
        with pytest.raises(B.BitarError) as e:
            eng.sync()
        assert e.value.code == -5
        got = prod.cpu().numpy()
        assert np.all(got[:8] == CANARY32) and np.all(got[8 + nseg:] == CANARY32)
        want = [ERR if v is None else len(v) for v in verdicts]
        assert got[8:8 + nseg].tolist() == want
        assert bool((out[:PAD] == CANARY).all()) and bool((out[PAD + nseg * seg:] == CANARY).all())
        for i, v in enumerate(verdicts):
            if v is not None:
                o = PAD + i * seg
                seg_out = out[o:o + seg].cpu().numpy()
                assert seg_out[:len(v)].tobytes() == v, i
                assert np.all(seg_out[len(v):] == CANARY), i
        # the engine works afterwards, and the error was reported once
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, 1, seg, out.data_ptr() + PAD,
                                 prod.data_ptr() + 32, capacity=seg)
        eng.sync()
        assert out[PAD:PAD + seg].cpu().numpy().tobytes() == verdicts[0]


def test_every_id_decodes_every_width(eng):
    import bitar_amd as B
    seg = 4096
    datas = [column(seg, w, 3 + w) for w in M.WIDTHS]
    streams = [M.encode(d, w, seg)[0] for d, w in zip(datas, M.WIDTHS)]
    stride = B.slot_size(B.CODEC_INTPACK8, seg)
    slab = np.zeros((4, stride), np.uint8)
    for i, s in enumerate(streams):
        slab[i, :len(s)] = np.frombuffer(s, np.uint8)
    d_slab = dev(slab.reshape(-1))
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    for w in M.WIDTHS:
        buf = Buffers(4, stride, seg)
        eng.decompress_slab_into(B.codec_intpack(w), d_slab, stride, d_sizes, 4, seg, buf.out_ptr,
                                 buf.prod_ptr, capacity=4 * seg)
        eng.sync()
        buf.check_output(np.concatenate(datas))


def test_compress_bits_refuses_intpack(eng):
    import bitar_amd as B
    src = dev(column(8192, 4, 1))
    buf = Buffers(2, 4352, 4096)
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    for w in M.WIDTHS:
        with pytest.raises(B.BitarError) as e:
            eng.compress_bits_into(B.codec_intpack(w), src, 4096, buf.slab_ptr, 4352,
                                   buf.sizes_ptr, bits)
        assert e.value.code == -4
    eng.sync()
    assert bool((buf.slab == CANARY).all())
