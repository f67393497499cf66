"""GPU tests of the FLTPACK codec (csrc/fltpack.hip) through the C ABI: the slots and sizes of
a compress equal the numpy model's streams (fltpack_model.py) byte for byte, the decoder
returns the input, and on mutated streams its verdict and its bytes are the model's, with
canaries around every buffer a call writes.

Shapes: segments of 65536 and 4096; last segments of 1, w - 1, w, w + 1 bytes, of one miniblock
(64 elements) and one block (256 elements) and one element more, of 59460 bytes (the
reference's segment) and a full one; the input at every byte offset 0..7, the output at every
byte offset 0..7, the streams of a pointer list at every byte offset 0..7."""
import numpy as np
import pytest

import fltpack_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEGS = (65536, 4096)
CANARY = 0xA5
CANARY32 = np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]
PAD = 256
ERR = np.array([0xFFFFFFFF], np.uint32).view(np.int32)[0]
F = {4: np.dtype("<f4"), 8: np.dtype("<f8")}
U = {4: np.dtype("<u4"), 8: np.dtype("<u8")}


@pytest.fixture(scope="module")
def eng():
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0)
    yield e
    e.close()


def lengths(w, seg):
    return [r for r in (1, w - 1, w, w + 1, 64 * w, 64 * w + 1, 256 * w, 256 * w + w, 59460,
                        65536) if r <= seg]


def nans(m, w):
    """m NaNs with distinct payloads"""
    base = 0x7FC00000 if w == 4 else 0x7FF8000000000000
    return (np.arange(1, m + 1).astype(U[w]) + U[w].type(base)).view(F[w])


def decimals(m, w, e, seed, span=100000):
    rng = np.random.default_rng(seed)
    return (rng.integers(-span, span, m) / 10.0 ** e).astype(F[w])


def noise(rng, m, w):
    """values no exponent holds: N(0,1) doubles; floats of the same kind scaled past the largest
    integer (many plain N(0,1) floats are 8-digit decimals: they pack at e = 8)"""
    return (rng.normal(0, 1, m) * (1 if w == 8 else 1e30)).astype(F[w])


def column(n, w, seed, seg):
    """n bytes whose segments take every form.  Per segment of `seg` bytes, in turn: 2-decimal
    values with exceptions at lane 0 and lane 63 of a miniblock, a miniblock of exceptions only,
    a constant block (widths 0) and an exception as the last element; integers (e = 0) without
    any exception; noise (stored); 1-decimal values with 5 % exceptions of every kind"""
    rng = np.random.default_rng(seed)
    per = max(seg // w, 1)
    m = n // w + 1
    v = np.zeros(m, F[w])
    odd = np.array([np.nan, np.inf, -np.inf, -0.0, 0.1 + 0.2, 1e-40 if w == 4 else 1e-310, 1 / 3,
                    1e30], F[w])
    for i, a in enumerate(range(0, m, per)):
        k = min(per, m - a)
        kind = i % 4
        if kind == 0:
            s = decimals(k, w, 2, seed + i)
            s[0:1] = np.nan
            s[63:64] = np.inf
            s[64:128] = nans(64, w)[:len(s[64:128])]
            s[256:512] = 7.25
            s[k - 1] = -0.0
        elif kind == 1:
            s = decimals(k, w, 0, seed + i, 1000)
        elif kind == 2:
            s = noise(rng, k, w)
        else:
            s = decimals(k, w, 1, seed + i)
            at = rng.random(k) < 0.05
            s[at] = odd[rng.integers(0, odd.size, int(at.sum()))]
        v[a:a + k] = s
    return v.view(np.uint8)[:n].copy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


class Buffers:
    """device buffers of one compress + decompress with canaries on both sides of each; the
    output starts out_off bytes past a 256-B boundary"""

    def __init__(self, nseg, stride, seg, out_off=0):
        self.nseg, self.stride, self.seg, self.out_off = nseg, stride, seg, out_off
        self.slab = torch.full((PAD + nseg * stride + PAD,), CANARY, dtype=torch.uint8,
                               device="cuda")
        self.sizes = torch.full((nseg + 16,), int(CANARY32), dtype=torch.int32, device="cuda")
        self.out = torch.full((PAD + nseg * seg + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        self.prod = torch.full((nseg + 16,), int(CANARY32), dtype=torch.int32, device="cuda")

    slab_ptr = property(lambda self: self.slab.data_ptr() + PAD)
    sizes_ptr = property(lambda self: self.sizes.data_ptr() + 32)
    out_ptr = property(lambda self: self.out.data_ptr() + PAD + self.out_off)
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
                (i, s[0], s[1], np.flatnonzero(slot[:want.size] != want)[:8].tolist())
            assert np.all(slot[want.size:] == CANARY), i

    def check_output(self, data):
        n = data.size
        prod = self.prod.cpu().numpy()
        assert np.all(prod[:8] == CANARY32) and np.all(prod[8 + self.nseg:] == CANARY32)
        want = [min(self.seg, n - i * self.seg) for i in range(self.nseg)]
        assert prod[8:8 + self.nseg].tolist() == want
        out = self.out.cpu().numpy()
        o = PAD + self.out_off
        assert np.all(out[:o] == CANARY) and np.all(out[o + n:] == CANARY)
        assert np.array_equal(out[o:o + n], data), np.flatnonzero(out[o:o + n] != data)[:8]


def check_case(eng, w, seg, data, in_off=0, out_off=0):
    import bitar_amd as B
    codec = B.codec_fltpack(w)
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec, seg)
    src = torch.zeros(in_off + n + PAD, dtype=torch.uint8, device="cuda")
    src[in_off:in_off + n] = dev(data)
    buf = Buffers(nseg, stride, seg, out_off)
    eng.compress_into(codec, src.data_ptr() + in_off, seg, buf.slab_ptr, stride, buf.sizes_ptr, n=n)
    eng.decompress_slab_into(codec, buf.slab_ptr, stride, buf.sizes_ptr, nseg, seg, buf.out_ptr,
                             buf.prod_ptr, capacity=nseg * seg)
    eng.sync()
    streams = M.encode(data, w, seg)
    buf.check_streams(streams)
    buf.check_output(data)
    return streams


def mode_of(s):
    return (s[0] >> 2) & 3


def nx_of(s):
    return s[4] | s[5] << 8


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_exact_bytes_and_round_trip(eng, w, seg):
    """four whole segments (one of every form) and a last one of each length"""
    forms = set()
    for r in lengths(w, seg):
        streams = check_case(eng, w, seg, column(4 * seg + r, w, seg + r + w, seg))
        forms |= {(mode_of(s), s[1]) for s in streams[:4]}
    assert forms == {(0, 2), (0, 0), (2, 0), (0, 1)}


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_every_alignment(eng, w, seg):
    """the input at each offset 0..7 and, each time, the output at another one (all of 0..7)"""
    data = column(2 * seg + 64 * w + 1, w, seg + w, seg)
    for off in range(8):
        check_case(eng, w, seg, data, in_off=off, out_off=(3 * off + 1) % 8)


def one_segment(eng, w, col):
    (s,) = check_case(eng, w, 65536, np.ascontiguousarray(col).view(np.uint8))
    return s


@pytest.mark.parametrize("w", M.WIDTHS)
def test_inputs(eng, w):
    m = 1000
    plain = decimals(m, w, 2, w)
    s = one_segment(eng, w, plain)                              # no exceptions
    assert mode_of(s) == 0 and s[1] == 2 and nx_of(s) == 0
    col = plain.copy()
    col[128] = np.nan                                           # lane 0 and lane 63
    col[191] = np.inf
    s = one_segment(eng, w, col)
    assert mode_of(s) == 0 and nx_of(s) == 2
    col = plain.copy()
    col[m - 1] = -0.0                                           # the segment's last element
    s = one_segment(eng, w, col)
    assert mode_of(s) == 0 and nx_of(s) == 1
    col[0] = np.nan                                             # ... and its first
    s = one_segment(eng, w, col)
    assert mode_of(s) == 0 and nx_of(s) == 2
    s = one_segment(eng, w, nans(m, w))                         # every element an exception
    assert mode_of(s) == 2
    col = plain.copy()
    col[256:512] = nans(256, w)                                 # a block of exceptions only
    s = one_segment(eng, w, col)
    assert mode_of(s) == 0 and nx_of(s) == 256 and list(s[10:14]) == [0] * 4
    col = plain.copy()
    col[512:768] = 12.5                                         # miniblocks of width 0
    s = one_segment(eng, w, col)
    assert mode_of(s) == 0 and list(s[14:18]) == [0] * 4 and s[7] > 0
    # the largest integers: 2^53 / the largest float below 2^31, and one step beyond
    big = np.array([2.0 ** 53, -2.0 ** 53, 2.0 ** 53 + 2] if w == 8 else
                   [2147483520.0, -2147483520.0, 2147483648.0], F[w])
    col = np.arange(512).astype(F[w])
    col[1:4] = big
    s = one_segment(eng, w, col)
    assert mode_of(s) == 0 and s[1] == 0 and nx_of(s) == 1 and s[6] == (55 if w == 8 else 32)
    # two segments whose exponents differ
    a, b = decimals(65536 // w, w, 0, 1, 1000), decimals(65536 // w, w, 3, 2)
    streams = check_case(eng, w, 65536, np.concatenate([a, b]).view(np.uint8))
    assert [(mode_of(s), s[1]) for s in streams] == [(0, 0), (0, 3)]


def test_empty_input_launches_nothing(eng):
    import bitar_amd as B
    buf = Buffers(1, 4352, 4096)
    src = torch.zeros(PAD, dtype=torch.uint8, device="cuda")
    for w in M.WIDTHS:
        eng.compress_into(B.codec_fltpack(w), src, 4096, buf.slab_ptr, 4352, buf.sizes_ptr, n=0)
        eng.decompress_slab_into(B.codec_fltpack(w), buf.slab_ptr, 4352, buf.sizes_ptr, 0, 4096,
                                 buf.out_ptr, buf.prod_ptr, capacity=0)
    eng.sync()
    for t in (buf.slab, buf.out):
        assert bool((t == CANARY).all())
    for t in (buf.sizes, buf.prod):
        assert bool((t == int(CANARY32)).all())


@pytest.mark.parametrize("w", M.WIDTHS)
def test_scattered_pointer_list_and_host_paths(eng, w):
    """one shape per width through bitar_hip_compress_scattered, bitar_hip_decompress with the
    streams at every byte offset 0..7, and the host-overlapped pair"""
    import bitar_amd as B
    codec = B.codec_fltpack(w)
    seg = 59460
    data = column(7 * seg + 64 * w + 1, w, 77 + w, seg)
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec, seg)
    streams = M.encode(data, w, seg)
    src = dev(data)

    # scattered: slot i of the call is slot perm[i] of the slab
    buf = Buffers(nseg, stride, seg)
    perm = [2, 0, 3, 1, 7, 6, 4, 5]
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

    # pointer list: stream i starts i bytes past a 16-B boundary
    room = (max(len(s) for s in streams) + 32) & ~15
    packed = np.full(nseg * room + 16, CANARY, np.uint8)
    ptrs = []
    for i, s in enumerate(streams):
        o = i * room + i
        packed[o:o + len(s)] = np.frombuffer(s, np.uint8)
        ptrs.append(o)
    d_packed = dev(packed)
    assert d_packed.data_ptr() % 16 == 0
    d_ptrs = dev(np.array(ptrs, np.int64) + d_packed.data_ptr())
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    buf = Buffers(nseg, stride, seg, out_off=5)
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
    """a packed stream with exceptions (first and last element, lanes 63 and 0 of neighbouring
    miniblocks, two neighbours) and a stored stream, of full segments of `seg` bytes"""
    m = seg // w
    col = decimals(m, w, 2, seg + w)
    col[[0, 63, 64, 200, 201, m - 1]] = nans(6, w)
    (packed,) = M.encode(col.view(np.uint8), w, seg)
    assert mode_of(packed) == 0 and nx_of(packed) == 6
    (stored,) = M.encode(noise(np.random.default_rng(seg), m, w).view(np.uint8), w, seg)
    assert mode_of(stored) == 2
    return [packed, stored]


def mutants(s, w):
    """deterministic mutations of the stream s -> [(bytes, size given to the decoder)]"""
    out = [(s, len(s))]

    def poke(at, value):
        if s[at] != value & 255:
            t = bytearray(s)
            t[at] = value & 255
            out.append((bytes(t), len(s)))

    packed = mode_of(s) == 0
    head = 6 if packed else 4
    for bit in range(8):  # each header byte (nx included), bit by bit; then some whole values
        for at in range(head):
            poke(at, s[at] ^ (1 << bit))
    for at in range(head):
        for value in (0, 1, 15, 16, 0x7F, 0xFF, s[at] + 1, s[at] - 1):
            poke(at, value)
    for lg in range(4):  # the tag's width, the tag's mode
        poke(0, (s[0] & ~3) | lg)
        poke(0, (s[0] & ~0x0C) | lg << 2)
    poke(0, 0x40 | (s[0] & 15))  # INTPACK's tag
    out += [(s, len(s) + 1), (s, len(s) - 1), (s, 3), (s, 0), (s, 4), (s, 5), (s, 6)]
    if packed:
        L = 1 + s[2] + (s[3] << 8)
        m, nmb, nblk = M._counts(L, w)
        for k in range(nmb):  # every widths[] byte
            poke(6 + k, 8 * w + 1)
            poke(6 + k, 255)
        poke(6, s[6] - 1)  # a valid width, but the size no longer adds up
        p = 6 + nmb + nblk * w + 8 * sum(s[6:6 + nmb])
        nx = nx_of(s)
        pos = [s[p + 2 * i] | s[p + 2 * i + 1] << 8 for i in range(nx)]
        for i in range(nx):  # every position: past the end, on and below its neighbours, moved
            lo, hi = p + 2 * i, p + 2 * i + 1
            for value in (m, 0xFFFF, pos[i - 1] if i else pos[i], pos[i - 1] - 1 if i else pos[i],
                          pos[i + 1] if i + 1 < nx else m, pos[i] + 1, pos[i] - 1):
                if 0 <= value <= 0xFFFF and value != pos[i]:
                    t = bytearray(s)
                    t[lo], t[hi] = value & 255, value >> 8
                    out.append((bytes(t), len(s)))
    return out


@pytest.mark.parametrize("seg", (4096, 65536))
@pytest.mark.parametrize("w", M.WIDTHS)
def test_hostile_streams_get_the_model_verdict(eng, w, seg):
    """every mutant is accepted with the model's bytes or rejected with SEGMENT_ERROR, the sync
    reports IOError exactly when one was rejected, nothing outside the output is written and
    the engine works afterwards"""
    import bitar_amd as B
    codec = B.codec_fltpack(w)
    stride = B.slot_size(codec, seg)
    for base in base_streams(w, seg):
        muts = mutants(base, w)
        nseg = len(muts)
        slab = np.full((nseg, stride), 0x5A, np.uint8)
        for i, (t, _) in enumerate(muts):
            slab[i, :len(t)] = np.frombuffer(t, np.uint8)
        verdicts = [M.decode(slab[i, :size].tobytes(), seg) for i, (_, size) in enumerate(muts)]
        assert verdicts[0] is not None and any(v is None for v in verdicts)
        if mode_of(base) == 0:  # (moved positions that stay in order are accepted)
            assert sum(v is not None for v in verdicts) > 4
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
        host = out.cpu().numpy()
        for i, v in enumerate(verdicts):
            seg_out = host[PAD + i * seg:PAD + (i + 1) * seg]
            if v is not None:
                assert seg_out[:len(v)].tobytes() == v, i
                assert np.all(seg_out[len(v):] == CANARY), i
            else:  # a rejected stream: nothing was written
                assert np.all(seg_out == CANARY), i
        # the engine works afterwards, and the error was reported once
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, 1, seg, out.data_ptr() + PAD,
                                 prod.data_ptr() + 32, capacity=seg)
        eng.sync()
        assert out[PAD:PAD + seg].cpu().numpy().tobytes() == verdicts[0]


@pytest.mark.parametrize("w", M.WIDTHS)
def test_any_residual_bits_decode_like_the_model(eng, w):
    """random payload and references under a valid header: accepted, arithmetic mod 2^(8w), any
    n converts and divides, exceptions patched"""
    import bitar_amd as B
    seg = 4096
    codec = B.codec_fltpack(w)
    stride = B.slot_size(codec, seg)
    (base,) = base_streams(w, seg)[:1]
    m, nmb, nblk = M._counts(seg, w)
    rng = np.random.default_rng(w)
    muts = []
    for e in (0, 1, 7, 15):
        t = bytearray(base)
        t[1] = e
        t[6:6 + nmb] = bytes([min(8 * w, 8 * w - 3 + k % 4) for k in range(nmb)])
        pay = 6 + nmb + nblk * w
        tail = bytes(base[pay + 8 * sum(base[6:6 + nmb]):])  # pos, val
        body = rng.integers(0, 256, nblk * w + 8 * sum(t[6:6 + nmb]), dtype=np.uint8).tobytes()
        t = bytes(t[:6 + nmb]) + body + tail
        if len(t) <= stride:
            muts.append(t)
    assert muts
    nseg = len(muts)
    slab = np.zeros((nseg, stride), np.uint8)
    for i, t in enumerate(muts):
        slab[i, :len(t)] = np.frombuffer(t, np.uint8)
    verdicts = [M.decode(t, seg) for t in muts]
    assert all(v is not None for v in verdicts)
    buf = Buffers(nseg, stride, seg)
    eng.decompress_slab_into(codec, dev(slab.reshape(-1)), stride,
                             dev(np.array([len(t) for t in muts], np.int32)), nseg, seg,
                             buf.out_ptr, buf.prod_ptr, capacity=nseg * seg)
    eng.sync()
    buf.check_output(np.frombuffer(b"".join(verdicts), np.uint8))


def test_ids_and_tags(eng):
    """either FLTPACK id decodes both widths; the FLTPACK ids reject INTPACK's tag and the
    INTPACK ids reject FLTPACK's"""
    import bitar_amd as B
    import intpack_model as I
    seg = 4096
    datas = [column(seg, w, 3 + w, seg) for w in M.WIDTHS]
    streams = [M.encode(d, w, seg)[0] for d, w in zip(datas, M.WIDTHS)]
    ints = np.arange(1024, dtype="<u4").view(np.uint8)
    streams.append(I.encode(ints, 4, seg)[0])
    assert streams[2][0] >> 4 == 4
    stride = B.slot_size(B.CODEC_FLTPACK32, seg)
    slab = np.zeros((3, stride), np.uint8)
    for i, s in enumerate(streams):
        slab[i, :len(s)] = np.frombuffer(s, np.uint8)
    d_slab = dev(slab.reshape(-1))
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    for codec in (B.CODEC_FLTPACK32, B.CODEC_FLTPACK64):
        buf = Buffers(2, stride, seg)
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, 2, seg, buf.out_ptr,
                                 buf.prod_ptr, capacity=2 * seg)
        eng.sync()
        buf.check_output(np.concatenate(datas))
    for codec, want in ((B.CODEC_FLTPACK64, [seg, seg, ERR]), (B.CODEC_INTPACK32, [ERR, ERR, seg])):
        buf = Buffers(3, stride, seg)
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, 3, seg, buf.out_ptr,
                                 buf.prod_ptr, capacity=3 * seg)
        with pytest.raises(B.BitarError) as e:
            eng.sync()
        assert e.value.code == -5
        assert buf.prod.cpu().numpy()[8:11].tolist() == want


def test_compress_bits_refuses_fltpack(eng):
    import bitar_amd as B
    src = dev(column(8192, 4, 1, 4096))
    buf = Buffers(2, 4352, 4096)
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    for w in M.WIDTHS:
        with pytest.raises(B.BitarError) as e:
            eng.compress_bits_into(B.codec_fltpack(w), src, 4096, buf.slab_ptr, 4352,
                                   buf.sizes_ptr, bits)
        assert e.value.code == -4
    eng.sync()
    assert bool((buf.slab == CANARY).all())
