"""GPU tests of the DICTPACK codec (csrc/dictpack.hip) through the C ABI: the slots and sizes of
a compress equal the numpy model's streams (dictpack_model.py) byte for byte, the decoder
returns the input, and on mutated streams its verdict is the model's, with canaries around
every buffer a call writes.

Shapes: segments of 65536 (16-B aligned everywhere), 59460 (the reference's segment: elements
straddle segment starts), 4096, 1000 / 999 (odd bases: every element unaligned), 72 and 7
(one partial miniblock, shorter than an element); lengths that end on and next to an element, a
miniblock (64 elements) and a block of four."""
import numpy as np
import pytest

import dictpack_model as M

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


def mode_of(s):
    return s[0] >> 3 & 1


def pool(d, w, seed):
    """d distinct rows of w random bytes"""
    rows = rnd(d * w, seed).reshape(d, w)
    rows[:, 0] = np.arange(d) & 255
    rows[:, w - 1] = np.arange(d) >> 8
    return rows


def column(n, w, seed):
    """n bytes whose segments take both forms: five stretches drawn from 1, 2, 37, 300 and 1000
    values (whole segments of them pack, at b = 0, 1, 6, 9 and 10) and random bytes (stored)"""
    rng = np.random.default_rng(seed)
    m = n // w + 1
    q = m // 8
    idx = np.zeros(m, np.int64)
    for j, d in enumerate((1, 2, 37, 300, 1000)):
        idx[j * q:(j + 1) * q] = rng.integers(0, d, q) + (0, 1, 3, 40, 340)[j]
    out = pool(1340, w, seed + 1)[idx].reshape(-1)[:n].copy()
    a = 5 * q * w  # (the last three eighths: whole segments of it are stored)
    out[a:] = rnd(n - a, seed + 2)
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
    codec = B.codec_dictpack(w)
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
        # (8 segments: each stretch of the column covers whole ones)
        for s in check_case(eng, w, seg, column(8 * seg + r, w, seg * 31 + r + w)):
            forms.add(mode_of(s))
    if seg >= 1000:
        assert forms == {0, 1}  # (packed and stored)
    if seg == 72:
        for n in range(1, w):  # shorter than an element
            check_case(eng, w, seg, rnd(n, n))


@pytest.mark.parametrize("w", M.WIDTHS)
def test_input_at_every_alignment(eng, w):
    for seg in (59460, 4096):
        for in_off in (0, 1, 3, 4, 15):
            check_case(eng, w, seg, column(8 * seg + 64 * w + 1, w, in_off + w), in_off=in_off)


CARDS = [1, 2, 3] + [x for k in range(2, 10) for x in (1 << k, (1 << k) + 1)] + [1023, 1024, 1025]


@pytest.mark.parametrize("w", M.WIDTHS)
def test_cardinalities(eng, w):
    """one segment of 65536 bytes per d, whose last value first shows in the segment's final
    element; then the same with a last segment that ends inside a miniblock"""
    seg = 65536
    m = seg // w
    rows = pool(1025, w, 50 + w)
    segs = []
    for d in CARDS:
        idx = np.random.default_rng(d).integers(0, max(d - 1, 1), m)
        idx[:d - 1] = np.arange(d - 1)[::-1]  # (first occurrences against the rows' order)
        idx[m - 1] = d - 1
        segs.append(rows[idx].reshape(-1))
    streams = check_case(eng, w, seg, np.concatenate(segs))
    for d, s in zip(CARDS, streams):
        if d == 1025:
            assert mode_of(s) == 1
        else:
            assert mode_of(s) == 0 and 1 + s[4] + (s[5] << 8) == d, d
    for d in (2, 3, 33, 513, 1024):
        mp = 2048 + 64 + 7  # the last miniblock holds 7 elements, the new value is the 7th
        idx = np.random.default_rng(d).integers(0, d - 1, mp)
        idx[:d - 1] = np.arange(d - 1)
        idx[mp - 1] = d - 1
        data = np.concatenate([segs[3], rows[idx].reshape(-1), rnd(w - 1, d)])
        streams = check_case(eng, w, seg, data)
        assert mode_of(streams[1]) == 0 and 1 + streams[1][4] + (streams[1][5] << 8) == d


@pytest.mark.parametrize("w", M.WIDTHS)
def test_break_even(eng, w):
    """for several d the shortest segment that packs and the one an element shorter, which is
    stored (found with the model's size formula)"""
    rows = pool(300, w, 60 + w)
    seen = set()
    for d in (1, 2, 3, 5, 17, 200):
        m = next(m for m in range(d, 1 << 14) if M.packed_size(m * w, w, d) < 4 + m * w)
        for mm, tail in ((m, 0), (m - 1, 0), (m, w - 1), (m - 1, w - 1)):
            if mm < d:
                continue
            data = np.concatenate([rows[np.arange(mm) % d].reshape(-1), rnd(tail, d)])
            (s,) = check_case(eng, w, 65536, data)
            assert mode_of(s) == (0 if M.packed_size(data.size, w, d) < 4 + data.size else 1)
            seen.add(mode_of(s))
    assert seen == {0, 1}


def hard_keys(w):
    """pools of values a lazy hash or compare gets wrong -> [(name, rows d x w)]"""
    U = {4: "<u4", 8: "<u8"}
    out = []
    top = np.zeros((256, w), np.uint8)
    top[:, :w - 1] = rnd(w - 1, 1)
    top[:, w - 1] = np.arange(256)
    out.append(("top byte only", top))
    low = np.zeros((256, w), np.uint8)
    low[:, 1:] = rnd(w - 1, 2)
    low[:, 0] = np.arange(256)
    out.append(("lowest byte only", low))
    for k in (8, 8 * w - 10):  # multiples of 2^k
        mult = b"".join((i << k).to_bytes(w, "little") for i in range(1000))
        out.append((f"multiples of 2^{k}", np.frombuffer(mult, np.uint8).reshape(1000, w)))
    if w == 16:
        for name, sl in (("upper 8 bytes only", slice(8, 16)), ("lower 8 bytes only", slice(0, 8))):
            rows = np.tile(rnd(16, 3), (700, 1))
            rows[:, sl] = rnd(700 * 8, 4).reshape(700, 8)
            rows[:, sl.start] = np.arange(700) & 255
            rows[:, sl.start + 1] = np.arange(700) >> 8
            out.append((name, rows))
    if w in U:
        bits = 8 * w
        sign, quiet = 1 << (bits - 1), (0xFF << 23 | 1 << 22) if w == 4 else (0x7FF << 52 | 1 << 51)
        pats = [0, sign, quiet, quiet | 1, quiet | 2, quiet | sign, quiet ^ (1 << (bits - 10)) | 1]
        out.append(("zeros and NaNs", np.array(pats, U[w]).view(np.uint8).reshape(len(pats), w)))
    return out


@pytest.mark.parametrize("w", M.WIDTHS)
def test_keys_that_punish_a_lazy_hash_or_compare(eng, w):
    for name, rows in hard_keys(w):
        assert np.unique(rows, axis=0).shape[0] == rows.shape[0], name
        for seg in (65536, 999):
            idx = np.random.default_rng(seg).integers(0, rows.shape[0], (2 * seg + 5) // w)
            streams = check_case(eng, w, seg, rows[idx].reshape(-1))
            assert seg == 999 or mode_of(streams[0]) == 0, name
    if w == 4:
        # pairs that are equal as one 8-byte unit but not element-wise: (a, b) (a, b) ... and
        # (a, b) against (a, c), (c, b)
        a, b, c = rnd(4, 1), rnd(4, 2), rnd(4, 3)
        for pat in ((a, b) * 600, (a, b, a, c, c, b) * 200):
            check_case(eng, 4, 4096, np.concatenate(pat))


def test_empty_input_launches_nothing(eng):
    import bitar_amd as B
    buf = Buffers(1, 4352, 4096)
    src = torch.zeros(PAD, dtype=torch.uint8, device="cuda")
    for w in M.WIDTHS:
        eng.compress_into(B.codec_dictpack(w), src, 4096, buf.slab_ptr, 4352, buf.sizes_ptr, n=0)
        eng.decompress_slab_into(B.codec_dictpack(w), buf.slab_ptr, 4352, buf.sizes_ptr, 0, 4096,
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
    codec = B.codec_dictpack(w)
    seg = 59460
    data = column(3 * seg + 64 * w + 1, w, 77 + w)
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec, seg)
    streams = M.encode(data, w, seg)
    assert {mode_of(s) for s in streams} == {0, 1}
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
    """a packed stream with b = 3, one with d = 1 and a stored one, each of a segment that ends
    inside a miniblock and has a tail"""
    L = seg - 5 * w - 3
    m = L // w
    rows = pool(5, w, seg + w)
    out = []
    for form, body in ((0, rows[np.random.default_rng(seg).integers(0, 5, m)]),
                       (0, rows[np.zeros(m, np.int64)]), (1, rnd(m * w, seg))):
        data = np.concatenate([body.reshape(-1), rnd(L - m * w, 5)])
        (s,) = M.encode(data, w, seg)
        assert mode_of(s) == form and M.decode(s, seg) == data.tobytes()
        out.append(s)
    assert out[0][4] == 4 and out[1][4] == 0
    return out


def mutants(s, w):
    """deterministic mutations of the stream s -> [(bytes, size given to the decoder)]"""
    out = [(s, len(s))]

    def poke(at, value, base=s):
        if base[at] != value & 255:
            t = bytearray(base)
            t[at] = value & 255
            out.append((bytes(t), len(s)))

    for bit in range(8):  # the six header bytes, bit by bit; then some whole values
        for at in range(6):
            poke(at, s[at] ^ (1 << bit))
    for at in range(6):
        for value in (0, 1, 0x7F, 0xFF, s[at] + 1, s[at] - 1):
            poke(at, value)
    for nib in range(16):  # the tag's nibble, its mode, its width
        poke(0, nib << 4 | s[0] & 15)
    poke(0, s[0] ^ 8)
    for lg in range(8):
        poke(0, s[0] & ~7 | lg)
    out += [(s, len(s) + 1), (s, len(s) - 1), (s, 3), (s, 0)]
    if mode_of(s) == 0:
        L = 1 + s[2] + (s[3] << 8)
        m, d = L // w, 1 + s[4] + (s[5] << 8)
        b = (d - 1).bit_length()
        for dd in (m + 1, 1025, 2 * d + 1, 2 if d > 2 else 3):  # too many; a d that changes b
            t = bytearray(s)
            t[4], t[5] = (dd - 1) & 255, (dd - 1) >> 8
            out.append((bytes(t), len(s)))
        # duplicate dictionary entries
        t = bytearray(s)
        t[6:6 + w] = s[6 + (d - 1) * w:6 + d * w]
        out.append((bytes(t), len(s)))
        if b:
            pay = 6 + d * w

            def with_index(t, value):
                u = bytearray(s)
                k, slot = divmod(t, 64)
                for j in range(b):
                    bit = slot * b + j
                    at = pay + k * 8 * b + bit // 8
                    u[at] = u[at] & ~(1 << bit % 8) | (value >> j & 1) << bit % 8
                return bytes(u)

            last_mb = (m - 1) // 64 * 64
            for t in (0, 63, 64, last_mb, m - 1):  # an index that is no entry; the largest that is
                out.append((with_index(t, d - 1), len(s)))
                out.append((with_index(t, d), len(s)))
                out.append((with_index(t, (1 << b) - 1), len(s)))
            for t in (m, (m + 63) // 64 * 64 - 1):  # non-zero padding slots: ignored
                out.append((with_index(t, (1 << b) - 1), len(s)))
    return out


@pytest.mark.parametrize("seg", (4096, 65536))
@pytest.mark.parametrize("w", M.WIDTHS)
def test_hostile_streams_get_the_model_verdict(eng, w, seg):
    """every mutant is accepted with the model's bytes or rejected with SEGMENT_ERROR, the sync
    reports IOError exactly when one was rejected, nothing outside the output is written and
    the engine works afterwards"""
    import bitar_amd as B
    codec = B.codec_dictpack(w)
    stride = B.slot_size(codec, seg)
    for base in base_streams(w, seg):
        muts = mutants(base, w)
        nseg = len(muts)
        slab = np.full((nseg, stride), 0x5A, np.uint8)
        for i, (t, _) in enumerate(muts):
            slab[i, :len(t)] = np.frombuffer(t, np.uint8)
        verdicts = [M.decode(slab[i, :size].tobytes(), seg) for i, (_, size) in enumerate(muts)]
        assert verdicts[0] is not None and any(v is None for v in verdicts)
        assert sum(v is not None for v in verdicts) > 1
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
            else:  # a rejected segment never writes past the length its header gives
                t = muts[i][0]
                L = 1 + t[2] + (t[3] << 8) if muts[i][1] >= 4 else 0
                assert np.all(seg_out[min(L, seg):] == CANARY), i
        # the engine works afterwards, and the error was reported once
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, 1, seg, out.data_ptr() + PAD,
                                 prod.data_ptr() + 32, capacity=seg)
        eng.sync()
        assert out[PAD:PAD + len(verdicts[0])].cpu().numpy().tobytes() == verdicts[0]


def test_every_id_decodes_every_width(eng):
    import bitar_amd as B
    seg = 4096
    datas = [column(8 * seg, w, 3 + w)[2 * seg:3 * seg] for w in M.WIDTHS]  # (37 values)
    streams = [M.encode(d, w, seg)[0] for d, w in zip(datas, M.WIDTHS)]
    assert all(mode_of(s) == 0 for s in streams)
    stride = B.slot_size(B.CODEC_DICTPACK32, seg)
    slab = np.zeros((3, stride), np.uint8)
    for i, s in enumerate(streams):
        slab[i, :len(s)] = np.frombuffer(s, np.uint8)
    d_slab = dev(slab.reshape(-1))
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    for w in M.WIDTHS:
        buf = Buffers(3, stride, seg)
        eng.decompress_slab_into(B.codec_dictpack(w), d_slab, stride, d_sizes, 3, seg, buf.out_ptr,
                                 buf.prod_ptr, capacity=3 * seg)
        eng.sync()
        buf.check_output(np.concatenate(datas))


def test_compress_bits_refuses_dictpack(eng):
    import bitar_amd as B
    src = dev(column(8192, 4, 1))
    buf = Buffers(2, 4352, 4096)
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    for w in M.WIDTHS:
        with pytest.raises(B.BitarError) as e:
            eng.compress_bits_into(B.codec_dictpack(w), src, 4096, buf.slab_ptr, 4352,
                                   buf.sizes_ptr, bits)
        assert e.value.code == -4
    eng.sync()
    assert bool((buf.slab == CANARY).all())
