"""GPU tests of the RUNPACK codec (csrc/runpack.hip) through the C ABI: the slots and sizes of a
compress equal the numpy model's streams (runpack_model.py) byte for byte, the decoder returns
the input, and on mutated streams its verdict is the model's, with canaries around every buffer
a call writes.

Shapes: segments of 65536 (16-B aligned everywhere), 59460 (the reference's segment: elements
straddle segment starts), 4096, 1000 / 999 (odd bases: every element unaligned), 72 and 7
(shorter than a step, shorter than an element); lengths that end on and next to an element, a
row of 64 elements and 256 of them.  Both kernels work on chunks of 16 bytes, 64 chunks a step,
so a step is 1024 / w elements; the decoder reads run lengths 64 at a time; the encoder keeps a
segment's first 256 or 1024 heads in LDS and takes another path when there are more."""
import numpy as np
import pytest

import runpack_model as M

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
    if w > 1:
        rows[:, w - 1] = np.arange(d) >> 8
    return rows


def runs(rows, lengths):
    """run k: row k (cyclically) of `rows`, lengths[k] times -> (elements, w)"""
    lengths = np.asarray(lengths)
    return np.repeat(rows[np.arange(lengths.size) % rows.shape[0]], lengths, axis=0)


def geometric(rng, m, mean):
    out = rng.geometric(1.0 / mean, m // mean + 64)
    while out.sum() < m:
        out = np.append(out, rng.geometric(1.0 / mean, 256))
    return out


def column(n, w, seed):
    """n bytes in eight stretches: one value throughout; runs of exactly 63, 64, 65, 256 and 257
    with runs of 1 between them; geometric run lengths of mean 3; of mean 300 (two stretches);
    and random bytes (three).  A stretch is n // 8 bytes, so runs cross rows of 64 elements and,
    where the segment is no multiple of the pattern, segment borders"""
    rng = np.random.default_rng(seed)
    m = n // w + 1
    q = m // 8
    rows = pool(251, w, seed + 1)  # (251 is prime: a cycle of lengths never lines up with it)
    parts = [runs(rows[7:8], [q])]
    cycle = np.array([63, 1, 64, 1, 1, 65, 256, 1, 257, 2, 300, 1, 1, 1])
    parts.append(runs(rows, np.tile(cycle, q // cycle.sum() + 1))[:q])
    parts.append(runs(rows, geometric(rng, q, 3))[:q])
    parts.append(runs(rows, geometric(rng, 2 * q, 300))[:2 * q])
    out = np.concatenate(parts).reshape(-1)
    out = np.concatenate([out, rnd(max(n - out.size, 0), seed + 2)])[:n]
    return out.copy()


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
    codec = B.codec_runpack(w)
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


def forms_of(streams):
    return {(mode_of(s), s[1]) for s in streams}


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_exact_bytes_and_round_trip(eng, w, seg):
    tails = (0, 256 * w + 3) if seg > 4096 else \
        sorted({0, 1, w - 1, w, 63 * w, 64 * w, 64 * w + 1, 256 * w + 3})
    cases = [column(8 * seg + r, w, seg * 31 + r + w) for r in tails]
    # the model first: the segments take both forms and, where a segment has room for a run
    # above 256, both widths of a length
    forms = set().union(*(forms_of(M.encode(c, w, seg)) for c in cases))
    if seg >= 1000:
        assert {(0, 1), (1, 0)} <= forms
    if seg // w > 257:
        assert (0, 2) in forms
    for c in cases:
        check_case(eng, w, seg, c)
    if seg == 72:
        for n in range(1, w):  # shorter than an element
            check_case(eng, w, seg, rnd(n, n))


@pytest.mark.parametrize("w", M.WIDTHS)
def test_input_at_every_alignment(eng, w):
    for seg in (59460, 4096):
        for in_off in (0, 1, 3, 4, 15):
            check_case(eng, w, seg, column(8 * seg + 64 * w + 1, w, in_off + w), in_off=in_off)


def partition(rng, m, r, last):
    """r run lengths that add up to m, the last of them `last`"""
    cuts = np.sort(rng.choice(np.arange(1, m - last), r - 2, replace=False)) if r > 2 else \
        np.zeros(0, np.int64)
    edges = np.concatenate([[0], cuts, [m - last, m]]) if r > 1 else np.array([0, m])
    return np.diff(edges)


@pytest.mark.parametrize("w", M.WIDTHS)
def test_run_counts_at_the_group_border(eng, w):
    """r = 1, 63, 64, 65, 128 and 129 runs in a segment (the decoder reads 64 lengths a step),
    the last run being the segment's final element alone, or ending on it; then r = m - 1,
    which the size rule stores"""
    seg = 4096
    m = seg // w
    rng = np.random.default_rng(w)
    rows = pool(251, w, 40 + w)
    segs, want_r = [], []
    for r in (1, 63, 64, 65, 128, 129):
        for last in (1, 2):
            if r == 1:
                last = m
            segs.append(runs(rows, partition(rng, m, r, last)).reshape(-1))
            want_r.append(r)
    streams = check_case(eng, w, seg, np.concatenate(segs))
    for r, s in zip(want_r, streams):
        assert mode_of(s) == 0 and 1 + s[4] + (s[5] << 8) == r
    # the same runs in segments that end w - 1 bytes into the next element (59 elements shorter)
    seg2 = seg - 59 * w + (w - 1)
    cut = [np.concatenate([s[:seg2 - (w - 1)], rnd(w - 1, 1)]) for s in segs]
    check_case(eng, w, seg2, np.concatenate(cut))
    for mm in (m, 200):
        lengths = np.ones(mm - 1, np.int64)
        lengths[mm // 2] = 2
        (s,) = check_case(eng, w, seg, runs(rows, lengths).reshape(-1))
        assert mode_of(s) == 1


@pytest.mark.parametrize("w", M.WIDTHS)
def test_run_counts_at_the_encoder_threshold(eng, w):
    """the encoder keeps a segment's first 256 (w >= 8) or 1024 heads and reads a segment with
    more of them a second time: r on either side of both numbers, for every width, in full
    segments and in one that ends w - 1 bytes into an element"""
    seg = 65536
    m = seg // w
    rng = np.random.default_rng(100 + w)
    rows = pool(251, w, 70 + w)
    counts = (255, 256, 257, 1023, 1024, 1025)
    segs = [runs(rows, partition(rng, m, r, 1 + r % 2)).reshape(-1) for r in counts]
    segs.append(np.concatenate([segs[2][:seg - 37 * w], rnd(w - 1, 3)]))
    streams = check_case(eng, w, seg, np.concatenate(segs))
    for r, s in zip(counts, streams):
        assert mode_of(s) == 0 and 1 + s[4] + (s[5] << 8) == r


@pytest.mark.parametrize("w", M.WIDTHS)
def test_break_even(eng, w):
    """for several r the shortest segment that takes the runs form and the one an element
    shorter, which is stored (found with the model's size formula); and the tie"""
    rows = pool(251, w, 60 + w)
    seen = set()
    for r in (1, 2, 3, 6, 14, 17, 200):
        m = next(m for m in range(r, 1 << 14) if M.runs_size(m * w, w, r, 1) < 4 + m * w)
        for mm, tail in ((m, 0), (m - 1, 0), (m, w - 1), (m - 1, w - 1)):
            if mm < r:
                continue
            lengths = np.ones(r, np.int64)
            lengths[r // 2] = mm - (r - 1)
            assert lengths.max() <= 256
            data = np.concatenate([runs(rows, lengths).reshape(-1), rnd(tail, r)])
            (s,) = check_case(eng, w, 65536, data)
            assert mode_of(s) == (0 if M.runs_size(data.size, w, r, 1) < 4 + data.size else 1)
            seen.add(mode_of(s))
    assert seen == {0, 1}
    m, r = {1: (4, 1), 2: (4, 2), 4: (3, 2), 8: (7, 6), 16: (15, 14)}[w]  # the tie: stored
    assert M.runs_size(m * w, w, r, 1) == 4 + m * w
    lengths = np.ones(r, np.int64)
    lengths[0] = m - (r - 1)
    (s,) = check_case(eng, w, 65536, runs(rows, lengths).reshape(-1))
    assert mode_of(s) == 1


def hard_values(w):
    """pools of neighbouring values a lazy compare takes for equal -> [(name, rows d x w)]"""
    U = {4: "<u4", 8: "<u8"}
    out = []
    top = np.zeros((256, w), np.uint8)
    top[:, :w - 1] = rnd(w - 1, 1)
    top[:, w - 1] = np.arange(256)
    out.append(("top byte only", top))
    if w > 1:
        low = np.zeros((256, w), np.uint8)
        low[:, 1:] = rnd(w - 1, 2)
        low[:, 0] = np.arange(256)
        out.append(("lowest byte only", low))
    if w == 16:
        for name, sl in (("upper 8 bytes only", slice(8, 16)), ("lower 8 bytes only", slice(0, 8))):
            rows = np.tile(rnd(16, 3), (250, 1))
            rows[:, sl] = rnd(250 * 8, 4).reshape(250, 8)
            rows[:, sl.start] = np.arange(250)
            out.append((name, rows))
    if w in U:
        bits = 8 * w
        sign, quiet = 1 << (bits - 1), (0xFF << 23 | 1 << 22) if w == 4 else (0x7FF << 52 | 1 << 51)
        pats = [0, sign, quiet, quiet | 1, quiet | 2, quiet | sign, quiet ^ (1 << (bits - 10)) | 1]
        out.append(("zeros and NaNs", np.array(pats, U[w]).view(np.uint8).reshape(len(pats), w)))
    return out


@pytest.mark.parametrize("w", M.WIDTHS)
def test_values_that_punish_a_lazy_compare(eng, w):
    for name, rows in hard_values(w):
        assert np.unique(rows, axis=0).shape[0] == rows.shape[0], name
        for seg in (65536, 999):
            rng = np.random.default_rng(seg)
            lengths = geometric(rng, (2 * seg + 5) // w, 9)
            data = runs(rows, lengths).reshape(-1)[:2 * seg + 5]
            streams = check_case(eng, w, seg, data)
            assert seg == 999 or mode_of(streams[0]) == 0, name
    # (a, b, a, b, ...): one run of 8-byte elements, no run at all of 4-byte ones
    ab = np.tile(np.concatenate([rnd(4, 1), rnd(4, 2)]), 512)
    (s,) = check_case(eng, w, 4096, ab)
    assert mode_of(s) == (0 if w >= 8 else 1)
    # a buffer of one repeated byte is one run at every width
    (s, t) = check_case(eng, w, 4096, np.full(4096 + 1000, 0x5C, np.uint8))
    assert mode_of(s) == 0 and s[4] == 0 and s[5] == 0 and mode_of(t) == 0 and t[4] == 0


def test_empty_input_launches_nothing(eng):
    import bitar_amd as B
    buf = Buffers(1, 4352, 4096)
    src = torch.zeros(PAD, dtype=torch.uint8, device="cuda")
    for w in M.WIDTHS:
        eng.compress_into(B.codec_runpack(w), src, 4096, buf.slab_ptr, 4352, buf.sizes_ptr, n=0)
        eng.decompress_slab_into(B.codec_runpack(w), buf.slab_ptr, 4352, buf.sizes_ptr, 0, 4096,
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
    codec = B.codec_runpack(w)
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
    """runs streams with bl = 1, with bl = 2 and of one run, a runs stream no encoder writes
    (r = m - 1, larger than the stored form) and a stored one, each of a segment that ends
    inside a chunk and has a tail where w allows one"""
    L = seg - 5 * w - min(3, w - 1)
    m = L // w
    rows = pool(251, w, seg + w)
    short = np.tile([1, 40, 7, 200, 256, 3, 63, 64, 65], m // 699 + 1)
    long_ = np.tile([300, 1, 257, 64, 1000, 2], m // 1624 + 1)
    out = []
    for form, bl, body in ((0, 1, runs(rows, short)[:m]),
                           (0, 1 if m <= 256 else 2, runs(rows, long_)[:m]),
                           (0, 1 if m <= 256 else 2, runs(rows[3:4], [m])),
                           (1, 0, rnd(m * w, seg).reshape(m, w))):
        data = np.concatenate([body.reshape(-1), rnd(L - m * w, 5)])
        (s,) = M.encode(data, w, seg)
        assert (mode_of(s), s[1]) == (form, bl) and M.decode(s, seg) == data.tobytes()
        out.append(s)
    mm = 200  # r = m - 1 by hand: elements 100 and 101 are one run of two
    body = pool(mm, w, 9)
    body[101] = body[100]
    values = np.delete(body, 101, axis=0)
    lengths = np.zeros(mm - 1, np.uint8)
    lengths[100] = 1
    s = bytes([0x70 | M._LOG[w], 1, (mm * w - 1) & 255, (mm * w - 1) >> 8, mm - 2, 0]) + \
        values.tobytes() + lengths.tobytes()
    assert len(s) > 4 + mm * w and M.decode(s, seg) == body.tobytes()
    out.append(s)
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
    for bl in (0, 1, 2, 3, 255):
        poke(1, bl)
    out += [(s, len(s) + 1), (s, len(s) - 1), (s, 3), (s, 0)]
    if mode_of(s) == 0:
        L = 1 + s[2] + (s[3] << 8)
        m, r, bl = L // w, 1 + s[4] + (s[5] << 8), s[1]
        for rr in (r - 1, r + 1, m + 1):
            if 1 <= rr <= 65536:
                t = bytearray(s)
                t[4], t[5] = (rr - 1) & 255, (rr - 1) >> 8
                out.append((bytes(t), len(s)))
        at = 6 + r * w
        field = lambda k: int.from_bytes(s[at + k * bl:at + (k + 1) * bl], "little")  # noqa: E731

        def with_lengths(changes):
            t = bytearray(s)
            for k, v in changes:
                t[at + k * bl:at + (k + 1) * bl] = v.to_bytes(bl, "little")
            return bytes(t)

        top = (1 << 8 * bl) - 1
        for k in sorted({0, r // 2, r - 1, min(63, r - 1), min(64, r - 1)}):
            if field(k) < top:
                out.append((with_lengths([(k, field(k) + 1)]), len(s)))  # one too many
            if field(k) > 0:
                out.append((with_lengths([(k, field(k) - 1)]), len(s)))
            out.append((with_lengths([(k, top)]), len(s)))  # 0xFF or 0xFFFF
        up = next((k for k in range(r) if field(k) < top), None)
        down = next((k for k in range(r - 1, -1, -1) if field(k) > 0 and k != up), None)
        if up is not None and down is not None:  # the sum holds: other bytes, accepted
            out.append((with_lengths([(up, field(up) + 1), (down, field(down) - 1)]), len(s)))
        if r > 1:  # equal neighbouring values
            t = bytearray(s)
            t[6:6 + w] = s[6 + w:6 + 2 * w]
            out.append((bytes(t), len(s)))
    return out


@pytest.mark.parametrize("seg", (4096, 65536))
@pytest.mark.parametrize("w", M.WIDTHS)
def test_hostile_streams_get_the_model_verdict(eng, w, seg):
    """every mutant is accepted with the model's bytes or rejected with SEGMENT_ERROR and its
    whole output range left as it was, the sync reports IOError exactly when one was rejected,
    nothing outside the output is written and the engine works afterwards"""
    import bitar_amd as B
    codec = B.codec_runpack(w)
    for base in base_streams(w, seg):
        muts = mutants(base, w)
        nseg = len(muts)
        stride = (max(len(t) for t, _ in muts) + 1 + 255) & ~255
        slab = np.full((nseg, stride), 0x5A, np.uint8)
        for i, (t, _) in enumerate(muts):
            slab[i, :len(t)] = np.frombuffer(t, np.uint8)
        verdicts = [M.decode(slab[i, :size].tobytes(), seg) for i, (_, size) in enumerate(muts)]
        assert verdicts[0] is not None and any(v is None for v in verdicts)
        if mode_of(base) == 0 and base[4] | base[5]:  # (more than one run: other bytes too)
            assert len({v for v in verdicts if v is not None}) > 1
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
            n = 0 if v is None else len(v)  # a rejected segment writes nothing at all
            assert seg_out[:n].tobytes() == (v or b""), i
            assert np.all(seg_out[n:] == CANARY), i
        # the engine works afterwards, and the error was reported once
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, 1, seg, out.data_ptr() + PAD,
                                 prod.data_ptr() + 32, capacity=seg)
        eng.sync()
        assert out[PAD:PAD + len(verdicts[0])].cpu().numpy().tobytes() == verdicts[0]


def test_lengths_that_add_up_to_2_32_are_rejected(eng):
    """through the pointer-list decode: w = 1, r = 65536, every length field FF FF (196614
    bytes, sum 2^32) between two streams that decode"""
    import bitar_amd as B
    seg = 65536
    bad = bytes([0x70, 0x02, 0xFF, 0xFF, 0xFF, 0xFF]) + bytes(65536) + b"\xff" * (2 * 65536)
    ones = bad[:6 + 65536] + bytes(2 * 65536)  # every length 1: decodes to zeros
    good = M.encode_segment(np.full(seg, 7, np.uint8), 1)
    streams = [good, bad, ones]
    assert len(bad) == 196614 and M.decode(bad, seg) is None
    assert M.decode(ones, seg) == bytes(seg)
    room = (len(bad) + 32) & ~15
    packed = np.full(3 * room + 16, CANARY, np.uint8)
    ptrs = []
    for i, s in enumerate(streams):
        o = i * room + 2 * i + 1
        packed[o:o + len(s)] = np.frombuffer(s, np.uint8)
        ptrs.append(o)
    d_packed = dev(packed)
    d_ptrs = dev(np.array(ptrs, np.int64) + d_packed.data_ptr())
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    buf = Buffers(3, 65792, seg)
    eng.decompress_into(B.CODEC_RUNPACK8, d_ptrs, d_sizes, 3, seg, buf.out_ptr, buf.prod_ptr,
                        capacity=3 * seg)
    with pytest.raises(B.BitarError) as e:
        eng.sync()
    assert e.value.code == -5
    assert buf.prod.cpu().numpy()[8:11].tolist() == [seg, ERR, seg]
    out = buf.out.cpu().numpy()
    assert np.all(out[:PAD] == CANARY) and np.all(out[PAD + 3 * seg:] == CANARY)
    assert np.all(out[PAD:PAD + seg] == 7)
    assert np.all(out[PAD + seg:PAD + 2 * seg] == CANARY)
    assert np.all(out[PAD + 2 * seg:PAD + 3 * seg] == 0)
    eng.decompress_into(B.CODEC_RUNPACK8, d_ptrs, d_sizes, 1, seg, buf.out_ptr, buf.prod_ptr,
                        capacity=seg)
    eng.sync()


def test_every_id_decodes_every_width(eng):
    import bitar_amd as B
    seg = 4096
    datas = [column(8 * seg, w, 3 + w)[seg:2 * seg] for w in M.WIDTHS]  # (the exact runs)
    streams = [M.encode(d, w, seg)[0] for d, w in zip(datas, M.WIDTHS)]
    assert all(mode_of(s) == 0 for s in streams)
    stride = B.slot_size(B.CODEC_RUNPACK8, seg)
    slab = np.zeros((5, stride), np.uint8)
    for i, s in enumerate(streams):
        slab[i, :len(s)] = np.frombuffer(s, np.uint8)
    d_slab = dev(slab.reshape(-1))
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    for w in M.WIDTHS:
        buf = Buffers(5, stride, seg)
        eng.decompress_slab_into(B.codec_runpack(w), d_slab, stride, d_sizes, 5, seg, buf.out_ptr,
                                 buf.prod_ptr, capacity=5 * seg)
        eng.sync()
        buf.check_output(np.concatenate(datas))


def test_compress_bits_refuses_runpack(eng):
    import bitar_amd as B
    src = dev(column(8192, 4, 1))
    buf = Buffers(2, 4352, 4096)
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    for w in M.WIDTHS:
        with pytest.raises(B.BitarError) as e:
            eng.compress_bits_into(B.codec_runpack(w), src, 4096, buf.slab_ptr, 4352,
                                   buf.sizes_ptr, bits)
        assert e.value.code == -4
    eng.sync()
    assert bool((buf.slab == CANARY).all())
