"""GPU tests of the CASCADE codec (csrc/cascade.hip) through the C ABI: the slots and sizes of a
compress equal the numpy model's streams (cascade_model.py) byte for byte, the decoder returns
the input, and on mutated streams its verdict is the model's, with canaries around every buffer
a call writes.

Shapes: segments of 65536 (16-B aligned everywhere), 59460 (elements straddle segment starts),
4096, 1000 / 999 (odd bases: every element unaligned), 72 and 7 (shorter than a step, shorter
than an element).  The encoder plans its runs in INTPACK blocks of 256 and miniblocks of 64 and
scans 1024 / w elements a step; the decoder fills its rings 64 runs at a time and expands windows
of 1024 / w elements: run counts and run lengths on either side of each of those numbers, and run
values that send the values sub-stream into each of INTPACK's three modes."""
import numpy as np
import pytest

import cascade_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEGS = (65536, 59460, 4096, 1000, 999, 72, 7)
CANARY = 0xA5
CANARY32 = np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]
PAD = 256
ERR = np.array([0xFFFFFFFF], np.uint32).view(np.int32)[0]
U = {1: "<u1", 2: "<u2", 4: "<u4", 8: "<u8"}


@pytest.fixture(scope="module")
def eng():
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0, num_streams=2)
    yield e
    e.close()


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def mode_of(s):
    return s[0] >> 3 & 1


def sub_modes(s):
    """(mode of the values sub-stream, mode of the lengths sub-stream) of a cascade stream"""
    vsize = 1 + s[6] + (s[7] << 8)
    return s[8] >> 2 & 3, s[8 + vsize] >> 2 & 3


def runs_of(s):
    return 1 + s[4] + (s[5] << 8)


def geometric(rng, m, mean):
    out = rng.geometric(1.0 / mean, m // mean + 64)
    while out.sum() < m:
        out = np.append(out, rng.geometric(1.0 / mean, 256))
    return out


def run_values(kind, r, w, seed):
    """r run values of width w, neighbours different -> (r,) unsigned"""
    rng = np.random.default_rng(seed)
    top = 1 << (8 * w)
    if kind == "sorted":  # delta wins
        v = (top // 3 + np.cumsum(rng.integers(1, 4, r).astype(object))) % top
    elif kind == "small":  # plain wins: a small range, neighbours apart by 1..3 mod 7
        v = (np.cumsum(rng.integers(1, 4, r)) % 7).astype(object) + (top >> 2)
    elif kind == "random":  # nothing to pack: the stored sub-stream (w >= 2)
        v = (rng.integers(0, top >> 1, r, dtype=np.uint64) * 2 + (np.arange(r, dtype=np.uint64) & 1)).astype(object)
    elif kind == "decreasing":  # falls through 0: the deltas are negative and the values wrap
        v = (5 * (r // 2) - 5 * np.arange(r).astype(object)) % top
        if w == 1:
            v = (3 * (r // 2) - 3 * np.arange(r).astype(object)) % top
    elif kind == "constant":  # a constant step: delta with every width 0
        v = (top // 5 + 7 * np.arange(r).astype(object)) % top
    else:
        raise KeyError(kind)
    return np.array([int(x) for x in v], dtype=np.uint64).astype(U[w])


def expand(values, lengths, w):
    """run k: values[k] (cyclically), lengths[k] times -> bytes"""
    lengths = np.asarray(lengths)
    v = values[np.arange(lengths.size) % values.size]
    return np.repeat(v, lengths).astype(U[w]).view(np.uint8)


def column(n, w, seed):
    """n bytes in eight stretches: one value throughout; sorted run values in runs of exactly
    63, 64, 65, 256 and 257 with runs of 1 between them; a small range in geometric runs of mean
    3; sorted values in runs of mean 300; decreasing values in runs of mean 20; random values in
    runs of mean 20; and random bytes (two).  A stretch is n // 8 bytes, so runs cross rows of 64
    elements and, where the segment is no multiple of the pattern, segment borders"""
    rng = np.random.default_rng(seed)
    m = n // w + 1
    q = m // 8
    parts = [expand(run_values("sorted", 1, w, seed), [q], w)]
    cycle = np.array([63, 1, 64, 1, 1, 65, 256, 1, 257, 2, 300, 1, 1, 1])
    parts.append(expand(run_values("sorted", q, w, seed + 1), np.tile(cycle, q // cycle.sum() + 1), w)[:q * w])
    parts.append(expand(run_values("small", q, w, seed + 2), geometric(rng, q, 3), w)[:q * w])
    parts.append(expand(run_values("sorted", q, w, seed + 3), geometric(rng, q, 300), w)[:q * w])
    parts.append(expand(run_values("decreasing", q, w, seed + 4), geometric(rng, q, 20), w)[:q * w])
    parts.append(expand(run_values("random", q, w, seed + 5), geometric(rng, q, 20), w)[:q * w])
    out = np.concatenate(parts)
    out = np.concatenate([out, rnd(max(n - out.size, 0), seed + 6)])[:n]
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
    codec = B.codec_cascade(w)
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
    tails = (0, 256 * w + 3) if seg > 4096 else \
        sorted({0, 1, w - 1, w, 63 * w, 64 * w, 64 * w + 1, 256 * w + 3})
    cases = [column(8 * seg + r, w, seg * 31 + r + w) for r in tails]
    # the model first: the segments take both forms and, where a segment has room, the values
    # take each of INTPACK's modes
    streams = [s for c in cases for s in M.encode(c, w, seg)]
    if seg >= 1000:
        assert {mode_of(s) for s in streams} == {0, 1}
        assert {0, 1} <= {sub_modes(s)[0] for s in streams if mode_of(s) == 0}
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


KINDS = ("sorted", "small", "random", "decreasing", "constant")
# the mode of the values sub-stream that a kind is there for (None: whatever is smallest)
WANT_MODE = {"sorted": 1, "small": 0, "random": 2, "decreasing": 1, "constant": 1}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_run_counts_and_value_kinds(eng, w, kind):
    """r = 1, 63, 64, 65 (a miniblock), 255, 256, 257 (a block), 1023, 1024, 1025 runs in a
    segment, the last run being the segment's final element alone or ending on it, for run
    values of every kind; in full segments and in ones that end w - 1 bytes into an element"""
    seg = 65536
    m = seg // w
    rng = np.random.default_rng(w)
    segs, want_r = [], []
    for r in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        last = m if r == 1 else 1 + r % 2
        values = run_values(kind, r, w, r)
        segs.append(expand(values, partition(rng, m, r, last), w))
        want_r.append(r)
    streams = check_case(eng, w, seg, np.concatenate(segs))
    for r, s in zip(want_r, streams):
        assert mode_of(s) == 0 and runs_of(s) == r
        if r >= 255 and WANT_MODE[kind] is not None and not (kind == "random" and w == 1):
            assert sub_modes(s)[0] == WANT_MODE[kind], (r, kind)
        if kind == "constant" and r > 2:  # header, element 0, widths and references: no payload
            nmb = (r + 63) // 64
            assert 1 + s[6] + (s[7] << 8) == 4 + w + nmb + (nmb + 3) // 4 * w
    seg2 = seg - 59 * w + (w - 1)
    cut = [np.concatenate([s[:seg2 - (w - 1)], rnd(w - 1, 1)]) for s in segs]
    check_case(eng, w, seg2, np.concatenate(cut))


def test_the_largest_run_count(eng):
    """r = 32768 is a cascade form (w = 1: pairs of bytes; w = 2: every element its own run, in
    sorted order); one more run, or alternating bytes, is stored"""
    pairs = np.repeat(np.arange(32768) % 251, 2).astype(np.uint8)
    (s,) = check_case(eng, 1, 65536, pairs)
    assert mode_of(s) == 0 and runs_of(s) == 32768
    alt = (np.arange(32768) & 1).astype(np.uint8)  # L = 32768 alternating bytes: r = m = 32768
    (s,) = check_case(eng, 1, 32768, alt)
    assert mode_of(s) == 0 and runs_of(s) == 32768
    alt = (np.arange(65536) & 1).astype(np.uint8)  # r = 65536
    (s,) = check_case(eng, 1, 65536, alt)
    assert mode_of(s) == 1
    more = pairs.copy()
    more[1] = 77  # 32769 runs
    (s,) = check_case(eng, 1, 65536, more)
    assert mode_of(s) == 1
    ramp = np.arange(32768).astype("<u2").view(np.uint8)
    (s,) = check_case(eng, 2, 65536, ramp)
    assert mode_of(s) == 0 and runs_of(s) == 32768


@pytest.mark.parametrize("w", M.WIDTHS)
def test_run_lengths_at_the_window_border(eng, w):
    """runs of 1, 256, 257 and of one decoder window (1024 / w elements) and one less and more,
    each length throughout a segment and all of them mixed; and one run of the whole segment"""
    seg = 65536
    m = seg // w
    win = 1024 // w
    lens = (1, 256, 257, win - 1, win, win + 1)
    segs = []
    for n in lens:
        if n == 1 and w == 1:
            n = 2  # (65536 runs of single bytes are stored: pairs)
        r = -(-m // n)
        segs.append(expand(run_values("sorted", r, w, n), np.full(r, n), w)[:seg])
    r = m // 300
    mixed = np.tile(np.array(lens), r // len(lens) + 1)
    segs.append(expand(run_values("small", mixed.size, w, 5), mixed, w)[:seg])
    segs.append(expand(run_values("sorted", 1, w, 6), [m], w))
    segs = [np.concatenate([s, expand(run_values("sorted", 1, w, 7), [m], w)])[:seg] for s in segs]
    streams = check_case(eng, w, seg, np.concatenate(segs))
    assert all(mode_of(s) == 0 for s in streams) and runs_of(streams[-1]) == 1
    # the same at an odd output and input base: segments of 999 and 59460 bytes
    check_case(eng, w, 59460, np.concatenate(segs), in_off=3)


def test_mixed_segments_in_one_call(eng):
    """cascade, stored, cascade, stored and a short last segment without and with a tail, in one
    call"""
    seg = 4096
    for w in M.WIDTHS:
        m = seg // w
        a = expand(run_values("sorted", 100, w, 1), geometric(np.random.default_rng(1), m, 9), w)[:seg]
        b = rnd(seg, 2)
        c = expand(run_values("small", 200, w, 3), geometric(np.random.default_rng(2), m, 5), w)[:seg]
        for tail in (0, w - 1):
            data = np.concatenate([a, b, c, b, c[:300 * w], rnd(tail, 4)])
            streams = check_case(eng, w, seg, data)
            assert [mode_of(s) for s in streams] == [0, 1, 0, 1, 0]


def test_empty_input_launches_nothing(eng):
    import bitar_amd as B
    buf = Buffers(1, 4352, 4096)
    src = torch.zeros(PAD, dtype=torch.uint8, device="cuda")
    for w in M.WIDTHS:
        eng.compress_into(B.codec_cascade(w), src, 4096, buf.slab_ptr, 4352, buf.sizes_ptr, n=0)
        eng.decompress_slab_into(B.codec_cascade(w), buf.slab_ptr, 4352, buf.sizes_ptr, 0, 4096,
                                 buf.out_ptr, buf.prod_ptr, capacity=0)
    eng.sync()
    for t in (buf.slab, buf.out):
        assert bool((t == CANARY).all())
    for t in (buf.sizes, buf.prod):
        assert bool((t == int(CANARY32)).all())


def test_every_id_decodes_every_width(eng):
    import bitar_amd as B
    seg = 4096
    datas = [column(8 * seg, w, 3 + w)[seg:2 * seg] for w in M.WIDTHS]  # (the exact runs)
    streams = [M.encode(d, w, seg)[0] for d, w in zip(datas, M.WIDTHS)]
    assert all(mode_of(s) == 0 for s in streams)
    stride = B.slot_size(B.CODEC_CASCADE8, seg)
    slab = np.zeros((4, stride), np.uint8)
    for i, s in enumerate(streams):
        slab[i, :len(s)] = np.frombuffer(s, np.uint8)
    d_slab = dev(slab.reshape(-1))
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    for w in M.WIDTHS:
        buf = Buffers(4, stride, seg)
        eng.decompress_slab_into(B.codec_cascade(w), d_slab, stride, d_sizes, 4, seg, buf.out_ptr,
                                 buf.prod_ptr, capacity=4 * seg)
        eng.sync()
        buf.check_output(np.concatenate(datas))


def test_pointer_list_at_odd_addresses(eng):
    """bitar_hip_decompress with the streams at odd addresses: every load of both sub-streams
    is unaligned"""
    import bitar_amd as B
    seg = 59460
    for w in M.WIDTHS:
        data = column(3 * seg + 64 * w + 1, w, 77 + w)
        streams = M.encode(data, w, seg)
        nseg = len(streams)
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
        buf = Buffers(nseg, B.slot_size(B.codec_cascade(w), seg), seg)
        eng.decompress_into(B.codec_cascade(w), d_ptrs, d_sizes, nseg, seg, buf.out_ptr,
                            buf.prod_ptr, capacity=nseg * seg)
        eng.sync()
        buf.check_output(data)


# ---- hostile streams ----------------------------------------------------------------------------

def base_streams(w, seg):
    """cascade streams whose values are delta-packed, plain-packed and stored, one of one run,
    a cascade stream no encoder writes (sub-streams in the stored mode, larger than 4 + L) and a
    stored one, each of a segment that ends inside a chunk and has a tail where w allows one"""
    L = seg - 5 * w - min(3, w - 1)
    m = L // w
    rng = np.random.default_rng(seg + w)
    out = []
    for kind, mean in (("sorted", 9), ("small", 5), ("random", 12), ("sorted", m)):
        lengths = geometric(rng, m, mean) if mean < m else np.array([m])
        body = expand(run_values(kind, lengths.size, w, 3), lengths, w)[:m * w]
        data = np.concatenate([body, rnd(L - m * w, 5)])
        (s,) = M.encode(data, w, seg)
        assert mode_of(s) == 0 and M.decode(s, seg) == data.tobytes()
        out.append(s)
    import intpack_model as IM
    mm = 40  # by hand: every element a run of one, both sub-streams stored
    body = expand(run_values("sorted", mm, w, 9), np.ones(mm, np.int64), w)
    vs = IM._header(2, w, mm * w) + body.tobytes()
    ls = IM._header(2, 2, mm * 2) + bytes(2 * mm)
    s = M.cascade_stream(mm * w, w, mm, vs, ls)
    assert len(s) > 4 + mm * w and M.decode(s, seg) == body.tobytes()
    out.append(s)
    data = rnd(L, seg)
    (s,) = M.encode(data, w, seg)
    assert mode_of(s) == 1
    out.append(s)
    return out


def mutants(s, w):
    """deterministic mutations of the stream s -> [(bytes, size given to the decoder)]"""
    out = [(s, len(s))]

    def poke(at, value, base=s):
        if at < len(base) and base[at] != value & 255:
            t = bytearray(base)
            t[at] = value & 255
            out.append((bytes(t), len(s)))

    for bit in range(8):  # the eight header bytes, bit by bit; then some whole values
        for at in range(8):
            poke(at, s[at] ^ (1 << bit))
    for at in range(8):
        for value in (0, 1, 0x7F, 0xFF, s[at] + 1, s[at] - 1):
            poke(at, value)
    for nib in range(16):  # the tag's nibble, its mode, its width
        poke(0, nib << 4 | s[0] & 15)
    poke(0, s[0] ^ 8)
    for lg in range(8):
        poke(0, s[0] & ~7 | lg)
    out += [(s, len(s) + 1), (s, len(s) - 1), (s, 7), (s, 3), (s, 0)]
    if mode_of(s) == 1:
        return out
    L = 1 + s[2] + (s[3] << 8)
    m, r = L // w, runs_of(s)
    vsize = 1 + s[6] + (s[7] << 8)

    def le16(at, v):
        if 0 <= v <= 65535:
            t = bytearray(s)
            t[at], t[at + 1] = v & 255, v >> 8
            out.append((bytes(t), len(s)))

    for rr in (r - 1, r + 1, m + 1, 32769, 65536):  # r
        le16(4, rr - 1)
    for vv in (vsize - 1, vsize + 1, 4, 3, 1, len(s) - 8, len(s) - 11, len(s) - 12, 65536):  # vsize
        le16(6, vv - 1)
    import intpack_model as IM
    for at, ww in ((8, w), (8 + vsize, 2)):  # both sub-stream headers
        for k in range(4):
            for bit in range(8):
                poke(at + k, s[at + k] ^ (1 << bit))
        mode = s[at] >> 2 & 3
        if mode != 2:  # a width byte above 8 w, and one changed within range (the size is off)
            wid_at = at + 4 + (ww if mode == 1 else 0)
            nmb = (r + 63) // 64
            for k in sorted({0, nmb // 2, nmb - 1}):
                poke(wid_at + k, 8 * ww + 1)
                poke(wid_at + k, 0xFF)
                poke(wid_at + k, s[wid_at + k] + 1)
    if r > 1:  # the values' last payload bytes: other values, accepted
        for at in (8 + vsize - 1, 8 + vsize - 2, 8 + vsize - 1 - w):
            poke(at, s[at] ^ 1)
            poke(at, s[at] ^ 0x80)
    if s[8] >> 2 & 3 == 2 and r > 1:  # stored values: equal neighbours
        t = bytearray(s)
        t[12:12 + w] = s[12 + w:12 + 2 * w]
        out.append((bytes(t), len(s)))
    # a length changed so the sum is m + 1 and m - 1: the lengths re-encoded by the model
    tail = L - m * w
    lengths = np.frombuffer(IM.decode(s[8 + vsize:len(s) - tail], 2 * r), "<u2").astype(np.int64)
    for k, d in ((0, 1), (r // 2, 1), (r - 1, 1), (0, -1), (r // 2, -1), (r - 1, -1)):
        if 0 <= lengths[k] + d <= 65535:
            ch = lengths.copy()
            ch[k] += d
            ls = IM.encode_segment(ch.astype("<u2").view(np.uint8), 2)
            t = s[:8 + vsize] + ls + s[len(s) - tail:]
            out.append((t, len(t)))
    if r > 1:  # one up, one down: the sum holds, other bytes, accepted
        up, down = 0, next((k for k in range(r - 1, 0, -1) if lengths[k] > 0), None)
        if down is not None and lengths[up] < 65535:
            ch = lengths.copy()
            ch[up] += 1
            ch[down] -= 1
            ls = IM.encode_segment(ch.astype("<u2").view(np.uint8), 2)
            t = s[:8 + vsize] + ls + s[len(s) - tail:]
            out.append((t, len(t)))
    return out


@pytest.mark.parametrize("seg", (4096, 65536))
@pytest.mark.parametrize("w", M.WIDTHS)
def test_hostile_streams_get_the_model_verdict(eng, w, seg):
    """every mutant is accepted with the model's bytes or rejected with SEGMENT_ERROR and its
    whole output range left as it was, the sync of its queue pair reports IOError exactly once, a
    good stream decodes on the other queue pair at the same time, nothing outside the output is
    written and the engine works afterwards"""
    import bitar_amd as B
    codec = B.codec_cascade(w)
    q0, q1 = eng.queue_pair_stream(0), eng.queue_pair_stream(1)
    for base in base_streams(w, seg):
        muts = mutants(base, w)
        nseg = len(muts)
        stride = (max(len(t) for t, _ in muts) + 1 + 255) & ~255
        slab = np.full((nseg, stride), 0x5A, np.uint8)
        for i, (t, _) in enumerate(muts):
            slab[i, :len(t)] = np.frombuffer(t, np.uint8)
        verdicts = [M.decode(slab[i, :size].tobytes(), seg) for i, (_, size) in enumerate(muts)]
        assert verdicts[0] is not None and any(v is None for v in verdicts)
        if mode_of(base) == 0 and runs_of(base) > 1:  # (more than one run: other bytes too)
            assert len({v for v in verdicts if v is not None}) > 1
        d_slab = dev(slab.reshape(-1))
        d_sizes = dev(np.array([size for _, size in muts], np.int32))
        out = torch.full((PAD + nseg * seg + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        prod = torch.full((nseg + 16,), int(CANARY32), dtype=torch.int32, device="cuda")
        g_out = torch.full((PAD + seg + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        g_prod = torch.full((1 + 16,), int(CANARY32), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # (the buffers were filled on torch's stream)
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, nseg, seg, out.data_ptr() + PAD,
                                 prod.data_ptr() + 32, capacity=nseg * seg, stream=q0)
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, 1, seg, g_out.data_ptr() + PAD,
                                 g_prod.data_ptr() + 32, capacity=seg, stream=q1)
        eng.sync(stream=q1)  # the good stream on the other queue pair: nothing to report
        with pytest.raises(B.BitarError) as e:
            eng.sync(stream=q0)
        assert e.value.code == -5
        eng.sync(stream=q0)  # reported once
        g = g_out.cpu().numpy()
        assert g_prod.cpu().numpy()[8] == len(verdicts[0])
        assert g[PAD:PAD + len(verdicts[0])].tobytes() == verdicts[0]
        assert np.all(g[:PAD] == CANARY) and np.all(g[PAD + len(verdicts[0]):] == CANARY)
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
        # the engine works afterwards
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, 1, seg, out.data_ptr() + PAD,
                                 prod.data_ptr() + 32, capacity=seg)
        eng.sync()
        assert out[PAD:PAD + len(verdicts[0])].cpu().numpy().tobytes() == verdicts[0]


def test_compress_bits_refuses_cascade(eng):
    import bitar_amd as B
    src = dev(column(8192, 4, 1))
    buf = Buffers(2, 4352, 4096)
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    for w in M.WIDTHS:
        with pytest.raises(B.BitarError) as e:
            eng.compress_bits_into(B.codec_cascade(w), src, 4096, buf.slab_ptr, 4352,
                                   buf.sizes_ptr, bits)
        assert e.value.code == -4
    eng.sync()
    assert bool((buf.slab == CANARY).all())
