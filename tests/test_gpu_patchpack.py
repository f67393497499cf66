"""GPU tests of the PATCHPACK codec (csrc/patchpack.hip) through the C ABI: the slots and sizes of
a compress equal the numpy model's streams (patchpack_model.py) byte for byte, the decoder returns
the input, and on mutated streams its verdict is the model's, with canaries around every buffer
a call writes.

Shapes: segments of 65536 (16-B aligned everywhere), 59460 (elements straddle segment starts),
4096, 1000 / 999 (odd bases: every element unaligned), 72 and 7 (a miniblock and a bit, shorter
than an element at w = 8).  The encoder plans blocks of 256 elements and miniblocks of 64 and
ranks a miniblock's exceptions across its lanes; the decoder checks positions 64 at a time and
merges them from a bitmap: outliers in lanes 0 and 63, at the last element of a partial miniblock
and at elements 0 and 1, exception counts on either side of 64 and above 1024, and columns that
send a segment into each mode."""
import numpy as np
import pytest

import patchpack_cases as C
import patchpack_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEGS = (65536, 59460, 4096, 1000, 999, 72, 7)
CANARY = 0xA5
CANARY32 = np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]
PAD = 256
ERR = np.array([0xFFFFFFFF], np.uint32).view(np.int32)[0]
U = {1: "<u1", 2: "<u2", 4: "<u4", 8: "<u8"}
KINDS = ("high", "gaps", "low", "noise")
WANT_MODE = {"high": 0, "gaps": 1, "low": 3, "noise": 2}


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
    return s[0] >> 2 & 3


def nx_of(s):
    return s[4] | s[5] << 8 if mode_of(s) != 2 else 0


def elements(kind, m, w, where, seed):
    """m elements of width w with outliers at the indices `where` -> (m,) unsigned
    high: 0..15, outliers near the largest signed value (plain).  gaps: sorted, steps 1..7, a
    long step before an outlier (delta).  low: a base + 0..15, outliers 0..3 (complement)"""
    rng = np.random.default_rng(seed)
    where = np.asarray(where, np.int64)
    top = 1 << (8 * w)
    if kind == "high":
        v = rng.integers(0, 16, m).astype(np.uint64)
        v[where] = np.uint64((top >> 1) - 1) - rng.integers(0, 4, where.size).astype(np.uint64)
    elif kind == "gaps":
        step = rng.integers(1, 8, m).astype(np.uint64)
        step[where] = np.uint64(top >> 2) + rng.integers(0, 4, where.size).astype(np.uint64)
        v = np.cumsum(step, dtype=np.uint64) + np.uint64(top // 3)
    elif kind == "low":
        v = rng.integers(0, 16, m).astype(np.uint64) + np.uint64(top >> 2)
        v[where] = rng.integers(0, 4, where.size).astype(np.uint64)
    else:
        return rnd(m * w, seed).view(U[w])
    return v.astype(U[w])  # (wraps mod 2^(8w))


def outlier_places(m, counts, seed):
    """counts[k] outliers in miniblock k: the first in lane 0, the second in the miniblock's last
    lane, the others anywhere between"""
    rng = np.random.default_rng(seed)
    out = []
    for k, c in enumerate(counts):
        lo, hi = 64 * k, min(64 * k + 64, m)
        if lo >= m or c == 0:
            continue
        lanes = [lo, hi - 1][:c]
        if c > 2 and hi - lo > 2:
            lanes += list(rng.choice(np.arange(lo + 1, hi - 1), min(c - 2, hi - lo - 2), replace=False))
        out += lanes
    return np.unique(np.array(out, np.int64))


def segment(kind, L, w, seed, counts=(0, 1, 2, 1, 0, 3, 1, 1)):
    """L bytes: elements of the given kind with counts[k % len] outliers in miniblock k, and the
    bytes of a cut element behind them"""
    m = L // w
    nmb = (m + 63) // 64
    per = [counts[k % len(counts)] for k in range(nmb)]
    v = elements(kind, m + 1, w, outlier_places(m, per, seed), seed)
    return v.view(np.uint8)[:L].copy()


def column(nseg, seg, w, seed, extra=0):
    """nseg segments of seg bytes, the kinds in turn, and `extra` more bytes"""
    parts = [segment(KINDS[i % 4], seg, w, seed + i) for i in range(nseg)]
    if extra:
        parts.append(segment("high", extra, w, seed + nseg))
    return np.concatenate(parts)


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
    """compress and decompress `data` -> the model's streams, which the slots equal; the segments
    are decoded under every PATCHPACK id"""
    import bitar_amd as B
    codec = B.codec_patchpack(w)
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
    for other in M.WIDTHS:
        if other != w:
            buf.out.fill_(CANARY)
            buf.prod.fill_(int(CANARY32))
            eng.decompress_slab_into(B.codec_patchpack(other), buf.slab_ptr, stride, buf.sizes_ptr,
                                     nseg, seg, buf.out_ptr, buf.prod_ptr, capacity=nseg * seg)
            eng.sync()
            buf.check_output(data)
    return streams


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_exact_bytes_and_round_trip(eng, w, seg):
    tails = (0, 256 * w + 3) if seg > 4096 else \
        sorted({0, 1, w - 1, w, 63 * w, 64 * w, 64 * w + 1, 256 * w + 3})
    cases = [column(8, seg, w, seg * 31 + r + w, extra=r) for r in tails]
    # the model first: where a segment has room, every mode is chosen, asserted from the tags
    streams = [s for c in cases for s in M.encode(c, w, seg)]
    if seg >= 999:
        assert {mode_of(s) for s in streams} == {0, 1, 2, 3}
        assert {mode_of(s) for s in streams if nx_of(s) > 0} == {0, 1, 3}
    for c in cases:
        check_case(eng, w, seg, c)
    if seg == 72:
        for n in range(1, w):  # shorter than an element
            check_case(eng, w, seg, rnd(n, n))


@pytest.mark.parametrize("w", M.WIDTHS)
def test_input_at_every_alignment(eng, w):
    for seg in (59460, 4096):
        for in_off in (0, 1, 3, 4, 15):
            check_case(eng, w, seg, column(4, seg, w, in_off + w, extra=64 * w + 1), in_off=in_off)


@pytest.mark.parametrize("w", M.WIDTHS)
def test_the_case_columns(eng, w):
    """the columns of DESIGN.md 4.28's table, at their own width and at this one"""
    for name, cw, col in C.table_columns(n=2 * 65536, seed=2800 + w):
        for ww in {cw, w}:
            check_case(eng, ww, 65536, col)


@pytest.mark.parametrize("kind", KINDS[:3])
@pytest.mark.parametrize("w", M.WIDTHS)
def test_exception_counts_per_miniblock_and_segment(eng, w, kind):
    """0, 1 and 2 outliers in every miniblock (lanes 0 and 63 among them), as many in a row as
    the width rule lets through, and segments of exactly 63, 64 and 65 exceptions and one above
    1024: one position chunk of the decoder, one and a bit, and many"""
    seg = 65536
    m = seg // w
    nmb = m // 64
    segs = [segment(kind, seg, w, 1 + w, counts=(c,)) for c in (0, 1, 2, 5)]
    many = -(-1025 // nmb)  # outliers a miniblock for more than 1024 a segment
    segs.append(segment(kind, seg, w, 2 + w, counts=(many,)))
    # one outlier in each of the first `total` miniblocks (a gap before element 0 is none: x_0 is
    # x_1's copy, so a sorted column gets one miniblock more)
    lost = 1 if kind == "gaps" else 0
    for total in (63, 64, 65):
        counts = [1] * (total + lost) + [0] * (nmb - total - lost)
        segs.append(segment(kind, seg, w, 3 + w, counts=counts))
    streams = check_case(eng, w, seg, np.concatenate(segs))
    assert all(mode_of(s) == WANT_MODE[kind] for s in streams[1:])
    nxs = [nx_of(s) for s in streams]
    assert nxs[:3] == [0, nmb - lost, 2 * nmb - lost] and nxs[4] > 1024 and nxs[5:] == [63, 64, 65]
    # the same cut so that the last miniblock is partial and its last element an outlier
    seg2 = seg - 59 * w + (w - 1)
    cut = [segment(kind, seg2, w, 4 + w, counts=(c,)) for c in (1, 2)]
    streams = check_case(eng, w, seg2, np.concatenate(cut))
    m2 = seg2 // w
    assert all(mode_of(s) == WANT_MODE[kind] for s in streams)
    s, tail = streams[1], seg2 - m2 * w  # (two outliers a miniblock: lane 0 and the last element)
    pos = np.frombuffer(s[len(s) - tail - nx_of(s) * (2 + w):len(s) - tail - nx_of(s) * w], "<u2")
    assert pos[-1] == m2 - 1 and m2 % 64 not in (0, 1)


@pytest.mark.parametrize("w", M.WIDTHS)
def test_delta_exceptions_at_elements_0_and_1(eng, w):
    """a gap before element 1 of a sorted column: x_1 and its copy x_0 are both exceptions"""
    for seg in (65536, 999):
        m = seg // w
        data = np.concatenate([elements("gaps", m + 1, w, where, 5).view(np.uint8)[:seg]
                               for where in ([1], [1, 2, 64], [2])])
        streams = check_case(eng, w, seg, data)
        for s, first in zip(streams, ([0, 1], [0, 1, 2], [2])):
            assert mode_of(s) == 1
            nx, tail = nx_of(s), seg - m * w
            pos = np.frombuffer(s[len(s) - tail - nx * (2 + w):len(s) - tail - nx * w], "<u2")
            assert pos[:len(first)].tolist() == first


def forced_streams(w, seg):
    """streams no encoder writes: 63 exceptions in every miniblock (width 0 forced on the
    complement mode, where one element per miniblock is the reference's), widths larger than
    needed with no exception, and each mode on a column that another mode suits"""
    L = seg - 5 * w - min(3, w - 1)
    m = L // w
    nmb = (m + 63) // 64
    v = np.random.default_rng(w).integers(1, 1 << 7, m + 1).astype(U[w])
    v[::64] = 0  # each miniblock's first element: the smallest
    data = v.view(np.uint8)[:L].copy()
    out = [(data, M.packed_stream(data, w, 0, np.zeros(nmb, np.uint8)))]
    assert nx_of(out[0][1]) == m - nmb
    out.append((data, M.packed_stream(data, w, 3, np.full(nmb, 8 * w, np.uint8))))
    for mode, kind in ((0, "gaps"), (1, "low"), (3, "high")):
        data = segment(kind, L, w, 7 + w)
        out.append((data, M.packed_stream(data, w, mode)))
    return out


@pytest.mark.parametrize("w", M.WIDTHS)
def test_streams_no_encoder_writes(eng, w):
    import bitar_amd as B
    for seg in (65536, 4096):
        cases = forced_streams(w, seg)
        stride = (max(len(s) for _, s in cases) + 255) & ~255  # (a packed form above 4 + L)
        slab = np.full((len(cases), stride), 0x5A, np.uint8)
        for i, (_, s) in enumerate(cases):
            assert M.decode(s, seg) == cases[i][0].tobytes()
            slab[i, :len(s)] = np.frombuffer(s, np.uint8)
        d_slab = dev(slab.reshape(-1))
        d_sizes = dev(np.array([len(s) for _, s in cases], np.int32))
        buf = Buffers(len(cases), stride, seg)
        eng.decompress_slab_into(B.codec_patchpack(w), d_slab, stride, d_sizes, len(cases), seg,
                                 buf.out_ptr, buf.prod_ptr, capacity=len(cases) * seg)
        eng.sync()
        prod = buf.prod.cpu().numpy()[8:8 + len(cases)]
        out = buf.out.cpu().numpy()
        assert np.all(out[:PAD] == CANARY) and np.all(out[PAD + len(cases) * seg:] == CANARY)
        for i, (data, _) in enumerate(cases):
            assert prod[i] == data.size
            got = out[PAD + i * seg:PAD + (i + 1) * seg]
            assert np.array_equal(got[:data.size], data) and np.all(got[data.size:] == CANARY)


def test_mixed_segments_in_one_call(eng):
    """plain, stored, delta, stored, complement and a short last segment without and with a tail,
    in one call"""
    seg = 4096
    for w in M.WIDTHS:
        a, c, e = (segment(k, seg, w, 3 + w) for k in ("high", "gaps", "low"))
        b = rnd(seg, 2)
        for tail in (0, w - 1):
            data = np.concatenate([a, b, c, b, e, a[:300 * w], rnd(tail, 4)])
            streams = check_case(eng, w, seg, data)
            assert [mode_of(s) for s in streams] == [0, 2, 1, 2, 3, 0]


def test_empty_input_launches_nothing(eng):
    import bitar_amd as B
    buf = Buffers(1, 4352, 4096)
    src = torch.zeros(PAD, dtype=torch.uint8, device="cuda")
    for w in M.WIDTHS:
        eng.compress_into(B.codec_patchpack(w), src, 4096, buf.slab_ptr, 4352, buf.sizes_ptr, n=0)
        eng.decompress_slab_into(B.codec_patchpack(w), buf.slab_ptr, 4352, buf.sizes_ptr, 0, 4096,
                                 buf.out_ptr, buf.prod_ptr, capacity=0)
    eng.sync()
    for t in (buf.slab, buf.out):
        assert bool((t == CANARY).all())
    for t in (buf.sizes, buf.prod):
        assert bool((t == int(CANARY32)).all())


def test_pointer_list_at_odd_addresses(eng):
    """bitar_hip_decompress with the streams at odd addresses: every load of the header arrays,
    the payload, the positions and the values is unaligned"""
    import bitar_amd as B
    seg = 59460
    for w in M.WIDTHS:
        data = column(4, seg, w, 77 + w, extra=64 * w + 1)
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
        buf = Buffers(nseg, B.slot_size(B.codec_patchpack(w), seg), seg)
        eng.decompress_into(B.codec_patchpack(w), d_ptrs, d_sizes, nseg, seg, buf.out_ptr,
                            buf.prod_ptr, capacity=nseg * seg)
        eng.sync()
        buf.check_output(data)


# ---- hostile streams ----------------------------------------------------------------------------

def base_streams(w, seg):
    """a stream of each packed mode with exceptions, one no encoder writes (63 exceptions a
    miniblock, larger than 4 + L) and a stored one, each of a segment that ends inside a
    miniblock and has a tail where w allows one"""
    L = seg - 5 * w - min(3, w - 1)
    out = []
    for kind in KINDS:
        (s,) = M.encode(segment(kind, L, w, seg + w), w, seg)
        assert mode_of(s) == WANT_MODE[kind]
        out.append(s)
    if seg <= 4096:
        out.append(forced_streams(w, seg)[0][1])
    return out


def mutants(s, w):
    """deterministic mutations of the stream s -> [(bytes, size given to the decoder)]"""
    out = [(s, len(s))]

    def poke(at, value, base=s):
        if 0 <= at < len(base) and base[at] != value & 255:
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
    for mode in range(4):
        poke(0, s[0] & ~12 | mode << 2)
    for lg in range(4):
        poke(0, s[0] & ~3 | lg)
    out += [(s, len(s) + 1), (s, len(s) - 1), (s, len(s) - 2 - w), (s, 7), (s, 5), (s, 3), (s, 0)]
    out.append((s + b"\0" * (2 + w), len(s) + 2 + w))
    if mode_of(s) == 2:
        return out
    mode = mode_of(s)
    L = 1 + s[2] + (s[3] << 8)
    m, nx = L // w, nx_of(s)
    nmb = (m + 63) // 64
    tail = L - m * w

    def le16(at, v, base=s, size=None):
        if 0 <= v <= 65535:
            t = bytearray(base)
            t[at], t[at + 1] = v & 255, v >> 8
            out.append((bytes(t), len(base) if size is None else size))

    for n in (nx - 1, nx + 1, 0, m, m + 1, 65535):  # nx alone: the size no longer fits
        le16(4, n)
    grown = s[:len(s) - tail] + bytes(2 + w) + s[len(s) - tail:]  # nx + 1 with room for it
    le16(4, nx + 1, grown)
    wid_at = 6 + (w if mode == 1 else 0)
    for k in sorted({0, nmb // 2, nmb - 1}):  # a width above 8 w, and one changed within range
        poke(wid_at + k, 8 * w + 1)
        poke(wid_at + k, 0xFF)
        poke(wid_at + k, s[wid_at + k] + 1)
        poke(wid_at + k, s[wid_at + k] - 1)
    pay_at = wid_at + nmb + (nmb + 3) // 4 * w
    pos_at = len(s) - tail - nx * (2 + w)
    for at in (wid_at - 1, pay_at - 1, pay_at, (pay_at + pos_at) // 2, pos_at - 1):
        poke(at, s[at] ^ 1)  # the base, a reference, payload bytes: other bytes, accepted
        poke(at, s[at] ^ 0x80)
    pos = np.frombuffer(s[pos_at:pos_at + 2 * nx], "<u2").astype(np.int64)

    def with_pos(p):
        out.append((s[:pos_at] + np.asarray(p).astype("<u2").tobytes() + s[pos_at + 2 * nx:], len(s)))

    for k in sorted({0, 1, 63, 64, nx // 2, nx - 1} & set(range(nx))):
        for v in (m, m + 1, 65535, pos[k - 1] if k else -1, pos[k - 1] - 1 if k else -1,
                  pos[k + 1] if k + 1 < nx else -1, pos[k] + 1, pos[k] - 1):
            if 0 <= v <= 65535 and v != pos[k]:
                p = pos.copy()
                p[k] = v
                with_pos(p)
    if nx > 2:
        p = pos.copy()
        p[[0, 1]] = p[[1, 0]]
        with_pos(p)
        with_pos(pos[::-1])
    val_at = pos_at + 2 * nx
    for at in (val_at, val_at + w - 1, val_at + nx * w - 1, val_at + (nx // 2) * w):
        poke(at, s[at] ^ 1)  # other values of exceptions: accepted
        poke(at, s[at] ^ 0x40)
    if tail:
        poke(len(s) - 1, s[-1] ^ 0xFF)
    # non-zero bits in the slot of an exception: ignored (the first exception of a miniblock of
    # width b > 0 has its top bit at bit (t + 1) * b - 1 of the miniblock's payload)
    widths = np.frombuffer(s[wid_at:wid_at + nmb], np.uint8).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(8 * widths)])
    done = 0
    for p in pos:
        k, t, b = int(p) // 64, int(p) % 64, int(widths[int(p) // 64])
        if b and done < 4:
            bit = (t + 1) * b - 1
            at = pay_at + int(offs[k]) + (bit >> 3)
            tt = bytearray(s)
            tt[at] |= 1 << (bit & 7)
            out.append((bytes(tt), len(s)))
            done += 1
    return out


def test_the_mutations_split_both_ways():
    """(no GPU needed, but this file's tests share the mutants:) at each width there are at least
    200 mutants, the model accepts a share and rejects a share, and among the accepted ones are
    streams that decode to other bytes and streams that decode to the same"""
    for w in M.WIDTHS:
        total = accepted = same = other = 0
        for base in base_streams(w, 4096):
            want = M.decode(base, 4096)
            verdicts = [M.decode(t[:size] if size <= len(t) else t + b"\x5a" * (size - len(t)),
                                 4096) for t, size in mutants(base, w)]
            total += len(verdicts)
            accepted += sum(v is not None for v in verdicts)
            same += sum(v == want for v in verdicts[1:])
            other += sum(v not in (None, want) for v in verdicts)
            if mode_of(base) != 2:
                assert sum(v is None for v in verdicts) >= 40
                assert sum(v not in (None, want) for v in verdicts) >= 8
        assert total >= 200 and accepted >= 50 and total - accepted >= 150, (w, total, accepted)
        assert same >= 4 and other >= 40, (w, same, other)


@pytest.mark.parametrize("seg", (4096, 65536))
@pytest.mark.parametrize("w", M.WIDTHS)
def test_hostile_streams_get_the_model_verdict(eng, w, seg):
    """every mutant is accepted with the model's bytes or rejected with SEGMENT_ERROR and its
    whole output range left as it was, the sync of its queue pair reports IOError exactly once, a
    good stream decodes on the other queue pair at the same time, nothing outside the output is
    written and the engine works afterwards"""
    import bitar_amd as B
    codec = B.codec_patchpack(w)
    q0, q1 = eng.queue_pair_stream(0), eng.queue_pair_stream(1)
    bases = base_streams(w, seg)
    if seg > 4096:
        bases = bases[1:3]  # (the model reads a 64 KiB stream in milliseconds, not less)
    count = 0
    for base in bases:
        muts = mutants(base, w)
        count += len(muts)
        nseg = len(muts)
        stride = (max(max(len(t), size) for t, size in muts) + 1 + 255) & ~255
        slab = np.full((nseg, stride), 0x5A, np.uint8)
        for i, (t, _) in enumerate(muts):
            slab[i, :len(t)] = np.frombuffer(t, np.uint8)
        verdicts = [M.decode(slab[i, :size].tobytes(), seg) for i, (_, size) in enumerate(muts)]
        assert verdicts[0] is not None and any(v is None for v in verdicts)
        if mode_of(base) != 2:
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
    assert count >= 200


def test_compress_bits_refuses_patchpack(eng):
    import bitar_amd as B
    src = dev(column(2, 4096, 4, 1))
    buf = Buffers(2, 4352, 4096)
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    for w in M.WIDTHS:
        with pytest.raises(B.BitarError) as e:
            eng.compress_bits_into(B.codec_patchpack(w), src, 4096, buf.slab_ptr, 4352,
                                   buf.sizes_ptr, bits)
        assert e.value.code == -4
    eng.sync()
    assert bool((buf.slab == CANARY).all())


def test_autopack_rejects_the_nibble(eng):
    """PATCHPACK is no candidate of AUTOPACK, whose decoder goes on rejecting tag nibble 9"""
    import bitar_amd as B
    seg = 4096
    (s,) = M.encode(segment("high", seg, 4, 9), 4, seg)
    stride = B.slot_size(B.CODEC_AUTOPACK32, seg)
    slab = np.zeros(stride, np.uint8)
    slab[:len(s)] = np.frombuffer(s, np.uint8)
    buf = Buffers(1, stride, seg)
    eng.decompress_slab_into(B.CODEC_AUTOPACK32, dev(slab), stride, dev(np.array([len(s)], np.int32)),
                             1, seg, buf.out_ptr, buf.prod_ptr, capacity=seg)
    with pytest.raises(B.BitarError) as e:
        eng.sync()
    assert e.value.code == -5
    assert buf.prod.cpu().numpy()[8] == ERR and bool((buf.out == CANARY).all())
