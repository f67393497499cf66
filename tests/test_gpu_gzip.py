"""GPU tests of the passes under a gzip member (RFC 1952), through the C ABI: exact bit
lengths from the two DEFLATE compressors (bitar_hip_compress_bits), the bit-granular join of
the segments' streams into ONE raw DEFLATE stream and its inverse (bitar_hip_deflate_join /
_split, csrc/deflate_join.hip), and the CRC-32 of a buffer from its segments' CRC-32s
(bitar_hip_crc32_combine).

The join is restated sequentially with Python integers (gzip_model.model_join); zlib is the
third-party decoder of every joined stream.

Shapes are the smallest at which each pass can go wrong.  The encoders store a segment only
when 5 * nblk + n < coded bytes + n / 16 (oracle BO_STORE_MARGIN), and the fixed code spends at
most 9 bits per byte, so no segment under 24 bytes is ever stored, while a 64-byte random
segment always is (stored 69 bytes < ceil((10 + 512) / 8) + 4 = 70).  Cases that need stored
segments among 13- or 16-byte coded ones therefore assemble their slab from two compress
calls of the same slot stride, one per segment size, with 64 random bytes for each stored
segment; the assertions on phases and block shapes fail (never skip) if the input stops
providing them.
"""
import zlib

import numpy as np
import pytest

from gzip_model import model_join

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEGMENT_ERROR = 0xFFFFFFFF
STORED = 1 << 23


@pytest.fixture(scope="module")
def eng():
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0)
    yield e
    e.close()


def codecs():
    import bitar_amd
    return {"fixed": bitar_amd.CODEC_DEFLATE, "dynamic": bitar_amd.CODEC_DEFLATE_DYNAMIC}


def up(a, dtype=np.uint8):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros(1, dtype)
    return torch.from_numpy(a.copy()).cuda()


def down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def text(n, seed=0):
    words = [b"segment", b"deflate", b"stream", b"block", b"gzip", b"member", b"the", b"of",
             b"header", b"index", b"join", b"split", b"wave", b"bits"]
    r = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        out += words[int(r.integers(len(words)))] + b" "
    return np.frombuffer(bytes(out[:n]), np.uint8)


# ---- building a slab ----------------------------------------------------------------------
class Slab:
    pass


def compress_parts(eng, codec, parts):
    """parts: [(uint8 array, seg)], each compressed by its own bitar_hip_compress_bits call;
    the slots are concatenated in order under one stride.  Also checks, per part, that a null
    `bits` gives exactly bitar_hip_compress's output."""
    import bitar_amd
    stride = max(bitar_amd.slot_size(codec, seg) for _, seg in parts)
    S = Slab()
    S.stride, S.slots, S.sizes, S.bits, S.plain = stride, [], [], [], []
    for data, seg in parts:
        n = data.size
        nseg = (n + seg - 1) // seg
        d = up(data)
        outs = []
        for mode in ("plain", "null", "bits"):
            slab = torch.full((nseg * stride,), 0xEE, dtype=torch.uint8, device="cuda")
            sizes = torch.full((nseg,), -2, dtype=torch.int32, device="cuda")
            bits = torch.full((nseg,), -2, dtype=torch.int32, device="cuda")
            if mode == "plain":
                eng.compress_into(codec, d, seg, slab, stride, sizes, n=n)
            else:
                eng.compress_bits_into(codec, d, seg, slab, stride, sizes,
                                       bits if mode == "bits" else None, n=n)
            eng.sync()
            outs.append((down(slab), down(sizes).astype(np.uint32), down(bits).astype(np.uint32)))
        (s0, z0, _), (s1, z1, b1), (s2, z2, b2) = outs
        assert np.array_equal(z0, z1) and np.array_equal(z0, z2)
        assert np.all(b1 == 0xFFFFFFFE), "a null bits pointer must store nothing"
        for i in range(nseg):
            a = s0[i * stride:i * stride + z0[i]]
            assert np.array_equal(a, s1[i * stride:i * stride + z0[i]]), (mode, i)
            assert np.array_equal(a, s2[i * stride:i * stride + z0[i]]), (mode, i)
            S.slots.append(a.tobytes())
            S.sizes.append(int(z0[i]))
            S.bits.append(int(b2[i]))
            S.plain.append(data[i * seg:(i + 1) * seg].tobytes())
    S.nseg = len(S.slots)
    host = np.zeros(S.nseg * stride, np.uint8)
    for i, s in enumerate(S.slots):
        host[i * stride:i * stride + len(s)] = np.frombuffer(s, np.uint8)
    S.d_slab = up(host)
    S.d_sizes = up(np.array(S.sizes, np.uint32).view(np.int32), np.int32)
    S.d_bits = up(np.array(S.bits, np.uint32).view(np.int32), np.int32)
    S.stored = [(s[0] & 6) == 0 for s in S.slots]
    return S


def check_block_facts(S):
    """what the join relies on: a coded segment is ONE block, BFINAL at bit 0, `bits` long up
    to and including its end-of-block code; a stored one is ceil(n / 65535) byte-aligned
    stored blocks, only the last header byte 1, bits = 8 * size"""
    for i, (slot, nb, plain) in enumerate(zip(S.slots, S.bits, S.plain)):
        assert len(slot) == (nb + 7) // 8, i
        if S.stored[i]:
            assert nb == 8 * len(slot), i
            n, p, q = len(plain), 0, 0
            nblk = (n + 65534) // 65535
            assert len(slot) == 5 * nblk + n, i
            for b in range(nblk):
                ln = min(65535, n - p)
                assert slot[q] == (1 if b + 1 == nblk else 0), (i, b)
                assert int.from_bytes(slot[q + 1:q + 3], "little") == ln, (i, b)
                assert int.from_bytes(slot[q + 3:q + 5], "little") == ln ^ 0xFFFF, (i, b)
                assert slot[q + 5:q + 5 + ln] == plain[p:p + ln], (i, b)
                p, q = p + ln, q + 5 + ln
            continue
        assert slot[0] & 1 and (slot[0] >> 1) & 3 in (1, 2), i
        v = int.from_bytes(slot, "little") & ((1 << nb) - 1)
        assert v == int.from_bytes(slot, "little"), "padding bits must be zero"
        # bits >= nb do not matter: the block ends inside the first nb bits ...
        ones = ((1 << (8 * len(slot))) - 1) >> nb << nb
        d = zlib.decompressobj(-15)
        assert d.decompress((v | ones).to_bytes(len(slot), "little")) == plain and d.eof, i
        # ... and bit nb - 1 does: it is the end-of-block code's last bit
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress((v ^ (1 << (nb - 1))).to_bytes(len(slot), "little"))
            assert not (d.eof and got == plain), i
        except zlib.error:
            pass


def join(eng, S, capacity=None, guard=64):
    # (capacity is a multiple of 4: the stream is written in whole dwords)
    cap = (sum(S.sizes) + S.nseg + 3) & ~3 if capacity is None else capacity
    buf = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    starts = torch.full((S.nseg + 1,), -1, dtype=torch.int64, device="cuda")
    eng.deflate_join(S.d_slab, S.stride, S.d_sizes, S.d_bits, S.nseg, starts, buf, capacity=cap)
    return buf, starts, cap


def check_case(eng, codec, parts, uniform_seg=None):
    import bitar_amd
    S = compress_parts(eng, codec, parts)
    check_block_facts(S)
    plain = b"".join(S.plain)
    want, wstarts = model_join(S.slots, S.bits)

    # positions only, then the stream
    only = torch.full((S.nseg + 1,), -1, dtype=torch.int64, device="cuda")
    eng.deflate_join(S.d_slab, S.stride, S.d_sizes, S.d_bits, S.nseg, only)
    buf, starts, cap = join(eng, S)
    eng.sync()
    assert down(only).tolist() == wstarts
    assert down(starts).tolist() == wstarts
    got = down(buf)
    assert len(want) <= cap
    assert got[:len(want)].tobytes() == want
    assert not got[len(want):cap].any(), "bytes behind the stream must be zero"
    assert np.all(got[cap:] == 0xA5), "written past capacity"
    assert zlib.decompress(want, -15) == plain

    # split(join(slab)) == slab
    entries = np.array([b | (STORED if st else 0) for b, st in zip(S.bits, S.stored)], np.int32)
    slab2 = torch.full((S.nseg * S.stride,), 0x5A, dtype=torch.uint8, device="cuda")
    sizes2 = torch.full((S.nseg,), -2, dtype=torch.int32, device="cuda")
    eng.deflate_split(buf, len(want), starts, up(entries, np.int32), S.nseg, slab2, S.stride,
                      sizes2)
    eng.sync()
    assert down(sizes2).astype(np.uint32).tolist() == S.sizes
    h2 = down(slab2)
    for i, s in enumerate(S.slots):
        assert h2[i * S.stride:i * S.stride + len(s)].tobytes() == s, i

    # the inflaters run unchanged on the split slots
    if uniform_seg:
        out = torch.zeros(S.nseg * uniform_seg, dtype=torch.uint8, device="cuda")
        prod = torch.zeros(S.nseg, dtype=torch.int32, device="cuda")
        eng.decompress_slab_into(bitar_amd.CODEC_DEFLATE, slab2, S.stride, sizes2, S.nseg,
                                 uniform_seg, out, prod, capacity=S.nseg * uniform_seg)
        eng.sync()
        assert down(prod).tolist() == [len(p) for p in S.plain]
        assert down(out)[:len(plain)].tobytes() == plain

    # CRC-32 of the whole input from its segments' CRC-32s
    check_crc(eng, np.frombuffer(plain, np.uint8), uniform_seg or parts[0][1])
    return S, want, wstarts


def check_crc(eng, data, seg):
    import bitar_amd
    n = data.size
    nseg = (n + seg - 1) // seg
    sums = torch.zeros(max(nseg, 1), dtype=torch.int64, device="cuda")
    crc = torch.full((1,), -2, dtype=torch.int32, device="cuda")
    if n:
        eng.checksum(bitar_amd.CHECKSUM_CRC32, up(data), seg, sums, n=n)
    eng.crc32_combine(sums, n, seg, crc)
    eng.sync()
    assert int(down(crc).astype(np.uint32)[0]) == zlib.crc32(data.tobytes())


# ---- cases --------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", ["fixed", "dynamic"])
def test_every_bit_phase(eng, codec):
    """16-byte all-literal segments of 138 + j bits walk the coded starts through all 8 bit
    phases; a stored segment follows every second one, entered at >= 4 distinct phases"""
    def lit(j):
        return np.array(list(range(200, 200 + j)) + list(range(10, 26 - j)), np.uint8)
    parts, js = [], []
    for p in range(15):
        a, b = p, (2 * p + 1) % 15
        parts.append((np.concatenate([lit(a), lit(b)]), 16))
        parts.append((rnd(64, 100 + p), 64))
        js += [a, b, None]
    S, _, starts = check_case(eng, codecs()[codec], parts)
    assert S.nseg == 45
    coded, stored = set(), set()
    for i, j in enumerate(js):
        if j is None:
            assert S.stored[i], i
            stored.add(starts[i] & 7)
        else:
            assert not S.stored[i] and S.bits[i] == 138 + j, (i, j, S.bits[i])
            assert S.sizes[i] in (18, 19)
            coded.add(starts[i] & 7)
    assert coded == set(range(8))
    assert len(stored) >= 4


@pytest.mark.parametrize("codec", ["fixed", "dynamic"])
@pytest.mark.parametrize("seg,n", [(1, 200), (13, 200)])
def test_shared_dwords(eng, codec, seg, n):
    """streams shorter than a dword: several segments share one output dword"""
    S, _, _ = check_case(eng, codecs()[codec], [(text(n, 5), seg)], uniform_seg=seg)
    if seg == 1:
        assert max(S.sizes) < 4


@pytest.mark.parametrize("codec", ["fixed", "dynamic"])
def test_scan_carry(eng, codec):
    """1100 segments: the scan's position and bit phase carry from tile to tile; every tenth
    segment is stored, so later positions depend on the phase the carry delivers"""
    parts = []
    for k in range(100):
        t = text(13 * 10, k).copy()
        t[:k % 8] = np.arange(200, 200 + k % 8)  # 9-bit literals: the ten coded segments' bits differ from part to part
        parts.append((t, 13))
        parts.append((rnd(64, 500 + k), 64))
    S, _, starts = check_case(eng, codecs()[codec], parts)
    assert S.nseg == 1100 and sum(S.stored) == 100
    assert len({starts[i] & 7 for i in range(S.nseg) if S.stored[i]}) >= 4


@pytest.mark.parametrize("codec", ["fixed", "dynamic"])
@pytest.mark.parametrize("order", ["RTR", "TRR", "RRT"])
def test_two_block_stored_segments(eng, codec, order):
    """a stored 65536-byte segment is two blocks (65535 + 1 bytes): in the joined stream the
    final flag lands on the SECOND block's header, and only when the segment is last"""
    seg = 65536
    data = np.concatenate([rnd(seg, 7 + k) if c == "R" else text(seg, 7 + k)
                           for k, c in enumerate(order)])
    S, want, starts = check_case(eng, codecs()[codec], [(data, seg)], uniform_seg=seg)
    assert S.stored == [c == "R" for c in order]
    for i, c in enumerate(order):
        if c != "R":
            continue
        assert S.sizes[i] == seg + 10
        first = starts[i]
        assert (want[first >> 3] >> (first & 7)) & 7 == 0  # BFINAL 0, BTYPE 00
        second = ((first + 3 + 7) >> 3) + 65539
        assert want[second] == (1 if i == 2 else 0)


@pytest.mark.parametrize("codec", ["fixed", "dynamic"])
def test_edge_sizes(eng, codec):
    c = codecs()[codec]
    check_case(eng, c, [(text(100, 1), 4096)], uniform_seg=4096)      # nseg = 1, coded
    check_case(eng, c, [(rnd(100, 1), 4096)], uniform_seg=4096)       # nseg = 1, stored
    check_case(eng, c, [(text(3 * 512 + 1, 2), 512)], uniform_seg=512)  # 1-byte last segment
    check_case(eng, c, [(rnd(3 * 512 + 1, 2), 512)], uniform_seg=512)


@pytest.mark.parametrize("codec", ["fixed", "dynamic"])
def test_empty_input(eng, codec):
    """n = 0: nothing is launched, the stream is 0 bits, the CRC-32 is that of nothing"""
    c = codecs()[codec]
    sizes = torch.full((1,), -2, dtype=torch.int32, device="cuda")
    bits = torch.full((1,), -2, dtype=torch.int32, device="cuda")
    slab = torch.full((256,), 0xEE, dtype=torch.uint8, device="cuda")
    eng.compress_bits_into(c, slab, 4096, slab, 256, sizes, bits, n=0)
    starts = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    buf = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")
    eng.deflate_join(slab, 256, sizes, bits, 0, starts, buf, capacity=0)
    eng.deflate_split(buf, 0, starts, bits, 0, slab, 256, sizes)
    eng.sync()
    assert down(starts).tolist() == [0]
    assert down(sizes)[0] == -2 and down(bits)[0] == -2
    assert np.all(down(buf) == 0xA5) and np.all(down(slab) == 0xEE)
    check_crc(eng, np.zeros(0, np.uint8), 4096)


def test_compress_bits_other_codecs_invalid(eng):
    import bitar_amd
    d = up(text(100))
    slab = eng.empty(4096)
    sizes = eng.empty(1, dtype=torch.int32)
    for c in (bitar_amd.CODEC_LZ4, bitar_amd.CODEC_ZSTD, bitar_amd.CODEC_LZ4_WIDE):
        with pytest.raises(bitar_amd.BitarError) as ex:
            eng.compress_bits_into(c, d, 100, slab, bitar_amd.slot_size(c, 100), sizes, sizes)
        assert ex.value.code == -4


@pytest.mark.parametrize("codec", ["fixed", "dynamic"])
def test_crc_combine_sizes(eng, codec):
    """more segments than the combining workgroup has threads, a short last segment, and
    exponents beyond one step"""
    for n, seg in [(1, 1), (300 * 7 + 3, 7), (1000 * 64, 64), (65536 * 3 + 5, 65536)]:
        check_crc(eng, rnd(n, n), seg)


def _small_case(eng, codec):
    parts = [(text(13 * 20, 3), 13), (rnd(64, 9), 64), (text(13 * 19, 4), 13)]
    S = compress_parts(eng, codec, parts)
    want, wstarts = model_join(S.slots, S.bits)
    return S, want, wstarts


@pytest.mark.parametrize("codec", ["fixed", "dynamic"])
@pytest.mark.parametrize("bad", ["start", "bits", "size", "stored_reach", "flags"])
def test_split_rejects_bad_entries(eng, codec, bad):
    """starts[] / entries[] come from an untrusted header: the bad slot is marked and never
    touched, the sync reports IOError, the neighbours are intact"""
    import bitar_amd
    S, want, wstarts = _small_case(eng, codecs()[codec])
    buf, starts, _ = join(eng, S)
    eng.sync()
    entries = np.array([b | (STORED if st else 0) for b, st in zip(S.bits, S.stored)], np.int64)
    st = np.array(wstarts, np.int64)
    k = 7
    total = 8 * len(want)
    if bad == "start":
        st[k] = total + 1
    elif bad == "bits":  # fits the slot, reaches past the stream
        st[k] = total - 100
        entries[k] = 8 * 100
    elif bad == "size":  # would not fit the slot
        st[k] = 0
        entries[k] = 8 * (S.stride + 1)
    elif bad == "stored_reach":  # a stored body that runs past the stream
        st[k] = total - 8 * 20
        entries[k] = (8 * 40) | STORED
    else:
        entries[k] |= 1 << 24
    slab2 = torch.full((S.nseg * S.stride,), 0x5A, dtype=torch.uint8, device="cuda")
    sizes2 = torch.full((S.nseg,), -2, dtype=torch.int32, device="cuda")
    eng.deflate_split(buf, len(want), up(st, np.int64), up(entries.astype(np.int32), np.int32),
                      S.nseg, slab2, S.stride, sizes2)
    with pytest.raises(bitar_amd.BitarError) as ex:
        eng.sync()
    assert ex.value.code == -5
    eng.sync()  # reported once
    z = down(sizes2).astype(np.uint32)
    h = down(slab2)
    for i, s in enumerate(S.slots):
        slot = h[i * S.stride:(i + 1) * S.stride]
        if i == k:
            assert z[i] == SEGMENT_ERROR and np.all(slot == 0x5A)
        else:
            assert z[i] == len(s) and slot[:len(s)].tobytes() == s, i


@pytest.mark.parametrize("codec", ["fixed", "dynamic"])
def test_join_capacity_and_failed_segment(eng, codec):
    """a stream that needs more than `capacity` sets the error word and changes nothing past
    it; a failed segment (SEGMENT_ERROR) joins as nothing and is reported"""
    import bitar_amd
    S, want, wstarts = _small_case(eng, codecs()[codec])
    buf, starts, cap = join(eng, S, capacity=(len(want) - 1) & ~3)
    with pytest.raises(bitar_amd.BitarError) as ex:
        eng.sync()
    assert ex.value.code == -5
    got = down(buf)
    assert np.all(got[cap:] == 0xA5)
    assert down(starts).tolist() == wstarts
    # the segments that end inside the capacity are written, the others not at all
    fit = max(i for i in range(S.nseg) if (wstarts[i + 1] + 7) // 8 <= cap)
    assert fit >= S.nseg - 3
    keep = wstarts[fit + 1] >> 3
    assert got[:keep].tobytes() == want[:keep]
    assert not got[(wstarts[fit + 1] + 7) // 8:cap].any()
    with pytest.raises(bitar_amd.BitarError) as ex:  # a capacity that is no whole dwords
        join(eng, S, capacity=len(want) | 1)
    assert ex.value.code == -4

    sizes = np.array(S.sizes, np.uint32)
    bits = np.array(S.bits, np.uint32)
    sizes[5] = bits[5] = SEGMENT_ERROR
    S.d_sizes = up(sizes.view(np.int32), np.int32)
    S.d_bits = up(bits.view(np.int32), np.int32)
    buf, starts, cap = join(eng, S)
    with pytest.raises(bitar_amd.BitarError) as ex:
        eng.sync()
    assert ex.value.code == -5
    slots = [s for i, s in enumerate(S.slots) if i != 5]
    w2, _ = model_join(slots, [b for i, b in enumerate(S.bits) if i != 5])
    assert down(buf)[:len(w2)].tobytes() == w2
