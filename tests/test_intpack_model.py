"""CPU tests of the INTPACK model (intpack_model.py): round trips, hand-written streams that
pin the field and bit order, the mode choice, every reject rule of the decoder, what the codec
buys on integer columns against the oracle's LZ4, and the library's surface.  No GPU."""
import numpy as np
import pytest

import filter_model as F
import intpack_model as M
import oracle_lib as O

SEGS = (65536, 59460, 4096, 1000, 999, 72, 7)


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def column(n, w, seed):
    """n bytes of a column whose segments take different modes: small-range noise, a sorted
    run, a constant run and a stretch of random bytes"""
    rng = np.random.default_rng(seed)
    m = n // w + 1
    v = rng.integers(0, 1 << min(8 * w - 1, 10), m).astype(M._U[w])
    q = m // 4
    step = rng.integers(0, 1 << min(4 * w, 6), q).astype(np.uint64)
    v[q:2 * q] = (np.cumsum(step) + np.uint64(12345)).astype(M._U[w])  # (wraps when narrow)
    v[2 * q:2 * q + q // 2] = 7
    out = v.view(np.uint8)[:n].copy()
    a = 3 * q * w
    b = min(n, a + q * w // 2)
    if b > a:
        out[a:b] = rnd(b - a, seed + 1)
    return out


def roundtrip(data, w, seg):
    streams = M.encode(data, w, seg)
    assert len(streams) == (data.size + seg - 1) // seg
    back = b"".join(M.decode(s, seg) for s in streams)
    assert back == data.tobytes()
    for i, s in enumerate(streams):
        L = min(seg, data.size - i * seg)
        assert len(s) <= 4 + L
        assert (s[0] >> 2) & 3 == 2 or len(s) < 4 + L
    return streams


@pytest.mark.parametrize("w", M.WIDTHS)
def test_round_trip(w):
    for seg in SEGS:
        for r in sorted({0, 1, w - 1, w, 63 * w, 64 * w, 64 * w + 1, 256 * w + 3}):
            n = 3 * seg + r
            roundtrip(column(n, w, seg + r), w, seg)
    for n in range(1, w):  # shorter than an element: stored
        (s,) = roundtrip(rnd(n, n), w, 72)
        assert (s[0] >> 2) & 3 == 2 and len(s) == 4 + n
    assert M.encode(np.zeros(0, np.uint8), w, 72) == []


def test_random_input_round_trips_stored():
    for w in M.WIDTHS:
        for seg in (65536, 999):
            data = rnd(2 * seg + 5, seg + w)
            for i, s in enumerate(roundtrip(data, w, seg)):
                L = min(seg, data.size - i * seg)
                assert (s[0] >> 2) & 3 == 2 and len(s) == 4 + L
                assert s[4:] == data[i * seg:i * seg + L].tobytes()


def test_golden_delta_stream():
    """w = 2, elements 0..69: every delta is 1, so ref = 1 and both widths are 0"""
    data = np.arange(70, dtype="<u2").view(np.uint8)
    want = bytes([0x45, 0x00, 0x8B, 0x00,  # tag: mode 1, log2 w = 1; L - 1 = 139
                  0x00, 0x00,              # base = element 0
                  0x00, 0x00,              # widths of the two miniblocks
                  0x01, 0x00])             # ref of the one block
    assert M.encode(data, 2, 65536) == [want]
    assert M.packed_sizes(data, 2) == (4 + 2 + 2 + 8 * (6 + 7), 10)
    assert M.decode(want, 140) == data.tobytes()


def test_golden_plain_streams():
    """mode 0 with the payload written out by hand: 2-bit fields inside a byte, and 3-bit
    fields across bytes (the residuals 0..7 pack as 0xFAC688, little-endian)"""
    data = (10 + np.arange(64) % 4).astype(np.uint8)
    want = bytes([0x40, 0x00, 0x3F, 0x00, 0x02, 0x0A]) + bytes([0xE4]) * 16
    assert M.encode(data, 1, 4096) == [want]
    assert M.decode(want, 64) == data.tobytes()

    data = (1000 + np.arange(64) % 8).astype("<u4").view(np.uint8)
    want = bytes([0x42, 0x00, 0xFF, 0x00, 0x03, 0xE8, 0x03, 0x00, 0x00]) + \
        bytes([0x88, 0xC6, 0xFA]) * 8
    assert M.encode(data, 4, 4096) == [want]
    assert M.decode(want, 256) == data.tobytes()

    # the same elements with 3 tail bytes and a second, partial miniblock (padding packs as 0)
    data = np.concatenate([data, np.array([1007, 1001], "<u4").view(np.uint8),
                           np.array([0xAA, 0xBB, 0xCC], np.uint8)])
    want = bytes([0x42, 0x00, 0x0A, 0x01, 0x03, 0x03, 0xE8, 0x03, 0x00, 0x00]) + \
        bytes([0x88, 0xC6, 0xFA]) * 8 + bytes([0x0F] + [0] * 23) + bytes([0xAA, 0xBB, 0xCC])
    assert M.encode(data, 4, 4096) == [want]
    assert M.decode(want, 4096) == data.tobytes()


def mode_of(stream):
    return (stream[0] >> 2) & 3


def widths_of(stream, w):
    L = 1 + stream[2] + (stream[3] << 8)
    nmb = (L // w + 63) // 64
    p = 4 + (w if mode_of(stream) == 1 else 0)
    return list(stream[p:p + nmb])


def test_mode_choice():
    rng = np.random.default_rng(5)
    # monotone int32 offsets of a string array
    offs = np.cumsum(rng.integers(0, 40, 16384)).astype("<u4").view(np.uint8)
    (s,) = roundtrip(offs, 4, 65536)
    assert mode_of(s) == 1 and max(widths_of(s, 4)) <= 6
    # small-range noise
    noise = (rng.integers(0, 1 << 62, 8192) % 1000).astype("<u8").view(np.uint8)
    (s,) = roundtrip(noise, 8, 65536)
    assert mode_of(s) == 0 and max(widths_of(s, 8)) == 10
    # a constant column: all widths 0
    const = np.full(8192, 0x6161616161616161, "<u8").view(np.uint8)
    (s,) = roundtrip(const, 8, 65536)
    assert mode_of(s) == 0 and set(widths_of(s, 8)) == {0}
    assert len(s) == 4 + 128 + 32 * 8
    # negative small values as int32: the reference is signed
    small = rng.integers(-5, 6, 4096).astype("<i4")
    small[:11] = np.arange(-5, 6)
    (s,) = roundtrip(small.view(np.uint8), 4, 65536)
    assert mode_of(s) == 0 and max(widths_of(s, 4)) == 4
    # values (and deltas) spanning the whole signed range in one block: width 8w
    for w in M.WIDTHS:
        info = np.iinfo(M._S[w])
        v = np.zeros(1024, M._S[w])
        v[:256] = np.array([info.min, info.max, 0])[rng.integers(0, 3, 256)]
        v[:3] = (info.min, info.max, info.min)
        (s,) = roundtrip(v.view(np.uint8), w, 65536)
        assert mode_of(s) == 0 and widths_of(s, w) == [8 * w] * 4 + [0] * 12
    # a delta that wraps past 2^(8w): sorted values with one wrap-around
    v = (np.arange(4096, dtype=np.uint64) * 3 + (1 << 32) - 6000).astype("<u4")
    assert v[0] > v[-1]
    (s,) = roundtrip(v.view(np.uint8), 4, 65536)
    assert mode_of(s) == 1 and set(widths_of(s, 4)) == {0}


def valid_stream(w=4, mode=1):
    rng = np.random.default_rng(9)
    if mode == 1:
        v = np.cumsum(rng.integers(0, 40, 1024)).astype(M._U[w])
    else:
        v = rng.integers(0, 100, 1024).astype(M._U[w])
    data = np.concatenate([v.view(np.uint8), np.array([1, 2, 3], np.uint8)[:w - 1]])
    (s,) = M.encode(data, w, 65536)
    assert mode_of(s) == mode and M.decode(s, data.size) == data.tobytes()
    return bytearray(s), data


def test_decode_rejects_unknown_tag():
    s, data = valid_stream()
    for tag in (s[0] & 0x0F, s[0] | 0x80, 0x50 | (s[0] & 15), (s[0] & 0xF3) | 0x0C):
        t = bytearray(s)
        t[0] = tag
        assert M.decode(t, data.size) is None, hex(tag)


def test_decode_rejects_reserved_byte():
    s, data = valid_stream()
    for v in (1, 0x80, 0xFF):
        t = bytearray(s)
        t[1] = v
        assert M.decode(t, data.size) is None


def test_decode_rejects_length_above_the_segment():
    s, data = valid_stream()
    assert M.decode(s, data.size - 1) is None
    assert M.decode(s, data.size) is not None
    stored = M.encode(rnd(100, 1), 1, 4096)[0]
    assert M.decode(stored, 99) is None and M.decode(stored, 100) is not None


def test_decode_rejects_width_above_the_element():
    for w in M.WIDTHS:
        s, data = valid_stream(w, 0)
        for bad in (8 * w + 1, 255):
            for k in (0, len(widths_of(s, w)) - 1):
                t = bytearray(s)
                t[4 + k] = bad
                assert M.decode(t, data.size) is None


def test_decode_rejects_size_mismatch():
    for mode in (0, 1):
        s, data = valid_stream(4, mode)
        assert M.decode(s + b"\0", data.size) is None
        assert M.decode(s[:-1], data.size) is None
        assert M.decode(s[:3], data.size) is None
        assert M.decode(s[:4], data.size) is None
        assert M.decode(b"", data.size) is None
        t = bytearray(s)  # a width one smaller: the computed size no longer matches
        k = 4 + (4 if mode else 0)
        t[k] -= 1
        assert M.decode(t, data.size) is None
    stored = M.encode(rnd(100, 1), 1, 4096)[0]
    assert M.decode(stored + b"\0", 100) is None and M.decode(stored[:-1], 100) is None


def test_decode_takes_the_width_from_the_tag():
    """a tag of another width changes the layout: the model decodes or rejects by the tag alone"""
    s, data = valid_stream(4, 0)
    assert M.decode(s, 65536) == data.tobytes()
    t = bytearray(s)
    t[0] = (t[0] & ~3) | 3
    assert M.decode(t, 65536) is None  # (the size no longer adds up)


@pytest.fixture(scope="module")
def kind5():
    return O.fill(5, 7, 4 << 20)


def test_int64_column_beats_lz4_behind_bitshuffle(kind5):
    """kind 5 (int64 in [0, 1000)) at 4 MiB, 64 KiB segments, width 8: INTPACK's total is below
    the oracle's LZ4 on the bitshuffled bytes, the best the filters reach"""
    seg = 65536
    total = sum(len(s) for s in M.encode(kind5, 8, seg))
    r, _, sizes = O.compress_segments(O.CODEC_LZ4, F.apply(F.BITSHUFFLE, kind5, 8, seg), seg,
                                      2 * seg, threads=4)
    assert r == 0
    lz4 = int(sizes.astype(np.uint64).sum())
    print(f"kind 5: intpack {total} B, bitshuffle + lz4 {lz4} B")
    assert total < lz4


def test_dictionary_index_column_packs_below_a_quarter():
    """kind 2's int32-pair column (MiB 2 of each 4 MiB period, values < 64): widths <= 6 of 32
    bits plus headers"""
    body = O.fill(2, 7, 4 << 20)[2 << 20:3 << 20]
    total = sum(len(s) for s in M.encode(body, 4, 65536))
    print(f"kind 2 column 2: intpack {total} B of {body.size}")
    assert 4 * total < body.size


def test_library_surface():
    import bitar_amd as B
    assert (B.CODEC_INTPACK8, B.CODEC_INTPACK16, B.CODEC_INTPACK32, B.CODEC_INTPACK64) == \
        (8, 9, 10, 11)
    assert [B.codec_intpack(w) for w in M.WIDTHS] == [8, 9, 10, 11]
    for bad in (0, 3, 16, None):
        with pytest.raises(ValueError):
            B.codec_intpack(bad)
    assert B.slot_size(B.CODEC_INTPACK64, 65536) == 65792
    assert B.slot_size(B.CODEC_INTPACK8, 1) == 256
    assert B.slot_size(B.CODEC_INTPACK32, 59460) == 59648
    assert B.slot_size(99, 100) == 0 and B.max_distance(99) == 0
    assert B.slot_size(7, 100) == 0 and B.slot_size(12, 100) == 0
    for w in M.WIDTHS:
        assert B.max_distance(B.codec_intpack(w)) == 0
