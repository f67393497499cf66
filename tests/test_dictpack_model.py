"""CPU tests of the DICTPACK model (dictpack_model.py): hand-written streams that pin the field
and bit order, round trips of low-cardinality columns and of the edge cases, the form choice,
every reject rule of the decoder, and the library's surface.  No GPU."""
import numpy as np
import pytest

import dictpack_model as M

SEGS = (65536, 59460, 4096, 1000, 999, 72, 7)


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def mode_of(s):
    return s[0] >> 3 & 1


def draw(values, n, seed, p=None):
    """n elements drawn from the rows of `values` (k x w bytes) -> their bytes"""
    rng = np.random.default_rng(seed)
    return values[rng.choice(values.shape[0], n, p=p)].reshape(-1)


def table_columns(n=1 << 20):
    """the low-cardinality columns DICTPACK is for -> [(name, w, bytes, least ratio at 64 KiB
    segments)]; the least ratio is the format's size formula at the largest d a segment can have"""
    rng = np.random.default_rng(2024)
    u8 = lambda a: np.ascontiguousarray(a).view(np.uint8)  # noqa: E731
    ids = u8(rng.integers(0, 1 << 63, 40).astype("<u8")).reshape(40, 8)
    zipf = u8(rng.integers(0, 1 << 63, 2000).astype("<u8")).reshape(2000, 8)
    pz = 1.0 / np.arange(1, 2001) ** 1.3
    f64 = u8(rng.normal(0, 1, 200).astype("<f8")).reshape(200, 8)
    f32 = u8(rng.normal(0, 1, 900).astype("<f4")).reshape(900, 4)
    uuid = rnd(500 * 16, 5).reshape(500, 16)
    dec = np.zeros((300, 16), np.uint8)
    dec[:, :8] = u8(rng.integers(100, 10_000_000, 300).astype("<u8")).reshape(300, 8)
    size = lambda w, d: M.packed_size(65536, w, d)  # noqa: E731
    return [("int64 ids, 40 distinct", 8, draw(ids, n // 8, 1), 65536 / size(8, 40)),
            ("int64 ids, Zipf(1.3) over 2000", 8, draw(zipf, n // 8, 2, pz / pz.sum()),
             65536 / size(8, 1024)),
            ("float64, 200 distinct", 8, draw(f64, n // 8, 3), 65536 / size(8, 200)),
            ("float32, 900 distinct", 4, draw(f32, n // 4, 4), 65536 / size(4, 900)),
            ("UUIDs, 500 distinct", 16, draw(uuid, n // 16, 5), 65536 / size(16, 500)),
            ("decimal128, 300 price points", 16, draw(dec, n // 16, 6), 65536 / size(16, 300))]


def roundtrip(data, w, seg):
    streams = M.encode(data, w, seg)
    assert len(streams) == (data.size + seg - 1) // seg
    assert b"".join(M.decode(s, seg) for s in streams) == data.tobytes()
    for i, s in enumerate(streams):
        L = min(seg, data.size - i * seg)
        assert s[0] >> 4 == 6 and s[0] & 7 == {4: 2, 8: 3, 16: 4}[w] and s[1] == 0
        assert 1 + s[2] + (s[3] << 8) == L
        assert len(s) == 4 + L if mode_of(s) else len(s) < 4 + L
    return streams


# ---- hand-written streams ---------------------------------------------------------------------

def test_golden_alternating_words():
    """w = 4, L = 256: 64 elements A, B, A, B ... -> d = 2, b = 1, every payload byte 0xAA"""
    A, B = bytes([0x11, 0x22, 0x33, 0x44]), bytes([0xF0, 0x0F, 0x00, 0xFF])
    want = bytes([0x62, 0x00, 0xFF, 0x00, 0x01, 0x00]) + A + B + bytes([0xAA] * 8)
    assert len(want) == 22
    data = np.frombuffer((A + B) * 32, np.uint8)
    assert M.encode_segment(data, 4) == want
    assert M.decode(want, 256) == data.tobytes()


def test_golden_sixteen_byte_elements():
    """w = 16, L = 83: X Y X Z Y and a tail of 3 bytes -> d = 3, b = 2, indices 0 1 0 2 1 in the
    bits 0..9 of one miniblock of 16 bytes"""
    X, Y, Z = bytes(range(16)), bytes(range(16, 32)), bytes([0xFF] * 15 + [0x00])
    tail = bytes([0xDE, 0xAD, 0x42])
    payload = bytes([0b10000100, 0b00000001] + [0] * 14)
    want = bytes([0x64, 0x00, 82, 0x00, 0x02, 0x00]) + X + Y + Z + payload + tail
    assert len(want) == 6 + 48 + 16 + 3
    data = np.frombuffer(X + Y + X + Z + Y + tail, np.uint8)
    assert M.encode_segment(data, 16) == want
    assert M.decode(want, 4096) == data.tobytes()


def test_golden_stored_and_single_value():
    five = bytes([9, 8, 7, 6, 5])  # shorter than an element: stored
    assert M.encode_segment(np.frombuffer(five, np.uint8), 8) == bytes([0x6B, 0, 4, 0]) + five
    # two different doubles: 6 + 16 + 8 > 4 + 16, stored
    two = bytes(range(16))
    assert M.encode_segment(np.frombuffer(two, np.uint8), 8) == bytes([0x6B, 0, 15, 0]) + two
    # one value three times and a tail: d = 1, no payload
    v = bytes([1, 0, 0, 0, 0, 0, 0, 0x80])
    s = M.encode_segment(np.frombuffer(v * 3 + b"\x07", np.uint8), 8)
    assert s == bytes([0x63, 0, 24, 0, 0, 0]) + v + b"\x07"
    assert M.decode(s, 25) == v * 3 + b"\x07"


# ---- round trips ------------------------------------------------------------------------------

def test_table_columns_round_trip_at_the_ratio_the_format_gives():
    for name, w, data, least in table_columns():
        streams = roundtrip(data, w, 65536)
        assert all(mode_of(s) == 0 for s in streams), name
        ratio = data.size / sum(len(s) for s in streams)
        print(f"{name}: {ratio:.2f} (at least {least:.2f})")
        assert ratio >= least * 0.999, name
    streams = roundtrip(rnd(1 << 18, 9), 8, 65536)  # random bytes: stored, 4 bytes a segment
    assert all(mode_of(s) == 1 and len(s) == 65540 for s in streams)


@pytest.mark.parametrize("w", M.WIDTHS)
def test_round_trip_lengths_and_segments(w):
    values = rnd(37 * w, w).reshape(37, w)
    for seg in SEGS:
        for r in sorted({0, 1, w - 1, w, 63 * w, 64 * w, 64 * w + 1, 256 * w + 3}):
            roundtrip(draw(values, (3 * seg + r) // w + 1, seg + r)[:3 * seg + r], w, seg)
    for n in range(1, w):  # shorter than an element: stored
        (s,) = roundtrip(rnd(n, n), w, 72)
        assert mode_of(s) == 1 and len(s) == 4 + n
    assert M.encode(np.zeros(0, np.uint8), w, 72) == []


@pytest.mark.parametrize("w", M.WIDTHS)
def test_cardinalities(w):
    """d = 1, 2, 3, 2^k, 2^k + 1, 1023 and 1024 pack at b = bit_length(d - 1); 1025 is stored; the
    dictionary is in order of first occurrence, also when the last value first shows in the last
    element"""
    L = 65536
    m = L // w
    for d in [1, 2, 3] + [x for k in range(2, 10) for x in (1 << k, (1 << k) + 1)] + \
            [1023, 1024, 1025]:
        values = rnd(d * w, d).reshape(d, w)
        values[:, 0] = np.arange(d) & 255  # (distinct rows)
        values[:, 1] = np.arange(d) >> 8
        idx = np.random.default_rng(d).integers(0, max(d - 1, 1), m)
        idx[:d - 1] = np.arange(d - 1)[::-1]  # first occurrences in reverse order of the rows
        idx[m - 1] = d - 1  # the last row first shows in the final element
        data = values[idx].reshape(-1)
        (s,) = roundtrip(data, w, L)
        if d > 1024 or M.packed_size(L, w, d) > 4 + L:
            assert mode_of(s) == 1
            continue
        assert mode_of(s) == 0 and 1 + s[4] + (s[5] << 8) == d
        order = list(range(d - 2, -1, -1)) + [d - 1] if d > 1 else [0]
        assert s[6:6 + d * w] == values[order].tobytes()
        assert len(s) == 6 + d * w + 8 * (d - 1).bit_length() * ((m + 63) // 64)


def test_byte_patterns_are_the_values():
    """+0.0 / -0.0 and NaNs of different payloads are distinct entries; nothing is normalised"""
    pats = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF8000000000000,
                     0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000000], "<u8")
    data = pats[np.random.default_rng(1).integers(0, 6, 4096)].view(np.uint8)
    data[:48] = pats.view(np.uint8)
    (s,) = roundtrip(data, 8, 65536)
    assert mode_of(s) == 0 and s[4] == 5 and s[6:54] == pats.tobytes()


def test_sizes_are_never_equal():
    """packed - stored = 2 + d*w + 8*b*nmb - m*w = 2 mod 4: `<` and `<=` choose alike"""
    for w in M.WIDTHS:
        for L in (1, w, 5 * w + 1, 999, 4096, 59460, 65536):
            for d in (1, 2, 3, 100, 1024):
                assert (M.packed_size(L, w, d) - (4 + L)) % 4 == 2


@pytest.mark.parametrize("w", M.WIDTHS)
def test_break_even(w):
    """around the break-even the encoder takes the smaller form"""
    values = rnd(64 * w, 3).reshape(64, w)
    values[:, 0] = np.arange(64)
    seen = set()
    for m in range(1, 200):
        for d in (1, 2, 3, 5, 9, 17, 33):
            if d > m:
                continue
            data = values[np.arange(m) % d].reshape(-1)
            (s,) = roundtrip(data, w, 4096)
            packs = M.packed_size(m * w, w, d) < 4 + m * w
            assert mode_of(s) == (0 if packs else 1)
            seen.add(packs)
    assert seen == {True, False}


# ---- what the decoder rejects -----------------------------------------------------------------

def packed_example(w, d=5, m=200, tail=3):
    values = rnd(d * w, 17).reshape(d, w)
    values[:, 0] = np.arange(d)
    data = np.concatenate([values[np.arange(m) % d].reshape(-1), rnd(tail, 1)])
    s = M.encode_segment(data, w)
    assert mode_of(s) == 0 and M.decode(s, 65536) == data.tobytes()
    return bytearray(s), data


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_tag_and_reserved_byte(w):
    s, _ = packed_example(w)
    for nib in range(16):
        t = bytearray(s)
        t[0] = nib << 4 | s[0] & 15
        assert (M.decode(t, 65536) is None) == (nib != 6)
    for lg in (0, 1, 5, 6, 7):
        t = bytearray(s)
        t[0] = s[0] & ~7 | lg
        assert M.decode(t, 65536) is None
    for v in (1, 0x80, 0xFF):
        t = bytearray(s)
        t[1] = v
        assert M.decode(t, 65536) is None
    assert M.decode(s[:3], 65536) is None and M.decode(b"", 65536) is None
    assert M.decode(s[:5], 65536) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_length_above_the_segment(w):
    s, data = packed_example(w)
    assert M.decode(s, data.size) == data.tobytes()
    assert M.decode(s, data.size - 1) is None
    stored = M.encode_segment(rnd(100, 2), w)
    assert mode_of(stored) == 1 and M.decode(stored, 100) is not None
    assert M.decode(stored, 99) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_dictionary_sizes(w):
    # d = m + 1 (with the size its formula gives)
    lg = {4: 2, 8: 3, 16: 4}[w]
    for d, verdict in ((4, bytes(4 * w)), (5, None)):
        t = bytes([0x60 | lg, 0, 4 * w - 1, 0, d - 1, 0]) + bytes(d * w) + \
            bytes(8 * (d - 1).bit_length())
        assert len(t) == M.packed_size(4 * w, w, d) and M.decode(t, 65536) == verdict
    # d = 1025 in a full segment
    L = 65536
    t = bytearray([0x60 | lg, 0, 0xFF, 0xFF, 0x00, 0x04]) + \
        bytes(M.packed_size(L, w, 1025) - 6)
    assert M.decode(t, L) is None
    t[4:6] = bytes([0xFF, 0x03])  # 1024 entries, all the same: accepted when the size fits
    if 1024 <= L // w:
        t = t[:M.packed_size(L, w, 1024)]
        assert M.decode(t, L) == bytes(L)
    # a d that changes b: the size no longer fits
    s, _ = packed_example(w, d=5)
    for d in (2, 4, 9):
        t = bytearray(s)
        t[4] = d - 1
        assert M.decode(t, 65536) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_size_mismatch(w):
    s, _ = packed_example(w)
    for t in (s + b"\0", s[:-1], s + bytes(8), s[:6]):
        assert M.decode(t, 65536) is None
    stored = M.encode_segment(rnd(100, 2), w)
    for t in (stored + b"\0", stored[:-1], stored[:4]):
        assert M.decode(t, 65536) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_an_index_that_is_no_entry(w):
    s, _ = packed_example(w, d=5, m=200)  # b = 3: indices 5, 6, 7 are no entries
    pay = 6 + 5 * w

    def with_index(t, value):
        u = bytearray(s)
        k, bit = divmod(t, 64)
        for j in range(3):
            at = pay + k * 24 + (bit * 3 + j) // 8
            u[at] = u[at] & ~(1 << (bit * 3 + j) % 8) | (value >> j & 1) << (bit * 3 + j) % 8
        return u

    for t in (0, 63, 64, 199):
        assert M.decode(with_index(t, 4), 65536) is not None
        for bad in (5, 7):
            assert M.decode(with_index(t, bad), 65536) is None
    for t in (200, 255):  # slots past m: ignored
        assert M.decode(with_index(t, 7), 65536) == M.decode(s, 65536)


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_accepts_duplicate_entries(w):
    s, data = packed_example(w, d=5, m=200, tail=0)
    s[6 + w:6 + 2 * w] = s[6:6 + w]  # entry 1 = entry 0
    want = data.reshape(200, w).copy()
    want[1::5] = want[0]
    assert M.decode(s, 65536) == want.tobytes()


# ---- the library's surface --------------------------------------------------------------------

def test_library_surface():
    import bitar_amd as B
    assert (B.CODEC_DICTPACK32, B.CODEC_DICTPACK64, B.CODEC_DICTPACK128) == (26, 27, 28)
    assert [B.codec_dictpack(w) for w in M.WIDTHS] == [26, 27, 28]
    for bad in (0, 1, 2, 3, 5, 32, None, "8"):
        with pytest.raises(ValueError):
            B.codec_dictpack(bad)
    for codec in (26, 27, 28):
        assert B.slot_size(codec, 65536) == 65792
        assert B.slot_size(codec, 1) == 256
        assert B.slot_size(codec, 59460) == 59648
        assert B.max_distance(codec) == 0
    for unknown in (24, 25, 7, 12, 16, 17, 20, 29, 99):
        assert B.slot_size(unknown, 100) == 0 and B.max_distance(unknown) == 0


def test_abi_is_untouched():
    import bitar_amd as B
    import test_abi
    assert B.lib().bitar_hip_abi_version() == 3
    assert sorted(B.ABI_SYMBOLS) == test_abi.header_symbols() and len(B.ABI_SYMBOLS) == 39
    assert not [s for s in B.ABI_SYMBOLS if "dictpack" in s]
