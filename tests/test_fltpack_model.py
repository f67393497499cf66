"""CPU tests of the FLTPACK model (fltpack_model.py): hand-written streams that pin the field
and bit order, round trips over decimal columns and every kind of exception, every reject rule
of the decoder, the ratio and stored conditions, and the library's surface.  No GPU."""
import numpy as np
import pytest

import fltpack_model as M

F = {4: np.dtype("<f4"), 8: np.dtype("<f8")}
U = {4: np.dtype("<u4"), 8: np.dtype("<u8")}


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def decimal_column(m, w, e, seed):
    """m elements that are integers over 10^e, as the parser of a decimal text would give them"""
    rng = np.random.default_rng(seed)
    span = 10 ** min(e + 3, 6 if w == 4 else 9)
    n = rng.integers(-span, span, m)
    return (n / 10.0 ** e).astype(F[w])


def specials(w):
    """NaNs with distinct payloads, the infinities, -0.0, denormals, 0.1 + 0.2, the largest
    encodable integers and one step beyond each"""
    f = F[w]
    if w == 8:
        nans = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000,
                         0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF], "<u8").view(f)
        edge = np.array([2.0 ** 53, -2.0 ** 53, 2.0 ** 53 + 2, -(2.0 ** 53) - 2, 2.0 ** 53 - 1], f)
        den = np.array([5e-324, -5e-324, 2.2250738585072009e-308], f)
    else:
        nans = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001, 0x7FFFFFFF],
                        "<u4").view(f)
        # (2^31 - 1 is no float: the largest float below it, and 2^31 itself)
        edge = np.array([2147483520.0, -2147483520.0, 2147483648.0, -2147483648.0], f)
        den = np.array([1e-45, -1e-45, 1.1754942e-38], f)
    rest = np.array([np.inf, -np.inf, -0.0, 0.0, 0.1 + 0.2, 1.0, -1.0, 1e15, 1e16, 1e300 if w == 8
                     else 1e38, 1 / 3], f)
    return np.concatenate([nans, edge, den, rest])


def roundtrip(data, w, seg=65536):
    data = as_bytes(data)
    streams = M.encode(data, w, seg)
    assert len(streams) == (data.size + seg - 1) // seg
    back = b"".join(M.decode(s, seg) for s in streams)
    assert back == data.tobytes()
    for i, s in enumerate(streams):
        L = min(seg, data.size - i * seg)
        assert s[0] >> 4 == 5 and (s[0] & 3) == (2 if w == 4 else 3)
        assert len(s) <= 4 + L
        assert mode_of(s) == 2 or len(s) < 4 + L
        assert mode_of(s) == 0 or s[1] == 0
    return streams


def mode_of(s):
    return (s[0] >> 2) & 3


def nx_of(s):
    return s[4] | s[5] << 8


# ---- hand-written streams ----------------------------------------------------------------------

def test_golden_packed_double():
    """64 doubles 10.01 .. 10.08 repeating (n = 1001 + i % 8 at e = 2), element 5 a NaN with a
    payload, 3 tail bytes: 3-bit residuals 0..7 pack as 0xFAC688 little-endian, the exception's
    slot packs 0"""
    v = ((1001 + np.arange(64) % 8) / 100.0).astype("<f8")
    u = v.view("<u8").copy()
    u[5] = 0x7FF8000000000001
    data = np.concatenate([as_bytes(u), np.array([0xAA, 0xBB, 0xCC], np.uint8)])
    want = bytes([0x53, 0x02, 0x02, 0x02,              # tag: packed, log2 w = 3; e = 2; L - 1 = 514
                  0x01, 0x00,                          # nx
                  0x03,                                # the miniblock's width
                  0xE9, 0x03, 0, 0, 0, 0, 0, 0,        # ref = 1001
                  0x88, 0x46, 0xF8]                    # residuals 0 1 2 3 4 (0) 6 7
                 + [0x88, 0xC6, 0xFA] * 7
                 + [0x05, 0x00,                        # pos
                    0x01, 0, 0, 0, 0, 0, 0xF8, 0x7F,   # val
                    0xAA, 0xBB, 0xCC])                 # tail
    assert len(want) == 6 + 1 + 8 + 8 * 3 + 1 * (2 + 8) + 3
    assert M.encode(data, 8, 4096) == [want]
    assert M.packed_size(data, 8) == len(want)
    assert M.decode(want, 515) == data.tobytes()


def test_golden_packed_float():
    """65 floats -0.3 .. 0.0 repeating (n = -3 + i % 4 at e = 1; the reference is negative), a
    second miniblock of one element (0.0, residual 3), no exception"""
    f = ((np.arange(65) % 4 - 3) / 10).astype("<f4")
    f[64] = 0.0
    want = bytes([0x52, 0x01, 0x03, 0x01,              # tag: packed, log2 w = 2; e = 1; L - 1 = 259
                  0x00, 0x00,                          # nx
                  0x02, 0x02,                          # widths
                  0xFD, 0xFF, 0xFF, 0xFF]              # ref = -3
                 + [0xE4] * 16                         # residuals 0 1 2 3
                 + [0x03] + [0] * 15)                  # residual 3, then padding
    assert M.encode(as_bytes(f), 4, 4096) == [want]
    assert M.decode(want, 260) == f.tobytes()


def test_golden_stored_streams():
    data = as_bytes(np.array([0.1 + 0.2], "<f8"))      # 17 significant digits: no e <= 15 fits
    want = bytes([0x5B, 0x00, 0x07, 0x00, 0x34, 0x33, 0x33, 0x33, 0x33, 0x33, 0xD3, 0x3F])
    assert M.encode(data, 8, 4096) == [want]
    assert M.decode(want, 8) == data.tobytes()
    data = np.array([1, 2, 3], np.uint8)               # shorter than a float: m = 0
    want = bytes([0x5A, 0x00, 0x02, 0x00, 1, 2, 3])
    assert M.encode(data, 4, 4096) == [want]
    assert M.decode(want, 3) == data.tobytes()


# ---- round trips ---------------------------------------------------------------------------------

@pytest.mark.parametrize("w", M.WIDTHS)
@pytest.mark.parametrize("e", (0, 1, 2, 6))
def test_decimal_columns_pack_without_exceptions(w, e):
    col = decimal_column(65536 // w + 100, w, e, 10 * e + w)
    streams = roundtrip(col, w)
    assert [mode_of(s) for s in streams] == [0, 0]
    assert [s[1] for s in streams] == [e, e]
    assert [nx_of(s) for s in streams] == [0, 0]


@pytest.mark.parametrize("w", M.WIDTHS)
def test_specials_are_exceptions(w):
    sp = specials(w)
    col = decimal_column(1024, w, 2, w)
    at = np.arange(sp.size) * 37 + 3
    col[at] = sp
    (s,) = roundtrip(col, w)
    assert mode_of(s) == 0 and s[1] == 2
    ok, n = M.to_int(col.view(U[w]), w, 2)
    assert nx_of(s) == int((~ok).sum())
    # what must be an exception whatever the exponent
    never = [i for i, v in enumerate(sp) if np.isnan(v) or np.isinf(v) or
             (v == 0 and np.signbit(v)) or (v != 0 and abs(v) < np.finfo(F[w]).tiny)]
    assert len(never) >= 11
    for e in range(16):
        ok, _ = M.to_int(sp.view(U[w]), w, e)
        assert not ok[never].any()
    ok, _ = M.to_int(np.array([0.1 + 0.2], "<f8").view("<u8"), 8, 15)
    assert not ok[0]


def test_limits():
    """|t| <= 2^53 for doubles, <= 2^31 - 1 for floats: at the limit encodable, beyond it not"""
    u = np.array([2.0 ** 53, -2.0 ** 53, 2.0 ** 53 + 2, -(2.0 ** 53) - 2], "<f8").view("<u8")
    ok, n = M.to_int(u, 8, 0)
    assert ok.tolist() == [True, True, False, False]
    assert n.tolist() == [2 ** 53, -2 ** 53, 0, 0]
    ok, _ = M.to_int(u, 8, 1)
    assert not ok.any()
    # floats: 2^31 - 1 is no float; the largest float below it is encodable, the next one,
    # 2^31, is one step beyond the limit
    f = np.array([2147483520.0, -2147483520.0, 2147483648.0, -2147483648.0], "<f4")
    assert np.nextafter(f[0], np.float32(np.inf)) == f[2]
    ok, n = M.to_int(f.view("<u4"), 4, 0)
    assert ok.tolist() == [True, True, False, False]
    assert n.tolist() == [2147483520, -2147483520, 0, 0]
    ok, _ = M.to_int(f.view("<u4"), 4, 1)
    assert not ok.any()
    col = np.arange(512, dtype="<f4")
    col[1:5] = f  # (outside the sample, which then chooses e = 0)
    (s,) = roundtrip(col, 4)
    assert mode_of(s) == 0 and s[1] == 0 and nx_of(s) == 2
    # (n + 2147483520: 2^32 - 256 in miniblock 0, below 2^31 only in miniblock 1)
    assert list(s[6:14]) == [32, 31, 32, 32, 6, 7, 8, 8]
    # a block whose only encodable element has n = 2^31 - 1, the largest signed value: the
    # reference is that value, not 0
    ok = np.zeros(256, bool)
    ok[7] = True
    n = np.zeros(256, "<i4")
    n[7] = 2 ** 31 - 1
    widths, refs, r = M._plan(ok, n, 4)
    assert refs.tolist() == [2 ** 31 - 1] and widths.tolist() == [0] * 4


@pytest.mark.parametrize("w", M.WIDTHS)
def test_block_of_exceptions_only(w):
    col = decimal_column(1024, w, 1, 5 + w)
    col[256:512] = np.nan
    col.view(U[w])[256:512] += np.arange(256, dtype=U[w])  # distinct payloads
    data = as_bytes(col)
    s = M._packed(data, w, 1)
    assert nx_of(s) == 256 and list(s[6:22][4:8]) == [0] * 4
    refs = np.frombuffer(s[22:22 + 4 * w], U[w])
    assert refs[1] == 0 and refs[0] != 0
    assert M.decode(s, data.size) == data.tobytes()
    roundtrip(col, w)
    allx = np.full(256, np.inf, F[w])                      # a whole segment of them: stored
    (s,) = roundtrip(allx, w)
    assert mode_of(s) == 2


@pytest.mark.parametrize("w", M.WIDTHS)
def test_lengths(w):
    col = decimal_column(65536 // w, w, 2, w)
    col[::97] = np.nan
    data = as_bytes(col)
    for L in (1, w - 1, w, w + 1, 64 * w, 64 * w + 1, 256 * w, 256 * w + w, 59460, 65536):
        (s,) = roundtrip(data[:L], w)
        assert (mode_of(s) == 2) == (L < 64 * w), L
        (s,) = roundtrip(data[data.size - L:], w)
    assert M.encode(np.zeros(0, np.uint8), w, 4096) == []
    # several segments with a short last one
    roundtrip(data[:3 * 4096 + 5], w, 4096)


def test_exponent_choice_per_segment():
    a = decimal_column(512, 8, 0, 1)
    b = decimal_column(512, 8, 3, 2)
    streams = roundtrip(np.concatenate([a, b]), 8, 4096)
    assert [s[1] for s in streams] == [0, 3]
    # a tie goes to the smallest e: a constant column costs 0 at every e that holds it
    (s,) = roundtrip(np.full(512, 2.5), 8)
    assert s[1] == 1
    # mostly 1-decimal with a few 3-decimal values: the exceptions are cheaper than the bits
    col = decimal_column(8192, 8, 1, 3)
    col[5::16 * 40] = 0.125
    (s,) = roundtrip(col, 8)
    assert s[1] == 1 and nx_of(s) == len(col[5::16 * 40])


# ---- the decoder's reject rules, one mutation apiece -------------------------------------------

def valid_stream(w=8):
    col = decimal_column(1024, w, 2, 20 + w)
    col[[3, 64, 700, 1023]] = np.nan
    data = np.concatenate([as_bytes(col), np.array([1, 2, 3], np.uint8)[:w - 1]])
    (s,) = M.encode(data, w, 65536)
    assert mode_of(s) == 0 and nx_of(s) == 4 and M.decode(s, data.size) == data.tobytes()
    return bytearray(s), data


def pos_at(s, w):
    L = 1 + s[2] + (s[3] << 8)
    m, nmb, nblk = M._counts(L, w)
    return 6 + nmb + nblk * w + 8 * sum(s[6:6 + nmb])


def mutated(s, at, value):
    t = bytearray(s)
    t[at] = value & 255
    return t


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_tag(w):
    s, data = valid_stream(w)
    for tag in (s[0] & 0x0F, 0x40 | (s[0] & 15), 0x60 | (s[0] & 15), s[0] | 0x80):  # high nibble
        assert M.decode(mutated(s, 0, tag), data.size) is None
    for mode in (1, 3):
        assert M.decode(mutated(s, 0, (s[0] & 0xF3) | mode << 2), data.size) is None
    for lg in (0, 1):
        assert M.decode(mutated(s, 0, (s[0] & 0xFC) | lg), data.size) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_exponent(w):
    s, data = valid_stream(w)
    for e in (16, 0x80, 0xFF):
        assert M.decode(mutated(s, 1, e), data.size) is None
    assert M.decode(mutated(s, 1, 15), data.size) is not None
    stored = M.encode(as_bytes(np.array([np.inf] * 4, F[w])), w, 4096)[0]
    assert mode_of(stored) == 2 and M.decode(stored, 4 * w) is not None
    assert M.decode(mutated(stored, 1, 1), 4 * w) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_length_above_the_segment(w):
    s, data = valid_stream(w)
    assert M.decode(s, data.size - 1) is None and M.decode(s, data.size) is not None
    stored = M.encode(as_bytes(np.array([np.inf] * 4, F[w])), w, 4096)[0]
    assert M.decode(stored, 4 * w - 1) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_exception_count_above_the_elements(w):
    data = as_bytes(decimal_column(2, w, 1, 1))
    s = bytearray(M._packed(data, w, 1))
    assert M.decode(s, 4096) == data.tobytes()
    # nx = 3 > m = 2, with the bytes the size formula then asks for
    t = mutated(s, 4, 3) + bytes(3 * (2 + w))
    assert M.decode(t, 4096) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_width_above_the_element(w):
    s, data = valid_stream(w)
    for bad in (8 * w + 1, 255):
        for k in (0, 15):
            assert M.decode(mutated(s, 6 + k, bad), data.size) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_positions(w):
    s, data = valid_stream(w)
    p = pos_at(s, w)
    assert [s[p + 2 * i] | s[p + 2 * i + 1] << 8 for i in range(4)] == [3, 64, 700, 1023]
    assert M.decode(mutated(s, p + 7, 4), data.size) is None       # 1023 -> 1024 + 255 >= m
    assert M.decode(mutated(s, p + 2, 3), data.size) is None       # 64 -> 3: equal to the one before
    assert M.decode(mutated(s, p + 2, 2), data.size) is None       # 64 -> 2: below it
    assert M.decode(mutated(s, p, 65), data.size) is None          # 3 -> 65: above the next
    ok = M.decode(mutated(s, p + 2, 65), data.size)                # 64 -> 65: still in order
    assert ok is not None and ok != data.tobytes()


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_size_mismatch(w):
    s, data = valid_stream(w)
    assert M.decode(s + b"\0", data.size) is None
    assert M.decode(s[:-1], data.size) is None
    for n in (0, 3, 4, 5, 6):
        assert M.decode(s[:n], data.size) is None
    assert M.decode(mutated(s, 6, s[6] - 1), data.size) is None    # a valid width, another sum
    assert M.decode(mutated(s, 4, s[4] + 1), data.size) is None    # one more exception
    stored = M.encode(as_bytes(np.array([np.inf] * 4, F[w])), w, 4096)[0]
    assert M.decode(stored + b"\0", 4096) is None and M.decode(stored[:-1], 4096) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_accepts_any_residual_bits(w):
    """arithmetic is mod 2^(8w), any n converts and divides, residuals at exception slots are
    ignored"""
    s, data = valid_stream(w)
    p = pos_at(s, w)
    m, nmb, nblk = M._counts(data.size, w)
    pay = 6 + nmb + nblk * w
    rng = np.random.default_rng(w)
    t = bytearray(s)
    t[pay:p] = rng.integers(0, 256, p - pay, dtype=np.uint8).tobytes()
    t[6 + nmb:pay] = rng.integers(0, 256, nblk * w, dtype=np.uint8).tobytes()   # the references
    out = M.decode(t, data.size)
    assert out is not None and len(out) == data.size
    got, want = np.frombuffer(out, np.uint8), data
    for i in (3, 64, 700, 1023):
        assert np.array_equal(got[i * w:(i + 1) * w], want[i * w:(i + 1) * w])
    assert np.array_equal(got[1024 * w:], want[1024 * w:])
    # a residual at an exception's slot alone changes nothing
    t = bytearray(s)
    b = s[6]
    assert b > 0
    bit = 3 * b                                                    # element 3's field
    t[pay + bit // 8] ^= 1 << (bit % 8)
    assert t != s and M.decode(t, data.size) == data.tobytes()


# ---- conditions ----------------------------------------------------------------------------------

def test_price_column_packs_below_a_third():
    """8192 doubles round(uniform(0, 1000), 2): 17 bits a value plus headers"""
    col = np.round(np.random.default_rng(2024).uniform(0, 1000, 8192), 2)
    (s,) = roundtrip(col, 8)
    print(f"prices: {len(s)} B of 65536, ratio {65536 / len(s):.2f}")
    assert mode_of(s) == 0 and s[1] == 2 and nx_of(s) == 0
    assert 3 * len(s) < 65536


def test_normal_doubles_are_stored():
    col = np.random.default_rng(7).normal(0, 1, 2 * 8192 + 100)
    streams = roundtrip(col, 8)
    data = as_bytes(col)
    for i, s in enumerate(streams):
        L = min(65536, data.size - i * 65536)
        assert mode_of(s) == 2 and len(s) == 4 + L
        assert s[4:] == data[i * 65536:i * 65536 + L].tobytes()


def test_library_surface():
    import bitar_amd as B
    assert (B.CODEC_FLTPACK32, B.CODEC_FLTPACK64) == (18, 19)
    assert [B.codec_fltpack(w) for w in M.WIDTHS] == [18, 19]
    for bad in (0, 1, 2, 3, 16, None, "8"):
        with pytest.raises(ValueError):
            B.codec_fltpack(bad)
    for codec in (18, 19):
        assert B.slot_size(codec, 65536) == 65792
        assert B.slot_size(codec, 1) == 256
        assert B.slot_size(codec, 59460) == 59648
        assert B.max_distance(codec) == 0
    for unknown in (7, 12, 16, 17, 20, 99):
        assert B.slot_size(unknown, 100) == 0 and B.max_distance(unknown) == 0
