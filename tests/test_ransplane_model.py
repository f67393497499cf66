"""The RANSPLANE format on the CPU: the numpy model (ransplane_model.py) against streams worked
out by hand from the format's rules, the cross-check sizes, every reject and accept rule on its
own, the tie, round trips, the sizes against shuffle + RANS on the inputs of DESIGN 4.26's table,
and the library's surface (ids, slots, reach)."""
import numpy as np
import pytest

import rans_model as R
import ransplane_cases as C
import ransplane_model as M

WIDTHS = M.WIDTHS
X0 = (1 << 16).to_bytes(4, "little")


# ---- worked examples ---------------------------------------------------------------------------

@pytest.mark.parametrize("w", WIDTHS)
def test_golden_stream_by_hand(w):
    """L = 2w + 1: plane 0 holds the bytes 0, w and 2w -- 'a', 'a', 'b' -- and plane p > 0 two bytes
    of the constant 0x10 + p.
    Plane 0: n = 3, nsym = 2, f = 1 + floor(c * 4094 / 3) = 2730 and 1365, the deficit 1 to 'a':
    2731 and 1365; cum 0 and 2731.  Plane p > 0: f = 4096, cum 0.
    One step (L <= 64), lane i has byte i, x = 2^16 everywhere and nobody emits (2^16 < f << 20).
      'a' (lanes 0 and w): 65536 = 23 * 2731 + 2723  ->  x = 23 * 4096 + 2723 + 0    =  96931
      'b' (lane 2w):       65536 = 48 * 1365 + 16    ->  x = 48 * 4096 + 16 + 2731   = 199355
      a constant:          65536 = 16 * 4096 + 0     ->  x = 16 * 4096 + 0 + 0       =  65536
    and the lanes past L keep 2^16.  freqs of plane 0: 2730 | 1364 << 12, 24 bits in 4 bytes; of a
    constant plane: 0xFFF in 2 bytes."""
    L = 2 * w + 1
    data = np.zeros(L, np.uint8)
    for p in range(1, w):
        data[p::w] = 0x10 + p
    data[[0, w, 2 * w]] = (97, 97, 98)
    f = M.normalise_planes(data, w)
    assert (f[0, 97], f[0, 98]) == (2731, 1365) and all(f[p, 0x10 + p] == 4096 for p in range(1, w))
    bitmaps = bytearray(32 * w)
    bitmaps[12] = 1 << (97 & 7) | 1 << (98 & 7)
    for p in range(1, w):
        bitmaps[32 * p + 2] = 1 << p  # 0x10 + p: byte 2, bit p
    freqs = (2730 | 1364 << 12).to_bytes(4, "little") + b"\xff\x0f" * (w - 1)
    states = [X0] * 64
    states[0] = states[w] = (96931).to_bytes(4, "little")
    states[2 * w] = (199355).to_bytes(4, "little")
    want = bytes([0xB0 | M.lg_of(w), 0, 2 * w, 0]) + bytes(bitmaps) + freqs + b"".join(states)
    s = M.planes_form(data, w)
    assert s == want and len(s) == 4 + 32 * w + 4 + 2 * (w - 1) + 256
    assert M.decode(s, L, w) == data.tobytes()  # (larger than 4 + L: no encoder writes it)
    assert M.encode_segment(data, w) == bytes([0xB8 | M.lg_of(w), 0, 2 * w, 0]) + data.tobytes()


@pytest.mark.parametrize("w", WIDTHS)
def test_golden_emission_order(w):
    """L = 128 zero bytes under f[0] = 1, f[1] = 4095 in every plane: step 1 runs first,
    2^16 >= 1 << 20 is false, x = 2^16 * 4096 = 2^28; step 0: every lane emits 0, x = 2^12, then
    2^24"""
    f = np.zeros((w, 256), np.int64)
    f[:, 0], f[:, 1] = 1, 4095
    data = np.zeros(128, np.uint8)
    words, states = M.encode_words(data, f)
    assert words.tolist() == [0] * 64 and states.tolist() == [1 << 24] * 64
    assert M.decode(M.planes_stream(128, f, words, states), 128, w) == bytes(128)


def test_a_lane_uses_its_plane_table():
    """two planes with the same two symbols and opposite frequencies: the words differ from those
    under either table alone"""
    rng = np.random.default_rng(3)
    data = np.where(rng.random(4096) < 0.9, 1, 2).astype(np.uint8)
    data[1::2] = 3 - data[1::2]  # plane 1: mostly 2
    f = M.normalise_planes(data, 2)
    assert f[0, 1] > 3000 and f[1, 2] > 3000
    s = M.encode_segment(data, 2)
    assert s[0] == 0xB1 and M.decode(s, 4096, 2) == data.tobytes()
    # one table sees a coin flip, 1 bit a byte: 512 bytes of words.  Two see H(0.9) = 0.47 bits:
    # 240 bytes, less the 36 bytes of the second bitmap and field
    assert len(s) < len(R.encode_segment(data)) - 200


# ---- the cross-check sizes ---------------------------------------------------------------------

@pytest.mark.parametrize("w", WIDTHS)
def test_cross_check_sizes(w):
    s = M.encode_segment(np.full(65536, 0x41, np.uint8), w)
    assert len(s) == 260 + 34 * w == {2: 328, 4: 396, 8: 532}[w]
    assert C.parts_of(s, w) == ([1] * w, [2] * w, 0)
    assert M.decode(s, 65536, w) == b"\x41" * 65536
    noise = np.random.default_rng(0).integers(0, 256, 65536, dtype=np.uint8)
    s = M.encode_segment(noise, w)
    assert len(s) == 65540 and s[0] == 0xB8 | M.lg_of(w)
    for L in (1, w - 1, w, 63, 64, 65, 127, 129):
        data = C.sparse(L, w, L)
        s = M.encode_segment(data, w)
        assert s == bytes([0xB8 | M.lg_of(w), 0, L - 1, 0]) + data.tobytes()
        assert M.decode(s, 4096, w) == data.tobytes()


# ---- the decoder's rules, each alone -----------------------------------------------------------

def poke(s, at, value):
    t = bytearray(s)
    t[at] = value & 255
    return bytes(t)


def stored_example(w):
    s = M.encode_segment(C.rnd(500, 1), w)
    assert s[0] == 0xB8 | M.lg_of(w)
    return s


@pytest.mark.parametrize("w", WIDTHS)
def test_decode_rejects_the_tag_and_byte_one(w):
    s, data = C.example(w)
    for nib in range(16):
        assert (M.decode(poke(s, 0, nib << 4 | s[0] & 15), 4096, w) == data) == (nib == 0xB)
    for lg in range(8):  # the width of the id alone
        for mode in (0, 8):
            t = poke(s, 0, 0xB0 | mode | lg)
            if lg != M.lg_of(w):
                assert M.decode(t, 4096, w) is None
    for other in WIDTHS:  # a stream of one width under another width's id
        if other != w:
            assert M.decode(s, 4096, other) is None
            assert M.decode(stored_example(w), 4096, other) is None
    for b1 in (1, 2, 0x80, 0xFF):
        assert M.decode(poke(s, 1, b1), 4096, w) is None
        assert M.decode(poke(stored_example(w), 1, b1), 4096, w) is None


@pytest.mark.parametrize("w", WIDTHS)
def test_decode_rejects_length_above_the_segment(w):
    s, data = C.example(w)
    assert M.decode(s, len(data), w) == data
    assert M.decode(s, len(data) - 1, w) is None
    stored = stored_example(w)
    assert M.decode(stored, 500, w) is not None and M.decode(stored, 499, w) is None


@pytest.mark.parametrize("w", WIDTHS)
def test_decode_rejects_sizes(w):
    s, data = C.example(w)
    for t in (s + b"\0", s[:-1], s[:-3], s + bytes(3), s[:3], b"", s[:M.fixed_size(w)],
              s[:M.fixed_size(w) + 2 * w - 1], s[:4 + 32 * w], s[:4 + 32 * w - 1]):
        assert M.decode(t, 4096, w) is None  # odd 2 * nw, a negative one, too short
    assert M.decode(s + b"\0\0", 4096, w) is None and M.decode(s[:-2], 4096, w) is None  # nw +- 1
    stored = stored_example(w)
    for t in (stored + b"\0", stored[:-1], stored[:4]):
        assert M.decode(t, 4096, w) is None
    # the smallest planes form: a symbol a plane, no words
    one = M.planes_form(np.zeros(w, np.uint8), w)
    assert len(one) == M.fixed_size(w) + 2 * w and M.decode(one, w, w) == bytes(w)
    assert M.decode(one[:-1], w, w) is None
    assert M.decode(one[:4 + 32 * w] + one[4 + 32 * w + 2:], w, w) is None


@pytest.mark.parametrize("w", WIDTHS)
def test_decode_rejects_a_planes_form_shorter_than_an_element(w):
    """L < w leaves a plane empty: no table describes it"""
    data = np.zeros(w, np.uint8)
    s = M.planes_form(data, w)
    assert M.decode(s, 4096, w) == bytes(w)
    for L in range(1, w):
        assert M.decode(s[:2] + bytes([L - 1, 0]) + s[4:], 4096, w) is None


@pytest.mark.parametrize("w", WIDTHS)
def test_decode_rejects_tables(w):
    s, data = C.example(w)
    f = C.frequencies_of(s, w)
    nsym, tsize, _ = C.parts_of(s, w)
    for p in range(w):
        bm = 4 + 32 * p
        assert M.decode(s[:bm] + bytes(32) + s[bm + 32:], 4096, w) is None  # an empty bitmap
        for d in (1, -1):  # the sum is 4097 and 4095
            g = f.copy()
            g[p, np.flatnonzero(f[p])[0]] += d
            if g[p].min() >= 0 and np.count_nonzero(g[p]) == nsym[p]:
                assert M.decode(C.with_frequencies(s, w, g), 4096, w) is None
        pad = (16 - 12 * nsym[p] % 16) % 16
        last = 4 + 32 * w + sum(tsize[:p + 1]) - 1
        for bit in range(8 - min(pad, 8), 8):  # the pad bits of the plane's field
            assert M.decode(poke(s, last, s[last] | 1 << bit), 4096, w) is None
        # one bit more in the bitmap: a symbol more, the fields are read differently
        absent = int(np.flatnonzero(f[p] == 0)[0])
        at = bm + (absent >> 3)
        assert M.decode(poke(s, at, s[at] | 1 << (absent & 7)), 4096, w) is None
    assert nsym[0] == 5 and (16 - 12 * nsym[0] % 16) % 16 == 4  # (pad bits were there to set)


@pytest.mark.parametrize("w", WIDTHS)
def test_decode_rejects_states_and_words(w):
    s, data = C.example(w)
    nsym, tsize, nw = C.parts_of(s, w)
    words_at = 4 + 32 * w + sum(tsize)
    at = words_at + 2 * nw
    for lane in (0, 17, 63):  # an initial state below 2^16
        t = s[:at + 4 * lane] + (0xFFFF).to_bytes(4, "little") + s[at + 4 * lane + 4:]
        assert M.decode(t, 4096, w) is None
    body = s[words_at:at]
    for k in (0, nw // 2, nw - 1):  # a word less: some refill finds none left; a word more: p != 0
        assert M.decode(s[:words_at] + body[:2 * k] + body[2 * k + 2:] + s[at:], 4096, w) is None
        assert M.decode(s[:words_at] + body[:2 * k] + b"\1\2" + body[2 * k:] + s[at:], 4096, w) is None
    # an altered word or state: the decoder does not land on 2^16
    assert M.decode(poke(s, words_at, s[words_at] ^ 1), 4096, w) is None
    assert M.decode(poke(s, at + 2, s[at + 2] ^ 1), 4096, w) is None
    # no words at all although the states need some
    assert M.decode(s[:words_at] + s[at:], 4096, w) is None


@pytest.mark.parametrize("w", WIDTHS)
def test_decode_accepts_non_canonical_streams(w):
    s, data = C.example(w)
    f = C.frequencies_of(s, w)
    arr = np.frombuffer(data, np.uint8)
    g = f.copy()  # any tables that sum to 4096
    present = np.flatnonzero(f[0])
    g[0, present[0]] += 5
    g[0, present[1]] -= 5
    t = M.planes_stream(arr.size, g, *M.encode_words(arr, g))
    assert t != s and M.decode(t, 4096, w) == data
    h = np.full((w, 256), 16, np.int64)  # tables with symbols the segment does not have
    t = M.planes_stream(arr.size, h, *M.encode_words(arr, h))
    assert M.decode(t, 4096, w) == data
    noise = C.rnd(300, 3)  # a planes form larger than 4 + L
    t = M.planes_form(noise, w)
    assert len(t) > 304 and M.decode(t, 300, w) == noise.tobytes()
    assert M.encode_segment(noise, w)[0] == 0xB8 | M.lg_of(w)


@pytest.mark.parametrize("w", WIDTHS)
def test_every_mutant_has_a_verdict(w):
    """the corpus of the GPU test (there over four streams a width): the model neither raises
    nor accepts a damaged stream unless the stream says the same"""
    s, data = C.example(w)
    muts = C.mutants(s, w)
    assert 150 < len(muts) < 900
    verdicts = [M.decode(t[:size] if size <= len(t) else t + b"\x5a" * (size - len(t)), 4096, w)
                for t, size in muts]
    assert verdicts[0] == data
    assert sum(v is None for v in verdicts) > 120 and sum(v is not None for v in verdicts) >= 3
    assert len({v for v in verdicts if v is not None}) > 1


# ---- the choice of form --------------------------------------------------------------------------

@pytest.mark.parametrize("w", WIDTHS)
def test_the_tie_is_stored(w):
    """16 symbols a plane: 4 bits a byte, so the planes form meets 4 + L near
    L = 2 * (4 + 32 w + 24 w + 256), or below it where a plane's few bytes have less than 4 bits
    each.  Among the lengths around it one gives a planes form of exactly
    4 + L bytes, which is stored, and one a form 2 bytes shorter, which is taken"""
    near = 2 * (4 + 56 * w + 256)
    found = {}
    for L in range(near - 400, near + 200):
        d = len(M.planes_form(C.tie_alphabet(L, w), w)) - (4 + L)
        if d in (0, -2) and d not in found:
            found[d] = L
    assert set(found) == {0, -2}, found
    data = C.tie_alphabet(found[0], w)
    s = M.encode_segment(data, w)
    assert s[0] == 0xB8 | M.lg_of(w) and len(s) == 4 + found[0]
    data = C.tie_alphabet(found[-2], w)
    s = M.encode_segment(data, w)
    assert s[0] == 0xB0 | M.lg_of(w) and len(s) == 4 + found[-2] - 2
    assert M.decode(s, 4096, w) == data.tobytes()


# ---- round trips and sizes -----------------------------------------------------------------------

@pytest.mark.parametrize("w", WIDTHS)
def test_round_trips(w):
    for L in (1, w - 1, w, w + 1, 63, 64, 65, 127, 128, 129, 4097, 59460, 65536):
        for data in (C.mixed(L, w, L), C.plane_shapes(L, w, L), C.sparse(L, w, L)):
            s = M.encode_segment(data, w)
            assert len(s) <= 4 + L and bool(s[0] & 8) == (len(s) == 4 + L)
            assert M.decode(s, 65536, w) == data.tobytes()
            if L >= w:
                t = M.planes_form(data, w)
                assert len(t) % 2 == 0 and M.decode(t, L, w) == data.tobytes()
    assert M.encode_segment(C.plane_shapes(65536, w, 2), w)[0] == 0xB0 | M.lg_of(w)


@pytest.mark.parametrize("w", WIDTHS)
def test_an_odd_segment_size_permutes_the_planes(w):
    """seg need not be a multiple of w: the planes of a segment that starts inside an element are
    the element's bytes rotated, and cost the same"""
    name = {2: "bf16 weights", 4: "float32 walk", 8: "float64 N(0, 1)"}[w]
    _, data = C.table_input(name, nseg=2, seg=59460 + 4)
    a = M.encode_segment(data[:59460], w)
    b = M.encode_segment(data[w - 1:w - 1 + 59460], w)
    assert a[0] == b[0] == 0xB0 | M.lg_of(w) and abs(len(a) - len(b)) < 0.005 * len(a)
    streams = M.encode(data, 59460, w)
    assert b"".join(M.decode(s, 59460, w) for s in streams) == data.tobytes()


@pytest.mark.parametrize("w", WIDTHS)
def test_a_late_bail_out_is_stored(w):
    data = C.near_noise(65536, w)
    t = M.planes_form(data, w)
    assert 4 + 65536 < len(t) < 1.06 * 65536
    assert M.encode_segment(data, w)[0] == 0xB8 | M.lg_of(w)


@pytest.mark.parametrize("name", list(C.TABLE_INPUTS))
def test_smaller_than_shuffle_and_rans(name):
    """DESIGN 4.26's ratio table: eight 64 KiB segments of each input; a table a plane is strictly
    smaller than RANS's one table over the same segments byte-shuffled at w"""
    w, data = C.table_input(name)
    planes = shuffled = 0
    for o in range(0, data.size, 65536):
        seg = data[o:o + 65536]
        s = M.encode_segment(seg, w)
        assert M.decode(s, 65536, w) == seg.tobytes()
        planes += len(s)
        shuffled += len(R.encode_segment(M.shuffle(seg, w)))
    print(f"{name}: width {w}, per-plane tables {data.size / planes:.3f}, "
          f"shuffle + RANS {data.size / shuffled:.3f}")
    assert planes < shuffled


# ---- the library's surface -----------------------------------------------------------------------

def test_library_surface():
    import bitar_amd as B
    import test_abi
    assert (B.CODEC_RANSPLANE16, B.CODEC_RANSPLANE32, B.CODEC_RANSPLANE64) == (81, 82, 83)
    assert B.COLUMN_CODECS["RANSPLANE"] == (80, 0xB, (2, 4, 8))
    assert [B.codec_ransplane(w) for w in WIDTHS] == [81, 82, 83]
    for codec in (81, 82, 83):
        assert tuple(B.slot_size(codec, seg) for seg in test_abi.SLOT_SEGS) == \
            (256, 256, 4352, 59648, 65792)
        assert B.max_distance(codec) == 0
    for unknown in (80, 84):
        assert B.slot_size(unknown, 100) == 0 and B.max_distance(unknown) == 0
    assert not hasattr(B, "CODEC_RANSPLANE8") and not hasattr(B, "CODEC_RANSPLANE128")
    for width in (1, 3, 16):
        with pytest.raises(ValueError) as e:
            B.codec_ransplane(width)
        assert str(e.value) == f"RANSPLANE element width must be 2, 4 or 8, not {width!r}"


def test_abi_is_untouched():
    import bitar_amd as B
    import test_abi
    assert B.lib().bitar_hip_abi_version() == 3
    assert sorted(B.ABI_SYMBOLS) == test_abi.header_symbols() and len(B.ABI_SYMBOLS) == 39
    assert B.CODEC_RANS == 72 and B.slot_size(B.CODEC_RANS, 4096) == 4352
