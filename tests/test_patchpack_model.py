"""The PATCHPACK model (patchpack_model.py) against streams worked out by hand, the width rule's
corners, INTPACK's stream on columns without outliers, the decoder's rejection rules one by one
and the ratios DESIGN.md 4.28 quotes.  No GPU."""
import numpy as np
import pytest

import intpack_model as IM
import patchpack_cases as C
import patchpack_model as M

U = {1: "<u1", 2: "<u2", 4: "<u4", 8: "<u8"}


def u8(values, w):
    return np.asarray(values).astype(U[w]).view(np.uint8)


def nx_of(s):
    return s[4] | s[5] << 8


def mode_of(s):
    return s[0] >> 2 & 3


# ---- streams worked out by hand ------------------------------------------------------------------

def test_golden_plain():
    """64 bytes 1, 2, 3, 4, ... with element 10 = 100: ref 1, residuals 0..3 and one of 99; at
    width 2 the cost is 16 + 3, at width 7 it is 56, at width 1 8 + 3 * 32"""
    v = np.tile([1, 2, 3, 4], 16)
    v[10] = 100
    s = M.encode_segment(u8(v, 1), 1)
    want = bytes.fromhex("90003f00" "0100" "02" "01") + \
        bytes.fromhex("e4e4c4e4") + bytes.fromhex("e4") * 12 + bytes.fromhex("0a00" "64")
    assert s == want and len(s) == 27
    assert M.decode(s, 64) == u8(v, 1).tobytes()


def test_golden_complement():
    """64 bytes 101..104 with element 10 = 0: plain needs 7 bits for all; the complements are
    154..151 and 255, ref 151, residuals 3..0 and one of 104"""
    v = np.tile([101, 102, 103, 104], 16)
    v[10] = 0
    s = M.encode_segment(u8(v, 1), 1)
    want = bytes.fromhex("9c003f00" "0100" "02" "97") + \
        bytes.fromhex("1b1b0b1b") + bytes.fromhex("1b") * 12 + bytes.fromhex("0a00" "ff")
    assert s == want
    assert M.decode(s, 64) == u8(v, 1).tobytes()
    assert M.packed_sizes(u8(v, 1), 1)[0] == 6 + 1 + 1 + 56


def test_golden_delta():
    """64 int16 1000, 1003, ... with a gap of 5000 before element 20: every delta is 3 but one of
    5003: width 0 and one exception"""
    v = 1000 + 3 * np.arange(64)
    v[20:] += 5000
    s = M.encode_segment(u8(v, 2), 2)
    want = bytes.fromhex("95007f00" "0100" "e803" "00" "0300" "1400" "8b13")
    assert s == want
    assert M.decode(s, 128) == u8(v, 2).tobytes()


def test_delta_exceptions_at_elements_0_and_1():
    """a gap before element 1: x_1 is an exception and so is x_0, its copy; the decoder takes
    element 0 from the base and ignores the exception there, whatever it holds"""
    v = 1000 + 3 * np.arange(64)
    v[1:] += 5000
    s = M.encode_segment(u8(v, 2), 2)
    want = bytes.fromhex("95007f00" "0200" "e803" "00" "0300" "00000100" "8b138b13")
    assert s == want
    assert M.decode(s, 128) == u8(v, 2).tobytes()
    t = bytearray(s)
    t[-4:-2] = b"\x55\xaa"  # the exception at position 0
    assert M.decode(bytes(t), 128) == u8(v, 2).tobytes()
    one = M.encode_segment(u8([7], 2), 2)  # m = 1: stored
    assert one == bytes.fromhex("99000100" "0700")
    assert M.decode(M.packed_stream(u8([7], 2), 2, 1), 2) == u8([7], 2).tobytes()


def test_stored_forms():
    rng = np.random.default_rng(1)
    for w in M.WIDTHS:
        noise = rng.integers(0, 256, 4096, dtype=np.uint8)
        s = M.encode_segment(noise, w)
        assert s == bytes([0x98 | M.WIDTHS.index(w), 0, 0xFF, 0x0F]) + noise.tobytes()
        for L in range(1, w):  # m = 0
            s = M.encode_segment(noise[:L], w)
            assert len(s) == 4 + L and mode_of(s) == 2 and M.decode(s, 8) == noise[:L].tobytes()


# ---- the width rule --------------------------------------------------------------------------------

def rule(lengths, w):
    bl = np.zeros((1, 64), np.int64)
    bl[0, :len(lengths)] = lengths
    return int(M.rule_widths(bl, w)[0])


def test_a_cost_tie_keeps_the_larger_width():
    """w = 4, an exception costs 6 bytes: four elements 3 bits above the rest cost 4 * 6 = 8 * 3"""
    assert rule([5] * 59 + [0] + [8] * 4, 4) == 8
    assert rule([5] * 60 + [0] + [8] * 3, 4) == 5   # 18 < 24
    assert rule([5] * 58 + [0] + [8] * 5, 4) == 8   # 30 > 24
    # through the writer: residuals of 5 bits, one 0, four of 8 bits
    v = np.full(64, 1000 + 31)
    v[0] = 1000
    v[[7, 8, 40, 63]] = 1000 + 255
    s = M.packed_stream(u8(v, 4), 4, 0)
    assert nx_of(s) == 0 and s[6] == 8
    v[7] = 1000 + 31
    s = M.packed_stream(u8(v, 4), 4, 0)
    assert nx_of(s) == 3 and s[6] == 5
    # w = 8, 10 bytes: four elements 5 bits above the rest, 40 = 8 * 5
    assert rule([3] * 60 + [8] * 4, 8) == 8 and rule([3] * 61 + [8] * 3, 8) == 3
    # a tie between two widths below B: the larger one
    # w = 2, 4 bytes: lengths 1 (x58), 3 (x2), 12 (x1): cost(1) = 8 + 12, cost(3) = 24 + 4
    assert rule([1] * 58 + [3, 3, 12], 2) == 1
    # w = 2: lengths 2 (x60), 3 (x2), 12: cost(2) = 16 + 12 = cost(3) = 24 + 4 = 28 -> 3
    assert rule([2] * 60 + [3, 3, 12], 2) == 3


def test_the_rule_against_an_enumeration():
    rng = np.random.default_rng(3)
    for w in M.WIDTHS:
        for _ in range(200):
            c = int(rng.integers(1, 65))
            top = int(rng.integers(0, 8 * w + 1))
            lengths = rng.integers(0, top + 1, c)
            if rng.random() < 0.5:
                lengths[rng.integers(0, c, rng.integers(0, 5))] = 8 * w
            B = int(lengths.max())
            costs = [8 * b + (2 + w) * int((lengths > b).sum()) for b in range(B + 1)]
            want = max(b for b in range(B + 1) if costs[b] == min(costs))
            assert rule(lengths, w) == want


def test_width_zero_with_exceptions():
    """a constant column with two outliers: every width 0, the outliers behind an empty payload"""
    v = np.full(256, 7)
    v[[3, 200]] = 1000
    s = M.encode_segment(u8(v, 4), 4)
    assert s == bytes.fromhex("9200ff03" "0200" "00000000" "07000000" "0300c800" "e8030000e8030000")
    assert M.decode(s, 1024) == u8(v, 4).tobytes()


def test_residuals_of_64_bits():
    """w = 8: a residual of bit length 64 is an exception like any other, and a miniblock whose
    residuals are all that long has width 64"""
    lo, hi = -2**63, 2**63 - 1
    v = lo + (np.arange(64) & 3).astype(object)
    v[5] = hi
    seg = np.array([int(x) & (2**64 - 1) for x in v], np.uint64).view(np.uint8)
    s = M.packed_stream(seg, 8, 0)
    assert s[6] == 2 and nx_of(s) == 1 and s[-10:] == bytes.fromhex("0500" "ffffffffffffff7f")
    assert M.decode(s, 512) == seg.tobytes()
    v = np.where(np.arange(64) & 1, hi, lo).astype(object)  # 32 exceptions of 10 bytes < 512
    seg = np.array([int(x) & (2**64 - 1) for x in v], np.uint64).view(np.uint8)
    s = M.packed_stream(seg, 8, 0)
    assert s[6] == 0 and nx_of(s) == 32 and M.decode(s, 512) == seg.tobytes()
    v[::2] = [lo + (k << 58) for k in range(32)]  # no two alike: 8 B = 512 against 10 * 63
    v[0] = lo
    seg = np.array([int(x) & (2**64 - 1) for x in v], np.uint64).view(np.uint8)
    s = M.packed_stream(seg, 8, 0)
    assert s[6] == 64 and nx_of(s) == 0 and len(s) == 6 + 1 + 8 + 512
    assert M.decode(s, 512) == seg.tobytes()


# ---- against INTPACK ---------------------------------------------------------------------------------

def test_without_outliers_it_is_intpacks_stream():
    """tag nibble 9 for 4 and LE16(0) behind the header: nothing else differs"""
    rng = np.random.default_rng(5)
    seen = set()
    cols = [(4, C.uniform(rng, 65536)), (4, C.uniform(rng, 59460)),
            (8, (10**12 + np.cumsum(rng.integers(100, 164, 8192))).astype("<i8").view(np.uint8)),
            (2, (np.cumsum(rng.integers(0, 16, 500)) % 65536).astype("<u2").view(np.uint8)),
            (1, rng.integers(16, 32, 999).astype(np.uint8))]
    for w, col in cols:
        i = IM.encode_segment(col, w)
        s = M.encode_segment(col, w)
        assert nx_of(s) == 0 and mode_of(s) in (0, 1)
        assert s == bytes([i[0] ^ 0xD0]) + i[1:4] + b"\0\0" + i[4:]
        seen.add(mode_of(s))
    assert seen == {0, 1}


def test_never_more_than_two_bytes_above_intpack():
    rng = np.random.default_rng(6)
    cols = [(w, col) for _, w, col in C.table_columns()]
    cols += [(w, rng.integers(0, 256, n, dtype=np.uint8)) for w in M.WIDTHS for n in (1, 63, 4096)]
    cols += [(w, col[:n]) for w, col in cols[:6] for n in (7, 72, 999, 4096)]
    for w, col in cols:
        for ww in {w, 1, 8}:
            s, i = M.encode_segment(col, ww), IM.encode_segment(col, ww)
            assert len(s) <= len(i) + 2 and len(s) <= 4 + col.size
            assert M.decode(s, col.size) == col.tobytes()


# ---- the decoder ---------------------------------------------------------------------------------------

def sample(w, mode, L=None):
    """a packed stream of the given mode with exceptions, a tail where w allows one"""
    rng = np.random.default_rng(w + mode)
    m = 300
    if mode == 1:
        step = rng.integers(1, 8, m)
        step[[1, 64, 127, 299]] = 50 if w == 1 else 5000
        v = (np.cumsum(step) + 17) & ((1 << min(8 * w, 62)) - 1)
    else:
        v = rng.integers(0, 16, m) + (40 if w == 1 else 10000)
        v[[0, 63, 64, 200, 299]] = (1 << (8 * w - 1)) - 1 if mode == 0 else 0
    seg = np.concatenate([u8(v, w), rng.integers(0, 256, min(3, w - 1), dtype=np.uint8)])
    s = M.encode_segment(seg, w)
    assert mode_of(s) == mode and nx_of(s) >= 4
    return seg, s


@pytest.mark.parametrize("w", M.WIDTHS)
def test_rejections_one_by_one(w):
    for mode in M.MODES:
        seg, s = sample(w, mode)
        L, m = seg.size, seg.size // w
        nmb, nblk = (m + 63) // 64, ((m + 63) // 64 + 3) // 4
        nx = nx_of(s)
        assert M.decode(s, L) == seg.tobytes() and M.decode(s, L + 1) == seg.tobytes()

        def poke(at, value, base=s):
            t = bytearray(base)
            t[at] = value
            return bytes(t)

        for nib in range(16):  # a high nibble other than 9
            assert (M.decode(poke(0, nib << 4 | s[0] & 15), L) is None) == (nib != 9)
        for v in (1, 0x80, 0xFF):  # byte 1
            assert M.decode(poke(1, v), L) is None
        assert M.decode(s, L - 1) is None  # L > seg
        for cut in (0, 3, 5, 6, 6 + nmb, len(s) - 1):  # too short
            assert M.decode(s[:cut], L) is None
        assert M.decode(s + b"\0", L) is None  # and too long
        wid_at = 6 + (w if mode == 1 else 0)
        for k in (0, nmb - 1):  # a width above 8w; one changed within range (the size is off)
            assert M.decode(poke(wid_at + k, 8 * w + 1), L) is None
            assert M.decode(poke(wid_at + k, 0xFF), L) is None
            assert M.decode(poke(wid_at + k, s[wid_at + k] + 1), L) is None
        for bad in (m + 1, 65535):  # nx > m, with the size to match or not
            t = poke(4, bad & 255)
            t = poke(5, bad >> 8, t)
            assert M.decode(t, L) is None
            assert M.decode(t + bytes((bad - nx) * (2 + w)), L) is None
        assert M.decode(poke(4, s[4] + 1), L) is None  # nx + 1: the size is off
        assert M.decode(poke(4, s[4] - 1), L) is None
        tail = L - m * w
        pos_at = len(s) - tail - nx * (2 + w)
        pos = np.frombuffer(s[pos_at:pos_at + 2 * nx], "<u2")

        def with_pos(p):
            return s[:pos_at] + np.asarray(p).astype("<u2").tobytes() + s[pos_at + 2 * nx:]

        assert M.decode(with_pos(pos), L) == seg.tobytes()
        for k in (0, nx - 1):  # a position at or past m
            for v in (m, m + 1, 65535):
                p = pos.copy()
                p[k] = v
                assert M.decode(with_pos(p), L) is None
        p = pos.copy()
        p[1] = p[0]  # equal neighbours
        assert M.decode(with_pos(p), L) is None
        p = pos.copy()
        p[[1, 2]] = p[[2, 1]]  # falling
        assert M.decode(with_pos(p), L) is None
        # the stored form: its size is 4 + L
        st = M._header(2, w, L) + seg.tobytes()
        assert M.decode(st, L) == seg.tobytes()
        assert M.decode(st + b"\0", L) is None and M.decode(st[:-1], L) is None
        assert M.decode(poke(1, 1, st), L) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_accepted_oddities(w):
    for mode in M.MODES:
        seg, s = sample(w, mode)
        L, m = seg.size, seg.size // w
        nmb = (m + 63) // 64
        # every mode that is not the smallest, and widths larger than needed
        for other in M.MODES:
            t = M.packed_stream(seg, w, other)
            assert M.decode(t, L) == seg.tobytes()
        wide = M.packed_stream(seg, w, mode, np.full(nmb, 8 * w, np.uint8))
        assert nx_of(wide) == 0 and len(wide) > 4 + L and M.decode(wide, L) == seg.tobytes()
        none = M.packed_stream(seg, w, mode, np.zeros(nmb, np.uint8))  # nearly all exceptions
        assert nx_of(none) > m // 2 and len(none) > 4 + L and M.decode(none, L) == seg.tobytes()
        # non-zero bits in an exception's slot: ignored.  Position 63 or 64 is one in every sample
        wid_at = 6 + (w if mode == 1 else 0)
        b0 = s[wid_at]
        if mode != 1:
            assert b0 > 0
            pay_at = wid_at + nmb + (nmb + 3) // 4 * w
            t = bytearray(s)
            t[pay_at + 8 * b0 - 1] |= 0x80  # the top bit of slot 63 of miniblock 0
            assert bytes(t) != s and M.decode(bytes(t), L) == seg.tobytes()
            t[pay_at] ^= 1 << (b0 % 8) if b0 < 8 else 0  # slot 1, no exception: other bytes
            if b0 < 8:
                assert M.decode(bytes(t), L) not in (None, seg.tobytes())
        # another value of an exception: other bytes, accepted
        t = bytearray(s)
        t[len(s) - (L - m * w) - 1] ^= 0x10
        assert M.decode(bytes(t), L) not in (None, seg.tobytes())


@pytest.mark.parametrize("w", M.WIDTHS)
def test_round_trips_at_the_borders(w):
    rng = np.random.default_rng(20 + w)
    for L in (1, w - 1, w, 63 * w, 64 * w, 65 * w, 256 * w, 257 * w, 59460, 65536):
        if L == 0:
            continue
        m = L // w
        for kind in range(4):
            if kind == 0:
                v = rng.integers(0, 50, m + 1)
                v[rng.random(m + 1) < 0.02] = (1 << (8 * w - 1)) - 1
            elif kind == 1:
                step = rng.integers(1, 9, m + 1)
                step[rng.random(m + 1) < 0.02] = 1 << (8 * w - 2)
                v = np.cumsum(step.astype(object)) % (1 << 8 * w)
                v = np.array([int(x) for x in v], np.uint64)
            elif kind == 2:
                v = (1 << (8 * w - 2)) + rng.integers(0, 50, m + 1)
                v[rng.random(m + 1) < 0.02] = 0
            else:
                v = rng.integers(0, 256, (m + 1) * w, dtype=np.uint8).view(U[w])
            seg = u8(v, w)[:L]
            s = M.encode_segment(seg, w)
            assert len(s) <= 4 + L and M.decode(s, L) == seg.tobytes()
            assert M.decode(s, 65536) == seg.tobytes()
            for mode in M.MODES:
                assert M.decode(M.packed_stream(seg, w, mode), L) == seg.tobytes()


# ---- ratios -----------------------------------------------------------------------------------------------

def test_the_ratios_of_the_table():
    """one segment of 64 KiB of each column of DESIGN.md 4.28's table: INTPACK's size, PATCHPACK's
    and its mode, pinned"""
    want = [(17420, 9440, 1), (17912, 13292, 1), (42668, 22072, 0), (29828, 11450, 3),
            (24124, 22450, 0), (20996, 20998, 0)]
    ratios = [(3.76, 6.94), (3.66, 4.93), (1.54, 2.97), (2.20, 5.72), (2.72, 2.92), (3.12, 3.12)]
    for (name, w, col), sizes, ratio in zip(C.table_columns(), want, ratios):
        assert col.size == 65536
        s, i = M.encode_segment(col, w), IM.encode_segment(col, w)
        assert (len(i), len(s), mode_of(s)) == sizes, name
        assert M.decode(s, 65536) == col.tobytes()
        assert (round(65536 / len(i), 2), round(65536 / len(s), 2)) == ratio, name
    # patching at least halves the 1 % columns' streams but for the offsets', and the column
    # without outliers pays LE16(0)
    assert all(p * 1.8 < i for i, p, _ in want[:4] if i != 17912)


# ---- the ids --------------------------------------------------------------------------------------------------

def test_ids_and_slot_sizes():
    import bitar_amd as B
    assert [B.codec_patchpack(w) for w in M.WIDTHS] == [104, 105, 106, 107]
    assert (B.CODEC_PATCHPACK8, B.CODEC_PATCHPACK16, B.CODEC_PATCHPACK32, B.CODEC_PATCHPACK64) == \
        (104, 105, 106, 107)
    assert B.COLUMN_CODECS["PATCHPACK"] == (104, 9, (1, 2, 4, 8))
    import os
    import re
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                          "bitar_hip.h")
    with open(header) as f:
        ids = dict(re.findall(r"\bBITAR_HIP_CODEC_PATCHPACK([0-9]+)\s*=\s*\(([0-9]+)\)", f.read()))
    assert ids == {"8": "104", "16": "105", "32": "106", "64": "107"}
    with pytest.raises(Exception):
        B.codec_patchpack(16)
    for codec in (104, 105, 106, 107):
        assert B.slot_size(codec, 65536) == 65536 + 256 and B.slot_size(codec, 59460) == 59648
        assert B.slot_size(codec, 252) == 256 and B.slot_size(codec, 253) == 512
        assert B.max_distance(codec) == 0
    for unknown in (108, 109, 103, 12, 89, 90, 99):
        assert B.slot_size(unknown, 100) == 0 and B.max_distance(unknown) == 0
    assert B.lib().bitar_hip_abi_version() == 3
