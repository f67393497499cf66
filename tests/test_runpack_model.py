"""CPU tests of the RUNPACK model (runpack_model.py): hand-written streams that pin the field
order, round trips of run-shaped columns and of the edge cases, the form choice with its tie,
the switch of the length width, every reject rule of the decoder each alone, the streams no
encoder writes that must decode, and the library's surface.  No GPU."""
import numpy as np
import pytest

import runpack_model as M
from bitar_amd import codec_runpack  # noqa: F401  (the codec under test: absent, nothing here runs)

SEGS = (65536, 59460, 4096, 1000, 999, 72, 7)
LOG = {1: 0, 2: 1, 4: 2, 8: 3, 16: 4}


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def mode_of(s):
    return s[0] >> 3 & 1


def runs_of(values, lengths):
    """rows `values` (r x w) repeated `lengths` times each -> their bytes"""
    return np.repeat(values, lengths, axis=0).reshape(-1)


def geometric_runs(rng, m, mean, values):
    """m elements in runs of geometric length (mean `mean`), a run's value drawn from the rows
    of `values` -> their bytes"""
    lengths = rng.geometric(1.0 / mean, m // mean + 64)
    while lengths.sum() < m:
        lengths = np.append(lengths, rng.geometric(1.0 / mean, 1024))
    rows = values[rng.integers(0, values.shape[0], lengths.size)]
    return np.repeat(rows, lengths, axis=0)[:m].reshape(-1)


def table_columns(n=1 << 20):
    """the columns of DESIGN.md 4.19 -> [(name, w, bytes)], n bytes each"""
    rng = np.random.default_rng(2025)
    u8 = lambda a: np.ascontiguousarray(a).view(np.uint8)  # noqa: E731
    stamps = 1_700_000_000_000 + 60_000 * np.sort(rng.integers(0, 50, n // 8))
    ids = rnd(4000 * 16, 9).reshape(4000, 16)
    flags = np.array([[0x00], [0xFF]], np.uint8)
    lengths = rng.geometric(1.0 / 200, n // 100)
    flag_col = np.repeat(flags[np.arange(lengths.size) & 1], lengths, axis=0)[:n].reshape(-1)
    assert flag_col.size == n
    keys = u8(rng.integers(0, 1 << 31, 1000).astype("<u4")).reshape(1000, 4)
    shorts = u8(rng.integers(0, 1 << 15, 3000).astype("<u2")).reshape(3000, 2)
    return [("int64 timestamps, 50 values, sorted", 8, u8(stamps.astype("<i8"))),
            ("16-byte ids, runs of mean 500", 16, geometric_runs(rng, n // 16, 500, ids)),
            ("byte flags 0x00 / 0xFF, runs of mean 200", 1, flag_col),
            ("int32 keys of 1000 values, runs of mean 20", 4, geometric_runs(rng, n // 4, 20, keys)),
            ("int16, runs of mean 3", 2, geometric_runs(rng, n // 2, 3, shorts)),
            ("random bytes", 1, rnd(n, 11))]


def roundtrip(data, w, seg):
    streams = M.encode(data, w, seg)
    assert len(streams) == (data.size + seg - 1) // seg
    assert b"".join(M.decode(s, seg) for s in streams) == data.tobytes()
    for i, s in enumerate(streams):
        L = min(seg, data.size - i * seg)
        assert s[0] >> 4 == 7 and s[0] & 7 == LOG[w]
        assert 1 + s[2] + (s[3] << 8) == L
        if mode_of(s):
            assert s[1] == 0 and len(s) == 4 + L
        else:
            assert s[1] in (1, 2) and len(s) < 4 + L
    return streams


# ---- hand-written streams ---------------------------------------------------------------------

def test_golden_bytes():
    """w = 1, L = 12: five 0x41, one 0x42, six 0x00 -> r = 3, bl = 1, lengths 4, 0, 5"""
    data = np.frombuffer(b"AAAAAB" + bytes(6), np.uint8)
    want = bytes([0x70, 0x01, 11, 0x00, 0x02, 0x00, 0x41, 0x42, 0x00, 0x04, 0x00, 0x05])
    assert len(want) == M.runs_size(12, 1, 3, 1) == 12
    assert M.encode_segment(data, 1) == want
    assert M.decode(want, 12) == data.tobytes()


def test_golden_sixteen_byte_elements():
    """w = 16, L = 16 * 300 + 3: X 257 times, Y 42 times, Z once and a tail of 3 bytes -> r = 3,
    bl = 2 (a run above 256), lengths 0x0100, 0x0029, 0x0000"""
    X, Y, Z = bytes(range(16)), bytes(range(16, 32)), bytes([0xFF] * 15 + [0x00])
    tail = bytes([0xDE, 0xAD, 0x42])
    L = 16 * 300 + 3
    want = bytes([0x74, 0x02, (L - 1) & 255, (L - 1) >> 8, 0x02, 0x00]) + X + Y + Z + \
        bytes([0x00, 0x01, 0x29, 0x00, 0x00, 0x00]) + tail
    assert len(want) == 6 + 3 * 18 + 3
    data = np.frombuffer(X * 257 + Y * 42 + Z + tail, np.uint8)
    assert M.encode_segment(data, 16) == want
    assert M.decode(want, 65536) == data.tobytes()


def test_golden_stored():
    data = np.frombuffer(bytes(range(7)), np.uint8)
    for w in M.WIDTHS:
        want = bytes([0x78 | LOG[w], 0, 6, 0]) + bytes(range(7))
        assert M.encode_segment(data, w) == want and M.decode(want, 7) == data.tobytes()


# r runs at bl = 1 tie with the stored form when r*(w + 1) + 2 = m*w: the smallest (m, r) per width
TIES = {1: (4, 1), 2: (4, 2), 4: (3, 2), 8: (7, 6), 16: (15, 14)}


@pytest.mark.parametrize("w", M.WIDTHS)
def test_tie_goes_to_stored(w):
    m, r = TIES[w]
    assert M.runs_size(m * w, w, r, 1) == 4 + m * w
    values = rnd(r * w, 5).reshape(r, w)
    values[:, 0] = np.arange(r)
    lengths = np.full(r, 1)
    lengths[0] = m - (r - 1)
    for tail in (0, w - 1):
        data = np.concatenate([runs_of(values, lengths), rnd(tail, 2)])
        s = M.encode_segment(data, w)
        assert mode_of(s) == 1 and len(s) == 4 + data.size
        # an element more of the first run tips it
        lengths[0] += 1
        data = np.concatenate([runs_of(values, lengths), rnd(tail, 2)])
        s = M.encode_segment(data, w)
        assert mode_of(s) == 0 and len(s) == 4 + data.size - w
        lengths[0] -= 1


@pytest.mark.parametrize("w", M.WIDTHS)
def test_length_width_switches_above_256(w):
    a, b = rnd(w, 1), rnd(w, 2)
    a[0], b[0] = 1, 2
    for n, bl in ((255, 1), (256, 1), (257, 2), (300, 2)):
        data = np.concatenate([np.tile(a, n), np.tile(b, 3)])
        s = M.encode_segment(data, w)
        assert mode_of(s) == 0 and s[1] == bl and s[4] == 1
        field = s[6 + 2 * w:6 + 2 * w + 2 * bl]
        want = bytes([n - 1, 2]) if bl == 1 else bytes([(n - 1) & 255, (n - 1) >> 8, 2, 0])
        assert field == want
        assert M.decode(s, 65536) == data.tobytes()


def test_a_run_of_65536():
    data = np.full(65536, 0x33, np.uint8)
    s = M.encode_segment(data, 1)
    assert s == bytes([0x70, 0x02, 0xFF, 0xFF, 0x00, 0x00, 0x33, 0xFF, 0xFF])
    assert M.decode(s, 65536) == data.tobytes()
    for w in M.WIDTHS[1:]:
        s = M.encode_segment(data, w)
        m = 65536 // w
        assert len(s) == 6 + w + 2 and s[-2:] == bytes([(m - 1) & 255, (m - 1) >> 8])


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_round_trips(w, seg):
    rng = np.random.default_rng(seg + w)
    values = rnd(300 * w, 3).reshape(300, w)
    for tail in (0, 1, w - 1, w, 64 * w + 1):
        m = (3 * seg + tail) // w + 1
        for mean in (3, 300):
            data = geometric_runs(rng, m, mean, values)[:3 * seg + tail]
            roundtrip(data, w, seg)
    roundtrip(rnd(2 * seg + 5, 1), w, seg)
    roundtrip(np.zeros(2 * seg + 5, np.uint8), w, seg)
    for n in range(1, min(w, seg)):
        roundtrip(rnd(n, n), w, seg)


def test_patterns_are_compared_as_bytes():
    z = np.array([0.0, -0.0, 0.0, -0.0], "<f8").view(np.uint8)
    s = M.encode_segment(np.tile(z, 64), 8)
    assert mode_of(s) == 1  # 256 runs of one: nothing to gain
    nans = np.array([0x7FF8000000000000, 0x7FF8000000000001], "<u8").view(np.uint8).reshape(2, 8)
    data = runs_of(nans, [100, 100])
    s = M.encode_segment(data, 8)
    assert mode_of(s) == 0 and s[4] == 1 and M.decode(s, 65536) == data.tobytes()
    # (a, b, a, b, ...) is one run of 8-byte elements and no run at all of 4-byte ones
    ab = np.tile(np.concatenate([rnd(4, 1), rnd(4, 2)]), 500)
    assert mode_of(M.encode_segment(ab, 4)) == 1
    s = M.encode_segment(ab, 8)
    assert mode_of(s) == 0 and s[4] == 0 and len(s) == 6 + 8 + 2


# ---- the 1 MiB ratios of DESIGN.md 4.19 --------------------------------------------------------

RATIOS = {
    "int64 timestamps, 50 values, sorted": 1405.6,
    "16-byte ids, runs of mean 500": 350.23,
    "byte flags 0x00 / 0xFF, runs of mean 200": 66.34,
    "int32 keys of 1000 values, runs of mean 20": 15.75,
    "int16, runs of mean 3": 2.0,
    "random bytes": 1.0,
}


def test_table_ratios():
    """the numbers of DESIGN.md 4.19's table, from this model on the columns above"""
    got = {}
    for name, w, data in table_columns():
        assert data.size == 1 << 20
        got[name] = round(data.size / sum(len(s) for s in roundtrip(data, w, 65536)), 2)
    print(got)
    assert got == RATIOS


# ---- what the decoder rejects -----------------------------------------------------------------

def runs_example(w, r=5, tail=3, long_run=False):
    values = rnd(r * w, 17).reshape(r, w)
    values[:, 0] = np.arange(r)
    lengths = np.arange(r) * 7 + 1
    if long_run:
        lengths[2] = 300
    data = np.concatenate([runs_of(values, lengths), rnd(min(tail, w - 1), 1)])
    s = M.encode_segment(data, w)
    assert mode_of(s) == 0 and s[4] == r - 1 and s[1] == (2 if long_run else 1) and M.decode(s, 65536) == data.tobytes()
    return bytearray(s), data


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_the_tag(w):
    s, data = runs_example(w)
    for nib in range(16):
        t = bytearray(s)
        t[0] = nib << 4 | s[0] & 15
        assert (M.decode(t, 65536) is None) == (nib != 7)
    for lg in (5, 6, 7):
        t = bytearray(s)
        t[0] = s[0] & ~7 | lg
        assert M.decode(t, 65536) is None
    assert M.decode(s[:3], 65536) is None and M.decode(b"", 65536) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_byte_one(w):
    s, _ = runs_example(w)
    for v in (0, 3, 0x80, 0xFF):  # runs: 1 or 2 only (and 2 changes the size)
        t = bytearray(s)
        t[1] = v
        assert M.decode(t, 65536) is None
    stored = bytearray(M.encode_segment(rnd(100, 2), w))
    assert mode_of(stored) == 1 and M.decode(stored, 100) is not None
    for v in (1, 2, 0xFF):  # stored: 0 only
        t = bytearray(stored)
        t[1] = v
        assert M.decode(t, 100) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_length_above_the_segment(w):
    s, data = runs_example(w)
    assert M.decode(s, data.size) == data.tobytes()
    assert M.decode(s, data.size - 1) is None
    stored = M.encode_segment(rnd(100, 2), w)
    assert M.decode(stored, 99) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_short_streams_and_run_counts(w):
    s, data = runs_example(w)
    assert M.decode(s[:5], 65536) is None and M.decode(s[:4], 65536) is None
    # r = m + 1 with the size its formula gives
    for r, verdict in ((4, bytes(4 * w)), (5, None)):
        t = bytes([0x70 | LOG[w], 1, 4 * w - 1, 0, r - 1, 0]) + bytes(r * w) + bytes(r)
        assert len(t) == M.runs_size(4 * w, w, r, 1) and M.decode(t, 65536) == verdict
    # r - 1 and r + 1 in a good stream: the size no longer fits
    for r in (4, 6):
        t = bytearray(s)
        t[4] = r - 1
        assert M.decode(t, 65536) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_size_mismatch(w):
    s, _ = runs_example(w)
    for t in (s + b"\0", s[:-1], s + bytes(8), s[:6]):
        assert M.decode(t, 65536) is None
    stored = M.encode_segment(rnd(100, 2), w)
    for t in (stored + b"\0", stored[:-1], stored[:4]):
        assert M.decode(t, 65536) is None


@pytest.mark.parametrize("long_run", (False, True))
@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_lengths_that_do_not_add_up(w, long_run):
    s, data = runs_example(w, long_run=long_run)
    bl = s[1]
    at = 6 + 5 * w
    for k in range(5):
        for delta in (1, -1):
            t = bytearray(s)
            v = t[at + k * bl] + delta
            if not 0 <= v <= 255:
                continue
            t[at + k * bl] = v
            assert M.decode(t, 65536) is None
    # one up and another down: accepted, with other bytes
    t = bytearray(s)
    t[at + 1 * bl] += 1
    t[at + 3 * bl] -= 1
    got = M.decode(t, 65536)
    assert got is not None and len(got) == data.size and got != data.tobytes()
    if bl == 2:
        t = bytearray(s)
        t[at + 2:at + 4] = b"\xff\xff"
        assert M.decode(t, 65536) is None


def sum_2_32_stream():
    """w = 1, L = 65536, r = 65536, every length field FF FF: the lengths add up to 2^32"""
    s = bytes([0x70, 0x02, 0xFF, 0xFF, 0xFF, 0xFF]) + bytes(65536) + b"\xff" * (2 * 65536)
    assert len(s) == 196614 == M.runs_size(65536, 1, 65536, 2)
    return s


def test_decode_rejects_the_sum_of_2_32():
    s = sum_2_32_stream()
    assert M.decode(s, 65536) is None
    # the same stream with every length 1 is fine (and far larger than the stored form)
    t = s[:6 + 65536] + bytes(2 * 65536)
    assert M.decode(t, 65536) == bytes(65536)


# ---- what no encoder writes and the decoder takes -----------------------------------------------

@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_accepts_non_canonical_streams(w):
    s, data = runs_example(w, tail=0)
    m = data.size // w
    # equal neighbouring values
    t = bytearray(s)
    t[6 + w:6 + 2 * w] = t[6:6 + w]
    want = data.reshape(m, w).copy()
    want[1:9] = want[0]
    assert M.decode(t, 65536) == want.tobytes()
    # bl = 2 where 1 would do
    lengths = bytes(s[6 + 5 * w:6 + 5 * w + 5])
    t = bytearray(s[:6 + 5 * w]) + b"".join(bytes([v, 0]) for v in lengths)
    t[1] = 2
    assert len(t) == M.runs_size(data.size, w, 5, 2) and M.decode(t, 65536) == data.tobytes()
    # a runs form larger than 4 + L: every element its own run
    one = rnd(8 * w, 3)
    t = bytes([0x70 | LOG[w], 1, 8 * w - 1, 0, 7, 0]) + one.tobytes() + bytes(8)
    assert len(t) > 4 + one.size and M.decode(t, 65536) == one.tobytes()


# ---- the library's surface --------------------------------------------------------------------

def test_library_surface():
    import bitar_amd as B
    ids = (B.CODEC_RUNPACK8, B.CODEC_RUNPACK16, B.CODEC_RUNPACK32, B.CODEC_RUNPACK64,
           B.CODEC_RUNPACK128)
    assert ids == (32, 33, 34, 35, 36)
    assert [B.codec_runpack(w) for w in M.WIDTHS] == [32, 33, 34, 35, 36]
    for bad in (0, 3, 5, 32, 64, -1, None, "8", 2.5):
        with pytest.raises(ValueError):
            B.codec_runpack(bad)
    for codec in ids:
        assert B.slot_size(codec, 65536) == 65792
        assert B.slot_size(codec, 1) == 256
        assert B.slot_size(codec, 59460) == 59648
        assert B.max_distance(codec) == 0
    for unknown in (7, 12, 16, 17, 20, 24, 25, 29, 30, 31, 37, 99):
        assert B.slot_size(unknown, 100) == 0 and B.max_distance(unknown) == 0


def test_abi_is_untouched():
    import bitar_amd as B
    import test_abi
    assert B.lib().bitar_hip_abi_version() == 3
    assert sorted(B.ABI_SYMBOLS) == test_abi.header_symbols() and len(B.ABI_SYMBOLS) == 39
    assert not [s for s in B.ABI_SYMBOLS if "runpack" in s]
    assert B.codec_runpack(8) == 35  # (fails where the codec is absent)
