"""CPU tests of the CASCADE model (cascade_model.py): hand-written streams that pin the field
order, round trips at every width and segment size, the form choice with its tie and its run
limit, every reject rule of the decoder each alone, the streams no encoder writes that must
decode, the ratios against RUNPACK and INTPACK on the columns of DESIGN.md 4.24, and the
library's surface.  No GPU."""
import numpy as np
import pytest

import cascade_cases as C
import cascade_model as M
import intpack_model as IM
import runpack_model as RM
from bitar_amd import codec_cascade  # noqa: F401  (the codec under test: absent, nothing here runs)

SEGS = (65536, 59460, 4096, 1000, 999, 72, 7)
LOG = {1: 0, 2: 1, 4: 2, 8: 3}
U = {1: "<u1", 2: "<u2", 4: "<u4", 8: "<u8"}


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def mode_of(s):
    return s[0] >> 3 & 1


def le16(v):
    return bytes([v & 255, v >> 8])


def ipk_stored(w, payload):
    """INTPACK's stored form of `payload` at width w"""
    return IM._header(2, w, len(payload)) + bytes(payload)


def by_hand(w, values, lengths, tail=b""):
    """the cascade stream of the runs (values[k], lengths[k]) with both sub-streams stored"""
    values, lengths = np.asarray(values, U[w]), np.asarray(lengths, np.int64)
    L = int(lengths.sum()) * w + len(tail)
    return M.cascade_stream(L, w, lengths.size, ipk_stored(w, values.tobytes()),
                            ipk_stored(2, (lengths - 1).astype("<u2").tobytes()), tail)


def expand(w, values, lengths, tail=b""):
    return np.repeat(np.asarray(values, U[w]), lengths).tobytes() + bytes(tail)


def roundtrip(data, w, seg):
    streams = M.encode(data, w, seg)
    assert len(streams) == (data.size + seg - 1) // seg
    assert b"".join(M.decode(s, seg) for s in streams) == data.tobytes()
    for i, s in enumerate(streams):
        L = min(seg, data.size - i * seg)
        assert s[0] >> 4 == 8 and s[0] & 7 == LOG[w] and s[1] == 0
        assert 1 + s[2] + (s[3] << 8) == L
        assert len(s) <= 4 + L
        if mode_of(s):
            assert len(s) == 4 + L
        else:
            assert len(s) < 4 + L
            # the sub-streams are INTPACK's own streams of the runs
            values, lengths = RM._runs(data[i * seg:i * seg + L], w)
            vs = IM.encode_segment(values.reshape(-1), w)
            ls = IM.encode_segment((lengths - 1).astype("<u2").view(np.uint8), 2)
            assert s[4:8] == le16(lengths.size - 1) + le16(len(vs) - 1)
            assert s[8:8 + len(vs) + len(ls)] == vs + ls
            assert s[8 + len(vs) + len(ls):] == data[i * seg + L // w * w:i * seg + L].tobytes()
    return streams


# ---- hand-written streams ---------------------------------------------------------------------

def test_golden_bytes():
    """w = 1, L = 32: the bytes 10, 11, 12, 13 eight times each.  Values: delta (base 10, one
    miniblock of width 0, reference 1); lengths: 7, 7, 7, 7, plain with reference 7"""
    data = np.repeat(np.array([10, 11, 12, 13], np.uint8), 8)
    values = bytes([0x44, 0, 3, 0, 10, 0, 1])
    lengths = bytes([0x41, 0, 7, 0, 0, 7, 0])
    want = bytes([0x80, 0, 31, 0, 3, 0, len(values) - 1, 0]) + values + lengths
    assert IM.encode_segment(np.array([10, 11, 12, 13], np.uint8), 1) == values
    assert IM.encode_segment(np.array([7, 0] * 4, np.uint8), 2) == lengths
    assert M.encode_segment(data, 1) == want and len(want) == 22
    assert M.decode(want, 32) == data.tobytes()


def test_golden_eight_byte_elements_with_a_tail():
    """w = 8, L = 8 * 300 + 3: X 257 times, X + 5 42 times, X + 10 once, and a tail of 3 bytes"""
    X = 0x0123456789ABCDEF
    tail = bytes([0xDE, 0xAD, 0x42])
    data = np.frombuffer(expand(8, [X, X + 5, X + 10], [257, 42, 1], tail), np.uint8)
    L = 2403
    values = bytes([0x47, 0, 23, 0]) + X.to_bytes(8, "little") + bytes([0]) + (5).to_bytes(8, "little")
    lengths = IM.encode_segment(np.array([256, 41, 0], "<u2").view(np.uint8), 2)
    assert lengths[0] == 0x49 and len(lengths) == 4 + 6  # nothing to gain: stored
    want = bytes([0x83, 0, (L - 1) & 255, (L - 1) >> 8, 2, 0, len(values) - 1, 0]) + values + \
        lengths + tail
    assert M.encode_segment(data, 8) == want
    assert M.decode(want, 65536) == data.tobytes()


def test_golden_stored():
    data = np.frombuffer(bytes(range(7)), np.uint8)
    for w in M.WIDTHS:
        want = bytes([0x88 | LOG[w], 0, 6, 0]) + bytes(range(7))
        assert M.encode_segment(data, w) == want and M.decode(want, 7) == data.tobytes()


# ---- the form choice --------------------------------------------------------------------------

@pytest.mark.parametrize("w", M.WIDTHS)
def test_a_segment_without_an_element_is_kept_raw(w):
    for n in range(1, w):
        s = M.encode_segment(rnd(n, n), w)
        assert mode_of(s) == 1 and len(s) == 4 + n and M.decode(s, 72) == rnd(n, n).tobytes()


@pytest.mark.parametrize("w", M.WIDTHS)
def test_tie_goes_to_stored(w):
    """one run of n elements: values 4 + w (stored), lengths 6 (stored), so 18 + w bytes against
    4 + n*w: the tie where one exists, and the first n that wins"""
    sizes = {n: len(M.cascade_stream(n * w, w, 1, ipk_stored(w, bytes(w)), ipk_stored(2, bytes(2))))
             for n in range(1, 40)}
    assert all(v == 18 + w for v in sizes.values())
    value = rnd(w, 3)
    for n in range(1, 40):
        for tail in (0, w - 1):
            data = np.concatenate([np.tile(value, n), rnd(tail, 1)])
            s = M.encode_segment(data, w)
            assert mode_of(s) == (0 if 18 + w + tail < 4 + data.size else 1)
            assert len(s) == min(18 + w + tail, 4 + data.size)
            assert M.decode(s, 65536) == data.tobytes()
    ties = [n for n in range(1, 40) if 18 + w == 4 + n * w]
    assert ties == {1: [15], 2: [8], 4: [], 8: []}[w]


def test_the_run_limit():
    """w = 1: 65536 alternating bytes are 65536 runs, stored; 32768 alternating bytes are exactly
    32768 runs, a cascade form; pairs in 65536 bytes too; one run more is stored"""
    alt = (np.arange(65536) & 1).astype(np.uint8)
    s = M.encode_segment(alt, 1)
    assert mode_of(s) == 1 and len(s) == 65540
    s = M.encode_segment(alt[:32768], 1)
    assert mode_of(s) == 0 and s[4:6] == b"\xff\x7f" and M.decode(s, 32768) == alt[:32768].tobytes()
    pairs = np.repeat(np.arange(32768) % 251, 2).astype(np.uint8)
    s = M.encode_segment(pairs, 1)
    assert mode_of(s) == 0 and s[4:6] == b"\xff\x7f" and M.decode(s, 65536) == pairs.tobytes()
    assert M.decode(s[:4] + le16(32768) + s[6:], 65536) is None  # r = 32769 <= m
    pairs[1] = 77
    assert mode_of(M.encode_segment(pairs, 1)) == 1


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_round_trips(w, seg):
    rng = np.random.default_rng(seg + w)
    for tail in (0, 1, w - 1, w, 64 * w + 1):
        n = 3 * seg + tail
        for mean in (3, 300):
            roundtrip(C.sorted_keys(rng, n + 8, w, mean, 8)[:n], w, seg)
            roundtrip(C.status(rng, n + 8, w, mean, 16)[:n], w, seg)
        if w > 1:
            roundtrip(C.random_keys(rng, n + 8, w, 20)[:n], w, seg)
    roundtrip(rnd(2 * seg + 5, 1), w, seg)
    roundtrip(np.zeros(2 * seg + 5, np.uint8), w, seg)
    for n in range(1, min(w, seg)):
        roundtrip(rnd(n, n), w, seg)


# ---- the ratios of DESIGN.md 4.24 -------------------------------------------------------------

# column -> the least factor by which CASCADE is smaller than RUNPACK
AT_LEAST = {
    "sorted int32 keys, runs ~20, steps 1..8": 3.0,
    "sorted int64 keys, runs ~20, steps 1..1000": 3.0,
    "int64 1-second ticks, ~50 rows per tick": 5.0,
    "int32 status 0..15, runs ~30": 2.5,
}


def test_table_ratios():
    """the 1 MiB columns from a fresh seeded generator: CASCADE against the models' own RUNPACK
    and INTPACK streams of the same data"""
    got = {}
    for name, w, data in C.table_columns():
        assert data.size == 1 << 20
        size = {"CASCADE": sum(len(s) for s in roundtrip(data, w, 65536)),
                "RUNPACK": sum(len(s) for s in RM.encode(data, w, 65536)),
                "INTPACK": sum(len(s) for s in IM.encode(data, w, 65536))}
        got[name] = {k: round(data.size / v, 2) for k, v in size.items()}
        print(name, got[name])
        if name in AT_LEAST:
            assert size["RUNPACK"] >= AT_LEAST[name] * size["CASCADE"], name
        # never more than a few bytes per segment above the better of the two
        assert size["CASCADE"] <= min(size["RUNPACK"], size["INTPACK"]) * 1.01 + 16 * 8, name
    name = "int64 random keys, runs ~20"
    assert abs(got[name]["CASCADE"] / got[name]["RUNPACK"] - 1) <= 0.01


# ---- what the decoder rejects -----------------------------------------------------------------

def example(w, r=5, tail=3):
    """a cascade stream with both sub-streams stored (every byte of it can be poked alone) and
    the segment it decodes to"""
    values = (np.arange(r) * 3 + 7).astype(U[w])
    lengths = np.arange(r) * 7 + 1
    t = rnd(min(tail, w - 1), 1).tobytes()
    s = by_hand(w, values, lengths, t)
    data = expand(w, values, lengths, t)
    assert M.decode(s, 65536) == data
    return bytearray(s), data


def packed_example(w, r=300, tail=3):
    """a cascade stream as the encoder writes it, both sub-streams packed"""
    values = (np.cumsum(np.arange(r) % 5 + 1) + 1000).astype(U[w]) if w > 1 else \
        (np.arange(r) % 200).astype(np.uint8)
    lengths = np.arange(r) % 9 + 1
    data = np.frombuffer(expand(w, values, lengths, rnd(min(tail, w - 1), 1).tobytes()), np.uint8)
    s = M.encode_segment(data, w)
    vsize = 1 + s[6] + (s[7] << 8)
    assert mode_of(s) == 0 and s[8] >> 2 & 3 != 2 and s[8 + vsize] >> 2 & 3 != 2
    assert M.decode(s, 65536) == data.tobytes()
    return bytearray(s), data.tobytes(), vsize


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_the_tag_and_byte_one(w):
    s, data = example(w)
    for nib in range(16):
        t = bytearray(s)
        t[0] = nib << 4 | s[0] & 15
        assert (M.decode(t, 65536) is None) == (nib != 8)
    for lg in (4, 5, 6, 7):
        t = bytearray(s)
        t[0] = s[0] & ~7 | lg
        assert M.decode(t, 65536) is None
    for v in (1, 2, 0x80, 0xFF):
        t = bytearray(s)
        t[1] = v
        assert M.decode(t, 65536) is None
    stored = bytearray(M.encode_segment(rnd(100, 2), w))
    assert mode_of(stored) == 1 and M.decode(stored, 100) is not None
    stored[1] = 1
    assert M.decode(stored, 100) is None
    assert M.decode(s[:3], 65536) is None and M.decode(b"", 65536) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_length_above_the_segment(w):
    s, data = example(w)
    assert M.decode(s, len(data)) == data
    assert M.decode(s, len(data) - 1) is None
    stored = M.encode_segment(rnd(100, 2), w)
    assert M.decode(stored, 100) is not None and M.decode(stored, 99) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_sizes(w):
    s, _ = example(w)
    for t in (s + b"\0", s[:-1], s[:7], s[:4], s[:8]):
        assert M.decode(t, 65536) is None
    stored = M.encode_segment(rnd(100, 2), w)
    for t in (stored + b"\0", stored[:-1], stored[:4]):
        assert M.decode(t, 65536) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_run_counts(w):
    # r = m is fine, r = m + 1 is not, with everything else in order
    for r, ok in ((4, True), (5, False)):
        t = M.cascade_stream(4 * w, w, r, ipk_stored(w, bytes(range(r * w))), ipk_stored(2, bytes(2 * r)))
        got = M.decode(t, 65536)
        assert (got == bytes(range(4 * w))) if ok else got is None
    s, _ = example(w)
    for r in (4, 6):  # r - 1 and r + 1 in a good stream: the sub-streams' L fields no longer fit
        t = bytearray(s)
        t[4] = r - 1
        assert M.decode(t, 65536) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_vsize(w):
    s, _ = example(w, tail=3)
    tail = min(3, w - 1)
    vsize = 1 + s[6] + (s[7] << 8)
    assert vsize == 4 + 5 * w
    for v in (vsize - 1, vsize + 1, 3, 1, len(s) - 8, len(s) - 8 - tail - 3, 65536):
        t = bytearray(s)
        t[6:8] = le16(v - 1)
        assert M.decode(t, 65536) is None, v
    # the largest vsize with room for a lengths header: still rejected, by the sub-streams
    t = bytearray(s)
    t[6:8] = le16(len(s) - 8 - tail - 4 - 1)
    assert M.decode(t, 65536) is None


@pytest.mark.parametrize("which", ("values", "lengths"))
@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_sub_stream_headers(w, which):
    s, _ = example(w)
    at = 8 if which == "values" else 8 + 4 + 5 * w
    ww = w if which == "values" else 2
    for nib in range(16):  # INTPACK's nibble
        if nib != 4:
            t = bytearray(s)
            t[at] = nib << 4 | s[at] & 15
            assert M.decode(t, 65536) is None
    t = bytearray(s)
    t[at] |= 3 << 2  # mode 3
    assert M.decode(t, 65536) is None
    for lg in range(4):  # another width in the tag
        if lg != LOG[ww]:
            t = bytearray(s)
            t[at] = s[at] & ~3 | lg
            assert M.decode(t, 65536) is None
    t = bytearray(s)
    t[at + 1] = 1  # its byte 1
    assert M.decode(t, 65536) is None
    for d in (1, -1):  # its L field
        t = bytearray(s)
        t[at + 2] = s[at + 2] + d
        assert M.decode(t, 65536) is None
    for mode in (0, 1):  # stored taken for packed: the size does not fit
        t = bytearray(s)
        t[at] = s[at] & ~(3 << 2) | mode << 2
        assert M.decode(t, 65536) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_packed_sub_streams_that_intpack_rejects(w):
    s, data, vsize = packed_example(w)
    for at, ww in ((8, w), (8 + vsize, 2)):
        mode = s[at] >> 2 & 3
        wid_at = at + 4 + (ww if mode == 1 else 0)
        for k in range(5):  # 300 runs: 5 miniblocks
            for v in (8 * ww + 1, 0xFF, s[wid_at + k] + 1, s[wid_at + k] - 1):
                if 0 <= v <= 255:
                    t = bytearray(s)
                    t[wid_at + k] = v
                    assert M.decode(t, 65536) is None, (at, k, v)
    # the lengths' size must be exactly the rest: a byte more or less between the two
    assert M.decode(s[:8 + vsize] + b"\0" + s[8 + vsize:], 65536) is None
    assert M.decode(s[:-1], 65536) is None and M.decode(s + b"\0", 65536) is None


@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_rejects_lengths_that_do_not_add_up(w):
    s, data = example(w)
    at = 8 + 4 + 5 * w + 4
    for k in range(5):
        for delta in (1, -1):
            t = bytearray(s)
            v = t[at + 2 * k] + delta
            if not 0 <= v <= 255:
                continue
            t[at + 2 * k] = v
            assert M.decode(t, 65536) is None
    t = bytearray(s)
    t[at + 3:at + 5] = b"\xff\xff"
    assert M.decode(t, 65536) is None
    # one up and another down: accepted, with other bytes
    t = bytearray(s)
    t[at + 2] += 1
    t[at + 6] -= 1
    got = M.decode(t, 65536)
    assert got is not None and len(got) == len(data) and got != data


# ---- what no encoder writes and the decoder takes -----------------------------------------------

@pytest.mark.parametrize("w", M.WIDTHS)
def test_decode_accepts_non_canonical_streams(w):
    s, data = example(w, tail=0)
    m = len(data) // w
    # equal neighbouring values
    t = bytearray(s)
    t[12 + w:12 + 2 * w] = t[12:12 + w]
    want = np.frombuffer(data, np.uint8).reshape(m, w).copy()
    want[1:9] = want[0]
    assert M.decode(t, 65536) == want.tobytes()
    # sub-streams stored where packing is smaller (example() itself), and packed in the mode that
    # is not the smallest: 300 sorted values in plain mode
    values = (np.arange(300) * 1000 + 5).astype(U[w])
    lengths = np.arange(300) % 9 + 1
    seg = np.frombuffer(expand(w, values, lengths), np.uint8)
    good = M.encode_segment(seg, w)
    vsize = 1 + good[6] + (good[7] << 8)
    assert good[8] >> 2 & 3 == (1 if w > 1 else good[8] >> 2 & 3)
    widths, refs, r = IM._plan(IM._values(values, 0), w)
    plain = IM._header(0, w, 300 * w) + widths.tobytes() + refs.astype(U[w]).tobytes() + \
        IM._pack(r, widths)
    assert IM.decode(plain, 300 * w) == values.tobytes()
    t = M.cascade_stream(seg.size, w, 300, plain, good[8 + vsize:])
    if w > 1:
        assert len(t) > len(good)
    assert M.decode(t, 65536) == seg.tobytes()
    # a cascade form larger than 4 + L: every element its own run
    one = np.arange(8).astype(U[w])
    t = by_hand(w, one, np.ones(8, np.int64))
    assert len(t) > 4 + 8 * w and M.decode(t, 65536) == one.tobytes()


# ---- the library's surface --------------------------------------------------------------------

def test_library_surface():
    import bitar_amd as B
    ids = (B.CODEC_CASCADE8, B.CODEC_CASCADE16, B.CODEC_CASCADE32, B.CODEC_CASCADE64)
    assert ids == (64, 65, 66, 67)
    assert B.COLUMN_CODECS["CASCADE"] == (64, 8, (1, 2, 4, 8))
    assert [B.codec_cascade(w) for w in M.WIDTHS] == [64, 65, 66, 67]
    for bad in (0, 3, 5, 16, 32, 64, -1, None, "8", 2.5):
        with pytest.raises(ValueError) as e:
            B.codec_cascade(bad)
        assert str(e.value) == f"CASCADE element width must be 1, 2, 4 or 8, not {bad!r}"
    for codec in ids:
        assert B.slot_size(codec, 65536) == 65792
        assert B.slot_size(codec, 1) == 256
        assert B.slot_size(codec, 59460) == 59648
        assert B.max_distance(codec) == 0
    for unknown in (68, 99):
        assert B.slot_size(unknown, 100) == 0 and B.max_distance(unknown) == 0


def test_abi_is_untouched():
    import bitar_amd as B
    import test_abi
    assert B.lib().bitar_hip_abi_version() == 3
    assert sorted(B.ABI_SYMBOLS) == test_abi.header_symbols() and len(B.ABI_SYMBOLS) == 39
    assert not [s for s in B.ABI_SYMBOLS if "cascade" in s]
    assert B.codec_cascade(8) == 67  # (fails where the codec is absent)
