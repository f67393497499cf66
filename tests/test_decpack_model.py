"""The DECPACK model (decpack_model.py) against streams worked out by hand, the size formula, the
decoder's rejection rules one by one, the ids and the Python API, the split of the GPU test's
mutants and the ratio DESIGN.md 4.30 quotes.  No GPU."""
import os
import re

import numpy as np
import pytest

import decpack_cases as C
import decpack_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGS = (65536, 59460, 4096, 1040, 1000, 999, 72, 7)
TAILS = (0, 1, 15, 16, 63 * 16, 64 * 16, 64 * 16 + 1)


def le(v):
    return (v & C.MASK).to_bytes(16, "little")


# ---- streams worked out by hand ------------------------------------------------------------------

def test_golden_plain():
    """64 elements -3 + (37 i mod 64): ref -3 (sign-extended FF bytes), the residuals are 0..63 in
    that order at 6 bits: 48 payload bytes, each three the 24 bits of four residuals"""
    r = [37 * i % 64 for i in range(64)]
    data = C.to_bytes([x - 3 for x in r])
    (s,) = M.encode(data, 1024)
    payload = b"".join((r[4 * i] | r[4 * i + 1] << 6 | r[4 * i + 2] << 12 | r[4 * i + 3] << 18)
                       .to_bytes(3, "little") for i in range(16))
    assert payload[:3] == bytes([0 | (37 & 3) << 6, 37 >> 2 | (10 & 15) << 4, 10 >> 4 | 47 << 2])
    assert s == bytes.fromhex("d000ff03" "06") + b"\xfd" + b"\xff" * 15 + payload
    assert len(s) == 4 + 1 + 16 + 48 and M.decode(s, 1024) == data.tobytes()


def test_golden_delta_across_2_64():
    """65 elements from 2^64 - 10 in steps of 3: every delta is 3, width 0 in both miniblocks; the
    base carries the low half FF..F6 and the sum crosses into the high half at element 4"""
    v = [(1 << 64) - 10 + 3 * i for i in range(65)]
    data = np.frombuffer(C.to_bytes(v).tobytes() + b"\x07", np.uint8)
    (s,) = M.encode(data, 2048)
    assert s == bytes.fromhex("d4001004") + le(v[0]) + b"\0\0" + le(3) + b"\x07"
    assert M.decode(s, 2048) == data.tobytes()
    assert v[3] < 1 << 64 <= v[4]


def test_golden_descending_and_step():
    """deltas of -5: the reference is -5, 16 bytes FB FF .. FF; a step at element 1 is x_0's too"""
    v = [1000 - 5 * i for i in range(64)]
    (s,) = M.encode(C.to_bytes(v), 1024)
    assert s == bytes.fromhex("d400ff03") + le(1000) + b"\0" + le(-5)
    w = [7] + [(1 << 100) + i for i in range(127)]
    (s,) = M.encode(C.to_bytes(w), 2048)
    # x_0 = x_1 = 2^100 - 7, the others 1: ref 1, 100 bits in the first miniblock, 0 in the second
    assert M.mode_of(s) == 1 and M.widths_of(s) == [100, 0]
    assert s[22:38] == le(1) and len(s) == 4 + 16 + 2 + 16 + 800
    assert M.decode(s, 2048) == C.to_bytes(w).tobytes()


def test_most_negative_reference_and_wrapping_residuals():
    """values -2^127 and 2^127 - 1 in one block: ref = the most negative value, the residual of
    the largest is 2^128 - 1 (width 128); a block straddling 0 has residuals that wrap"""
    v = [-(1 << 127), (1 << 127) - 1] + [0] * 62
    s = M.packed_stream(C.to_bytes(v), 0)
    assert M.widths_of(s) == [128] and s[5:21] == le(C.MOST_NEGATIVE)
    assert M.decode(s, 1024) == C.to_bytes(v).tobytes()
    (t,) = M.encode(C.to_bytes(v), 1024)
    assert M.mode_of(t) == 2  # 4 + 1 + 16 + 1024 is not below 4 + 1024
    v = [-5, 10] * 32
    (s,) = M.encode(C.to_bytes(v), 1024)
    assert M.mode_of(s) == 0 and s[5:21] == le(-5) and M.widths_of(s) == [4]  # 10 - (-5) = 15


def test_stored_forms():
    noise = C.noise_segment(4096, 1)
    assert M.encode_segment(noise) == bytes([0xD8, 0, 0xFF, 0x0F]) + noise.tobytes()
    for L in range(1, 48):  # m = 0, 1, 2: nothing to gain
        s = M.encode_segment(noise[:L])
        assert len(s) == 4 + L and M.mode_of(s) == 2 and M.decode(s, 64) == noise[:L].tobytes()
    one = C.to_bytes([77])
    for mode in (0, 1):  # their packed forms decode all the same (x_0 = 0 when m = 1)
        assert M.decode(M.packed_stream(one, mode), 16) == one.tobytes()
    assert M.packed_stream(one, 1) == bytes.fromhex("d4000f00") + le(77) + b"\0" + le(0)


# ---- round trips, the size formula, the stored rule -----------------------------------------------

@pytest.mark.parametrize("seg", SEGS)
def test_round_trip_size_formula_and_stored_rule(seg):
    for r in TAILS:
        data = C.column(8, seg, seg * 31 + r, extra=r)
        streams = M.encode(data, seg)
        assert len(streams) == -(-data.size // seg)
        for i, s in enumerate(streams):
            part = data[i * seg:(i + 1) * seg]
            L = part.size
            assert M.decode(s, seg) == part.tobytes()
            assert s[1] == 0 and 1 + s[2] + (s[3] << 8) == L and s[0] & 0xF3 == 0xD0
            sizes = M.packed_sizes(part)
            if M.mode_of(s) == 2:
                assert len(s) == 4 + L and min(sizes) >= 4 + L
            else:
                mode = M.mode_of(s)
                assert len(s) == M.size(L, mode, M.widths_of(s)) == sizes[mode] < 4 + L
                assert mode == (1 if sizes[1] < sizes[0] else 0)
            if seg < 16:
                assert M.mode_of(s) == 2
        if seg >= 999:
            assert {M.mode_of(s) for s in streams} == {0, 1, 2}


def test_the_width_columns_hit_every_width():
    """what the GPU test relies on: the miniblocks of a width segment take exactly the widths
    asked for, with the largest residual where it was put"""
    n = len(C.EDGE_WIDTHS)
    for place in (0, -1):
        seg = 65536 - 59 * 16 + 5
        data = C.width_segment(seg, place, 10, shift=0)
        (s,) = M.encode(data, seg)
        m = seg // 16
        nmb = (m + 63) // 64
        assert M.mode_of(s) == 0 and m % 64 == 5
        assert M.widths_of(s) == [C.EDGE_WIDTHS[k % n] for k in range(nmb)]
        v = M.elements(data)
        refs = [int.from_bytes(s[4 + nmb + 16 * i:4 + nmb + 16 * i + 16], "little")
                for i in range((nmb + 3) // 4)]
        for k, b in enumerate(M.widths_of(s)):
            count = min(64, m - 64 * k)
            at = 64 * k + (0 if place == 0 else count - 1)
            assert (v[at] - refs[k // 4]) & C.MASK == (1 << b) - 1


def test_forced_forms_decode():
    L = 4096 - 5 * 16 - 3
    nmb = (L // 16 + 63) // 64
    plain, asc = C.width_segment(L, -1, 5), C.delta_segment(L, "asc", 6)
    for data, mode in ((plain, 0), (plain, 1), (asc, 0), (asc, 1)):
        for widths in (None, [128] * nmb):
            s = M.packed_stream(data, mode, widths)
            assert M.decode(s, 4096) == data.tobytes()
            assert len(s) == M.size(L, mode, M.widths_of(s))
    assert len(M.packed_stream(plain, 0, [128] * nmb)) > 4 + L


# ---- the decoder's rejections, one by one -----------------------------------------------------------

def test_rejections():
    seg = 4096
    plain, delta, stored = C.base_streams(M, seg)
    for s in (plain, delta, stored):
        assert M.decode(s, seg) is not None
        assert M.decode(s, seg - 100) is None          # L > seg
        assert M.decode(s[:3], seg) is None and M.decode(b"", seg) is None
        for tag in (0x40, 0x90, 0xC0, 0xE0):           # another nibble
            assert M.decode(bytes([tag | s[0] & 15]) + s[1:], seg) is None
        assert M.decode(bytes([s[0] | 12]) + s[1:], seg) is None      # mode 3
        for low in (1, 2, 3):                          # the low two bits
            assert M.decode(bytes([s[0] | low]) + s[1:], seg) is None
        assert M.decode(s[:1] + b"\x01" + s[2:], seg) is None         # byte 1
        assert M.decode(s + b"\0", seg) is None and M.decode(s[:-1], seg) is None
    for s in (plain, delta):
        at = 4 + (16 if M.mode_of(s) == 1 else 0)
        assert M.decode(s[:at + 3], seg) is None       # too short for the header arrays
        t = bytearray(s)
        t[at] = 129                                    # a width above 128
        assert M.decode(bytes(t), seg) is None
        t[at] = s[at] + 1                              # the size no longer fits
        assert M.decode(bytes(t), seg) is None


def test_the_mutations_split_both_ways():
    """the hostile streams of tests/test_gpu_decpack.py, judged by the model alone: at least 80
    mutants per run, at least 30 rejected, at least 10 accepted with other bytes"""
    for seg in (4096, 65536):
        total = rejected = other = 0
        for base in C.base_streams(M, seg):
            want = M.decode(base, seg)
            muts = C.mutants(base)
            verdicts = [M.decode(C.given(t, size), seg) for t, size in muts]
            assert verdicts[0] == want and want is not None
            # a flipped bit of the tag or of byte 1 always rejects; one of L rejects unless the
            # size formula gives the same for the other L (16 or 32 bytes more or less inside the
            # last miniblock: elements from the slots past m, or fewer elements)
            for (t, size), v in zip(muts[1:33], verdicts[1:33]):
                assert size == len(base) and t[4:] == base[4:] and t[:4] != base[:4]
                if t[2:4] == base[2:4]:
                    assert v is None
                elif v is not None:
                    assert len(v) != len(want) and (len(v) - len(want)) % 16 == 0
            total += len(verdicts)
            rejected += sum(v is None for v in verdicts)
            other += sum(v not in (None, want) for v in verdicts)
        assert total >= 80 and rejected >= 30 and other >= 10, (seg, total, rejected, other)


# ---- the ids and the Python API ---------------------------------------------------------------------

def test_the_id_and_the_header():
    import bitar_amd as B
    text = open(os.path.join(ROOT, "include", "bitar_hip_codecs.h")).read()
    ids = dict(re.findall(r"^\s*(BITAR_HIP_CODEC_\w+)\s*=\s*\(?(\d+)\)?", text, re.M))
    assert ids == {"BITAR_HIP_CODEC_DECPACK128": "260"}
    assert B.CODEC_DECPACK128 == 260 == int(ids["BITAR_HIP_CODEC_DECPACK128"])
    assert B.COLUMN_CODECS["DECPACK"] == (256, 0xD, (16,))
    assert B.codec_decpack(16) == 260
    # a header of its own, as bitar_hip_snappy.h is: neither includes the other
    assert "#include" not in text
    assert "bitar_hip_codecs.h\"" not in open(os.path.join(ROOT, "include", "bitar_hip.h")).read() \
        .replace("(bitar_hip_codecs.h", "")


@pytest.mark.parametrize("width", list(range(16)) + [32, 17, 64, None, "16"])
def test_codec_decpack_refuses_other_widths(width):
    import bitar_amd as B
    with pytest.raises(ValueError) as e:
        B.codec_decpack(width)
    assert "DECPACK element width must be 16" in str(e.value)
    with pytest.raises(ValueError):  # (and INTPACK goes on refusing 16)
        B.codec_intpack(16)


def test_slots_and_distance():
    import bitar_amd as B
    for seg in (7, 72, 4096, 59460, 65536):
        assert B.slot_size(260, seg) == B.slot_size(B.CODEC_INTPACK64, seg) == (seg + 4 + 255) & ~255
    assert B.max_distance(260) == 0
    for other in (256, 257, 258, 259, 261):
        assert B.slot_size(other, 65536) == 0 and B.max_distance(other) == 0


# ---- the columns of DESIGN.md 4.30 -----------------------------------------------------------------

def test_the_table_columns():
    """prices pack to 24 bits: 64 miniblocks of 192 bytes + 64 widths + 16 references + 4 = 12612
    bytes a segment, ratio 5.2; signed amounts to 21 bits; the running total goes into delta
    mode across 2^64; random values are stored"""
    cols = C.table_columns(n=4 * 65536)
    modes, ratios = [], []
    for name, col in cols:
        streams = M.encode(col, 65536)
        assert b"".join(M.decode(s, 65536) for s in streams) == col.tobytes()
        modes.append({M.mode_of(s) for s in streams})
        ratios.append(col.size / sum(len(s) for s in streams))
    assert modes == [{0}, {0}, {1}, {2}]
    assert all(len(s) == 4 + 64 + 256 + 64 * 8 * 24 == 12612 for s in M.encode(cols[0][1], 65536))
    assert abs(ratios[0] - 65536 / 12612) < 1e-9 and round(ratios[0], 2) == 5.2
    assert round(ratios[1], 2) == 5.92 and ratios[2] > 6 and ratios[3] == 65536 / 65540
    lo = cols[2][1].view("<u8")
    assert lo[1] == 0 and lo[-1] == 1  # the total starts below 2^64 and ends above it
