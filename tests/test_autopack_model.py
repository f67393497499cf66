"""CPU tests of the AUTOPACK model (autopack_model.py): the worked examples byte for byte, the
ties (at the stored form and between two packed forms), the choice per segment on the columns the
four codecs were built for and on the mixed buffer the codec was proposed on, the tag dispatch of
the decoder with every format's rejects, and the library's surface.  No GPU."""
import numpy as np
import pytest

import autopack_cases as C
import autopack_model as M
import intpack_model as IM
import runpack_model as RM
from bitar_amd import codec_autopack  # noqa: F401  (the codec under test: absent, nothing here runs)

LOG = {1: 0, 2: 1, 4: 2, 8: 3, 16: 4}


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def sizes_of(segment, w):
    return {name: len(s) for name, s in M.candidate_streams(segment, w)}


# ---- the rule ---------------------------------------------------------------------------------

def test_candidates():
    assert M.CANDIDATES == {1: ("RUNPACK", "INTPACK"), 2: ("RUNPACK", "INTPACK"),
                            4: ("RUNPACK", "INTPACK", "DICTPACK", "FLTPACK"),
                            8: ("RUNPACK", "INTPACK", "DICTPACK", "FLTPACK"),
                            16: ("RUNPACK", "DICTPACK")}


def test_golden_worked_examples():
    one = np.full(4096, 7, np.uint8)
    # w = 8: DICTPACK's 14 bytes (one entry, no payload) against RUNPACK's 16 and INTPACK's 28
    assert sizes_of(one, 8) == {"RUNPACK": 16, "INTPACK": 28, "DICTPACK": 14, "FLTPACK": 4100}
    assert M.encode_segment(one, 8) == bytes([0x63, 0, 0xFF, 0x0F, 0, 0]) + bytes([7] * 8)
    # w = 1: RUNPACK's 9 bytes, one run of 4096 with a 2-byte length
    assert sizes_of(one, 1) == {"RUNPACK": 9, "INTPACK": 84}
    assert M.encode_segment(one, 1) == bytes([0x70, 2, 0xFF, 0x0F, 0, 0, 7, 0xFF, 0x0F])
    # w = 16: DICTPACK's 22 against RUNPACK's 23
    assert sizes_of(one, 16) == {"RUNPACK": 23, "DICTPACK": 22}
    assert M.encode_segment(one, 16) == bytes([0x64, 0, 0xFF, 0x0F, 0, 0]) + bytes([7] * 16)


@pytest.mark.parametrize("w", M.WIDTHS)
def test_tie_at_stored_goes_to_runpack(w):
    for L in (7, 72, 1000, 4096, 65536):
        data = rnd(L, L + w)
        got = sizes_of(data, w)
        assert set(got.values()) == {4 + L}, "random bytes pack under no candidate"
        s = M.encode_segment(data, w)
        assert s == bytes([0x78 | LOG[w], 0, (L - 1) & 255, (L - 1) >> 8]) + data.tobytes()
        assert s == RM.encode_segment(data, w)


def test_ties_between_packed_forms():
    """A search of small shapes (up to 512 elements of runs or cycles of up to 8 values) finds
    ties between two packed forms; these three are held.  The earlier candidate's stream is
    taken."""
    # w = 1, 129 equal bytes: RUNPACK's one run with a 1-byte length and INTPACK's all-zero
    # widths are both 8 bytes
    a = np.full(129, 0xAB, np.uint8)
    assert sizes_of(a, 1) == {"RUNPACK": 8, "INTPACK": 8}
    assert M.encode_segment(a, 1) == RM.encode_segment(a, 1) == bytes([0x70, 1, 128, 0, 0, 0, 0xAB, 128])
    # w = 8 (and 4), 65 equal elements: INTPACK and DICTPACK tie below RUNPACK
    for w, size in ((8, 14), (4, 10)):
        b = np.tile(rnd(w, 3), 65)
        got = sizes_of(b, w)
        assert got["INTPACK"] == got["DICTPACK"] == size and got["RUNPACK"] == size + 1
        assert M.encode_segment(b, w) == IM.encode_segment(b, w)
    # w = 4, five elements in three runs of small values: RUNPACK and INTPACK tie at 21
    c = np.zeros(20, np.uint8)
    c[0:8:4], c[8:16:4], c[16] = 0, 1, 2
    got = sizes_of(c, 4)
    assert got["RUNPACK"] == got["INTPACK"] == 21 == min(got.values())
    assert M.encode_segment(c, 4) == RM.encode_segment(c, 4)


def test_a_tie_is_found_by_the_search():
    rng = np.random.default_rng(1)
    ties = set()
    for w in M.WIDTHS:
        vals = rng.integers(0, 256, (4, w), dtype=np.uint8)
        for m in range(1, 513, 4):
            for r in (1, 3):
                if r > m:
                    continue
                data = vals[np.arange(m) * r // m].reshape(-1)
                cs = M.candidate_streams(data, w)
                best = min(len(s) for _, s in cs)
                tied = tuple(n for n, s in cs if len(s) == best)
                if best < 4 + data.size and len(tied) > 1:
                    ties.add((w, tied))
                    assert M.encode_segment(data, w) == cs[[n for n, _ in cs].index(tied[0])][1]
    assert (1, ("RUNPACK", "INTPACK")) in ties and (8, ("INTPACK", "DICTPACK")) in ties


# ---- the choice ---------------------------------------------------------------------------------

def test_mixed_buffer_every_candidate_wins_and_the_total_is_below_every_single_codec():
    buf = C.mixed_int64()
    assert buf.size == 10 * 65536
    streams = M.encode(buf, 8, 65536)
    kinds = C.formats(streams)
    # sorted stamps, prices, ids, narrow integers, random 63-bit values (INTPACK saves their
    # top bit) -- twice
    assert kinds == ["RUNPACK", "FLTPACK", "DICTPACK", "INTPACK", "INTPACK"] * 2
    total = sum(len(s) for s in streams)
    single = {name: sum(len(s) for s in Mo.encode(buf, 8, 65536)) for name, Mo in M.ORDER}
    # (the generator's seed is fixed: these are its figures)
    assert total == 204600
    assert single == {"RUNPACK": 525232, "INTPACK": 413008, "DICTPACK": 419280, "FLTPACK": 559916}
    assert all(total < v for v in single.values())
    assert b"".join(M.decode(s, 65536) for s in streams) == buf.tobytes()


def own_columns():
    """the columns of the codecs' own model tests (DICTPACK's and RUNPACK's table columns,
    INTPACK's mode column, FLTPACK's decimal columns), 256 KiB each, and per width the stretches
    the GPU tests use"""
    import test_dictpack_model as TD
    import test_fltpack_model as TF
    import test_intpack_model as TI
    import test_runpack_model as TR
    cols = [(name, w, data) for name, w, data, _ in TD.table_columns(1 << 18)]
    cols += TR.table_columns(1 << 18)
    cols += [(f"intpack column, width {w}", w, TI.column(1 << 18, w, 3)) for w in IM.WIDTHS]
    cols += [(f"decimal column, width {w}", w, TF.as_bytes(TF.decimal_column((1 << 18) // w, w, 2, 1)))
             for w in (4, 8)]
    cols += [(f"stretches of width {w}", w, C.stretches(w, 4096)) for w in M.WIDTHS]
    return cols


def test_size_is_the_minimum_of_the_candidates_per_segment():
    for name, w, data in own_columns():
        for seg in (65536, 59460):
            mine = M.encode(data, w, seg)
            theirs = {c: M.MODELS[c].encode(data, w, seg) for c in M.CANDIDATES[w]}
            for i, s in enumerate(mine):
                cand = [theirs[c][i] for c in M.CANDIDATES[w]]
                assert len(s) == min(len(c) for c in cand), (name, seg, i)
                assert s == next(c for c in cand if len(c) == len(s)), (name, seg, i)
            assert b"".join(M.decode(s, seg) for s in mine) == data.tobytes(), name


@pytest.mark.parametrize("w", M.WIDTHS)
def test_stretches_show_every_applicable_tag(w):
    for seg in (65536, 59460, 4096, 1000):
        kinds = set(C.formats(M.encode(C.stretches(w, seg), w, seg)))
        assert kinds == set(M.CANDIDATES[w]) | {"stored"}, (w, seg)


# ---- the decoder ----------------------------------------------------------------------------------

def base_streams():
    """one packed stream per format (width 8 where the format has it, 4096-byte segment)"""
    rng = np.random.default_rng(5)
    out = {}
    for kind, name in C.BUILT_FOR.items():
        s = M.MODELS[name].encode_segment(C.segment(kind, 4096, 8, rng), 8)
        assert M.format_of(s) == name and len(s) < 4100
        out[name] = s
    return out


def test_decode_agrees_with_each_formats_model_rejects_included():
    for name, s in base_streams().items():
        Mo = M.MODELS[name]
        assert M.decode(s, 4096) == Mo.decode(s, 4096) is not None
        assert M.decode(s, 4095) is None  # (L above the segment: every format rejects)
        rejected = 0
        for at in range(8):
            for bit in range(8):
                t = bytearray(s)
                t[at] ^= 1 << bit
                want = Mo.decode(bytes(t), 4096) if t[0] >> 4 == s[0] >> 4 else \
                    M.MODELS[M.NIBBLES[t[0] >> 4]].decode(bytes(t), 4096) if t[0] >> 4 in M.NIBBLES \
                    else None
                assert M.decode(bytes(t), 4096) == want
                rejected += want is None
        assert rejected > 8, name
        for cut in (0, 1, 3, len(s) - 1):
            assert M.decode(s[:cut], 4096) is None
        assert M.decode(s + b"\0", 4096) is None


def test_decode_rejects_foreign_nibbles_and_the_empty_stream():
    assert M.decode(b"", 65536) is None
    for name, s in base_streams().items():
        for nib in list(range(0, 4)) + list(range(8, 16)):
            t = bytes([nib << 4 | s[0] & 15]) + s[1:]
            assert M.format_of(t) is None and M.decode(t, 4096) is None, (name, nib)


def test_every_stream_decodes_under_its_own_codec():
    for w in M.WIDTHS:
        data = C.stretches(w, 1000)
        for s, part in zip(M.encode(data, w, 1000), range(0, data.size, 1000)):
            assert M.MODELS[M.format_of(s)].decode(s, 1000) == data[part:part + 1000].tobytes()


# ---- the library's surface --------------------------------------------------------------------

def test_library_surface():
    import bitar_amd as B
    ids = (B.CODEC_AUTOPACK8, B.CODEC_AUTOPACK16, B.CODEC_AUTOPACK32, B.CODEC_AUTOPACK64,
           B.CODEC_AUTOPACK128)
    assert ids == (40, 41, 42, 43, 44)
    assert [B.codec_autopack(w) for w in M.WIDTHS] == [40, 41, 42, 43, 44]
    for bad in (0, 3, 5, 32, 64, -1, None, "8", 2.5):
        with pytest.raises(ValueError):
            B.codec_autopack(bad)
    for codec in ids:
        assert B.slot_size(codec, 65536) == 65792
        assert B.slot_size(codec, 1) == 256
        assert B.slot_size(codec, 59460) == 59648
        assert B.max_distance(codec) == 0
    for unknown in (7, 12, 16, 17, 20, 24, 25, 29, 30, 31, 37, 38, 39, 45, 99):
        assert B.slot_size(unknown, 100) == 0 and B.max_distance(unknown) == 0


def test_abi_is_untouched():
    import bitar_amd as B
    import test_abi
    assert B.lib().bitar_hip_abi_version() == 3
    assert sorted(B.ABI_SYMBOLS) == test_abi.header_symbols() and len(B.ABI_SYMBOLS) == 39
    assert not [s for s in B.ABI_SYMBOLS if "autopack" in s]
    assert B.codec_autopack(8) == 43  # (fails where the codec is absent)
