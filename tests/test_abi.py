"""CPU tests of the C-ABI boundary: the library builds, loads, and exports every symbol
include/bitar_hip.h declares.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

import bitar_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    with open(os.path.join(ROOT, "include", "bitar_hip.h")) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(bitar_hip_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(bitar_amd.LIB_PATH):
        bitar_amd.build()
    L = ctypes.CDLL(bitar_amd.LIB_PATH)
    declared = header_symbols()
    assert len(declared) >= 19
    for name in declared:
        assert hasattr(L, name), name
    assert sorted(bitar_amd.ABI_SYMBOLS) == declared


def test_abi_version_and_slot_sizes():
    L = bitar_amd.lib()
    assert L.bitar_hip_abi_version() == 3
    # LZ4_compressBound(65536) = 65809 -> 256-B rounded slot
    assert bitar_amd.slot_size(bitar_amd.CODEC_LZ4, 65536) == 66048
    assert bitar_amd.slot_size(bitar_amd.CODEC_LZ4, 59460) >= 59460 + 59460 // 255 + 16
    assert bitar_amd.slot_size(bitar_amd.CODEC_DEFLATE, 59460) >= (59460 * 9 + 7) // 8 + 16
    assert bitar_amd.slot_size(99, 100) == 0


def test_encoder_reach():
    """bitar_hip_max_distance: the encoders' match-distance cap, which the oracle restates
    (BO_MAX_DIST / the wide parse's cap) and the front-end reports as its window."""
    B = bitar_amd
    for c in (B.CODEC_LZ4, B.CODEC_DEFLATE, B.CODEC_DEFLATE_DYNAMIC, B.CODEC_ZSTD):
        assert B.max_distance(c) == 2560
    assert B.max_distance(B.CODEC_LZ4_WIDE) == 14848
    assert B.max_distance(99) == 0


# bitar_hip_slot_size(id, seg) for seg in SLOT_SEGS, and bitar_hip_max_distance(id), of every id
# 0..63 as the library gave them before the column codecs shared one table: an id not listed gives
# 0 for both (the gaps between the families: 7, 12-17, 20-25, 29-31, 37-39, 45 and up).  A column
# codec's max distance of 0 is "none", an unlisted id's is "unknown".
SLOT_SEGS = (1, 7, 4096, 59460, 65536)
_COLUMN_SLOTS = (256, 256, 4352, 59648, 65792)
SLOTS_AND_REACH = {
    1: ((256, 256, 4352, 59904, 66048), 2560),
    2: ((256, 256, 4864, 67072, 73984), 2560),
    3: ((768, 768, 4864, 60160, 66304), 2560),
    4: ((256, 256, 4864, 67072, 73984), 2560),
    5: ((256, 256, 4352, 59904, 66048), 14848),
    6: ((256, 256, 4352, 59648, 65792), 2560),
    8: (_COLUMN_SLOTS, 0), 9: (_COLUMN_SLOTS, 0), 10: (_COLUMN_SLOTS, 0), 11: (_COLUMN_SLOTS, 0),
    18: (_COLUMN_SLOTS, 0), 19: (_COLUMN_SLOTS, 0),
    26: (_COLUMN_SLOTS, 0), 27: (_COLUMN_SLOTS, 0), 28: (_COLUMN_SLOTS, 0),
    32: (_COLUMN_SLOTS, 0), 33: (_COLUMN_SLOTS, 0), 34: (_COLUMN_SLOTS, 0), 35: (_COLUMN_SLOTS, 0),
    36: (_COLUMN_SLOTS, 0),
    40: (_COLUMN_SLOTS, 0), 41: (_COLUMN_SLOTS, 0), 42: (_COLUMN_SLOTS, 0), 43: (_COLUMN_SLOTS, 0),
    44: (_COLUMN_SLOTS, 0),
}


def test_slot_sizes_and_reach_of_every_id():
    B = bitar_amd
    for codec in range(64):
        slots, reach = SLOTS_AND_REACH.get(codec, ((0,) * len(SLOT_SEGS), 0))
        assert tuple(B.slot_size(codec, seg) for seg in SLOT_SEGS) == slots, codec
        assert B.max_distance(codec) == reach, codec


# family -> (its widths, the text of its ValueError)
COLUMN_WIDTHS = {
    "INTPACK": ((1, 2, 4, 8), "1, 2, 4 or 8"),
    "FLTPACK": ((4, 8), "4 or 8"),
    "DICTPACK": ((4, 8, 16), "4, 8 or 16"),
    "RUNPACK": ((1, 2, 4, 8, 16), "1, 2, 4, 8 or 16"),
    "AUTOPACK": ((1, 2, 4, 8, 16), "1, 2, 4, 8 or 16"),
}


def header_codecs():
    with open(os.path.join(ROOT, "include", "bitar_hip.h")) as f:
        text = f.read()
    return {name: int(value) for name, value in
            re.findall(r"\bBITAR_HIP_CODEC_([A-Z]+PACK[0-9]+)\s*=\s*([0-9]+)", text)}


@pytest.mark.parametrize("family", sorted(COLUMN_WIDTHS))
def test_column_codec_ids_are_the_headers(family):
    widths, text = COLUMN_WIDTHS[family]
    header = header_codecs()
    assert sum(len(w) for w, _ in COLUMN_WIDTHS.values()) == len(header) == 19
    codec_of = getattr(bitar_amd, "codec_" + family.lower())
    for w in widths:
        assert codec_of(w) == header[f"{family}{8 * w}"]
        assert getattr(bitar_amd, f"CODEC_{family}{8 * w}") == header[f"{family}{8 * w}"]
    for w in (0, 3, 5, 32, 64, -1, 2.5, "4", None, [4], *range(1, 17)):
        if w in widths:
            continue
        with pytest.raises(ValueError) as e:
            codec_of(w)
        assert str(e.value) == f"{family} element width must be {text}, not {w!r}"


def test_no_device_is_not_an_error_for_count():
    # in the build container there is no GPU: the count is 0, not a crash
    n = bitar_amd.device_count()
    assert n >= 0
