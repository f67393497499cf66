"""CPU test of the runtime's codec tables: bitar_hip_slot_size and bitar_hip_max_distance of every
id 0..255 against tests/golden/codec_table.json, recorded from the library before its four id
chains (the two validity checks, the slot bound, the reach) became one lookup.  An id the file
does not list gives 0 for both.  No compute calls (no GPU here)."""
import json
import os

import bitar_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "codec_table.json")) as f:
    GOLDEN = json.load(f)
SEGS = (1, 255, 4096, 59460, 65536)


def test_golden_covers_the_segment_sizes():
    assert tuple(GOLDEN["segs"]) == SEGS
    assert all(0 <= int(c) < 256 and len(row["slot_size"]) == len(SEGS)
               for c, row in GOLDEN["codecs"].items())


def test_slot_size_of_every_id():
    if not os.path.exists(bitar_amd.LIB_PATH):
        bitar_amd.build()
    for codec in range(256):
        row = GOLDEN["codecs"].get(str(codec))
        want = row["slot_size"] if row else [0] * len(SEGS)
        assert [bitar_amd.slot_size(codec, seg) for seg in SEGS] == want, codec


def test_max_distance_of_every_id():
    for codec in range(256):
        row = GOLDEN["codecs"].get(str(codec))
        assert bitar_amd.max_distance(codec) == (row["max_distance"] if row else 0), codec
