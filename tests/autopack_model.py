"""numpy restatement of AUTOPACK (include/bitar_hip.h): test infrastructure,
built from the four codecs' models and adding only the choice and the tag dispatch.

AUTOPACK has no format of its own.  A segment's stream is the shortest of its candidates'
streams for that segment and element width w, a tie going to the earlier candidate:

  w = 1, 2    RUNPACK, INTPACK
  w = 4, 8    RUNPACK, INTPACK, DICTPACK, FLTPACK
  w = 16      RUNPACK, DICTPACK

The decoder gives a stream whose byte 0 has the high nibble 4, 5, 6 or 7 to INTPACK's, FLTPACK's,
DICTPACK's or RUNPACK's decoder and rejects every other stream, the empty one included.
"""
import numpy as np

import dictpack_model as DM
import fltpack_model as FM
import intpack_model as IM
import runpack_model as RM

WIDTHS = (1, 2, 4, 8, 16)
MAX_SEG = 65536
# in the rule's order; a model is a candidate at the widths it has
ORDER = (("RUNPACK", RM), ("INTPACK", IM), ("DICTPACK", DM), ("FLTPACK", FM))
CANDIDATES = {w: tuple(name for name, M in ORDER if w in M.WIDTHS) for w in WIDTHS}
MODELS = dict(ORDER)
# the high nibble of byte 0 -> the format
NIBBLES = {4: "INTPACK", 5: "FLTPACK", 6: "DICTPACK", 7: "RUNPACK"}


def candidate_streams(segment, w):
    """-> [(name, stream)] of every candidate of the width, in the rule's order"""
    return [(name, MODELS[name].encode_segment(segment, w)) for name in CANDIDATES[w]]


def encode_segment(segment, w):
    streams = [s for _, s in candidate_streams(segment, w)]
    return min(streams, key=len)  # (min keeps the first of equals)


def encode(data, w, seg):
    """-> the list of per-segment streams of `data` cut into segments of `seg` bytes"""
    data = np.ascontiguousarray(data, np.uint8)
    return [encode_segment(data[o:o + seg], w) for o in range(0, data.size, seg)]


def format_of(stream):
    """the format a stream's tag names, or None"""
    return NIBBLES.get(stream[0] >> 4) if len(stream) else None


def decode(stream, seg):
    """-> the segment's bytes, or None when the decoder must reject the stream"""
    name = format_of(bytes(stream))
    return None if name is None else MODELS[name].decode(stream, seg)
