"""numpy restatement of the CASCADE codec (include/bitar_hip.h): test
infrastructure, written from the format's definition on top of the RUNPACK model's runs and the
INTPACK model's streams, and sharing nothing with the kernels.

One stream per segment of L bytes (1..65536), element width w in {1, 2, 4, 8}, m = L // w
elements compared as byte patterns, the last L - m*w bytes are the tail:

  byte 0      tag = 0x80 | mode << 3 | log2(w)     mode 0 cascade, 1 stored
  byte 1      0
  bytes 2..3  LE16(L - 1)
  stored:     L raw bytes                                            size = 4 + L
  cascade:    LE16(r - 1)   r = number of runs, 1 <= r <= min(m, 32768)
              LE16(vsize - 1)
              values        an INTPACK stream (tag 0x4_, any of its three modes) of width w whose
                            "segment" is the r*w bytes of the runs' values; vsize bytes
              lengths       an INTPACK stream of width 2 whose "segment" is the 2r bytes
                            LE16(run length - 1) of the runs
              tail
  size = 8 + vsize + lsize + (L - m*w)

The encoder's runs are maximal, the two sub-streams are what intpack_model.encode_segment returns
for those bytes, and the cascade form is taken when r <= 32768 and its size is strictly below
4 + L; the stored form otherwise (m = 0 and a tie included).  The decoder also takes what no
encoder writes: equal neighbouring values, a sub-stream in a mode that is not its smallest, a
cascade form larger than 4 + L.
"""
import numpy as np

import intpack_model as IM
import runpack_model as RM

WIDTHS = (1, 2, 4, 8)
MAX_SEG = 65536
MAX_RUNS = 32768
_LOG = {1: 0, 2: 1, 4: 2, 8: 3}


def _header(mode, w, L):
    return bytes([0x80 | mode << 3 | _LOG[w], 0, (L - 1) & 255, (L - 1) >> 8])


def _le16(v):
    return bytes([v & 255, v >> 8])


def cascade_stream(L, w, r, values, lengths, tail=b""):
    """the cascade form of a segment of L bytes with r runs from the two sub-streams as given"""
    return _header(0, w, L) + _le16(r - 1) + _le16(len(values) - 1) + bytes(values) + \
        bytes(lengths) + bytes(tail)


def encode_segment(segment, w):
    segment = np.ascontiguousarray(segment, np.uint8)
    L = segment.size
    assert 1 <= L <= MAX_SEG and w in WIDTHS
    m = L // w
    stored = _header(1, w, L) + segment.tobytes()
    if m == 0:
        return stored
    values, lengths = RM._runs(segment, w)
    r = lengths.size
    if r > MAX_RUNS:
        return stored
    vs = IM.encode_segment(values.reshape(-1), w)
    ls = IM.encode_segment((lengths - 1).astype("<u2").view(np.uint8), 2)
    if not 8 + len(vs) + len(ls) + (L - m * w) < 4 + L:
        return stored
    s = cascade_stream(L, w, r, vs, ls, segment[m * w:].tobytes())
    assert len(s) == 8 + len(vs) + len(ls) + (L - m * w)
    return s


def encode(data, w, seg):
    """-> the list of per-segment streams of `data` cut into segments of `seg` bytes"""
    data = np.ascontiguousarray(data, np.uint8)
    return [encode_segment(data[o:o + seg], w) for o in range(0, data.size, seg)]


def _sub(stream, w, n):
    """the n elements of width w of an INTPACK sub-stream, or None when it must be rejected"""
    if len(stream) < 4 or stream[0] & 3 != _LOG[w]:
        return None
    if 1 + stream[2] + (stream[3] << 8) != n * w:
        return None
    return IM.decode(stream, n * w)  # (its own rules; L <= "seg" holds: they are equal)


def decode(stream, seg):
    """-> the segment's bytes, or None when the decoder must reject the stream"""
    s = bytes(stream)
    if len(s) < 4:
        return None
    tag = s[0]
    lg = tag & 7
    if tag >> 4 != 8 or lg > 3 or s[1] != 0:
        return None
    w = 1 << lg
    L = 1 + s[2] + (s[3] << 8)
    if L > seg:
        return None
    if tag & 8:
        return s[4:] if len(s) == 4 + L else None
    if len(s) < 8:
        return None
    m = L // w
    tail = L - m * w
    r = 1 + s[4] + (s[5] << 8)
    vsize = 1 + s[6] + (s[7] << 8)
    if r > min(m, MAX_RUNS) or len(s) < 8 + vsize + 4 + tail:
        return None
    values = _sub(s[8:8 + vsize], w, r)
    lengths = _sub(s[8 + vsize:len(s) - tail], 2, r)
    if values is None or lengths is None:
        return None
    lengths = np.frombuffer(lengths, "<u2").astype(np.int64) + 1
    if int(lengths.sum()) != m:
        return None
    rows = np.frombuffer(values, np.uint8).reshape(r, w)
    return np.repeat(rows, lengths, axis=0).tobytes() + s[len(s) - tail:len(s)]
