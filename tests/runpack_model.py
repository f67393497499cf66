"""numpy restatement of the RUNPACK codec (include/bitar_hip.h): test
infrastructure, written from the format's definition and sharing nothing with the kernels.

One stream per segment of L bytes (1..65536), element width w in {1, 2, 4, 8, 16}, m = L // w
elements compared as byte patterns (+0.0 and -0.0, and NaNs of different payloads, are distinct
values), the last L - m*w bytes are the tail:

  byte 0      tag = 0x70 | mode << 3 | log2(w)     mode 0 runs, 1 stored
  byte 1      bl, bytes per run length: 1 or 2 (0 in the stored form)
  bytes 2..3  LE16(L - 1)
  stored:     L raw bytes                                            size = 4 + L
  runs:       LE16(r - 1)   r = number of runs, 1 <= r <= m
              values[r]     each run's element, w bytes, in order
              lengths[r]    (run length - 1), bl bytes each, little-endian
              tail
  size = 6 + r*(w + bl) + (L - m*w)

The encoder's runs are maximal, bl is 1 when every run is at most 256 elements long and 2
otherwise, and the runs form is taken when its size is strictly below 4 + L; the stored form
otherwise (m = 0 and a tie included).  The decoder also takes what no encoder writes: equal
neighbouring values, bl = 2 where 1 would do, a runs form larger than 4 + L.
"""
import numpy as np

WIDTHS = (1, 2, 4, 8, 16)
MAX_SEG = 65536
_LOG = {1: 0, 2: 1, 4: 2, 8: 3, 16: 4}


def _header(mode, w, bl, L):
    return bytes([0x70 | mode << 3 | _LOG[w], bl, (L - 1) & 255, (L - 1) >> 8])


def runs_size(L, w, r, bl):
    """the runs form's size of a segment of L bytes with r runs and bl bytes per length"""
    return 6 + r * (w + bl) + (L - L // w * w)


def _runs(segment, w):
    """-> (the rows that start a maximal run, every run's length)"""
    m = segment.size // w
    rows = segment[:m * w].reshape(m, w)
    head = np.ones(m, bool)
    head[1:] = np.any(rows[1:] != rows[:-1], axis=1)
    at = np.flatnonzero(head)
    return rows[at], np.diff(np.append(at, m))


def encode_segment(segment, w):
    segment = np.ascontiguousarray(segment, np.uint8)
    L = segment.size
    assert 1 <= L <= MAX_SEG and w in WIDTHS
    m = L // w
    stored = _header(1, w, 0, L) + segment.tobytes()
    if m == 0:
        return stored
    values, lengths = _runs(segment, w)
    r = lengths.size
    bl = 1 if lengths.max() <= 256 else 2
    if not runs_size(L, w, r, bl) < 4 + L:
        return stored
    s = _header(0, w, bl, L) + bytes([(r - 1) & 255, (r - 1) >> 8]) + values.tobytes() + \
        (lengths - 1).astype("<u1" if bl == 1 else "<u2").tobytes() + segment[m * w:].tobytes()
    assert len(s) == runs_size(L, w, r, bl)
    return s


def encode(data, w, seg):
    """-> the list of per-segment streams of `data` cut into segments of `seg` bytes"""
    data = np.ascontiguousarray(data, np.uint8)
    return [encode_segment(data[o:o + seg], w) for o in range(0, data.size, seg)]


def decode(stream, seg):
    """-> the segment's bytes, or None when the decoder must reject the stream"""
    s = np.frombuffer(bytes(stream), np.uint8)
    if s.size < 4:
        return None
    tag, bl = int(s[0]), int(s[1])
    lg = tag & 7
    if tag >> 4 != 7 or lg > 4:
        return None
    w = 1 << lg
    L = 1 + int(s[2]) + (int(s[3]) << 8)
    if L > seg:
        return None
    if tag & 8:
        return s[4:].tobytes() if bl == 0 and s.size == 4 + L else None
    if bl not in (1, 2) or s.size < 6:
        return None
    m = L // w
    r = 1 + int(s[4]) + (int(s[5]) << 8)
    if r > m or s.size != runs_size(L, w, r, bl):
        return None
    values = s[6:6 + r * w].reshape(r, w)
    lengths = s[6 + r * w:6 + r * (w + bl)].view("<u1" if bl == 1 else "<u2").astype(np.int64) + 1
    if int(lengths.sum()) != m:  # (a python int: up to 2^32 and never wrapped)
        return None
    return np.repeat(values, lengths, axis=0).tobytes() + s[s.size - (L - m * w):s.size].tobytes()
