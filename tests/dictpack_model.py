"""numpy restatement of the DICTPACK codec (include/bitar_hip.h): test
infrastructure, written from the format's definition and sharing nothing with the kernels.

One stream per segment of L bytes (1..65536), element width w in {4, 8, 16}, m = L // w elements
compared as byte patterns (+0.0 and -0.0, and NaNs of different payloads, are distinct values),
the last L - m*w bytes are the tail:

  byte 0      tag = 0x60 | mode << 3 | log2(w)     mode 0 packed, 1 stored; log2(w) 2, 3 or 4
  byte 1      0
  bytes 2..3  LE16(L - 1)
  stored:     L raw bytes                                            size = 4 + L
  packed:     LE16(d - 1)   d = number of dictionary entries, 1 <= d <= min(m, 1024)
              dict[d]       the distinct elements, w bytes each, in order of first occurrence
              payload       nmb = ceil(m / 64) miniblocks of 8*b bytes, b = bit_length(d - 1)
                            (b = 0, no payload, when d = 1); element t's dictionary index at bits
                            [t*b, (t+1)*b) of the miniblock's little-endian bit string; slots
                            past m are written as 0
              tail
  size = 6 + d*w + 8*b*nmb + (L - m*w)

Packed when the segment has at most 1024 distinct elements and the packed size is below 4 + L;
stored otherwise (m = 0 included).  The sizes differ by 2 mod 4 for every w here, so they are
never equal and `<` and `<=` are the same rule.  The decoder ignores bits in slots past m and
accepts duplicate dictionary entries; an index >= d in a slot below m rejects the stream.
"""
import numpy as np

WIDTHS = (4, 8, 16)
MAX_SEG = 65536
MAX_DICT = 1024
_LOG = {4: 2, 8: 3, 16: 4}


def _header(mode, w, L):
    return bytes([0x60 | mode << 3 | _LOG[w], 0, (L - 1) & 255, (L - 1) >> 8])


def packed_size(L, w, d):
    """the packed form's size of a segment of L bytes with d distinct elements"""
    m = L // w
    return 6 + d * w + 8 * (d - 1).bit_length() * ((m + 63) // 64) + (L - m * w)


def _indices(segment, w):
    """-> (dictionary rows in order of first occurrence, every element's index into it)"""
    m = segment.size // w
    rows = segment[:m * w].reshape(m, w)
    keys = np.ascontiguousarray(rows).view(np.dtype((np.void, w))).reshape(m)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    rank = np.empty(first.size, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    return rows[np.sort(first)], rank[inverse.reshape(m)]


def _pack(idx, b):
    """the payload of the indices at b bits each, padded with 0 to whole miniblocks"""
    if b == 0:
        return b""
    nmb = (idx.size + 63) // 64
    v = np.zeros(nmb * 64, np.uint32)
    v[:idx.size] = idx
    bits = ((v[:, None] >> np.arange(b, dtype=np.uint32)) & 1).astype(np.uint8)
    return np.packbits(bits.reshape(-1), bitorder="little").tobytes()


def encode_segment(segment, w):
    segment = np.ascontiguousarray(segment, np.uint8)
    L = segment.size
    assert 1 <= L <= MAX_SEG and w in WIDTHS
    m = L // w
    stored = _header(1, w, L) + segment.tobytes()
    if m == 0:
        return stored
    entries, idx = _indices(segment, w)
    d = entries.shape[0]
    if d > MAX_DICT or not packed_size(L, w, d) < 4 + L:
        return stored
    s = _header(0, w, L) + bytes([(d - 1) & 255, (d - 1) >> 8]) + entries.tobytes() + \
        _pack(idx, (d - 1).bit_length()) + segment[m * w:].tobytes()
    assert len(s) == packed_size(L, w, d)
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
    tag = int(s[0])
    lg = tag & 7
    if tag >> 4 != 6 or not 2 <= lg <= 4 or s[1] != 0:
        return None
    w = 1 << lg
    L = 1 + int(s[2]) + (int(s[3]) << 8)
    if L > seg:
        return None
    if tag & 8:
        return s[4:].tobytes() if s.size == 4 + L else None
    if s.size < 6:
        return None
    m = L // w
    d = 1 + int(s[4]) + (int(s[5]) << 8)
    if d > min(m, MAX_DICT) or s.size != packed_size(L, w, d):
        return None
    b = (d - 1).bit_length()
    entries = s[6:6 + d * w].reshape(d, w)
    idx = np.zeros(m, np.int64)
    if b:
        nmb = (m + 63) // 64
        bits = np.unpackbits(s[6 + d * w:6 + d * w + 8 * b * nmb], bitorder="little")
        idx = (bits.reshape(nmb * 64, b).astype(np.int64) << np.arange(b)).sum(axis=1)[:m]
    if np.any(idx >= d):
        return None
    return entries[idx].tobytes() + s[s.size - (L - m * w):s.size].tobytes()
