"""Python restatement of the DECPACK codec (include/bitar_hip_codecs.h): test
infrastructure, written from the format's definition with Python integers and sharing nothing
with the kernels.

One stream per segment of L bytes (1..65536), w = 16, m = L // 16 little-endian elements read as
integers mod 2^128, the last L - 16 m bytes are the tail:

  byte 0      tag = 0xD0 | mode << 2 | (log2(w) - 4)   mode 0 plain, 1 delta, 2 stored
  byte 1      0
  bytes 2..3  LE16(L - 1)
  stored:     L raw bytes
  packed:     [mode 1: base = element 0, 16 bytes]
              widths[nmb]  one byte, 0..128, per miniblock of 64 elements, nmb = ceil(m / 64)
              refs[nblk]   16 bytes each, per block of 4 miniblocks, nblk = ceil(nmb / 4)
              payload      miniblock k = 8 * widths[k] bytes, element t at bits [t*b, (t+1)*b) of
                           the little-endian bit string, slots past m pack as 0
              tail

mode 0: x_i = v_i.  mode 1: x_i = v_i - v_(i-1) mod 2^128 for i >= 1, x_0 = x_1 (0 when m = 1).
ref = the block's smallest x read as signed; residual = x - ref mod 2^128; widths[k] = bit length
of the miniblock's largest residual.  Mode 1 only when strictly smaller than mode 0; stored when
the winner is not strictly smaller than 4 + L.
"""
W = 16
MAX_SEG = 65536
MASK = (1 << 128) - 1
TAG = 0xD0


def _counts(L):
    m = L // W
    nmb = (m + 63) // 64
    return m, nmb, (nmb + 3) // 4


def elements(segment):
    """the m elements of a segment's bytes, unsigned"""
    segment = bytes(segment)
    return [int.from_bytes(segment[i:i + W], "little") for i in range(0, len(segment) // W * W, W)]


def _signed(x):
    return x - (1 << 128) if x >> 127 else x


def _values(v, mode):
    if mode == 0:
        return list(v)
    x = [0] + [(b - a) & MASK for a, b in zip(v, v[1:])]
    if len(v) > 1:
        x[0] = x[1]
    return x


def _plan(x):
    """-> (widths, refs (unsigned), residuals)"""
    refs = [min(x[o:o + 256], key=_signed) for o in range(0, len(x), 256)]
    r = [(xi - refs[i // 256]) & MASK for i, xi in enumerate(x)]
    widths = [max(r[o:o + 64]).bit_length() for o in range(0, len(x), 64)]
    return widths, refs, r


def size(L, mode, widths):
    m, nmb, nblk = _counts(L)
    return 4 + (W if mode == 1 else 0) + nmb + W * nblk + 8 * sum(widths) + (L - W * m)


def _pack(r, widths):
    out = []
    for k, b in enumerate(widths):
        bits = 0
        for t, v in enumerate(r[64 * k:64 * k + 64]):
            assert v >> b == 0
            bits |= v << (t * b)
        out.append(bits.to_bytes(8 * b, "little"))
    return b"".join(out)


def _header(mode, L):
    return bytes([TAG | mode << 2, 0, (L - 1) & 255, (L - 1) >> 8])


def stored_stream(segment):
    segment = bytes(segment)
    return _header(2, len(segment)) + segment


def packed_stream(data, mode, widths=None):
    """the packed form of one segment's bytes in the given mode (0 or 1), whatever its size;
    `widths` forces the miniblocks' widths (each at least what the residuals need)"""
    data = bytes(data)
    L = len(data)
    assert 1 <= L <= MAX_SEG and mode in (0, 1)
    v = elements(data)
    need, refs, r = _plan(_values(v, mode))
    if widths is None:
        widths = need
    widths = [int(b) for b in widths]
    assert len(widths) == len(need) and all(n <= b <= 128 for n, b in zip(need, widths))
    s = _header(mode, L) + (data[:W] if mode == 1 else b"") + bytes(widths) + \
        b"".join(x.to_bytes(W, "little") for x in refs) + _pack(r, widths) + data[len(v) * W:]
    assert len(s) == size(L, mode, widths)
    return s


def packed_sizes(segment):
    """(size of mode 0, size of mode 1) of one segment's bytes"""
    v = elements(segment)
    return tuple(size(len(segment), mode, _plan(_values(v, mode))[0]) for mode in (0, 1))


def encode_segment(segment):
    segment = bytes(segment)
    L = len(segment)
    assert 1 <= L <= MAX_SEG
    sizes = packed_sizes(segment)
    mode = 1 if sizes[1] < sizes[0] else 0
    if not sizes[mode] < 4 + L:
        return stored_stream(segment)
    return packed_stream(segment, mode)


def encode(data, seg):
    """-> the list of per-segment streams of `data` cut into segments of `seg` bytes"""
    data = bytes(data)
    return [encode_segment(data[o:o + seg]) for o in range(0, len(data), seg)]


def mode_of(stream):
    return (stream[0] >> 2) & 3


def widths_of(stream):
    """the widths array of a packed stream"""
    mode = mode_of(stream)
    assert mode in (0, 1)
    L = 1 + stream[2] + (stream[3] << 8)
    p = 4 + (W if mode == 1 else 0)
    return list(stream[p:p + _counts(L)[1]])


def decode(stream, seg):
    """-> the segment's bytes, or None when the decoder must reject the stream"""
    s = bytes(stream)
    if len(s) < 4:
        return None
    tag, mode = s[0], (s[0] >> 2) & 3
    if tag >> 4 != 0xD or mode == 3 or tag & 3 or s[1] != 0:
        return None
    L = 1 + s[2] + (s[3] << 8)
    if L > seg:
        return None
    if mode == 2:
        return s[4:] if len(s) == 4 + L else None
    m, nmb, nblk = _counts(L)
    p = 4 + (W if mode == 1 else 0)
    if len(s) < p + nmb + W * nblk:
        return None
    widths = list(s[p:p + nmb])
    if any(b > 128 for b in widths) or len(s) != size(L, mode, widths):
        return None
    q = p + nmb
    refs = [int.from_bytes(s[q + W * i:q + W * i + W], "little") for i in range(nblk)]
    q += W * nblk
    x = []
    for k, b in enumerate(widths):
        bits = int.from_bytes(s[q:q + 8 * b], "little")
        q += 8 * b
        for t in range(64):
            x.append(((bits >> (t * b)) & ((1 << b) - 1)) + refs[k // 4] & MASK)
    x = x[:m]
    if mode == 1 and m:
        x[0] = int.from_bytes(s[4:4 + W], "little")
        for i in range(1, m):
            x[i] = (x[i] + x[i - 1]) & MASK
    return b"".join(v.to_bytes(W, "little") for v in x) + s[q:]
