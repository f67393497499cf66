"""numpy restatement of the INTPACK codec (include/bitar_hip.h): test
infrastructure, written from the format's definition and sharing nothing with the kernels.

One stream per segment of L bytes (1..65536), element width w in {1, 2, 4, 8}, m = L // w
little-endian elements, the last L - m*w bytes are the tail:

  byte 0      tag = 0x40 | mode << 2 | log2(w)     mode 0 packed, 1 packed with delta, 2 stored
  byte 1      0
  bytes 2..3  LE16(L - 1)
  stored:     L raw bytes
  packed:     [mode 1: base = element 0, w bytes]
              widths[nmb]  one byte per miniblock of 64 elements, nmb = ceil(m / 64)
              refs[nblk]   one w-byte LE reference per block of 4 miniblocks, nblk = ceil(nmb / 4)
              payload      miniblock k = 8 * widths[k] bytes, element t at bits [t*b, (t+1)*b) of
                           the little-endian bit string, elements past m pack as 0
              tail

mode 0: x_i = v_i.  mode 1: x_i = v_i - v_(i-1) mod 2^(8w) for i >= 1, x_0 = x_1 (0 when m = 1).
ref = the block's minimum x read as signed; residual = x - ref mod 2^(8w), read unsigned;
widths[k] = bit length of the miniblock's largest residual.  Mode 1 only when strictly smaller
than mode 0; stored when the winner is not strictly smaller than 4 + L.
"""
import numpy as np

WIDTHS = (1, 2, 4, 8)
MAX_SEG = 65536
_U = {1: np.uint8, 2: np.dtype("<u2"), 4: np.dtype("<u4"), 8: np.dtype("<u8")}
_S = {1: np.int8, 2: np.dtype("<i2"), 4: np.dtype("<i4"), 8: np.dtype("<i8")}


def _counts(L, w):
    m = L // w
    nmb = (m + 63) // 64
    return m, nmb, (nmb + 3) // 4


def _values(v, mode):
    """the x_i of a segment's elements v (unsigned dtype)"""
    if mode == 0:
        return v.copy()
    x = np.zeros_like(v)
    x[1:] = v[1:] - v[:-1]  # (unsigned: wraps mod 2^(8w))
    if v.size > 1:
        x[0] = x[1]
    return x


def _plan(x, w):
    """-> (widths, refs (unsigned), residuals padded to nmb x 64)"""
    m = x.size
    _, nmb, nblk = _counts(m * w, w)
    s = np.full(nblk * 256, np.iinfo(_S[w]).max, dtype=_S[w])
    s[:m] = x.view(_S[w])
    refs = s.reshape(nblk, 256).min(axis=1).view(_U[w])
    r = np.zeros(nblk * 256, dtype=_U[w])
    r[:m] = x - np.repeat(refs, 256)[:m]
    r = r.reshape(nblk * 4, 64)[:nmb]
    widths = np.array([int(v).bit_length() for v in r.max(axis=1)], np.uint8)
    return widths, refs, r


def _size(L, w, mode, widths):
    m, nmb, nblk = _counts(L, w)
    return 4 + (w if mode == 1 else 0) + nmb + nblk * w + 8 * int(widths.sum(dtype=np.int64)) + \
        (L - m * w)


def _pack(r, widths):
    """the payload of the miniblocks r (nmb x 64) at the given widths"""
    out = [None] * len(widths)
    for b in np.unique(widths):
        b = int(b)
        rows = np.flatnonzero(widths == b)
        if b == 0:
            for k in rows:
                out[k] = b""
            continue
        sh = np.arange(b, dtype=r.dtype)
        bits = ((r[rows][:, :, None] >> sh) & 1).astype(np.uint8)  # [row, element, bit]
        packed = np.packbits(bits.reshape(len(rows), 64 * b), axis=1, bitorder="little")
        for n, k in enumerate(rows):
            out[k] = packed[n].tobytes()
    return b"".join(out)


def _header(mode, w, L):
    return bytes([0x40 | mode << 2 | WIDTHS.index(w), 0, (L - 1) & 255, (L - 1) >> 8])


def packed_sizes(segment, w):
    """(size of mode 0, size of mode 1) of one segment's bytes"""
    segment = np.asarray(segment, np.uint8)
    L = segment.size
    v = segment[:L // w * w].view(_U[w])
    return tuple(_size(L, w, mode, _plan(_values(v, mode), w)[0]) for mode in (0, 1))


def encode_segment(segment, w):
    segment = np.ascontiguousarray(segment, np.uint8)
    L = segment.size
    assert 1 <= L <= MAX_SEG and w in WIDTHS
    m = L // w
    v = segment[:m * w].view(_U[w])
    plans = [_plan(_values(v, mode), w) for mode in (0, 1)]
    sizes = [_size(L, w, mode, plans[mode][0]) for mode in (0, 1)]
    mode = 1 if sizes[1] < sizes[0] else 0
    if not sizes[mode] < 4 + L:
        return _header(2, w, L) + segment.tobytes()
    widths, refs, r = plans[mode]
    s = _header(mode, w, L) + (v[:1].tobytes() if mode == 1 else b"") + widths.tobytes() + \
        refs.astype(_U[w]).tobytes() + _pack(r, widths) + segment[m * w:].tobytes()
    assert len(s) == sizes[mode]
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
    tag, mode = int(s[0]), (int(s[0]) >> 2) & 3
    if tag >> 4 != 4 or mode == 3 or s[1] != 0:
        return None
    w = WIDTHS[tag & 3]
    L = 1 + int(s[2]) + (int(s[3]) << 8)
    if L > seg:
        return None
    if mode == 2:
        return s[4:].tobytes() if s.size == 4 + L else None
    m, nmb, nblk = _counts(L, w)
    p = 4 + (w if mode == 1 else 0)
    if s.size < p + nmb + nblk * w:
        return None
    widths = s[p:p + nmb]
    if np.any(widths > 8 * w) or s.size != _size(L, w, mode, widths):
        return None
    refs = s[p + nmb:p + nmb + nblk * w].view(_U[w])
    q = p + nmb + nblk * w
    r = np.zeros((nmb, 64), _U[w])
    for k in range(nmb):
        b = int(widths[k])
        if b:
            bits = np.unpackbits(s[q:q + 8 * b], bitorder="little").reshape(64, b)
            r[k] = (bits.astype(_U[w]) << np.arange(b, dtype=_U[w])).sum(axis=1, dtype=_U[w])
            q += 8 * b
    x = (r.reshape(-1)[:m] + np.repeat(refs, 256)[:m]).astype(_U[w])
    if mode == 1 and m:
        x[0] = s[4:4 + w].view(_U[w])[0]
        x = np.cumsum(x, dtype=_U[w])
    return x.tobytes() + s[q:].tobytes()
