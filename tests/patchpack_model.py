"""numpy restatement of the PATCHPACK codec (include/bitar_hip.h): test
infrastructure, written from the format's definition and sharing nothing with the kernels (the
block plan and the bit packing are intpack_model's, whose format PATCHPACK extends).

One stream per segment of L bytes (1..65536), element width w in {1, 2, 4, 8}, m = L // w
little-endian elements, the last L - m*w bytes are the tail:

  byte 0      tag = 0x90 | mode << 2 | log2(w)     mode 0 plain, 1 delta, 2 stored, 3 complement
  byte 1      0
  bytes 2..3  LE16(L - 1)
  stored:     L raw bytes
  packed:     LE16 nx      number of exceptions
              [mode 1: base = element 0, w bytes]
              widths[nmb]  one byte per miniblock of 64 elements, nmb = ceil(m / 64)
              refs[nblk]   one w-byte LE reference per block of 4 miniblocks, nblk = ceil(nmb / 4)
              payload      miniblock k = 8 * widths[k] bytes, INTPACK's packing; the slots of the
                           exceptions and of the elements past m pack as 0
              pos[nx]      LE16 element indices, strictly increasing, each < m
              val[nx]      the exceptions' x, w bytes each
              tail

mode 0: x_i = v_i.  mode 3: x_i = ~v_i.  mode 1: x_i = v_i - v_(i-1) mod 2^(8w), x_0 = x_1 (0
when m = 1).  ref = the block's minimum x read as signed (exceptions included); residual r = x -
ref mod 2^(8w).  In a miniblock with bit lengths l_t and B = max l_t, cost(b) = 8 b + (2 + w) *
#{t : l_t > b} for b = 0..B; widths[k] is the LARGEST b of minimal cost and the exceptions are the
elements with l_t > widths[k].  The smallest of the three packed sizes wins, a tie goes to plain,
then delta, then complement; stored when the winner is not strictly smaller than 4 + L.
"""
import numpy as np

import intpack_model as IM

WIDTHS = IM.WIDTHS
MAX_SEG = IM.MAX_SEG
MODES = (0, 1, 3)  # the packed modes, in the order ties are broken
_U = IM._U


def _counts(L, w):
    return IM._counts(L, w)


def _values(v, mode):
    """the x_i of a segment's elements v (unsigned dtype)"""
    if mode == 3:
        return ~v
    return IM._values(v, mode)


def _bit_lengths(r):
    bl = np.zeros(r.shape, np.int64)
    for b in range(8 * r.dtype.itemsize):
        bl += (r >> r.dtype.type(b)) != 0
    return bl


def rule_widths(bl, w):
    """the width rule: bl = bit lengths (nmb x 64, 0 in the slots past m) -> widths (nmb,)"""
    b = np.arange(8 * w + 1)
    n = (bl[:, :, None] > b).sum(axis=1)  # n(b), [miniblock, b]
    cost = 8 * b + (2 + w) * n  # (for b > B: 8 b > 8 B = cost(B), never the minimum)
    best = cost.min(axis=1, keepdims=True)
    return (8 * w - np.argmax((cost == best)[:, ::-1], axis=1)).astype(np.uint8)


def _plan(x, w, widths=None):
    """-> (widths, refs, residuals nmb x 64 with the exceptions' slots 0, positions of the
    exceptions); widths: forced ones (the exceptions are then what does not fit them)"""
    _, refs, r = IM._plan(x, w)
    bl = _bit_lengths(r)
    if widths is None:
        widths = rule_widths(bl, w)
    widths = np.asarray(widths, np.uint8)
    exc = bl > widths[:, None].astype(np.int64)
    r = np.where(exc, r.dtype.type(0), r)
    return widths, refs, r, np.flatnonzero(exc.reshape(-1))


def _size(L, w, mode, widths, nx):
    m, nmb, nblk = _counts(L, w)
    return 6 + (w if mode == 1 else 0) + nmb + nblk * w + 8 * int(widths.sum(dtype=np.int64)) + \
        nx * (2 + w) + (L - m * w)


def _header(mode, w, L):
    return bytes([0x90 | mode << 2 | WIDTHS.index(w), 0, (L - 1) & 255, (L - 1) >> 8])


def packed_sizes(segment, w):
    """(size of mode 0, of mode 1, of mode 3) of one segment's bytes"""
    segment = np.asarray(segment, np.uint8)
    L = segment.size
    v = segment[:L // w * w].view(_U[w])
    out = []
    for mode in MODES:
        widths, _, _, pos = _plan(_values(v, mode), w)
        out.append(_size(L, w, mode, widths, pos.size))
    return tuple(out)


def packed_stream(segment, w, mode, widths=None):
    """the packed form of a segment in the given mode, whether or not an encoder would choose
    it; with forced widths (each 0..8w) whatever does not fit becomes an exception"""
    segment = np.ascontiguousarray(segment, np.uint8)
    L = segment.size
    assert 1 <= L <= MAX_SEG and w in WIDTHS and mode in MODES
    m = L // w
    v = segment[:m * w].view(_U[w])
    x = _values(v, mode)
    widths, refs, r, pos = _plan(x, w, widths)
    assert pos.size <= min(m, 65535)
    s = _header(mode, w, L) + bytes([pos.size & 255, pos.size >> 8]) + \
        ((v[:1].tobytes() if m else bytes(w)) if mode == 1 else b"") + widths.tobytes() + \
        refs.astype(_U[w]).tobytes() + IM._pack(r, widths) + pos.astype("<u2").tobytes() + \
        x[pos].astype(_U[w]).tobytes() + segment[m * w:].tobytes()
    assert len(s) == _size(L, w, mode, widths, pos.size)
    return s


def encode_segment(segment, w):
    segment = np.ascontiguousarray(segment, np.uint8)
    L = segment.size
    assert 1 <= L <= MAX_SEG and w in WIDTHS
    sizes = packed_sizes(segment, w)
    best = min(range(3), key=lambda i: (sizes[i], i))
    if not sizes[best] < 4 + L:
        return _header(2, w, L) + segment.tobytes()
    return packed_stream(segment, w, MODES[best])


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
    if tag >> 4 != 9 or s[1] != 0:
        return None
    w = WIDTHS[tag & 3]
    L = 1 + int(s[2]) + (int(s[3]) << 8)
    if L > seg:
        return None
    if mode == 2:
        return s[4:].tobytes() if s.size == 4 + L else None
    m, nmb, nblk = _counts(L, w)
    if s.size < 6:
        return None
    nx = int(s[4]) + (int(s[5]) << 8)
    if nx > m:
        return None
    p = 6 + (w if mode == 1 else 0)
    if s.size < p + nmb + nblk * w:
        return None
    widths = s[p:p + nmb]
    if np.any(widths > 8 * w) or s.size != _size(L, w, mode, widths, nx):
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
    pos = s[q:q + 2 * nx].view("<u2").astype(np.int64)
    q += 2 * nx
    if np.any(pos >= m) or np.any(pos[1:] <= pos[:-1]):
        return None
    val = s[q:q + nx * w].view(_U[w])
    q += nx * w
    x = (r.reshape(-1)[:m] + np.repeat(refs, 256)[:m]).astype(_U[w])
    x[pos] = val  # (whatever the exceptions' slots hold is ignored)
    if mode == 1 and m:
        x[0] = s[6:6 + w].view(_U[w])[0]
        x = np.cumsum(x, dtype=_U[w])
    if mode == 3:
        x = ~x
    return x.tobytes() + s[q:].tobytes()
