"""numpy restatement of the FLTPACK codec (include/bitar_hip.h): test
infrastructure, written from the format's definition and sharing nothing with the kernels.

One stream per segment of L bytes (1..65536), element width w in {4, 8} (IEEE float / double),
m = L // w little-endian elements, the last L - m*w bytes are the tail:

  byte 0      tag = 0x50 | mode << 2 | log2(w)     mode 0 packed, 2 stored
  byte 1      e, the decimal exponent, 0..15 (0 in the stored form)
  bytes 2..3  LE16(L - 1)
  stored:     L raw bytes
  packed:     LE16 nx      number of exceptions, nx <= m
              widths[nmb]  one byte per miniblock of 64 elements, nmb = ceil(m / 64)
              refs[nblk]   one w-byte LE signed reference per block of 4 miniblocks
              payload      miniblock k = 8 * widths[k] bytes, element t at bits [t*b, (t+1)*b) of
                           the little-endian bit string
              pos[nx]      LE16 element indices, strictly increasing, each < m
              val[nx]      the exceptions' raw w-byte elements, in the same order
              tail
  size = 6 + nmb + nblk*w + 8*sum(widths) + nx*(2 + w) + (L - m*w)

An element v is encodable at e when t = rint(double(v) * 10^e) is finite, |t| <= 2^53 (w = 8) or
2^31 - 1 (w = 4), and double(n) / 10^e for n = int(t), rounded to float for w = 4, has exactly
the bit pattern of v.  Everything else is an exception.  ref = the block's smallest n over its
encodable elements (0 without any); residual = n - ref mod 2^(8w), 0 at exceptions and past m.

The exponent: over the sample (elements 0, 16, 32, ...), for each e the cost is
x_e * (8w + 16) + (count - x_e) * b_e with x_e the sample's exceptions and b_e the bit length
of max n - min n over its encodable elements (0 without any); the smallest cost wins, the
smallest e among equals.  Stored when the packed size at that e is not strictly below 4 + L.
"""
import numpy as np

WIDTHS = (4, 8)
MAX_SEG = 65536
MAX_EXP = 15
_U = {4: np.dtype("<u4"), 8: np.dtype("<u8")}
_S = {4: np.dtype("<i4"), 8: np.dtype("<i8")}
_F = {4: np.dtype("<f4"), 8: np.dtype("<f8")}
_LIMIT = {4: float(2 ** 31 - 1), 8: float(2 ** 53)}
POW10 = np.array([float(10 ** e) for e in range(16)], np.float64)


def _counts(L, w):
    m = L // w
    nmb = (m + 63) // 64
    return m, nmb, (nmb + 3) // 4


def to_float(n, w, e):
    """the elements (unsigned bit patterns) that the signed integers n stand for at e"""
    with np.errstate(all="ignore"):
        q = n.astype(np.float64) / POW10[e]
        return q.astype(_F[w]).view(_U[w])


def to_int(u, w, e):
    """-> (encodable, n) of the elements with the bit patterns u; n is 0 where not encodable"""
    with np.errstate(all="ignore"):
        t = np.rint(u.view(_F[w]).astype(np.float64) * POW10[e])
        ok = np.isfinite(t) & (np.abs(t) <= _LIMIT[w])
        n = np.where(ok, t, 0.0).astype(_S[w])
    ok &= to_float(n, w, e) == u
    n[~ok] = 0
    return ok, n


def choose_exponent(u, w):
    sample = u[::16]
    best, best_cost = 0, None
    for e in range(MAX_EXP + 1):
        ok, n = to_int(sample, w, e)
        good = int(ok.sum())
        x = sample.size - good
        b = (int(n[ok].max()) - int(n[ok].min())).bit_length() if good else 0
        cost = x * (8 * w + 16) + good * b
        if best_cost is None or cost < best_cost:
            best, best_cost = e, cost
    return best


def _plan(ok, n, w):
    """-> (widths, refs (signed), residuals padded to nmb x 64)"""
    m = n.size
    _, nmb, nblk = _counts(m * w, w)
    top = np.iinfo(_S[w]).max
    s = np.full(nblk * 256, top, dtype=_S[w])
    s[:m] = np.where(ok, n, top)
    g = np.zeros(nblk * 256, bool)
    g[:m] = ok
    refs = np.where(g.reshape(nblk, 256).any(axis=1), s.reshape(nblk, 256).min(axis=1), 0)
    refs = refs.astype(_S[w])
    r = np.zeros(nblk * 256, dtype=_U[w])
    r[:m] = (n.view(_U[w]) - np.repeat(refs.view(_U[w]), 256)[:m]) * ok.astype(_U[w])
    r = r.reshape(nblk * 4, 64)[:nmb]
    widths = np.array([int(v).bit_length() for v in r.max(axis=1)], np.uint8)
    return widths, refs, r


def _size(L, w, widths, nx):
    m, nmb, nblk = _counts(L, w)
    return 6 + nmb + nblk * w + 8 * int(np.asarray(widths).sum(dtype=np.int64)) + nx * (2 + w) + \
        (L - m * w)


def _pack(r, widths):
    """the payload of the miniblocks r (nmb x 64) at the given widths"""
    out = []
    for row, b in zip(r, widths):
        b = int(b)
        if b:
            bits = ((row[:, None] >> np.arange(b, dtype=r.dtype)) & 1).astype(np.uint8)
            out.append(np.packbits(bits.reshape(-1), bitorder="little").tobytes())
    return b"".join(out)


def _header(mode, w, e, L):
    return bytes([0x50 | mode << 2 | (2 if w == 4 else 3), e, (L - 1) & 255, (L - 1) >> 8])


def _packed(segment, w, e):
    """the packed form of a segment at the exponent e (whatever its size)"""
    L = segment.size
    m = L // w
    u = segment[:m * w].view(_U[w])
    ok, n = to_int(u, w, e)
    widths, refs, r = _plan(ok, n, w)
    pos = np.flatnonzero(~ok)
    s = _header(0, w, e, L) + int(pos.size).to_bytes(2, "little") + widths.tobytes() + \
        refs.tobytes() + _pack(r, widths) + pos.astype("<u2").tobytes() + u[pos].tobytes() + \
        segment[m * w:].tobytes()
    assert len(s) == _size(L, w, widths, pos.size)
    return s


def packed_size(segment, w, e=None):
    """the size of the packed form of one segment's bytes (at the chosen exponent unless given)"""
    segment = np.ascontiguousarray(segment, np.uint8)
    if e is None:
        e = choose_exponent(segment[:segment.size // w * w].view(_U[w]), w)
    return len(_packed(segment, w, e))


def encode_segment(segment, w):
    segment = np.ascontiguousarray(segment, np.uint8)
    L = segment.size
    assert 1 <= L <= MAX_SEG and w in WIDTHS
    e = choose_exponent(segment[:L // w * w].view(_U[w]), w)
    s = _packed(segment, w, e)
    if not len(s) < 4 + L:
        return _header(2, w, 0, L) + segment.tobytes()
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
    tag, mode, lg, e = int(s[0]), (int(s[0]) >> 2) & 3, int(s[0]) & 3, int(s[1])
    if tag >> 4 != 5 or mode in (1, 3) or lg < 2 or e > MAX_EXP:
        return None
    w = 1 << lg
    L = 1 + int(s[2]) + (int(s[3]) << 8)
    if L > seg:
        return None
    if mode == 2:
        return s[4:].tobytes() if e == 0 and s.size == 4 + L else None
    m, nmb, nblk = _counts(L, w)
    if s.size < 6:
        return None
    nx = int(s[4]) + (int(s[5]) << 8)
    if nx > m or s.size < 6 + nmb + nblk * w:
        return None
    widths = s[6:6 + nmb]
    if np.any(widths > 8 * w) or s.size != _size(L, w, widths, nx):
        return None
    q = 6 + nmb
    refs = s[q:q + nblk * w].view(_U[w])
    q += nblk * w
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
    n = (r.reshape(-1)[:m] + np.repeat(refs, 256)[:m]).astype(_U[w]).view(_S[w])
    out = to_float(n, w, e)
    out[pos] = val
    return out.tobytes() + s[q:].tobytes()
