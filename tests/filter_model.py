"""numpy restatement of the per-segment filters (include/bitar_hip.h, bitar_hip_filter_apply /
_invert): test infrastructure, written from the definition and sharing nothing with the kernel.

S = the L bytes of a segment, w = the element width:
  SHUFFLE     m = L // w;  T[j*m + i] = S[i*w + j];  the last L - m*w bytes keep their places.
  BITSHUFFLE  m8 = (L // w) & ~7;  plane p = 8*j + b occupies T[p*(m8/8), (p+1)*(m8/8)), and bit
              t of its byte q is bit b of S[(8q + t)*w + j];  the last L - m8*w bytes keep theirs.
"""
import numpy as np

SHUFFLE, BITSHUFFLE = 1, 2
WIDTHS = (2, 4, 8, 16)
SEGMENT_ERROR = 0xFFFFFFFF


def shuffle(s, w):
    s = np.asarray(s, np.uint8)
    m = s.size // w
    return np.concatenate([s[:m * w].reshape(m, w).T.reshape(-1), s[m * w:]])


def unshuffle(t, w):
    t = np.asarray(t, np.uint8)
    m = t.size // w
    return np.concatenate([t[:m * w].reshape(w, m).T.reshape(-1), t[m * w:]])


def bitshuffle(s, w):
    s = np.asarray(s, np.uint8)
    m8 = (s.size // w) & ~7
    body = s[:m8 * w].reshape(m8, w)
    # bits[i, j, b] = bit b of byte j of element i
    bits = np.unpackbits(body.reshape(m8, w, 1), axis=2, bitorder="little")
    # plane (j, b) = the bit of elements 0..m8-1, packed LSB first
    planes = np.packbits(bits.transpose(1, 2, 0).reshape(w * 8, m8), axis=1, bitorder="little")
    return np.concatenate([planes.reshape(-1), s[m8 * w:]])


def unbitshuffle(t, w):
    t = np.asarray(t, np.uint8)
    m8 = (t.size // w) & ~7
    planes = t[:m8 * w].reshape(w * 8, m8 // 8)
    bits = np.unpackbits(planes, axis=1, bitorder="little").reshape(w, 8, m8)
    body = np.packbits(bits.transpose(2, 0, 1), axis=2, bitorder="little")
    return np.concatenate([body.reshape(-1), t[m8 * w:]])


_FWD = {SHUFFLE: shuffle, BITSHUFFLE: bitshuffle}
_INV = {SHUFFLE: unshuffle, BITSHUFFLE: unbitshuffle}


def _segments(fn, data, w, seg, lens, out):
    """segment i (lens[i] bytes, or min(seg, n - i*seg)) of `data` through fn into a copy of
    `out`; a length above min(seg, n - i*seg) leaves the segment's output as it was"""
    data = np.asarray(data, np.uint8)
    n = data.size
    res = np.zeros(n, np.uint8) if out is None else np.array(out, np.uint8)
    nseg = (n + seg - 1) // seg if lens is None else len(lens)
    for i in range(nseg):
        off = i * seg
        if off >= n:
            break
        room = min(seg, n - off)
        ln = room if lens is None else int(lens[i])
        if ln > room:
            continue
        res[off:off + ln] = fn(data[off:off + ln], w)
    return res


def apply(filt, data, w, seg, lens=None, out=None):
    return _segments(_FWD[filt], data, w, seg, lens, out)


def invert(filt, data, w, seg, lens=None, out=None):
    return _segments(_INV[filt], data, w, seg, lens, out)
