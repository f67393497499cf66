"""numpy restatement of the RANSPLANE codec (include/bitar_hip.h): test
infrastructure, written from the format's definition and sharing nothing with the kernels.

RANS (rans_model.py) with one order-0 table per byte plane of an element of w = 2, 4 or 8 bytes.
One stream per segment of L bytes (1..65536), lg = log2(w):

  byte 0      0xB0 | mode << 3 | lg    mode 0 planes, 1 stored
  byte 1      0
  bytes 2..3  LE16(L - 1)
  stored:     L raw bytes                                            size = 4 + L
  planes:     bitmaps  w x 32 bytes, plane 0 first; in plane p's bitmap bit s (byte s >> 3,
                       bit s & 7) is set iff byte value s occurs among the bytes i < L with
                       i % w == p (i counts from the segment's first byte)
              freqs    w fields, plane 0 first, each RANS's freqs field of that plane
              words    nw little-endian 16-bit words, in the order the encoder emitted them
              states   64 x LE32, the encoder's final state of lane 0..63
  size = 4 + 32w + sum(tsize_p) + 2*nw + 256,   tsize_p = 2 * ceil(12 * nsym_p / 16)

Frequencies per plane: RANS's rule over the plane's n_p bytes.  Coder: RANS's, with the f and
cum of plane i % w for symbol i (lane i % 64, step i // 64; 64 is a multiple of w, so a lane
codes one plane for the whole segment).

The planes form is taken iff L >= w and its size is strictly below 4 + L.
"""
import numpy as np

from rans_model import LANES, MAX_SEG, SCALE, SCALE_BITS, X0, normalise, pack_table, table_size

WIDTHS = (2, 4, 8)
NIBBLE = 0xB


def lg_of(w):
    assert w in WIDTHS
    return w.bit_length() - 1


def fixed_size(w):
    """header, bitmaps and states"""
    return 4 + 32 * w + 256


def _header(mode, w, L):
    return bytes([0xB0 | mode << 3 | lg_of(w), 0, (L - 1) & 255, (L - 1) >> 8])


def plane_counts(segment, w):
    """-> the w histograms (w x 256) of the segment's byte planes"""
    seg = np.ascontiguousarray(segment, np.uint8)
    return np.stack([np.bincount(seg[p::w], minlength=256) for p in range(w)])


def normalise_planes(segment, w):
    """-> the w x 256 frequencies of a segment of at least w bytes"""
    return np.stack([normalise(c) for c in plane_counts(segment, w)])


def encode_words(segment, f):
    """the coder alone: -> (the emitted words, the 64 final states) of `segment` under the
    per-plane frequencies f (w x 256)"""
    seg = np.ascontiguousarray(segment, np.uint8)
    f = np.asarray(f, np.int64)
    w = f.shape[0]
    L = seg.size
    cum = np.cumsum(f, axis=1) - f
    T = (L + LANES - 1) // LANES
    padded = np.zeros(T * LANES, np.uint8)
    padded[:L] = seg
    sym = padded.reshape(T, LANES)
    lanes = np.arange(LANES)
    plane = lanes % w
    x = np.full(LANES, X0, np.int64)
    words = []
    for t in range(T - 1, -1, -1):
        act = t * LANES + lanes < L
        fs, cs = f[plane, sym[t]], cum[plane, sym[t]]
        assert (fs[act] >= 1).all()
        emit = act & (x >= (fs << 20))
        words.append((x[emit] & 0xFFFF).astype("<u2"))
        x = np.where(emit, x >> 16, x)
        fs1 = np.where(act, fs, 1)
        x = np.where(act, (x // fs1) * SCALE + x % fs1 + cs, x)
        assert (x < 1 << 32).all() and (x >= X0).all()
    words = np.concatenate(words) if words else np.zeros(0, "<u2")
    return words, x.astype("<u4")


def planes_stream(L, f, words, states):
    """the planes form of a segment of L bytes from its parts as given (f: w x 256)"""
    f = np.asarray(f, np.int64)
    w = f.shape[0]
    tables = [pack_table(fp) for fp in f]
    return _header(0, w, L) + b"".join(t[:32] for t in tables) + b"".join(t[32:] for t in tables) + \
        np.asarray(words, "<u2").tobytes() + np.asarray(states, "<u4").tobytes()


def planes_form(segment, w):
    """the planes form of a segment of at least w bytes, whatever its size"""
    seg = np.ascontiguousarray(segment, np.uint8)
    assert seg.size >= w
    f = normalise_planes(seg, w)
    words, states = encode_words(seg, f)
    s = planes_stream(seg.size, f, words, states)
    assert len(s) == fixed_size(w) + sum(table_size(int((fp > 0).sum())) for fp in f) + 2 * words.size
    return s


def stored_form(segment, w):
    seg = np.ascontiguousarray(segment, np.uint8)
    return _header(1, w, seg.size) + seg.tobytes()


def encode_segment(segment, w):
    seg = np.ascontiguousarray(segment, np.uint8)
    L = seg.size
    assert 1 <= L <= MAX_SEG
    if L >= w:
        s = planes_form(seg, w)
        if len(s) < 4 + L:
            return s
    return stored_form(seg, w)


def encode(data, seg, w):
    """-> the list of per-segment streams of `data` cut into segments of `seg` bytes"""
    data = np.ascontiguousarray(data, np.uint8)
    return [encode_segment(data[o:o + seg], w) for o in range(0, data.size, seg)]


def decode(stream, seg, w):
    """-> the segment's bytes under the id of width w, or None when the decoder must reject"""
    s = bytes(stream)
    if len(s) < 4:
        return None
    tag = s[0]
    if tag >> 4 != NIBBLE or (tag & 7) != lg_of(w) or s[1] != 0:
        return None
    L = 1 + s[2] + (s[3] << 8)
    if L > seg:
        return None
    if tag & 8:
        return s[4:] if len(s) == 4 + L else None
    if L < w or len(s) < 4 + 32 * w:
        return None
    present = np.unpackbits(np.frombuffer(s[4:4 + 32 * w], np.uint8), bitorder="little") \
        .astype(bool).reshape(w, 256)
    nsym = present.sum(axis=1)
    if (nsym == 0).any():
        return None
    tsize = [table_size(int(n)) for n in nsym]
    rest = len(s) - fixed_size(w) - sum(tsize)
    if rest < 0 or rest & 1:
        return None
    nw = rest // 2
    f = np.zeros((w, 256), np.int64)
    at = 4 + 32 * w
    for p in range(w):
        bits = int.from_bytes(s[at:at + tsize[p]], "little")
        at += tsize[p]
        if bits >> (12 * int(nsym[p])):
            return None  # (pad bits)
        f[p, present[p]] = [1 + (bits >> (12 * k) & 0xFFF) for k in range(int(nsym[p]))]
        if int(f[p].sum()) != SCALE:
            return None
    cum = np.cumsum(f, axis=1) - f
    slot2sym = np.stack([np.repeat(np.arange(256), fp) for fp in f])
    words = np.frombuffer(s[at:at + 2 * nw], "<u2").astype(np.int64)
    x = np.frombuffer(s[len(s) - 256:], "<u4").astype(np.int64)
    if (x < X0).any():
        return None
    T = (L + LANES - 1) // LANES
    out = np.zeros(T * LANES, np.uint8)
    lanes = np.arange(LANES)
    plane = lanes % w
    p = nw
    for t in range(T):
        act = t * LANES + lanes < L
        slot = x & (SCALE - 1)
        sym = slot2sym[plane, slot]
        out[t * LANES:(t + 1) * LANES] = sym
        x = np.where(act, f[plane, sym] * (x >> SCALE_BITS) + slot - cum[plane, sym], x)
        need = x < X0
        n = int(need.sum())
        if n > p:
            return None
        x[need] = x[need] << 16 | words[p - n:p]
        p -= n
    if p != 0 or (x != X0).any():
        return None
    return out[:L].tobytes()


def shuffle(segment, w):
    """the byte shuffle filter of one segment: plane 0's bytes, then plane 1's ...; the bytes
    past the last whole element stay where they are"""
    seg = np.ascontiguousarray(segment, np.uint8)
    n = seg.size // w * w
    return np.concatenate([seg[:n].reshape(-1, w).T.reshape(-1), seg[n:]])
