"""numpy restatement of the RANS codec (include/bitar_hip.h): test
infrastructure, written from the format's definition and sharing nothing with the kernels.

One stream per segment of L bytes (1..65536):

  byte 0      tag = 0xA0 | mode        mode 0 rans, 1 stored
  byte 1      0
  bytes 2..3  LE16(L - 1)
  stored:     L raw bytes                                            size = 4 + L
  rans:       bitmap   32 bytes, bit s (byte s >> 3, bit s & 7) set iff byte value s occurs
              freqs    for the k-th present symbol in ascending order, f - 1 in bits
                       [12k, 12k + 12) of a little-endian bit string, zero-padded to an EVEN
                       number of bytes
              words    nw little-endian 16-bit words, in the order the encoder emitted them
              states   64 x LE32, the encoder's final state of lane 0..63
  size = 36 + tsize + 2*nw + 256,   tsize = 2 * ceil(12 * nsym / 16)

Frequencies: c[s] the count of s, f[s] = 1 + floor(c[s] * (4096 - nsym) / L) for present s, the
deficit 4096 - sum(f) added to the most frequent symbol (the lowest value on a tie); cum[s] the
sum of f[t] over t < s.

Coder: 64 states of 32 bits, symbol i belongs to lane i % 64 and step i // 64, every state
starts at 2^16.  The encoder runs the steps from the last to the first; an active lane with
state x and symbol s emits x & 0xFFFF and shifts x right by 16 when x >= f[s] << 20, then
x = (x // f[s]) * 4096 + x % f[s] + cum[s].  A step's words are appended in ascending lane order.
The decoder runs the steps forward with p = nw: slot = x & 4095, s the symbol whose
[cum, cum + f) holds slot, x = f[s] * (x >> 12) + slot - cum[s]; the n lanes with x < 2^16 then
take x = x << 16 | words[p - n + r] (r their rank in lane order) and p -= n.

The rans form is taken iff its size is strictly below 4 + L.
"""
import numpy as np

MAX_SEG = 65536
LANES = 64
SCALE_BITS = 12
SCALE = 1 << SCALE_BITS
X0 = 1 << 16
FIXED = 36 + 256  # header, bitmap and states


def _header(mode, L):
    return bytes([0xA0 | mode, 0, (L - 1) & 255, (L - 1) >> 8])


def table_size(nsym):
    return 2 * ((12 * nsym + 15) // 16)


def normalise(counts):
    """counts (256 non-negative ints, not all zero) -> the 256 frequencies"""
    c = np.asarray(counts, np.int64)
    assert c.shape == (256,) and (c >= 0).all()
    L = int(c.sum())
    assert L >= 1
    present = c > 0
    nsym = int(present.sum())
    f = np.where(present, 1 + c * (SCALE - nsym) // L, 0)
    deficit = SCALE - int(f.sum())
    assert 0 <= deficit < nsym
    f[int(np.argmax(c))] += deficit  # (argmax: the first, so the lowest value, on a tie)
    assert int(f.sum()) == SCALE and (f[present] >= 1).all()
    return f


def pack_table(f):
    """-> the bitmap and the freqs field of the frequencies f"""
    f = np.asarray(f, np.int64)
    bitmap = np.packbits(f > 0, bitorder="little").tobytes()
    v = 0
    for k, s in enumerate(np.flatnonzero(f)):
        v |= (int(f[s]) - 1) << (12 * k)
    return bitmap + v.to_bytes(table_size(int((f > 0).sum())), "little")


def encode_words(segment, f):
    """the coder alone: -> (the emitted words, the 64 final states) of `segment` under the
    frequencies f (every byte value of the segment must have f >= 1)"""
    seg = np.ascontiguousarray(segment, np.uint8)
    L = seg.size
    f = np.asarray(f, np.int64)
    cum = np.cumsum(f) - f
    T = (L + LANES - 1) // LANES
    padded = np.zeros(T * LANES, np.uint8)
    padded[:L] = seg
    sym = padded.reshape(T, LANES)
    x = np.full(LANES, X0, np.int64)
    lanes = np.arange(LANES)
    words = []
    for t in range(T - 1, -1, -1):
        act = t * LANES + lanes < L
        fs, cs = f[sym[t]], cum[sym[t]]
        assert (fs[act] >= 1).all()
        emit = act & (x >= (fs << 20))
        words.append((x[emit] & 0xFFFF).astype("<u2"))
        x = np.where(emit, x >> 16, x)
        fs1 = np.where(act, fs, 1)
        x = np.where(act, (x // fs1) * SCALE + x % fs1 + cs, x)
        assert (x < 1 << 32).all() and (x >= X0).all()
    words = np.concatenate(words) if words else np.zeros(0, "<u2")
    return words, x.astype("<u4")


def rans_stream(L, f, words, states):
    """the rans form of a segment of L bytes from its parts as given"""
    return _header(0, L) + pack_table(f) + np.asarray(words, "<u2").tobytes() + \
        np.asarray(states, "<u4").tobytes()


def rans_form(segment):
    """the rans form of the segment whatever its size"""
    seg = np.ascontiguousarray(segment, np.uint8)
    f = normalise(np.bincount(seg, minlength=256))
    words, states = encode_words(seg, f)
    s = rans_stream(seg.size, f, words, states)
    assert len(s) == FIXED + table_size(int((f > 0).sum())) + 2 * words.size
    return s


def encode_segment(segment):
    seg = np.ascontiguousarray(segment, np.uint8)
    L = seg.size
    assert 1 <= L <= MAX_SEG
    s = rans_form(seg)
    return s if len(s) < 4 + L else _header(1, L) + seg.tobytes()


def encode(data, seg):
    """-> the list of per-segment streams of `data` cut into segments of `seg` bytes"""
    data = np.ascontiguousarray(data, np.uint8)
    return [encode_segment(data[o:o + seg]) for o in range(0, data.size, seg)]


def decode(stream, seg):
    """-> the segment's bytes, or None when the decoder must reject the stream"""
    s = bytes(stream)
    if len(s) < 4:
        return None
    tag = s[0]
    if tag >> 4 != 0xA or tag & 15 > 1 or s[1] != 0:
        return None
    L = 1 + s[2] + (s[3] << 8)
    if L > seg:
        return None
    if tag & 1:
        return s[4:] if len(s) == 4 + L else None
    if len(s) < FIXED + 2:
        return None
    present = np.unpackbits(np.frombuffer(s[4:36], np.uint8), bitorder="little").astype(bool)
    nsym = int(present.sum())
    if nsym == 0:
        return None
    tsize = table_size(nsym)
    rest = len(s) - FIXED - tsize
    if rest < 0 or rest & 1:
        return None
    nw = rest // 2
    bits = int.from_bytes(s[36:36 + tsize], "little")
    if bits >> (12 * nsym):
        return None  # (pad bits)
    f = np.zeros(256, np.int64)
    f[present] = [1 + (bits >> (12 * k) & 0xFFF) for k in range(nsym)]
    if int(f.sum()) != SCALE:
        return None
    cum = np.cumsum(f) - f
    slot2sym = np.repeat(np.arange(256), f)
    words = np.frombuffer(s[36 + tsize:36 + tsize + 2 * nw], "<u2").astype(np.int64)
    x = np.frombuffer(s[len(s) - 256:], "<u4").astype(np.int64)
    if (x < X0).any():
        return None
    T = (L + LANES - 1) // LANES
    out = np.zeros(T * LANES, np.uint8)
    lanes = np.arange(LANES)
    p = nw
    for t in range(T):
        act = t * LANES + lanes < L
        slot = x & (SCALE - 1)
        sym = slot2sym[slot]
        out[t * LANES:(t + 1) * LANES] = sym
        x = np.where(act, f[sym] * (x >> SCALE_BITS) + slot - cum[sym], x)
        need = x < X0
        n = int(need.sum())
        if n > p:
            return None
        x[need] = x[need] << 16 | words[p - n:p]
        p -= n
    if p != 0 or (x != X0).any():
        return None
    return out[:L].tobytes()


def entropy_bytes(segment):
    """the order-0 entropy of the segment, in bytes"""
    c = np.bincount(np.ascontiguousarray(segment, np.uint8), minlength=256).astype(np.float64)
    c = c[c > 0]
    return float(-(c * np.log2(c / c.sum())).sum() / 8)


def text_like(rng, n):
    """n bytes with the histogram of log-like text (letters by a Zipf law, spaces, digits,
    a few marks) and no structure beyond it"""
    alphabet = np.frombuffer(b" etaoinshrdlcumwfgypbvkjxqz0123456789.,:-=/[]\n\"ETAOINS_", np.uint8)
    p = 1.0 / (np.arange(alphabet.size) + 2.0)
    return rng.choice(alphabet, n, p=p / p.sum()).astype(np.uint8)
