"""The decimal128 columns DECPACK is measured on: Arrow's 16-byte little-endian
two's-complement integers.  Shared by the model's tests, the GPU tests, smoke() and
scripts/measure_decpack.py."""
import numpy as np


def decimal128(lo, hi):
    """n 16-byte elements from their low (uint64) and high (int64 or uint64) halves -> bytes"""
    out = np.empty((len(lo), 2), "<u8")
    out[:, 0] = np.asarray(lo).astype(np.uint64)
    out[:, 1] = np.asarray(hi).astype(np.int64).view(np.uint64)
    return out.view(np.uint8).reshape(-1)


def from_int64(v):
    """int64 values sign-extended to decimal128 -> bytes"""
    v = np.asarray(v, np.int64)
    return decimal128(v.view(np.uint64), v >> 63)


def prices(rng, n):
    """n bytes of DECIMAL(12,2) prices, unscaled values uniform in [0, 10^7)"""
    return from_int64(rng.integers(0, 10**7, n // 16))


def signed_amounts(rng, n):
    """n bytes of signed amounts in +-10^6: high bytes 00 and FF side by side"""
    return from_int64(rng.integers(-10**6, 10**6 + 1, n // 16))


def running_total(rng, n):
    """n bytes of an ascending running total of steps below 10^6 that starts 10^6 steps' worth
    below 2^64 and passes it: the sum carries out of the low 64 bits (delta mode)"""
    m = n // 16
    step = rng.integers(1, 10**6, m).astype(np.uint64)
    start = np.uint64(2**64 - (10**6 // 2) * min(m, 4096) // 2)
    lo = start + np.cumsum(step, dtype=np.uint64)  # (wraps mod 2^64)
    hi = np.cumsum(np.concatenate([[lo[0] < start], lo[1:] < lo[:-1]]).astype(np.int64))
    return decimal128(lo, hi)


def random_values(rng, n):
    """n bytes of random 16-byte values: stored"""
    return rng.integers(0, 256, n // 16 * 16, dtype=np.uint8)


def table_columns(n=1 << 16, seed=3000):
    """-> [(name, bytes)], n bytes each, from a fresh generator"""
    rng = np.random.default_rng(seed)
    return [
        ("DECIMAL(12,2) prices, uniform in [0, 1e7)", prices(rng, n)),
        ("signed amounts in +-1e6", signed_amounts(rng, n)),
        ("ascending running total that passes 2^64", running_total(rng, n)),
        ("random 16-byte values", random_values(rng, n)),
    ]


# ---- the shapes of the tests: Python integers -> bytes -------------------------------------------

MASK = (1 << 128) - 1
MOST_NEGATIVE = 1 << 127  # the two's-complement pattern of -2^127
EDGE_WIDTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)


def to_bytes(values, L=None):
    """integers (mod 2^128) as 16-byte little-endian elements -> uint8 array, cut to L bytes"""
    b = b"".join((int(v) & MASK).to_bytes(16, "little") for v in values)
    return np.frombuffer(b if L is None else b[:L], np.uint8).copy()


def _ints(rng, n, bits):
    """n random integers below 2^bits"""
    if bits == 0:
        return [0] * n
    raw = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    return [int.from_bytes(r.tobytes(), "little") >> (128 - bits) for r in raw]


def width_segment(L, place, seed, widths=EDGE_WIDTHS, shift=0):
    """L bytes whose miniblock k takes width widths[(k + shift) % len] in mode 0: residuals below
    2^b over the block's reference, the largest one (2^b - 1) in the miniblock's first
    (place = 0) or last (place = -1) element, a zero residual in another.  A block with a
    miniblock of 127 or 128 bits has the most negative value for its reference, the others a
    reference on either side of 0, so that the values straddle 0 and the residuals wrap."""
    rng = np.random.default_rng(seed)
    m = L // 16
    out = []
    for blk in range(0, m, 256):
        ks = range(blk // 64, (min(blk + 256, m) + 63) // 64)
        bs = [widths[(k + shift) % len(widths)] for k in ks]
        if max(bs) >= 127:
            ref = -(1 << 127)
        else:
            ref = -_ints(rng, 1, 60)[0] if (blk // 256) % 2 == 0 else _ints(rng, 1, 100)[0]
        for k, b in zip(ks, bs):
            count = min(64, m - 64 * k)
            r = _ints(rng, count, b)
            at = 0 if place == 0 else count - 1
            r[at] = (1 << b) - 1
            if count > 1:
                r[(at + 1) % count] = 0
            out += [ref + x for x in r]
    out.append(_ints(rng, 1, 128)[0])  # the bytes of a cut element behind them
    return to_bytes(out, L)


def delta_segment(L, kind, seed):
    """L bytes of a column that takes the delta mode: "asc" steps of 61..62 bits from just below
    2^64, so that the running sum carries out of the low 64 bits every few elements, inside
    miniblocks and across their edges; "desc" the same downwards from 2^100 (negative deltas);
    "step" small steps after a jump of 2^100 at element 1 (x_0 = x_1)"""
    rng = np.random.default_rng(seed)
    m = L // 16
    step = [(1 << 61) + x for x in _ints(rng, m + 1, 61)]
    if kind == "asc":
        v, sign = (1 << 64) - 5, 1
    elif kind == "desc":
        v, sign = (1 << 100) + 7, -1
    else:
        v, sign = 3, 1
        step = [(1 << 100)] + [1 + x for x in _ints(rng, m, 12)]
    out = []
    for s in step:
        out.append(v)
        v += sign * s
    return to_bytes(out, L)


def noise_segment(L, seed):
    return np.random.default_rng(seed).integers(0, 256, L, dtype=np.uint8)


KINDS = ("plain", "noise", "asc", "noise", "desc", "plain-last", "step", "asc")


def segment(kind, L, seed):
    if kind == "plain":
        return width_segment(L, 0, seed, shift=seed)
    if kind == "plain-last":
        return width_segment(L, -1, seed, shift=seed)
    if kind == "noise":
        return noise_segment(L, seed)
    return delta_segment(L, kind, seed)


def column(nseg, seg, seed, extra=0):
    """nseg segments of seg bytes, the kinds in turn, and `extra` more bytes"""
    parts = [segment(KINDS[i % len(KINDS)], seg, seed + i) for i in range(nseg)]
    if extra:
        parts.append(segment("plain-last", extra, seed + nseg))
    return np.concatenate(parts)


# ---- hostile streams -------------------------------------------------------------------------------

def base_streams(model, seg):
    """a stream of each mode, of a segment that ends inside a miniblock and has a tail"""
    L = seg - 5 * 16 - 3
    out = []
    for kind, mode in (("plain-last", 0), ("asc", 1), ("noise", 2)):
        (s,) = model.encode(segment(kind, L, seg + mode), seg)
        assert model.mode_of(s) == mode
        out.append(s)
    return out


def mutants(s):
    """deterministic mutations of the stream s -> [(bytes, size given to the decoder)]"""
    out = [(s, len(s))]

    def poke(at, value):
        if 0 <= at < len(s) and s[at] != value & 255:
            t = bytearray(s)
            t[at] = value & 255
            out.append((bytes(t), len(s)))

    for at in range(4):  # every bit of the four header bytes
        for bit in range(8):
            poke(at, s[at] ^ (1 << bit))
    for nib in range(16):  # the tag's nibble, its mode, its low bits
        poke(0, nib << 4 | s[0] & 15)
    for mode in range(4):
        poke(0, s[0] & ~12 | mode << 2)
    for low in range(4):
        poke(0, s[0] & ~3 | low)
    out += [(s, len(s) + 1), (s, len(s) - 1), (s, 0), (s, 3), (s, 5), (s, 19)]
    out.append((s + bytes(16), len(s) + 16))
    mode = (s[0] >> 2) & 3
    if mode == 2:
        return out
    L = 1 + s[2] + (s[3] << 8)
    m = L // 16
    nmb = (m + 63) // 64
    wid_at = 4 + (16 if mode == 1 else 0)
    for k in sorted({0, nmb // 2, nmb - 1}):
        for value in (s[wid_at + k] + 1, s[wid_at + k] - 1, 129, 0xFF):
            if 0 <= value <= 255:
                poke(wid_at + k, value)
    ref_at = wid_at + nmb
    pay_at = ref_at + (nmb + 3) // 4 * 16
    end = len(s) - (L - 16 * m)
    places = [ref_at, ref_at + 15, pay_at, (pay_at + end) // 2, end - 1]
    if mode == 1:
        places += [4, 19]
    for at in places:  # the base element, a reference, payload bytes: other bytes, accepted
        poke(at, s[at] ^ 1)
        poke(at, s[at] ^ 0x80)
    if L > 16 * m:
        poke(len(s) - 1, s[-1] ^ 0xFF)
    return out


def given(t, size):
    """the `size` bytes the decoder is given of the mutant t: cut, or padded as the slab is"""
    return t[:size] if size <= len(t) else t + b"\x5a" * (size - len(t))
