"""Inputs and mutated streams shared by the RANSPLANE tests (test_ransplane_model.py on the CPU,
test_gpu_ransplane.py on the device): test infrastructure."""
import numpy as np

import rans_cases as RC
import ransplane_model as M
from rans_model import table_size

rnd = RC.rnd


# ---- the inputs of DESIGN 4.26's ratio table: name -> (element width, generator of n bytes) ------

def bf16_weights(rng, n):
    """N(0, 0.02) float32 truncated to its high 16 bits"""
    x = rng.normal(0, 0.02, n // 2).astype("<f4")
    return (x.view("<u4") >> 16).astype("<u2").view(np.uint8)


def f16_normal(rng, n):
    return rng.normal(0, 0.02, n // 2).astype("<f2").view(np.uint8)


def f32_normal(rng, n):
    return rng.normal(0, 1, n // 4).astype("<f4").view(np.uint8)


def f32_walk(rng, n):
    return np.cumsum(rng.normal(0, 0.01, n // 4)).astype("<f4").view(np.uint8)


def f64_normal(rng, n):
    return rng.normal(0, 1, n // 8).astype("<f8").view(np.uint8)


def i64_timestamps(rng, n):
    """millisecond timestamps whose steps jitter over 0..2000"""
    steps = rng.integers(0, 2001, n // 8)
    return (1_700_000_000_000 + np.cumsum(steps)).astype("<i8").view(np.uint8)


TABLE_INPUTS = {
    "bf16 weights": (2, bf16_weights),
    "float16 N(0, 0.02)": (2, f16_normal),
    "float32 N(0, 1)": (4, f32_normal),
    "float32 walk": (4, f32_walk),
    "float64 N(0, 1)": (8, f64_normal),
    "int64 ms timestamps": (8, i64_timestamps),
}


def table_input(name, nseg=8, seg=65536):
    """-> (w, the bytes) of a row of the table: nseg segments from default_rng(0)"""
    w, gen = TABLE_INPUTS[name]
    return w, np.ascontiguousarray(gen(np.random.default_rng(0), nseg * seg))


# ---- shapes ------------------------------------------------------------------------------------

def interleave(planes):
    """w equally long byte arrays -> the segment whose plane p is planes[p]"""
    return np.ascontiguousarray(np.stack(planes, axis=1)).reshape(-1)


def sparse(n, w, seed):
    """a constant plane 0, few symbols in the others: every plane compresses if anything does"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 3, n, dtype=np.uint8) + 0x30
    out[::w] = 0x7F
    return out


def plane_shapes(n, w, seed):
    """planes of every shape in one segment: a constant (f = 4096: the lane never emits), 2
    symbols, 17, a skewed 256 and noise, in turn over the w planes"""
    m = (n + w - 1) // w
    kinds = (lambda k: np.full(m, 0xC3, np.uint8),
             lambda k: RC.two_symbols(m, seed + k),
             lambda k: RC.alphabet(m, 17, seed + k),
             lambda k: RC.alphabet(m, 256, seed + k),
             lambda k: RC.rnd(m, seed + k))
    order = {2: (0, 3), 4: (0, 1, 2, 4), 8: (0, 1, 2, 3, 4, 0, 2, 1)}[w]
    if seed & 1:  # (the other shapes of the five at width 2)
        order = {2: (1, 4), 4: (3, 2, 4, 0), 8: order[::-1]}[w]
    return interleave([kinds[k](p) for p, k in enumerate(order)])[:n].copy()


def near_noise(n, seed):
    """252 of the 256 byte values, evenly, a plane: the planes form is a few per cent above
    4 + L, so the coder leaves for the stored form in its last steps"""
    return np.random.default_rng(seed).integers(2, 254, n, dtype=np.uint8)


def mixed(n, w, seed):
    """floats of the width, plane shapes, a constant stretch, noise and sparse bytes: the
    segments of one call take both forms"""
    rng = np.random.default_rng(seed)
    q = n // 5 + w
    gen = {2: bf16_weights, 4: f32_walk, 8: f64_normal}[w]
    parts = [gen(rng, q // w * w), plane_shapes(q, w, seed + 1), np.full(q, 9, np.uint8),
             rnd(q, seed + 2), sparse(q, w, seed + 3)]
    return np.concatenate(parts)[:n].copy()


def tie_alphabet(L, w):
    """the fixed alphabet of the tie search: 16 symbols a plane, evenly"""
    return np.random.default_rng(w).integers(0, 16, L, dtype=np.uint8)


# ---- the parts of a planes-form stream ---------------------------------------------------------

def parts_of(s, w):
    """([nsym_p], [tsize_p], nw) of a planes-form stream"""
    present = np.unpackbits(np.frombuffer(s[4:4 + 32 * w], np.uint8)).reshape(w, 256)
    nsym = [int(x) for x in present.sum(axis=1)]
    tsize = [table_size(k) for k in nsym]
    return nsym, tsize, (len(s) - M.fixed_size(w) - sum(tsize)) // 2


def frequencies_of(s, w):
    """the w x 256 frequencies a planes-form stream declares"""
    present = np.unpackbits(np.frombuffer(s[4:4 + 32 * w], np.uint8), bitorder="little") \
        .astype(bool).reshape(w, 256)
    nsym, tsize, _ = parts_of(s, w)
    f = np.zeros((w, 256), np.int64)
    at = 4 + 32 * w
    for p in range(w):
        bits = int.from_bytes(s[at:at + tsize[p]], "little")
        at += tsize[p]
        f[p, present[p]] = [1 + (bits >> (12 * k) & 0xFFF) for k in range(nsym[p])]
    return f


def with_frequencies(s, w, f):
    """the stream s with its bitmaps and freqs fields replaced by those of f"""
    _, tsize, _ = parts_of(s, w)
    L = 1 + s[2] + (s[3] << 8)
    none = np.zeros(0, np.uint8)
    return M.planes_stream(L, f, none, none) + s[4 + 32 * w + sum(tsize):]


def mutants(s, w):
    """deterministic mutations of the stream s of width w -> [(bytes, size given to the
    decoder)], the stream itself first: the header bytes, every bitmap, every freqs field and its
    pad bits, the first and last words, the states, and sizes off by 1, 2 and 3"""
    out = [(s, len(s))]

    def poke(at, value):
        if 0 <= at < len(s) and s[at] != value & 255:
            t = bytearray(s)
            t[at] = value & 255
            out.append((bytes(t), len(t)))

    for at in range(4):  # every header bit
        for bit in range(8):
            poke(at, s[at] ^ (1 << bit))
    for nib in range(16):
        poke(0, nib << 4 | s[0] & 15)
        poke(0, s[0] & 0xF0 | nib)
    for d in (1, 2, 3):  # extensions and truncations
        out += [(s + bytes(d), len(s) + d), (s, len(s) - d)]
    out += [(s, 3), (s, 0), (s, M.fixed_size(w) + 2 * w - 1), (s, M.fixed_size(w)), (s, 4 + 32 * w)]
    if s[0] & 8:
        return out
    nsym, tsize, nw = parts_of(s, w)
    f = frequencies_of(s, w)
    tables_at = 4 + 32 * w
    words_at = tables_at + sum(tsize)
    for p in range(w):
        bm = 4 + 32 * p
        t = bytearray(s)  # an empty bitmap
        t[bm:bm + 32] = bytes(32)
        out.append((bytes(t), len(t)))
        present, absent = np.flatnonzero(f[p]), np.flatnonzero(f[p] == 0)
        for v in {int(present[0]), int(present[-1])}:  # a symbol less
            poke(bm + (v >> 3), s[bm + (v >> 3)] ^ (1 << (v & 7)))
        for v in {int(absent[0]), int(absent[-1])} if absent.size else ():  # a symbol more
            poke(bm + (v >> 3), s[bm + (v >> 3)] ^ (1 << (v & 7)))
        at = tables_at + sum(tsize[:p])
        for bit in (0, 3, 7):  # the first frequency
            poke(at, s[at] ^ (1 << bit))
        for k in (1, 2):  # the field's last two bytes: a frequency's high bits or pad bits
            for bit in range(8):
                poke(at + tsize[p] - k, s[at + tsize[p] - k] ^ (1 << bit))
        if nsym[p] >= 2:
            g = f.copy()  # a swapped pair: the sum holds, other bytes or a reject
            a, b = present[0], present[-1]
            g[p, a], g[p, b] = f[p, b], f[p, a]
            if not np.array_equal(g, f):
                out.append((with_frequencies(s, w, g), len(s)))
            g = f.copy()  # one up, one down: still 4096
            lo, hi = present[int(np.argmin(f[p, present]))], present[int(np.argmax(f[p, present]))]
            g[p, lo] += 1
            g[p, hi] -= 1
            out.append((with_frequencies(s, w, g), len(s)))
            g[p, lo] += 1  # 4097
            out.append((with_frequencies(s, w, g), len(s)))
    # streams no encoder writes, accepted: the segment coded again under an altered table (the
    # same bytes from another stream), and other bytes under the stream's own tables
    data = np.frombuffer(M.decode(s, M.MAX_SEG, w), np.uint8)
    p = int(np.argmax(nsym))
    if nsym[p] >= 2:
        g = f.copy()
        present = np.flatnonzero(f[p])
        lo, hi = present[int(np.argmin(f[p, present]))], present[int(np.argmax(f[p, present]))]
        g[p, lo] += 1
        g[p, hi] -= 1
        t = M.planes_stream(data.size, g, *M.encode_words(data, g))
        out.append((t, len(t)))
    other = data.copy()  # (every plane backward: its symbols stay its own)
    for q in range(w):
        other[q::w] = data[q::w][::-1]
    t = M.planes_stream(other.size, f, *M.encode_words(other, f))
    out.append((t, len(t)))
    body, states = s[words_at:words_at + 2 * nw], s[words_at + 2 * nw:]
    if nw:  # dropped, added and altered words: the first and the last
        for k in sorted({0, nw - 1}):
            t = s[:words_at] + body[:2 * k] + body[2 * k + 2:] + states
            out.append((t, len(t)))
            t = s[:words_at] + body[:2 * k] + b"\x34\x12" + body[2 * k:] + states
            out.append((t, len(t)))
            for bit in (0, 7, 8, 15):
                poke(words_at + 2 * k + bit // 8, s[words_at + 2 * k + bit // 8] ^ (1 << bit % 8))
    t = s[:words_at] + b"\x00\x00" + body + states
    out.append((t, len(t)))
    for lane in (0, 1, 31, 63):  # states below 2^16, and others
        at = words_at + 2 * nw + 4 * lane
        for value in (b"\xff\xff\x00\x00", b"\x00\x00\x00\x00", b"\x01\x00\x01\x00",
                      b"\x00\x00\x00\x80"):
            t = s[:at] + value + s[at + 4:]
            if t != s:
                out.append((t, len(t)))
        for bit in (0, 15, 16, 31):
            poke(at + bit // 8, s[at + bit // 8] ^ (1 << bit % 8))
    return out


def example(w, L=1500):
    """a planes-form stream of L bytes whose planes have 5, 3, 17, 2, ... symbols (5: 4 pad bits
    in the freqs field) and more than a step of words -> (stream, the bytes)"""
    m = (L + w - 1) // w
    nsyms = (5, 3, 17, 2, 9, 1, 33, 6)[:w]
    data = interleave([RC.alphabet(m, k, 7 * w + p) for p, k in enumerate(nsyms)])[:L].copy()
    s = M.encode_segment(data, w)
    assert s[0] == 0xB0 | M.lg_of(w) and parts_of(s, w)[0] == list(nsyms) and parts_of(s, w)[2] > 64
    return s, data.tobytes()
