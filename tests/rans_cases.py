"""Inputs and mutated streams shared by the RANS tests (test_rans_model.py on the CPU,
test_gpu_rans.py on the device): test infrastructure."""
import numpy as np

import rans_model as M


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def tie_input(L):
    """the tie input: the rans form is 2 bytes above 4 + L at 438, level at 440 (stored)
    and 2 below at 442"""
    return np.random.default_rng(0).integers(0, 16, L, dtype=np.uint8)


def alphabet(n, nsym, seed):
    """n bytes over nsym byte values with a skewed histogram, every value present when n allows"""
    rng = np.random.default_rng(seed)
    values = rng.permutation(256)[:nsym].astype(np.uint8)
    p = 1.0 / (np.arange(nsym) + 1.0)
    out = values[rng.choice(nsym, n, p=p / p.sum())]
    k = min(n, nsym)
    out[rng.permutation(n)[:k]] = values[:k]
    return out


def stress_histogram(seed=0):
    """127 symbols x 512, one x 384 and 128 singletons: the histogram on which the plain
    "floor, bump zeros, take from the largest" rule fails; 65536 bytes, shuffled"""
    counts = [512] * 127 + [384] + [1] * 128
    out = np.repeat(np.arange(256, dtype=np.uint8), counts)
    return np.random.default_rng(seed).permutation(out)


def mostly_one(n, seed):
    """one symbol but for a handful of others: hardly a word is emitted"""
    out = np.full(n, 0x41, np.uint8)
    rng = np.random.default_rng(seed)
    out[rng.permutation(n)[:max(1, n // 4000)]] = 0x42
    return out


def smooth_walk_shuffled(n, seed):
    """a smooth float32 walk, byte-transposed (shuffle filter, width 4)"""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(0, 0.01, n // 4)).astype("<f4")
    return np.ascontiguousarray(x.view(np.uint8).reshape(-1, 4).T).reshape(-1)


def normal_shuffled(n, seed):
    x = np.random.default_rng(seed).normal(0, 1, n // 4).astype("<f4")
    return np.ascontiguousarray(x.view(np.uint8).reshape(-1, 4).T).reshape(-1)


def two_symbols(n, seed):
    return (np.random.default_rng(seed).random(n) < 0.02).astype(np.uint8) * 7 + 3


def mixed(n, seed):
    """text-like bytes, a small alphabet, a constant stretch, noise, a float walk: the segments of
    one call take both forms"""
    rng = np.random.default_rng(seed)
    q = n // 5 + 1
    parts = [M.text_like(rng, q), alphabet(q, 16, seed + 1), np.full(q, 9, np.uint8),
             rnd(q, seed + 2), smooth_walk_shuffled(q + 4, seed + 3)[:q]]
    return np.concatenate(parts)[:n].copy()


def parts_of(s):
    """(nsym, tsize, nw) of a rans-form stream"""
    nsym = int(np.unpackbits(np.frombuffer(s[4:36], np.uint8)).sum())
    tsize = M.table_size(nsym)
    return nsym, tsize, (len(s) - M.FIXED - tsize) // 2


def frequencies_of(s):
    """the 256 frequencies a rans-form stream declares"""
    present = np.unpackbits(np.frombuffer(s[4:36], np.uint8), bitorder="little").astype(bool)
    nsym, tsize, _ = parts_of(s)
    bits = int.from_bytes(s[36:36 + tsize], "little")
    f = np.zeros(256, np.int64)
    f[present] = [1 + (bits >> (12 * k) & 0xFFF) for k in range(nsym)]
    return f


def mutants(s):
    """deterministic mutations of the stream s -> [(bytes, size given to the decoder)], the
    stream itself first"""
    out = [(s, len(s))]

    def poke(at, value, base=None):
        base = s if base is None else base
        if 0 <= at < len(base) and base[at] != value & 255:
            t = bytearray(base)
            t[at] = value & 255
            out.append((bytes(t), len(t)))

    for at in range(4):  # every header bit
        for bit in range(8):
            poke(at, s[at] ^ (1 << bit))
    for nib in range(16):
        poke(0, nib << 4 | s[0] & 15)
        poke(0, s[0] & 0xF0 | nib)
    for d in (1, 2):  # sizes +-1 / +-2
        out += [(s + bytes(d), len(s) + d), (s, len(s) - d)]
    out += [(s, 3), (s, 0), (s, M.FIXED + 1), (s, M.FIXED)]
    if s[0] & 1:
        return out
    nsym, tsize, nw = parts_of(s)
    words_at = 36 + tsize
    for at in range(4, words_at):  # every table bit: bitmap, frequencies and pad
        for bit in range(8):
            poke(at, s[at] ^ (1 << bit))
    t = bytearray(s)  # an empty bitmap
    t[4:36] = bytes(32)
    out.append((bytes(t), len(t)))
    f = frequencies_of(s)
    present = np.flatnonzero(f)
    if nsym >= 2:  # a swapped frequency pair: the sum holds, other bytes or a reject
        for a, b in ((0, 1), (0, nsym - 1), (nsym // 2, nsym // 2 - 1)):
            g = f.copy()
            g[present[a]], g[present[b]] = f[present[b]], f[present[a]]
            out.append((s[:4] + M.pack_table(g) + s[words_at:], len(s)))
        g = f.copy()  # one up, one down: still 4096
        lo, hi = present[int(np.argmin(f[present]))], present[int(np.argmax(f[present]))]
        g[lo] += 1
        g[hi] -= 1
        out.append((s[:4] + M.pack_table(g) + s[words_at:], len(s)))
        # streams no encoder writes, accepted: the segment coded again under that table (the same
        # bytes from another stream), and other bytes under the stream's own table
        data = np.frombuffer(M.decode(s, M.MAX_SEG), np.uint8)
        t = M.rans_stream(data.size, g, *M.encode_words(data, g))
        out.append((t, len(t)))
        other = data[::-1].copy()
        t = M.rans_stream(other.size, f, *M.encode_words(other, f))
        out.append((t, len(t)))
    body, states = s[words_at:words_at + 2 * nw], s[words_at + 2 * nw:]
    if nw:  # dropped, added and altered words
        for k in sorted({0, nw // 2, nw - 1}):
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
