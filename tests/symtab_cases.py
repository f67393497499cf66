"""Inputs and stream mutations shared by the SYMTAB tests (test infrastructure)."""
import numpy as np

import symtab_model as M


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


SYLLABLES = ("an ar be bo ca chi da de el en fa fi ga go ha hu il is ja jo ka ki la le ma mi na ne "
             "ol or pa pe qu ra ri sa so ta ti ul ur va vi wa we xa ya yo za zu son ton lin ber "
             "man sen ley ard ett ing").split()


def names(n, seed=7):
    """n bytes of person names: syllable words of 2..4 syllables, capitalised, first and last
    name separated by a blank and names by a line feed"""
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n:
        k = rng.integers(2, 5, 2)
        idx = rng.integers(0, len(SYLLABLES), int(k.sum()))
        first = "".join(SYLLABLES[i] for i in idx[:k[0]]).capitalize()
        last = "".join(SYLLABLES[i] for i in idx[k[0]:]).capitalize()
        line = (first + " " + last + "\n").encode()
        out.append(line)
        size += len(line)
    return np.frombuffer(b"".join(out)[:n], np.uint8).copy()


def text(n, seed):
    """log-like lines: a few fixed words, numbers and names"""
    rng = np.random.default_rng(seed)
    words = [b"GET", b"POST", b"/api/v1/", b"users", b"items", b"status=", b"200", b"404",
             b"INFO", b"WARN", b"request", b"took", b"ms", b"host-", b"id="]
    out, size = [], 0
    while size < n:
        k = rng.integers(0, len(words), 6)
        line = b" ".join(words[i] for i in k) + b" %d\n" % int(rng.integers(0, 100000))
        out.append(line)
        size += len(line)
    return np.frombuffer(b"".join(out)[:n], np.uint8).copy()


def phrases(n, seed):
    """one log line over and over with a running number: coded from a few hundred bytes on"""
    out, size, k = [], 0, seed
    while size < n:
        line = b"id=%d status=200 GET /api/v1/users\n" % k
        out.append(line)
        size += len(line)
        k += 1
    return np.frombuffer(b"".join(out)[:n], np.uint8).copy()


def alphabet64(n, seed):
    """n bytes drawn evenly from 64 random byte values: hundreds of pairs with equal gains and
    more pair keys than free slots"""
    rng = np.random.default_rng(seed)
    values = rng.permutation(256)[:64].astype(np.uint8)
    return values[rng.integers(0, 64, n)]


def all_bytes(n, seed):
    """all 256 byte values, 0x00 and 0xFF frequent and in runs: escapes, zero bytes inside
    symbols"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    pick = rng.random(n)
    a[pick < 0.47] = 0
    a[pick > 0.53] = 0xFF
    a[:256] = np.arange(256, dtype=np.uint8)[:min(n, 256)]
    return a


def symbol_at_ends(L):
    """a segment of the 8-byte word `ABCDEFGH` with single other bytes set in so that the word
    ends on a chunk's last byte and on the segment's last byte"""
    word = np.frombuffer(b"ABCDEFGH", np.uint8)
    a = np.tile(word, L // 8 + 1)[:L].copy()
    if L >= 16:
        a[L - 8:] = word
        k = (L - 8) % 8
        a[L - 8 - k:L - 8] = 0x2E
    return a


def collide(n=4096):
    """single bytes whose pair keys share slots: of the pairs (a, b) the keys a * 512 + b that
    fall into one slot, found by search, laid out so that each is seen often"""
    by_slot = {}
    for a in range(32, 96):
        for b in range(32, 96):
            by_slot.setdefault(M.slot_of(a * 512 + b), []).append((a, b))
    groups = [v for v in by_slot.values() if len(v) >= 2][:8]
    assert groups
    out = []
    for g in groups:
        for a, b in g:
            out += [a, b, 0x0A] * 5
    reps = n // len(out) + 1
    return np.array(out * reps, np.uint8)[:n], groups


def equal_gains(n=8192):
    """every byte value once a chunk, ascending in the even chunks and descending in the odd
    ones: 256 items and 510 pairs, all of one gain, compete for 255 places"""
    up = np.arange(256, dtype=np.uint8)
    return np.tile(np.concatenate([up, up[::-1]]), n // 512 + 1)[:n].copy()


def mixed(n, seed):
    """text, noise, names and a constant stretch by turns, in pieces of 1..3 KiB"""
    rng = np.random.default_rng(seed)
    parts, size = [], 0
    while size < n:
        k = int(rng.integers(1024, 3072))
        kind = int(rng.integers(0, 4))
        p = (text(k, size), rnd(k, size), names(k, size), np.full(k, 0x41, np.uint8))[kind]
        parts.append(p)
        size += k
    return np.concatenate(parts)[:n]


def _put16(s, at, v):
    s[at] = v & 255
    s[at + 1] = v >> 8 & 255


def mutants(stream):
    """[(bytes, size)]: the stream itself first, then single mutations of it -- every header
    field, lengths, codes out of range, nc off by one, truncation and extension, a 255 added or
    removed.  `size` is the csize handed to the decoder (the bytes may be longer)."""
    s0 = bytes(stream)
    out = [(s0, len(s0))]

    def add(b, size=None):
        b = bytes(b)
        out.append((b, len(b) if size is None else size))

    for v in (0x00, 0xA0, 0xB0, 0xD0, 0xC2, 0xC3, 0xCF, s0[0] ^ 1):
        m = bytearray(s0)
        m[0] = v
        add(m)
    for v in {0, 1, s0[1] + 1 & 255, s0[1] - 1 & 255, 255}:
        m = bytearray(s0)
        m[1] = v
        add(m)
    L = 1 + s0[2] + (s0[3] << 8)
    for v in (L - 2, L, 0, 0xFFFF, L - 1 + 256 & 0xFFFF):
        m = bytearray(s0)
        _put16(m, 2, v & 0xFFFF)
        add(m)
    for k in (1, 2, 3, 4, 5, 6, 7, len(s0) // 2):
        add(s0[:len(s0) - k])
        add(s0 + b"\xff" * k)
        add(s0 + b"\x00" * k)
        add(s0 + b"\x00" * k, len(s0))  # (bytes behind the stream are not the stream's)
    if s0[0] & 1:
        return out
    nsym, nc = s0[1], s0[4] | s0[5] << 8
    lens, syms, codes, lits = M.parts_of(s0)
    codes_at = 6 + nsym + sum(lens)
    for v in (nc - 1, nc + 1, 0, 1, 0xFFFF, nc ^ 0x100):
        m = bytearray(s0)
        _put16(m, 4, v & 0xFFFF)
        add(m)
    for k in sorted({0, nsym // 2, nsym - 1}):
        for v in (0, 9, 255, lens[k] % 8 + 1, (lens[k] + 6) % 8 + 1):
            m = bytearray(s0)
            m[6 + k] = v
            add(m)
    rng = np.random.default_rng(len(s0))
    for k in sorted({0, 1, nc // 2, nc - 2, nc - 1} & set(range(nc))) + \
            rng.integers(0, nc, 24).tolist():
        for v in (nsym, 254, 255, 0, nsym - 1, (codes[k] + 1) % nsym):
            m = bytearray(s0)
            m[codes_at + k] = v
            add(m)
        # a 255 put in (with and without its literal), a code taken out
        add(s0[:codes_at + k] + b"\xff" + s0[codes_at + k:])
        m = bytearray(s0[:codes_at + k] + b"\xff" + s0[codes_at + k:] + b"a")
        _put16(m, 4, nc + 1)
        add(m)
        m = bytearray(s0[:codes_at + k] + s0[codes_at + k + 1:])
        _put16(m, 4, nc - 1)
        add(m)
    esc = [k for k in range(nc) if codes[k] == 255][:4]
    for k in esc:  # a 255 taken out: with and without its literal
        m = bytearray(s0[:codes_at + k] + s0[codes_at + k + 1:])
        _put16(m, 4, nc - 1)
        add(m)
        add(m[:-1])
        m = bytearray(s0)
        m[codes_at + k] = 0
        add(m)
        add(m[:-1])
    for k in range(min(len(syms), 3)):  # a symbol's byte changed: accepted, other bytes
        m = bytearray(s0)
        m[6 + nsym + sum(lens[:k])] ^= 0x20
        add(m)
    return out
