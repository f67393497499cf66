"""Reader and writer of the SYMTAB format (bitar_amd/csrc/symtab.hip) in plain
Python: test infrastructure, the normative restatement of the format and of the encoder's rule.

One stream per segment of L bytes, 1..65536:

    byte 0      0xC0 | mode            mode 0 coded, 1 stored
    byte 1      nsym, 1..255           (0 in the stored form)
    bytes 2..3  LE16(L - 1)
    stored:     L raw bytes                                     size = 4 + L
    coded:      LE16 nc                number of codes, >= 1
                lens[nsym]             one byte each, 1..8
                syms                   the symbols' bytes, concatenated in code order
                codes[nc]              c < nsym: symbol c;  255: the next unread byte of lits
                lits[nx]               nx = the number of codes equal to 255
    size = 6 + nsym + sum(lens) + nc + nx

The coded form is taken iff it is strictly smaller than 4 + L.  The decoder rejects a high nibble
other than 0xC, a mode above 1, byte 1 other than 0 when stored, L > seg, nsym = 0 or nc = 0 when
coded, a length of 0 or above 8, a code in [nsym, 255), a stream whose size is not exactly the
formula, and lengths that do not sum to exactly L (an escape counts 1).  Everything else decodes;
duplicate symbols are allowed.

The encoder's rule.  The segment is cut into chunks of 256 bytes (the last may be short); the
sample is all of them when L <= 16384 and those whose index is a multiple of 4 otherwise.  Items
are the 256 byte values (ids 0..255) and the symbols of the current table T (id 256 + c).  T
starts empty; in each of five generations every sample chunk is parsed greedily -- at a position
the longest symbol of T that matches inside the chunk, or else the single byte -- and c1[x] counts
the parsed items.  An adjacent pair (x, y) of a chunk with len(x) + len(y) <= 8 has
key = x * 512 + y and slot = (key * 0x9E3779B1 mod 2^32) >> 20; of the keys that share a slot in a
generation only the smallest is counted.  Candidates, in index order: items with c1 > 0 (index =
id, gain = c1 * len), then occupied slots (index = 512 + slot, gain = count * total length).  With
more than 255 candidates, thr is the 255th largest gain: every candidate above thr is taken, then
those equal to thr in index order until 255 are.  The new T is the taken candidates in index
order.  After the fifth generation the whole segment is parsed greedily with T (a match may not
pass the segment's end): a symbol gives its code, a byte not in T gives 255 and goes to lits.

Two streams by hand.

1. b"abababab" (L = 8, one chunk).  Generation 1 (T empty) parses 8 single bytes: c1[a] = 4,
   c1[b] = 4; pairs (a, b) x 4 with key 0x61 * 512 + 0x62 = 49762, slot 2487, and (b, a) x 3 with
   key 50273, slot 1731; four candidates, so all are taken, in index order:
   T = [a, b, ba, ab].  Generation 2 parses ab ab ab ab (the longest match at every position):
   c1[256 + 3] = 4, the pair (ab, ab) x 3 has total length 4: T = [ab, abab] -- the pair was
   promoted.  Generation 3 parses abab abab: T = [abab, abababab].  Generations 4 and 5 parse one
   item, no pair: T = [abababab].  The stream:
       c0 01 07 00 | 01 00 | 08 | 61 62 61 62 61 62 61 62 | 00             17 bytes
   which is not below 4 + 8 = 12, so the segment is stored: c1 00 07 00 61 62 61 62 61 62 61 62.
   Sixteen times the same, b"ab" * 64 (L = 128), ends with T = [abababab] as well (generation 3
   has T = [abab, abababab], and a pair of two abab is 8 bytes but a pair with abababab is more)
   and is coded: c0 01 7f 00 | 10 00 | 08 | 61 62 61 62 61 62 61 62 | 00 * 16, 31 bytes.

2. An escape of byte 0xFF.  L = 16390: the chunks 0, 4, 8, ... 64 are the sample, and byte 300
   (chunk 1) is sampled out.  With the segment all b"a" but a 0xFF at 300, the tables are
   [a, aa], [aa, aaaa], [aaaa, aaaaaaaa] (the last chunk has 6 bytes: it parses aaaa aa, whose
   pair of 6 bytes joins), [aaaaaa, aaaaaaaa] and at last T = [aaaaaaaa, aaaaaa]: the 8-byte
   symbol has id 256 + 1 in generation 5, the 6-byte one is item 256 + 0 and no pair is short
   enough.  The emit parses 37 codes 0 up to byte 296; there neither symbol matches, and the four
   a's are escapes as much as the 0xFF behind them; 2011 codes 0 follow and the last byte is an
   escape again: nc = 37 + 5 + 2011 + 1 = 2054, lits = 61 61 61 61 ff 61, 2082 bytes:
       c0 02 05 40 | 06 08 | 08 06 | 61 * 14 | 00 * 37  ff * 5  00 * 2011  ff | 61 61 61 61 ff 61
"""
import numpy as np

MAX_SEG = 65536
CHUNK = 256
SAMPLE_ALL = 16384  # segments up to this length are sampled whole
GENERATIONS = 5
MAX_SYMS = 255
MAX_LEN = 8
ESC = 255
SLOTS = 4096
HASH_MUL = 0x9E3779B1


def _header(mode, nsym, L):
    return bytes([0xC0 | mode, nsym, (L - 1) & 255, (L - 1) >> 8])


def slot_of(key):
    return ((key * HASH_MUL) & 0xFFFFFFFF) >> 20


def sample_chunks(L):
    """[(lo, hi)] of the sample's chunks"""
    n = (L + CHUNK - 1) // CHUNK
    step = 1 if L <= SAMPLE_ALL else 4
    return [(CHUNK * i, min(CHUNK * i + CHUNK, L)) for i in range(0, n, step)]


def _lookup(table):
    """first byte -> [(symbol, code)], the longest first"""
    by = {}
    for c, s in enumerate(table):
        by.setdefault(s[0], []).append((s, c))
    for v in by.values():
        v.sort(key=lambda e: -len(e[0]))
    return by


def parse(buf, lo, hi, lookup):
    """greedy parse of buf[lo:hi]: [(item id, length)], no match passing hi"""
    out = []
    p = lo
    while p < hi:
        item, n = buf[p], 1
        for s, c in lookup.get(buf[p], ()):
            if p + len(s) <= hi and buf.startswith(s, p):
                item, n = 256 + c, len(s)
                break
        out.append((item, n))
        p += n
    return out


def count_generation(buf, chunks, table):
    """-> c1[512], {slot: (key, count, total length)} of one generation's parse"""
    lookup = _lookup(table)
    c1 = [0] * 512
    pairs = []
    for lo, hi in chunks:
        items = parse(buf, lo, hi, lookup)
        for x, _ in items:
            c1[x] += 1
        for (x, nx), (y, ny) in zip(items, items[1:]):
            if nx + ny <= MAX_LEN:
                pairs.append((x * 512 + y, nx + ny))
    smallest = {}
    for key, n in pairs:
        s = slot_of(key)
        if s not in smallest or key < smallest[s][0]:
            smallest[s] = (key, n)
    slots = {s: [key, 0, n] for s, (key, n) in smallest.items()}
    for key, _ in pairs:
        e = slots[slot_of(key)]
        if e[0] == key:
            e[1] += 1
    return c1, {s: tuple(e) for s, e in slots.items()}


def item_bytes(x, table):
    return bytes([x]) if x < 256 else table[x - 256]


def candidates(c1, slots, table):
    """[(index, gain, string)] in index order"""
    out = []
    for x in range(512):
        if c1[x]:
            s = item_bytes(x, table)
            out.append((x, c1[x] * len(s), s))
    for slot in sorted(slots):
        key, count, n = slots[slot]
        s = item_bytes(key >> 9, table) + item_bytes(key & 511, table)
        assert len(s) == n
        out.append((512 + slot, count * n, s))
    return out


def select(cands):
    """the taken candidates, in index order"""
    if len(cands) <= MAX_SYMS:
        return list(cands)
    thr = sorted((g for _, g, _ in cands), reverse=True)[MAX_SYMS - 1]
    room = MAX_SYMS - sum(g > thr for _, g, _ in cands)
    out = []
    for c in cands:
        if c[1] > thr:
            out.append(c)
        elif c[1] == thr and room:
            out.append(c)
            room -= 1
    return out


def next_table(buf, chunks, table):
    c1, slots = count_generation(buf, chunks, table)
    return [s for _, _, s in select(candidates(c1, slots, table))]


def build_table(segment, generations=GENERATIONS):
    buf = bytes(segment)
    chunks = sample_chunks(len(buf))
    table = []
    for _ in range(generations):
        table = next_table(buf, chunks, table)
    return table


def coded_stream(L, table, codes, lits):
    """the coded form of a segment of L bytes from its parts as given"""
    return _header(0, len(table), L) + bytes([len(codes) & 255, len(codes) >> 8 & 255]) + \
        bytes(len(s) for s in table) + b"".join(table) + bytes(codes) + bytes(lits)


def emit(buf, table):
    """-> codes, lits of the whole segment's greedy parse"""
    codes, lits = bytearray(), bytearray()
    for x, _ in parse(buf, 0, len(buf), _lookup(table)):
        if x < 256:
            codes.append(ESC)
            lits.append(x)
        else:
            codes.append(x - 256)
    return bytes(codes), bytes(lits)


def coded_form(segment):
    """the coded form of the segment whatever its size, or None when nc does not fit LE16"""
    buf = bytes(np.ascontiguousarray(segment, np.uint8))
    table = build_table(buf)
    codes, lits = emit(buf, table)
    if len(codes) > 0xFFFF:
        return None
    return coded_stream(len(buf), table, codes, lits)


def encode_segment(segment):
    seg = np.ascontiguousarray(segment, np.uint8)
    L = seg.size
    assert 1 <= L <= MAX_SEG
    s = coded_form(seg)
    return s if s is not None and len(s) < 4 + L else _header(1, 0, L) + seg.tobytes()


def encode(data, seg):
    """-> the list of per-segment streams of `data` cut into segments of `seg` bytes"""
    data = np.ascontiguousarray(data, np.uint8)
    return [encode_segment(data[o:o + seg]) for o in range(0, data.size, seg)]


def parts_of(stream):
    """(lens, symbols, codes, lits) of a coded stream the decoder accepts"""
    s = bytes(stream)
    nsym, nc = s[1], s[4] | s[5] << 8
    lens = list(s[6:6 + nsym])
    at, syms = 6 + nsym, []
    for n in lens:
        syms.append(s[at:at + n])
        at += n
    return lens, syms, s[at:at + nc], s[at + nc:]


def decode(stream, seg):
    """-> the segment's bytes, or None when the decoder must reject the stream"""
    s = bytes(stream)
    if len(s) < 4:
        return None
    tag, nsym = s[0], s[1]
    if tag >> 4 != 0xC or tag & 15 > 1:
        return None
    L = 1 + s[2] + (s[3] << 8)
    if L > seg:
        return None
    if tag & 1:
        return s[4:] if nsym == 0 and len(s) == 4 + L else None
    if nsym == 0 or len(s) < 6 + nsym:
        return None
    nc = s[4] | s[5] << 8
    if nc == 0:
        return None
    lens = s[6:6 + nsym]
    if any(n < 1 or n > MAX_LEN for n in lens):
        return None
    codes_at = 6 + nsym + sum(lens)
    if len(s) < codes_at + nc:
        return None
    codes = s[codes_at:codes_at + nc]
    nx = codes.count(ESC)
    if len(s) != codes_at + nc + nx:
        return None
    if any(nsym <= c < ESC for c in codes):
        return None
    if sum(1 if c == ESC else lens[c] for c in codes) != L:
        return None
    _, syms, _, lits = parts_of(s)
    out, k = bytearray(), 0
    for c in codes:
        if c == ESC:
            out.append(lits[k])
            k += 1
        else:
            out += syms[c]
    return bytes(out)
