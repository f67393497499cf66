"""Whole-buffer raw Snappy streams in pure Python (test infrastructure): the join of the
per-segment streams of BITAR_HIP_CODEC_SNAPPY into one stock stream, and the boundary scan that
finds, without a serial walk, where each 64 KiB block of output begins in such a stream
(bitar_amd/csrc/snappy.hip).

  join(streams, n)      varint(n) + every segment's stream less its own preamble
  serial_split(stream)  the rule: a plain element walk -> (status, starts)
  scan(stream, T, ...)  the kernels' method, tile for tile and round for round -> Scan
  decode_joined(...)    the verdict of scan + one headless fragment decode per block

A stream is cut into tiles of T bytes.  A tile walk from an entry e inside tile j follows the
elements while they start before the tile's end and returns x, the first chain position at or
past the end (INF when an element reads past the stream), and o, the output bytes of the
elements that started in the tile.  Round 1 walks every tile from a guess (tile 0 from the
byte after the preamble, tile j from j * T); a resolve carries the true chain position c over
the tiles' latest x, finds the tiles whose entry differs (dirty) and, where the first few
elements from c leave the tile by themselves (up to FOLLOW of them, as long as they average
FOLLOW_BYTES from the second on: long literals), takes their end and output as the tile's result
instead; the next round walks the dirty tiles from their new entries.  Past a dirty tile the
resolve goes on with the x of that tile's round-1 walk, not of its latest: a walk from a wrong
entry may end on a wrong chain, which periodic data can keep alive for many tiles, while the
guesses start afresh at every tile.  At the fixpoint every active tile's (entry, x, o) comes
from one walk and entry[j + 1] == x[j] from the preamble on, so the chain is
the true one.  After `max_rounds` rounds one serial walk from the first unsettled tile finishes.
"""
import numpy as np

import snappy_model as M

BLOCK = 65536
OK, UNSUPPORTED, INVALID, INCOMPLETE = 0, 1, 2, 3
STATUS = {OK: "ok", UNSUPPORTED: "unsupported", INVALID: "invalid", INCOMPLETE: "incomplete"}
INF = 0xFFFFFFFF
TILE = 4096            # the shipped tile
MAX_ROUNDS = 64        # the shipped default of max_rounds
FOLLOW, FOLLOW_BYTES = 16, 64  # the resolve's own walk: elements, and their mean size to go on
NO_SERIAL_FINISH = 0x80000000  # ORed into max_rounds: no serial finish (status incomplete)


def join(streams, n):
    """one raw Snappy stream of the segments' streams (64 KiB segments)"""
    out = bytearray(M.varint(n))
    for s in streams:
        out += s[M.preamble(s)[1]:]
    return bytes(out)


def nfrag(n):
    return (n + BLOCK - 1) // BLOCK


def parse(s, pos):
    """the element at pos < len(s) -> (position of the next element or INF when it reads past
    the stream, its output bytes)"""
    tag = s[pos]
    kind, code = tag & 3, tag >> 2
    if kind == M.LITERAL:
        extra = 0 if code < 60 else code - 59
        if pos + 1 + extra > len(s):
            return INF, 0
        length = code + 1 if code < 60 else \
            int.from_bytes(s[pos + 1:pos + 1 + extra], "little") + 1
        nxt = pos + 1 + extra + length
        return (nxt, length) if nxt <= len(s) else (INF, 0)
    extra = {M.COPY1: 1, M.COPY2: 2, M.COPY4: 4}[kind]
    if pos + 1 + extra > len(s):
        return INF, 0
    return pos + 1 + extra, (4 + (code & 7) if kind == M.COPY1 else code + 1)


def serial_split(stream):
    """(status, starts): starts[k] = the stream offset at which output position k * 65536
    begins, starts[nfrag] = len(stream); starts is None unless the status is OK"""
    s = bytes(stream)
    pre = M.preamble(s)
    if pre is None:
        return INVALID, None
    n, pos = pre
    starts, out, straddle = [], 0, False
    while pos < len(s):
        nxt, length = parse(s, pos)
        if nxt == INF:
            return INVALID, None
        if out % BLOCK == 0 and out < n:
            starts.append(pos)
        above = (out | (BLOCK - 1)) + 1  # the first block border inside the element, if any
        if above < out + length and above < n:
            straddle = True
        out += length
        pos = nxt
    if out != n:
        return INVALID, None
    if straddle:
        return UNSUPPORTED, None
    assert len(starts) == nfrag(n)
    return OK, starts + [len(s)]


def tile_walk(s, end, e):
    """(x, o) of a walk from e to the tile's end"""
    pos, o = e, 0
    while pos < end:
        nxt, length = parse(s, pos)
        if nxt == INF:
            return INF, o
        o += length
        pos = nxt
    return pos, o


class Scan:
    """status, starts (None unless OK), rounds (launches of the tile walk), walks (tile walks
    in all), serial (the serial finish ran)"""

    def __init__(self, status, starts, rounds, walks, serial):
        self.status, self.starts, self.rounds, self.walks, self.serial = \
            status, starts, rounds, walks, serial


def _finish_walk(s, n, end, pos, out, starts):
    """a walk with the running output count: block starts written, -> (x, out, straddle)"""
    straddle = False
    while pos < end:
        nxt, length = parse(s, pos)
        if nxt == INF:
            return INF, out, straddle
        if out % BLOCK == 0 and out < n:
            starts[out // BLOCK] = pos
        above = (out | (BLOCK - 1)) + 1
        if above < out + length and above < n:
            straddle = True
        out += length
        pos = nxt
    return pos, out, straddle


def scan(stream, T=TILE, max_rounds=0):
    s = bytes(stream)
    L = len(s)
    serial_ok = not (max_rounds & NO_SERIAL_FINISH)
    max_rounds = (max_rounds & ~NO_SERIAL_FINISH) or MAX_ROUNDS
    pre = M.preamble(s)
    if pre is None:
        return Scan(INVALID, None, 0, 0, False)
    n, p0 = pre
    ntile = max((L + T - 1) // T, 1)
    end = [min((j + 1) * T, L) for j in range(ntile)]
    # round 1: every tile from its guess
    rec = []
    for j in range(ntile):
        e = p0 if j == 0 else j * T
        rec.append((e,) + tile_walk(s, end[j], e))
    guess = [(x, o) for _, x, o in rec]  # round 1's results stay: the resolve's estimates
    rounds, walks = 1, ntile
    cur = [None] * ntile  # (c, output position) at each tile, final up to the first dirty one
    cur[0] = (p0, 0)
    first = 0
    while True:
        # resolve, from the first tile that is not final
        c, acc = cur[first]
        dirty = []
        for j in range(first, ntile):
            cur[j] = (c, acc)
            if c >= end[j]:      # a long literal jumped over the tile (or the chain is dead)
                continue
            entry, x, o = rec[j]
            if entry != c:
                # follow the chain from c while it is sparse: it may leave the tile by itself
                q, osum, left = c, 0, False
                for k in range(FOLLOW):
                    nxt, length = parse(s, q)
                    osum += length
                    if nxt >= end[j]:
                        left = True
                        break
                    q = nxt
                    if k >= 1 and q - c < FOLLOW_BYTES * (k + 1):
                        break
                if left:
                    rec[j] = (c, nxt, osum)
                    x, o = nxt, osum
                else:
                    dirty.append((j, c))
                    x, o = guess[j]  # (a walk from a wrong entry may sit on a wrong chain)
                    if x == INF and end[j] < L:
                        x = end[j]  # (a guess that died in a garbage literal: the next guess)
            c, acc = x, acc + o
        if not dirty or rounds >= max_rounds:
            break
        first = dirty[0][0]
        for j, e in dirty:
            rec[j] = (e,) + tile_walk(s, end[j], e)
        rounds += 1
        walks += len(dirty)
    starts = [INF] * (nfrag(n) + 1)
    straddle = False
    settled = dirty[0][0] if dirty else ntile
    if dirty:
        if not serial_ok:
            return Scan(INCOMPLETE, None, rounds, walks, False)
        # the serial finish: one walk from the first unsettled tile to the end
        c, acc = cur[settled]
        c, acc, straddle = _finish_walk(s, n, L, c, acc, starts)
    if c != L or acc != n:
        return Scan(INVALID, None, rounds, walks, bool(dirty))
    # the finish: the tiles whose output range holds a block border walk once more
    for j in range(settled):
        cj, base = cur[j]
        if cj >= end[j]:
            continue
        entry, x, o = rec[j]
        assert entry == cj
        if (base + BLOCK - 1) // BLOCK * BLOCK < base + o:
            x2, out2, st = _finish_walk(s, n, end[j], cj, base, starts)
            assert (x2, out2) == (x, base + o)
            straddle = straddle or st
    if straddle:
        return Scan(UNSUPPORTED, None, rounds, walks, bool(dirty))
    starts[nfrag(n)] = L
    assert INF not in starts[:-1]
    return Scan(OK, starts, rounds, walks, bool(dirty))


def fragments(stream, starts):
    """the headless fragment k as the stream the per-segment decoder reads: its length and body"""
    n = M.preamble(stream)[0]
    return [M.varint(min(BLOCK, n - k * BLOCK)) + stream[starts[k]:starts[k + 1]]
            for k in range(nfrag(n))]


def decode_joined(stream, capacity):
    """(verdict, blocks): verdict "invalid" (no preamble, a declared length above the capacity
    or the scan's invalid), "unsupported", "reject" (a fragment rejects: blocks holds None for
    it) or "ok"; blocks = each fragment's bytes"""
    pre = M.preamble(stream)
    if pre is None or pre[0] > capacity:
        return "invalid", None
    status, starts = serial_split(stream)
    if status != OK:
        return STATUS[status], None
    blocks = [M.decode(f, BLOCK) for f in fragments(stream, starts)]
    return ("reject" if any(b is None for b in blocks) else "ok"), blocks


# ---- streams built by hand ---------------------------------------------------------------------

def literal_code(data, code):
    """a literal element with its length written under tag code 60..63 (1..4 length bytes)"""
    return bytes([code << 2]) + (len(data) - 1).to_bytes(code - 59, "little") + bytes(data)


def copy4(offset, length):
    return bytes([M.COPY4 | (length - 1) << 2]) + offset.to_bytes(4, "little")


def _rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def hand_built():
    """[(name, stream, scan status, fragment verdict, pyarrow must accept)]: one stream per class;
    the fragment verdict is "ok" or "reject" where the scan is OK, else None"""
    r = _rnd(BLOCK + 64, 77)
    big = M.literal(r[:BLOCK])
    near = M.literal(r[:BLOCK - 6])
    out = [
        ("literal across a block", M.varint(BLOCK + 10) + near + M.literal(r[:16]),
         UNSUPPORTED, None, True),
        ("copy across a block", M.varint(BLOCK + 10) + near + M.copy(100, 12) + M.literal(r[:4]),
         UNSUPPORTED, None, True),
        ("copy into the previous block", M.varint(BLOCK + 14) + big + M.copy(200, 10) +
         M.literal(r[:4]), OK, "reject", True),
        ("copy-4 inside a block", M.varint(BLOCK + 16) + big + M.literal(r[:8]) + copy4(8, 8),
         OK, "ok", True),
        ("truncated last element", M.varint(BLOCK + 10) + big + M.literal(r[:10])[:8],
         INVALID, None, False),
        ("trailing bytes", M.varint(BLOCK + 10) + big + M.literal(r[:10]) + b"\x00z",
         INVALID, None, False),
        ("declared one above", M.varint(BLOCK + 11) + big + M.literal(r[:10]),
         INVALID, None, False),
        ("declared one below", M.varint(BLOCK + 9) + big + M.literal(r[:10]),
         INVALID, None, False),
        ("non-minimal preamble", bytes([0x8A, 0x80, 0x84, 0x80, 0x00]) + big + M.literal(r[:10]),
         OK, "ok", True),
    ]
    return out


def sized_stream(length, seed=0):
    """a stream of exactly `length` bytes (>= 200, < 16384 + 2): short literals"""
    rng = np.random.default_rng(1000 + seed)
    body, rem, n = bytearray(), length - 2, 0
    while rem:
        k = rem - 1 if rem <= 61 else min(int(rng.integers(1, 61)), rem - 3)
        body += M.literal(_rnd(k, n))
        rem -= k + 1
        n += k
    assert 128 <= n < 16384
    return M.varint(n) + bytes(body)


EDGE_ELEMENTS = ("literal-1", "literal-2", "literal-3", "literal-4", "copy-1", "copy-2", "copy-4")


def edge_stream(kind, at, T=TILE):
    """an element of header class `kind` that begins at stream position `at` (near a tile's
    end), short literals before and behind it"""
    head = sized_stream(at)
    n0, p = M.preamble(head)
    data = _rnd(20, at)
    el, out = {
        "literal-1": (M.literal(data), 20), "literal-2": (literal_code(data, 60), 20),
        "literal-3": (literal_code(data, 61), 20), "literal-4": (literal_code(data, 62), 20),
        "copy-1": (M.copy(7, 9), 9), "copy-2": (M.copy(300, 33), 33), "copy-4": (copy4(9, 21), 21),
    }[kind]
    tail = b"".join(M.literal(_rnd(30, k)) for k in range(3))
    n = n0 + out + 90
    assert len(M.varint(n)) == p
    s = M.varint(n) + head[p:] + el + tail
    assert parse(s, at)[0] == at + len(el)
    return s


def skipping_stream(tail_stream):
    """a 64 KiB literal from mid-tile to mid-tile (it jumps over 15 tiles of 4096), then the
    fragments of tail_stream (a joined stream)"""
    n, p = M.preamble(tail_stream)
    return M.varint(BLOCK + n) + M.literal(_rnd(BLOCK, 5)) + tail_stream[p:]


def periodic_stream(ntile, T=TILE):
    """literals of 59 bytes whose every byte is that literal's own tag: a walk from any position
    finds 60-byte elements and stays in its residue class, so a wrong entry never merges with
    the chain and one more tile becomes final per round (T mod 60 != 0)"""
    assert T % 60
    tag = 58 << 2
    count = ntile * T // 60
    return M.varint(59 * count) + bytes([tag]) * (60 * count)


# ---- the mutation corpus -----------------------------------------------------------------------

def _swallow(stream, rng):
    """two byte edits that keep the stream valid for stock readers: the last literal of one
    block takes the first literal of the next block (tag and bytes) as its own data, and a later
    copy gives the extra output bytes back.  None where no border of the stream has the shape."""
    status, starts = serial_split(stream)
    assert status == OK
    order = list(range(1, len(starts) - 1))
    rng.shuffle(order)
    for k in order:
        # the elements of blocks k - 1 and k with their positions
        pos, els = starts[k - 1], []
        while pos < starts[k + 1]:
            nxt, length = parse(stream, pos)
            els.append((pos, nxt, length))
            pos = nxt
        i = next(i for i, e in enumerate(els) if e[0] == starts[k])
        a, b = els[i - 1], els[i]
        ta, tb = stream[a[0]], stream[b[0]]
        code = ta >> 2
        if ta & 3 or tb & 3 or code > 61:
            continue
        hb = b[1] - b[0] - b[2]
        grown = a[2] + hb + b[2]
        if grown > (60 if code < 60 else 256 if code == 60 else BLOCK):
            continue  # (the literal's header keeps its size)
        for c in els[i + 1:]:
            tc = stream[c[0]]
            if (tc & 3 == M.COPY2 and c[2] > hb) or (tc & 3 == M.COPY1 and c[2] - 4 >= hb):
                t = bytearray(stream)
                if code < 60:
                    t[a[0]] = (grown - 1) << 2
                else:
                    t[a[0] + 1:a[0] + code - 58] = (grown - 1).to_bytes(code - 59, "little")
                t[c[0]] = tc - 4 * hb
                return bytes(t)
    return None


def _far_offset(stream, rng):
    """one byte set: the high offset byte of a seeded copy-2 element"""
    status, starts = serial_split(stream)
    assert status == OK
    pos, at = starts[0], []
    while pos < len(stream):
        if stream[pos] & 3 == M.COPY2:
            at.append(pos)
        pos = parse(stream, pos)[0]
    if not at:
        return None
    t = bytearray(stream)
    t[at[int(rng.integers(0, len(at)))] + 2] = int(rng.integers(1, 256))
    return bytes(t)


def mutation_corpus(bases, seed=2000):
    """seeded byte mutations of joined streams -> [(mutant, index of its base)]: per base 12
    single bit flips, 8 bytes set, 4 truncations, 4 streams with bytes appended, 6 double bit
    flips, up to 2 swallows (a literal made to take the next block's first literal) and 4 high
    offset bytes of a copy-2 set"""
    out = []
    for b, s in enumerate(bases):
        rng = np.random.default_rng(seed + 17 * b)
        for _ in range(12):
            t = bytearray(s)
            t[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
            out.append((bytes(t), b))
        for _ in range(8):
            t = bytearray(s)
            t[int(rng.integers(0, len(s)))] = int(rng.integers(0, 256))
            out.append((bytes(t), b))
        for _ in range(4):
            out.append((s[:int(rng.integers(1, len(s)))], b))
        for _ in range(4):
            out.append((s + _rnd(int(rng.integers(1, 9)), int(rng.integers(0, 1 << 30))), b))
        for _ in range(6):
            t = bytearray(s)
            for _ in range(2):
                t[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
            out.append((bytes(t), b))
        for edit in (_swallow, _swallow, _far_offset, _far_offset, _far_offset, _far_offset):
            t = edit(s, rng)
            if t is not None:
                out.append((t, b))
    return out
