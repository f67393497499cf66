"""The LZ4 emitter (compress.hip Lz4Out::bulk: the record lanes store their sequences' header
bytes, only the literal bytes are gathered, a flush is cut into chunks that fit the staging
ring) on inputs built so that the oracle's streams hold every boundary of that code:

  * literal runs of 0, 1, 14, 15, 16, 269 and >= 270 bytes (no / one literal-length byte; the
    general path from 270 on);
  * matches of 4, 18, 19, 20, 273 and >= 274 bytes (likewise);
  * back-to-back matches: several empty literal runs in one flush (they share a start);
  * consecutive sequences of 200-269 literals: a flush whose output exceeds the staging
    ring, so more than one chunk is taken;
  * a special record (run >= 270) between ordinary ones: a flush split in two ranges;
  * a literal run that starts below the input ring (> 4 KiB of literals: probe-skipped);
  * a segment that ends a few bytes after its last match.

The input is made of units: a source block, then (literals, match) pairs whose matches copy
from that block.  The oracle's LZ4 parse looks up and inserts every position only within 128
bytes of a match's end and every second or fourth position beyond (bo_window_parse_flags), and
its hash table is small, so a copy is found at its first byte and full length only when its
source is recent and was scanned position by position: a source block is 96-byte pseudo-random
chunks, each followed by an 8-byte copy from its own start, and sits right before its unit.
The compressed slots and sizes are compared with the oracle's (`compress_segments`), for LZ4
and LZ4_WIDE at 64 KiB and 2 KiB segments; `test_inputs_hold_every_class` (no GPU needed)
walks the oracle's streams and asserts that each class occurs, so the input cannot silently
stop covering them.
"""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_lz4 import down, eng, up  # noqa: F401  (fixture reuse)

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

SEGS = (65536, 2048)
CODECS = (("LZ4", O.CODEC_LZ4), ("LZ4_WIDE", O.CODEC_LZ4_WIDE))

LITS = (0, 1, 14, 15, 16, 269)
MATCHES = (4, 18, 19, 20, 273)
WANTED = {("ll", n) for n in LITS} | {("ml", n) for n in MATCHES} | \
    {"ll>=270", "ml>=274", "back_to_back", "many_chunks", "split_flush", "short_tail"}
WANTED_64K = WANTED | {"below_ring"}
CHUNK = 96


class _Seg:
    """one segment's bytes"""

    def __init__(self, rng, seg):
        self.rng, self.seg, self.out, self.src, self.own = rng, seg, bytearray(), 0, 0

    def lits(self, n):
        self.own = len(self.out)
        self.out += self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def source(self, n):
        """a source block for n bytes of matches (from its byte 16 on: the chunk's first bytes
        occur twice)"""
        start = len(self.out)
        while len(self.out) - start < n + 24:
            c = len(self.out)
            self.lits(CHUNK)
            self.out += self.out[c + 4:c + 12]
        self.src = start + 16

    def match(self, n, own=False):
        """n bytes copied from the source block, or from the last literal stretch itself"""
        p = self.own if own else self.src
        assert p + n <= len(self.out)
        self.out += self.out[p:p + n]
        if not own:
            self.src += n + 1  # (the byte after a source is never the next one's first)

    def with_unit(self, unit, own):
        """a copy of this segment with the unit appended"""
        s = _Seg(self.rng, self.seg)
        s.out = bytearray(self.out)
        if not own:
            s.source(sum(ml + 1 for _, ml in unit))
        for ll, ml in unit:
            s.lits(ll)
            s.match(ml, own)
        return s

    def close(self):
        """fill up, and end the segment 6 bytes after a 16-byte match"""
        fill = self.seg - 22 - len(self.out)
        assert fill >= 32  # (the fill's last 32 bytes are the last match's source)
        self.lits(fill - 32)
        self.lits(32)
        self.match(16, own=True)
        self.lits(self.seg - len(self.out))
        assert len(self.out) == self.seg
        return bytes(self.out)


def _units(seg):
    """the script: (unit, own); a unit's matches share one source block, so they add up to
    < 80 bytes or the unit is a single pair.  own: the matches copy from the literal run before
    them instead (no source block between the pairs; found up to a probe stride late)"""
    short = [(3, 6), (2, 5), (7, 9), (1, 4), (5, 12)]
    units = [[(ll, ml) for ml in MATCHES[:4]] for ll in LITS[:5]]
    units += [[(0, 5)] * 7, short]                                   # back to back
    units += [[(269, 273)], [(2, 6)], [(270, 8)], short]             # 269 / 273 / >= 270
    units += [[(269, 20)], [(16, 273)], [(269, 273)]]                # (a source may be evicted)
    units += [[(3, 274)], [(1, 8)], [(40, 300)], short]              # >= 274
    units += [short[:4] + [(400, 12)] + short[:4], short]            # a flush split
    if seg >= 16384:
        units += [[(6000, 12)], short]                               # below the input ring
    units = [(u, False) for u in units]
    # many chunks: six runs of 200-269 literals in a row
    units.append(([(30, 12)] + [(ll, 70) for ll in (204, 205, 203, 206, 202, 204)], True))
    return units


def emit_input(seg):
    """a few segments of `seg` bytes and a short last one"""
    rng = np.random.default_rng(5151 + seg)
    segs, cur = [], _Seg(rng, seg)
    cur.lits(300)
    rnd = 0
    while rnd < 3 or len(segs) < 2:
        rnd += 1
        for unit, own in _units(seg):
            nxt = cur.with_unit(unit, own)
            if len(nxt.out) + 64 > seg:  # (it does not fit: into a new segment)
                segs.append(cur.close())
                cur = _Seg(rng, seg)
                cur.lits(40 + 7 * len(segs))
                nxt = cur.with_unit(unit, own)
                assert len(nxt.out) + 64 <= seg
            cur = nxt
    segs.append(cur.close())
    last = _Seg(rng, seg).with_unit([(30, 5), (0, 5), (16, 19), (15, 18)], False)
    last.lits(9)
    return np.frombuffer(b"".join(segs) + bytes(last.out), np.uint8)


def walk_block(blk):
    """an LZ4 block's sequences [(literals, offset, match length)] and its final literals"""
    seqs, i, n = [], 0, len(blk)
    while True:
        tok = blk[i]
        i += 1
        ll = tok >> 4
        if ll == 15:
            while blk[i] == 255:
                ll += 255
                i += 1
            ll += blk[i]
            i += 1
        i += ll
        if i >= n:
            assert i == n
            return seqs, ll
        off = blk[i] | blk[i + 1] << 8
        i += 2
        ml = (tok & 15) + 4
        if ml == 19:
            while blk[i] == 255:
                ml += 255
                i += 1
            ml += blk[i]
            i += 1
        seqs.append((ll, off, ml))


def classes(seqs, final):
    got = {("ll", ll) for ll, _, _ in seqs} | {("ml", ml) for _, _, ml in seqs}
    lls = [ll for ll, _, _ in seqs]
    special = [ll >= 270 or ml >= 274 for ll, _, ml in seqs]
    if any(ll >= 270 for ll in lls):
        got.add("ll>=270")
    if any(ml >= 274 for _, _, ml in seqs):
        got.add("ml>=274")
    if any(ll > 4096 + 128 for ll in lls):
        got.add("below_ring")
    if final <= 12:
        got.add("short_tail")
    for k in range(len(seqs)):
        if lls[k:k + 4] == [0] * 4:
            got.add("back_to_back")
        # 6 ordinary sequences in a row, > 1200 output bytes: several times the staging ring
        run = lls[k:k + 6]
        if len(run) == 6 and all(200 <= ll < 270 for ll in run) and not any(special[k:k + 6]):
            got.add("many_chunks")
        # a special record with four short ordinary ones on either side (a flush holds >= 48)
        if special[k] and 4 <= k <= len(seqs) - 5 and not any(special[k - 4:k]) and \
                not any(special[k + 1:k + 5]) and sum(lls[k - 4:k] + lls[k + 1:k + 5]) < 200:
            got.add("split_flush")
    return got


def _oracle(codec, data, seg, stride=None):
    stride = stride or (O.lz4_bound(seg) + 63) // 64 * 64
    r, slab, sizes = O.compress_segments(codec, data, seg, stride)
    assert r == 0
    return stride, slab, sizes


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("name,codec", CODECS)
def test_inputs_hold_every_class(name, codec, seg):
    """no GPU needed: the oracle's streams of the inputs contain every boundary class"""
    data = emit_input(seg)
    assert data.size > 2 * seg
    stride, slab, sizes = _oracle(codec, data, seg)
    got = set()
    for i in range(sizes.size):
        seqs, final = walk_block(slab[i * stride:i * stride + sizes[i]].tobytes())
        got |= classes(seqs, final)
    want = WANTED_64K if seg == 65536 else WANTED
    assert want <= got, sorted(want - got, key=str)


@gpu
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("name,codec", CODECS)
def test_emitter_bit_exact_vs_oracle(eng, name, codec, seg):
    import bitar_amd
    data = emit_input(seg)
    n = data.size
    slab, stride, sizes = eng.compress(getattr(bitar_amd, "CODEC_" + name), up(data)[:n], seg)
    eng.sync()
    _, oslab, osizes = _oracle(codec, data, seg, stride)
    gsizes = down(sizes).astype(np.uint32)
    assert np.array_equal(gsizes, osizes)
    gslab = down(slab)
    for i in range(gsizes.size):
        a = gslab[i * stride:i * stride + gsizes[i]]
        b = oslab[i * stride:i * stride + osizes[i]]
        assert np.array_equal(a, b), f"segment {i}"
    out, prod = eng.decompress(bitar_amd.CODEC_LZ4, slab, stride, sizes, seg)
    eng.sync()
    assert np.array_equal(down(out)[:n], data)
