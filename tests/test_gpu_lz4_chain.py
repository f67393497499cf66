"""The window parse's greedy match chain (window_parse.hip.h step 3: the matches of a 64-position
window chosen in lane order, each one the first valid lane at or past the previous match's end,
a match that reached 32 bytes extended cooperatively before the chain goes on) on inputs built so
that the oracle's LZ4 parse holds every shape of chain:

  * windows with exactly k selected matches, k = 1 .. 16 (4-byte repeats, 16 of them back to back);
  * a first valid lane of 0, 1, 62 and 63, and windows entered inside a match (pos > x);
  * chains whose last match ends at lane 63 (with and without a match starting at lane 63) and at 64;
  * one extension lane (a match of >= 32 bytes) at lanes 0, 31 and 63, a match of exactly 31 and 32
    bytes, two extension lanes in one window of which the second is reached only through the
    first's extension, and a chain of short matches behind an extension;
  * extensions past one 256-byte step, and past the input ring (read from HBM);
  * a window after a probe hit (a match behind >= 320 literals) and a window after skipped windows
    (a match right behind one of >= 192 bytes), and segments of the generator's kinds 0, 1, 2, 5, 6;
  * the segment's last windows, for segment lengths 13, 64 + 12 and 4096 + 5 (2112 segments of 13
    bytes: the call takes the cost-ordered dispatch).

A unit of the built segments is a window of random bytes (the source) and a window whose matches
copy from it; a unit is drawn again until the oracle's parse of the segment so far holds exactly
the wanted matches, and `test_inputs_hold_every_chain` (no GPU needed) asserts the match list per
window from the oracle's streams, so a case cannot silently test nothing.  The GPU's slots and
sizes must equal the oracle's (`compress_segments`) for LZ4, and for LZ4_WIDE on the same inputs,
with cost-ordered and with plain dispatch, and decode back to the input with our decoder and
with liblz4.

The stock-stream batches at the end go through the near decoder's deferral to the far kernel
(lz4_decompress.hip): deferred segments first, in the middle and last of a batch of our own and
liblz4 streams, every segment deferred, and none.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
import stock_lib as S
from test_gpu_lz4 import down, eng, up  # noqa: F401  (fixture reuse)
from test_gpu_lz4_emit import walk_block

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

SEG = 4096
W = 64  # window
TAIL = 96  # random bytes behind a segment under construction


def matches(blk):
    """[(position, length, distance)] of an LZ4 block's matches, and its final literals"""
    seqs, final = walk_block(bytes(blk))
    out, p = [], 0
    for ll, off, ml in seqs:
        p += ll
        out.append((p, ml, off))
        p += ml
    return out, final


def oracle_matches(data):
    r, comp = O.lz4_compress(bytes(data))
    assert r == 0
    return matches(comp)[0]


class _Build:
    """one segment, unit by unit; `want`: window start -> [(lane, length)] of its matches"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.b = bytearray()
        self.want = {}

    def rand(self, n):
        self.b += self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def unit(self, ms):
        """a source window, then matches ms = [(lane, length)] (lanes counted from the window
        behind the source; a lane >= 64 lies in the window after it), padded to a window's end"""
        assert len(self.b) % W == 0
        base = bytes(self.b)
        for _ in range(400):
            self.b = bytearray(base)
            self.rand(W)
            xt = len(self.b)
            for lane, ln in ms:
                self.rand(xt + lane - len(self.b))
                s = xt - W + int(self.rng.integers(0, W - 3))
                for k in range(ln):  # (a copy may run into its own output)
                    self.b.append(self.b[s + k])
            self.rand(-len(self.b) % W)
            tail = np.random.default_rng(1).integers(0, 256, TAIL, dtype=np.uint8).tobytes()
            got = [(p - xt, ml) for p, ml, _ in oracle_matches(bytes(self.b) + tail) if p >= xt - W]
            if got == list(ms):
                break
        else:
            raise AssertionError(f"no draw gives {ms}")
        for lane, ln in ms:
            self.want.setdefault(xt + lane // W * W, []).append((lane % W, ln))
        return self

    def close(self, seg=SEG):
        assert len(self.b) + W <= seg
        self.rand(seg - len(self.b))
        return bytes(self.b)


def _even(k):
    return [(i * W // k, 4) for i in range(k)]


@functools.lru_cache(maxsize=None)
def built():
    """[(segment bytes, want)] of the unit-built segments"""
    out = []
    b = _Build(101)  # exactly k matches, k = 1 .. 16
    for k in range(1, 17):
        b.unit(_even(k))
    out.append((b.close(), b.want))
    b = _Build(102)  # first valid lanes, chain ends, windows entered inside a match
    for ms in ([(0, 4)], [(1, 4)], [(62, 4)], [(63, 4)], [(62, 8), (72, 4)], [(59, 4)], [(60, 4)],
               [(3, 4), (59, 4)], [(5, 4), (60, 4)], [(59, 4), (63, 4)], [(10, 4), (59, 4), (63, 5)],
               [(63, 4), (67, 4), (127, 4)], [(0, 4), (63, 9), (72, 5), (120, 8)],
               [(1, 5), (6, 4), (10, 6), (16, 4), (61, 7), (68, 4)]):
        b.unit(ms)
    out.append((b.close(), b.want))
    b = _Build(103)  # extension lanes
    for ms in ([(0, 40)], [(31, 40)], [(63, 40)], [(0, 31), (40, 4)], [(0, 32), (40, 4)],
               [(4, 33), (40, 4)], [(2, 36), (38, 40)], [(5, 4), (20, 33), (53, 4)],
               [(2, 36), (40, 4), (50, 4), (60, 4)], [(0, 4), (4, 32), (36, 4), (40, 35)],
               [(1, 33), (34, 33), (67, 33)], [(9, 4), (30, 70), (101, 4), (110, 45)]):
        b.unit(ms)
    out.append((b.close(), b.want))
    b = _Build(104)  # long extensions: past one step, past the ring (HBM), skipped windows behind
    for ms in ([(7, 600)], [(0, 4), (30, 4)], [(10, 2000)], [(0, 4), (20, 4), (40, 5)]):
        b.unit(ms)
    out.append((b.close(), b.want))
    b = _Build(105)
    for ms in ([(63, 300)], [(2, 4), (9, 4)], [(33, 1700)], [(1, 4), (60, 4)], [(5, 256 + 32)]):
        b.unit(ms)
    out.append((b.close(), b.want))
    return out


@functools.lru_cache(maxsize=None)
def probe_segments():
    """random stretches (probed with stride 2, then 4) with copies behind them, and long copies
    (skipped windows) with short ones right behind"""
    rng = np.random.default_rng(106)
    segs = []
    for lits in (330, 700, 1500):
        b = bytearray(rng.integers(0, 256, lits, dtype=np.uint8).tobytes())
        while len(b) + 700 < SEG:
            for back, ln in ((lits // 2, 48), (100, 300), (30, 8), (200, 24)):
                s = len(b) - back
                for k in range(ln):
                    b.append(b[s + k])
                b += rng.integers(0, 256, 9, dtype=np.uint8).tobytes()
            b += rng.integers(0, 256, lits, dtype=np.uint8).tobytes()
        b += rng.integers(0, 256, SEG - len(b), dtype=np.uint8).tobytes()
        segs.append(bytes(b))
    return segs


@functools.lru_cache(maxsize=None)
def structured_input():
    """the built segments, the probe segments and 4 KiB of each generator kind: one call"""
    segs = [s for s, _ in built()] + probe_segments()
    segs += [O.fill(kind, 9, 2 * SEG).tobytes() for kind in (0, 1, 2, 5, 6)]
    return np.frombuffer(b"".join(segs), np.uint8)


def _low_entropy(rng, n):
    """runs and short periods over a few symbols: matches everywhere, up to the segment's end"""
    how = int(rng.integers(0, 4))
    if how == 0:
        return np.full(n, rng.integers(0, 256), np.uint8)
    if how == 1:
        return np.resize(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8), n)
    if how == 2:
        return rng.integers(0, int(rng.integers(2, 5)), n).astype(np.uint8)
    return rng.integers(0, 256, n, dtype=np.uint8)


EDGE_SEGS = ((13, 2112), (W + 12, 64), (SEG + 5, 16))  # (segment length, segments)


def _edge_window(seg):
    """start of the first window that applies the end-of-segment limits (the parse's x_edge)"""
    last_start, match_limit = seg - 12, seg - 5
    int_end = min(last_start + 1, match_limit - 32 if match_limit > 32 else 0)
    return (max(int_end - (W - 1), 0) + W - 1) // W * W if int_end >= W else 0


@functools.lru_cache(maxsize=None)
def _edge_units():
    """31 units of 1 .. 16 matches: 3968 bytes"""
    b = _Build(107)
    for k in range(31):
        b.unit(_even(1 + k % 16))
    return bytes(b.b)


@functools.lru_cache(maxsize=None)
def edge_input(seg, nseg):
    rng = np.random.default_rng(200 + seg)
    segs = []
    for i in range(nseg):
        if seg > SEG:  # (units up to the last two windows, so that these are scanned, not probed)
            b = np.concatenate([np.frombuffer(_edge_units(), np.uint8),
                                _low_entropy(rng, seg - len(_edge_units()))])
        else:
            b = _low_entropy(rng, seg)
        if i % 4 == 3 and seg >= 48:  # a match at the last position that may start one
            back = 40 if seg < 2 * W else 100  # (its source: in the window before its own)
            b[-back:] = rng.integers(0, 256, back, dtype=np.uint8)
            b[-12:-5] = b[-back:7 - back]
        segs.append(b)
    return np.concatenate(segs)


def _oracle(codec, data, seg, stride=None):
    stride = stride or (O.lz4_bound(seg) + 63) // 64 * 64
    r, slab, sizes = O.compress_segments(codec, data, seg, stride)
    assert r == 0
    return stride, slab, sizes


def test_inputs_hold_every_chain():
    """no GPU needed: the oracle's parse of the inputs has the chains the cases are named after"""
    data = structured_input()
    stride, slab, sizes = _oracle(O.CODEC_LZ4, data, SEG)
    counts = set()
    for i, (seg, want) in enumerate(built()):
        got = {}
        for p, ml, _ in matches(slab[i * stride:i * stride + sizes[i]])[0]:
            got.setdefault(p // W * W, []).append((p % W, ml))
        for x, ms in want.items():
            assert got.get(x) == ms, (i, x, ms, got.get(x))
            assert got.get(x - W) is None or x - W in want, (i, x)  # (the source window: no match)
            counts.add(len(ms))
    assert set(range(1, 17)) <= counts
    first = {ms[0][0] for _, want in built() for ms in want.values()}
    assert {0, 1, 62, 63} <= first
    ends = {ms[-1][0] + ms[-1][1] for _, want in built() for ms in want.values()}
    assert {63, 64} <= ends
    ext = {lane for _, want in built() for ms in want.values() for lane, ln in ms if ln >= 32}
    assert {0, 31, 63} <= ext
    assert any(sum(ln >= 32 for _, ln in ms) >= 2 for _, want in built() for ms in want.values())
    longest = max(ln for _, want in built() for ms in want.values() for _, ln in ms)
    assert longest >= 1600  # (the ring runs at most 1536 bytes ahead of the window)
    # probe hits and skipped windows
    nb = len(built())
    for i in range(nb, nb + len(probe_segments())):
        ms = matches(slab[i * stride:i * stride + sizes[i]])[0]
        ends_before = [0] + [p + ml for p, ml, _ in ms]
        assert any(p - e >= 320 for (p, _, _), e in zip(ms, ends_before)), i
        assert any(ml >= 192 and q - (p + ml) < W for (p, ml, _), (q, _, _) in zip(ms, ms[1:])), i
    # the last windows
    for seg, nseg in EDGE_SEGS:
        data = edge_input(seg, nseg)
        assert data.size == seg * nseg
        stride, slab, sizes = _oracle(O.CODEC_LZ4, data, seg)
        last, at_limit, at_start, per_window = 0, 0, 0, 0
        for i in range(nseg):
            ms = matches(slab[i * stride:i * stride + sizes[i]])[0]
            last += any(p >= _edge_window(seg) for p, _, _ in ms)
            at_limit += any(p + ml == seg - 5 for p, ml, _ in ms)
            at_start += any(p == seg - 12 for p, _, _ in ms)
            per_window = max(per_window, max([sum(q // W == p // W for q, _, _ in ms)
                                              for p, _, _ in ms] or [0]))
        assert last >= 4 and at_limit >= 4, (seg, last, at_limit)
        assert seg < 48 or at_start >= 2, (seg, at_start)
        assert seg < W or per_window >= (8 if seg > SEG else 4), (seg, per_window)


CODECS = (("LZ4", O.CODEC_LZ4), ("LZ4_WIDE", O.CODEC_LZ4_WIDE))
CASES = (("structured", SEG),) + tuple((f"edge{seg}", seg) for seg, _ in EDGE_SEGS)


def _case_input(case):
    if case == "structured":
        return structured_input()
    return edge_input(*[e for e in EDGE_SEGS if f"edge{e[0]}" == case][0])


@pytest.fixture(scope="module")
def plain():
    import bitar_amd
    e = bitar_amd.Engine(0, flags=bitar_amd.FLAG_PLAIN_ORDER)
    yield e
    e.close()


@gpu
@pytest.mark.parametrize("order", ["cost", "plain"])
@pytest.mark.parametrize("name,codec", CODECS)
@pytest.mark.parametrize("case,seg", CASES)
def test_chain_bit_exact_vs_oracle(eng, plain, case, seg, name, codec, order):
    import bitar_amd
    e = eng if order == "cost" else plain
    data = _case_input(case)
    n = data.size
    slab, stride, sizes = e.compress(getattr(bitar_amd, "CODEC_" + name), up(data)[:n], seg)
    e.sync()
    _, oslab, osizes = _oracle(codec, data, seg, stride)
    gsizes = down(sizes).astype(np.uint32)
    assert np.array_equal(gsizes, osizes)
    gslab = down(slab)
    col = np.arange(stride, dtype=np.uint32)[None, :]
    m = col < osizes[:, None]
    if not np.array_equal(gslab[:osizes.size * stride].reshape(-1, stride)[m],
                          oslab[:osizes.size * stride].reshape(-1, stride)[m]):
        for i in range(gsizes.size):
            a = gslab[i * stride:i * stride + gsizes[i]]
            b = oslab[i * stride:i * stride + osizes[i]]
            assert np.array_equal(a, b), f"segment {i}"
    out, prod = e.decompress(bitar_amd.CODEC_LZ4, slab, stride, sizes, seg)
    e.sync()
    assert np.array_equal(down(out)[:n], data)
    assert int(down(prod).astype(np.int64).sum()) == n
    assert np.array_equal(S.decompress(S.LZ4, gslab, stride, gsizes, n, seg), data)


# ---- the near decoder's deferral to the far kernel ---------------------------------------
FAR_SEG = 32768


@functools.lru_cache(maxsize=None)
def far_streams():
    """(input, our streams' oracle slab, liblz4's slab): segments whose second half repeats
    the first, so that liblz4 (64 KiB of history) codes matches 16 KiB back, past the near
    decoder's ring, and our parse (2560 bytes) none of them"""
    rng = np.random.default_rng(300)
    nseg = 12
    parts = []
    for _ in range(nseg):
        half = O.fill(1, int(rng.integers(1, 1000)), FAR_SEG // 2)
        half[::7] = rng.integers(0, 256, half[::7].size, dtype=np.uint8)
        parts += [half, half]
    host = np.concatenate(parts)
    sslab, sstride, ssz = S.compress(S.LZ4, host, FAR_SEG, 1)
    for i in range(nseg):
        ms = matches(sslab[i * sstride:i * sstride + ssz[i]])[0]
        assert any(off > 8192 for _, _, off in ms), i
    stride, oslab, osz = _oracle(O.CODEC_LZ4, host, FAR_SEG, sstride)
    return host, (oslab, osz), (sslab, ssz), stride


@gpu
@pytest.mark.parametrize("order", ["cost", "plain"])
@pytest.mark.parametrize("stock", [(0, 5, 11), tuple(range(12)), (), (0, 1, 2, 3, 4, 5, 6, 10, 11)])
def test_deferred_segments(eng, order, stock):
    """segments `stock` of the batch are liblz4's streams (deferred to the far kernel), the
    others our own; in a batch of 12 and, for the cost-ordered dispatch, of 2052 segments"""
    import bitar_amd
    host, (oslab, osz), (sslab, ssz), stride = far_streams()
    base = 12
    reps = 171 if order == "cost" else 1  # (>= 2048 segments: the ordered path)
    flags = bitar_amd.FLAG_COUNT_PATHS | (bitar_amd.FLAG_PLAIN_ORDER if order == "plain" else 0)
    e = bitar_amd.Engine(0, flags=flags)
    try:
        slab = np.zeros(base * stride, np.uint8)
        sizes = np.zeros(base, np.uint32)
        for i in range(base):
            src, z = (sslab, ssz) if i in stock else (oslab, osz)
            slab[i * stride:i * stride + z[i]] = src[i * stride:i * stride + z[i]]
            sizes[i] = z[i]
        slab, sizes, ref = np.tile(slab, reps), np.tile(sizes, reps), np.tile(host, reps)
        nseg = base * reps
        out = e.empty(nseg * FAR_SEG)
        prod = e.empty(nseg, dtype=torch.int32)
        e.decompress_slab_into(bitar_amd.CODEC_LZ4, up(slab), stride,
                               up(sizes.view(np.uint8)).view(torch.int32), nseg, FAR_SEG, out,
                               prod, capacity=nseg * FAR_SEG)
        e.sync()
        assert np.array_equal(down(prod).view(np.uint32), np.full(nseg, FAR_SEG, np.uint32))
        assert np.array_equal(down(out), ref)
        assert e.path_counters()["lz4_far"] == len(stock) * reps
    finally:
        e.close()
