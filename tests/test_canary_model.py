"""The canary tests' own parts, checked without a GPU: the guarded views of tests/gpu_canary.py
flag a byte planted in any region they watch, and the streams tests/mutation_corpora.py
builds for tests/test_gpu_canaries.py are what they claim -- spacers that decode to nothing,
end-room streams that fill a segment of their plain size exactly and end in short sequences
of every copy branch -- under the oracle and the stock libraries."""
import ctypes
import zlib

import numpy as np
import pytest

import gpu_canary as C
import mutation_corpora as M
import oracle_lib as O

torch = pytest.importorskip("torch")

CODECS = [(O.CODEC_LZ4, O.lz4_decompress), (O.CODEC_DEFLATE, O.inflate),
          (O.CODEC_ZSTD, O.zstd_decompress)]
IDS = ["lz4", "deflate", "zstd"]


# ---- the helper ----------------------------------------------------------------------------
@pytest.mark.parametrize("residue", range(16))
def test_guarded_bytes_place_and_flag(residue):
    g = C.GuardedBytes(1000, residue, name="out")
    assert g.ptr % 16 == residue and g.view.data_ptr() == g.ptr
    assert g.start >= C.GUARD and g.buf.numel() - g.start - g.n >= C.GUARD
    g.load(np.arange(1000) % 251)
    g.check()
    assert np.array_equal(g.payload(), (np.arange(1000) % 251).astype(np.uint8))
    g.buf[g.start - 1] = 7
    g.buf[g.start - 40] = C.FILL  # (a stray copy of payload bytes shows too)
    with pytest.raises(AssertionError, match=r"out: front guard damaged, 2 bytes, first 40 and "
                                             r"last 1 bytes before"):
        g.check()
    g.buf[g.start - 1] = g.buf[g.start - 40] = C.GUARD_BYTE
    g.check()
    g.buf[g.start + g.n] = 0
    g.buf[g.start + g.n + 31] = 0
    with pytest.raises(AssertionError, match=r"out: back guard damaged, 2 bytes, first 0 and "
                                             r"last 31 bytes past"):
        g.check()


def test_guarded_bytes_spacer_range():
    g = C.GuardedBytes(4 * 100, 9, name="out")
    g.load(np.full(100, 1), at=0)
    g.load(np.full(100, 2), at=200)
    g.check_fill(100, 200, "spacer 1")
    g.check_fill(300, 400, "spacer 3")
    g.view[300] = C.GUARD_BYTE  # (guard bytes copied into a payload range show)
    g.view[331] = 0
    g.check_fill(100, 200, "spacer 1")
    with pytest.raises(AssertionError, match=r"spacer 3 \[300, 400\) written, 2 bytes, first at "
                                             r"\+0 and last at \+31"):
        g.check_fill(300, 400, "spacer 3")
    g.check()  # (the guards themselves are intact)


def test_guarded_words_flag():
    w = C.GuardedWords(5, name="produced")
    assert w.ptr % 4 == 0 and w.view.data_ptr() == w.ptr
    w.load([1, 2, 0xFFFFFFFF, 4, 5])
    w.check()
    assert w.values().tolist() == [1, 2, 0xFFFFFFFF, 4, 5]
    w.buf[C.WORDS + 5] = 0
    with pytest.raises(AssertionError, match=r"produced: back guard damaged, 1 words, first 0"):
        w.check()
    w.buf[C.WORDS + 5] = C.GUARD_WORD - (1 << 32)
    w.buf[C.WORDS - 1] = 3
    with pytest.raises(AssertionError, match=r"produced: front guard damaged, 1 words, first 1"):
        w.check()


def test_guarded_slots_flag():
    s = C.GuardedSlots(3, 512, name="slots")
    assert all(p % 16 == 0 for p in s.ptrs)
    assert [b - a for a, b in zip(s.ptrs, s.ptrs[1:])] == [512 + C.GUARD] * 2
    assert s.ptr_tensor().tolist() == s.ptrs
    s.check()
    for i in range(3):
        assert np.all(s.slot(i) == C.FILL)
        s.buf[s.offset(i):s.offset(i) + 512] = i  # a call's own slots: any bytes
    s.check()
    s.buf[s.offset(1) + 512 + 15] = 0
    with pytest.raises(AssertionError, match=r"guard between slots 1 and 2 damaged, 1 bytes, "
                                             r"first 15 and last 15 bytes past the end of slot 1"):
        s.check()
    s.buf[s.offset(1) + 512 + 15] = C.GUARD_BYTE
    s.buf[s.offset(0) - 1] = 0
    with pytest.raises(AssertionError, match="front guard"):
        s.check()
    s.buf[s.offset(0) - 1] = C.GUARD_BYTE
    s.buf[s.offset(2) + 512] = 0
    with pytest.raises(AssertionError, match="back guard"):
        s.check()


# ---- the alignment plan --------------------------------------------------------------------
def test_plan_reaches_every_residue_of_input_and_output_segments():
    """at seg = 4099 the 17-segment call alone puts an input segment and an output segment
    at every address residue mod 16, from any base; the bases add the slab-less ends"""
    assert 4099 in C.SEGS and 17 * 4099 + 1 in C.plan_sizes(4099)
    for base in C.RESIDUES:  # (d_in and out use the same bases)
        assert C.segment_residues(base, 4099, 17 * 4099 + 1) == set(range(16))
    for seg in C.SEGS:
        sizes = C.plan_sizes(seg)
        assert sizes and all((n + seg - 1) // seg >= 4 for n in sizes)
        tails = {n % seg for n in sizes}
        if seg >= 4099:
            assert tails == {1, 15, 17}
        assert 0 not in tails or seg == 1  # a short last segment wherever one exists
    # every base residue 0..15 is reached by some segment start of the plan at >= 4 KiB
    reached = set()
    for seg in (s for s in C.SEGS if s >= 4096):
        for n in C.plan_sizes(seg):
            for base in C.RESIDUES:
                reached |= C.segment_residues(base, seg, n)
    assert reached == set(range(16))


# ---- spacers -------------------------------------------------------------------------------
@pytest.mark.parametrize("codec,decode", CODECS, ids=IDS)
def test_spacers_decode_to_nothing(codec, decode):
    s = M.spacer(codec)
    for cap in (0, 1, 4096, 65536):
        assert decode(s, cap) == (0, b"")
    if codec == O.CODEC_DEFLATE:
        assert zlib.decompress(s, -15) == b""
        assert M.spacer(O.CODEC_DEFLATE_DYN) == s
    elif codec == O.CODEC_LZ4:
        assert M.spacer(O.CODEC_LZ4_WIDE) == s
        L = M.liblz4()
        if L is not None:
            buf = ctypes.create_string_buffer(16)
            assert L.LZ4_decompress_safe(s, buf, len(s), 16) == 0
    else:
        assert O.zstd_compress(b"") == (0, s)
        Z = M.libzstd()
        if Z is not None:
            buf = ctypes.create_string_buffer(16)
            assert Z.ZSTD_decompress(buf, 16, s, len(s)) == 0


# ---- end-room streams ----------------------------------------------------------------------
def _stock_decode(codec, stream, cap):
    """the stock library's output, or None where the library is absent"""
    if codec == O.CODEC_DEFLATE:
        return zlib.decompress(stream, -15)
    buf = ctypes.create_string_buffer(cap + 16)
    if codec == O.CODEC_LZ4:
        L = M.liblz4()
        if L is None:
            return None
        r = L.LZ4_decompress_safe(stream, buf, len(stream), cap)
        assert r >= 0
        return buf.raw[:r]
    Z = M.libzstd()
    if Z is None:
        return None
    r = Z.ZSTD_decompress(buf, cap, stream, len(stream))
    assert not Z.ZSTD_isError(r)
    return buf.raw[:r]


@pytest.mark.parametrize("codec,decode", CODECS, ids=IDS)
def test_end_room_streams_fill_their_segment_exactly(codec, decode):
    streams = M.end_room_streams(codec)
    assert len(streams) >= 5
    names = [e["name"] for e in streams]
    assert len(set(names)) == len(names)
    assert 2 * sum(len(e["plain"]) % 16 != 0 for e in streams) >= len(streams)
    for e in streams:
        p = len(e["plain"])
        assert decode(e["stream"], p) == (0, e["plain"]), e["name"]
        assert decode(e["stream"], p + 64) == (0, e["plain"]), e["name"]
        for short in (1, 8, 33):
            r, _ = decode(e["stream"], p - short)
            assert r != 0, (e["name"], short)
        stock = _stock_decode(codec, e["stream"], p)
        assert stock is None or stock == e["plain"], e["name"]


@pytest.mark.parametrize("codec,decode", CODECS, ids=IDS)
def test_end_room_streams_end_in_the_claimed_shapes(codec, decode):
    """the last ~200 output bytes (of a "long" stream: the ~200 before its long matches):
    literal runs of every length 1..16, matches of min..16 bytes, an offset from every branch
    of lanes::copy_match -- from the builder's sequence list for LZ4 (the block itself is
    parsed back), from the plain's construction otherwise"""
    minm = 4 if codec == O.CODEC_LZ4 else 3
    streams = M.end_room_streams(codec)
    assert sum("long" in e["name"] for e in streams) >= 1
    for e in streams:
        plain = e["plain"]
        shapes, more = e["shapes"][:M.TAIL_SEQUENCES], e["shapes"][M.TAIL_SEQUENCES:]
        assert len(shapes) == M.TAIL_SEQUENCES
        assert sorted(s[0] for s in shapes) == list(range(1, 17)), e["name"]
        assert all(minm <= s[2] <= 16 for s in shapes)
        assert {s[2] for s in shapes} >= {minm, 16}
        for lo, hi in M.OFFSET_CLASSES[:3]:
            assert any(lo <= s[1] <= hi for s in shapes), (e["name"], lo)
        assert any(s[1] >= 32 for s in shapes), e["name"]
        tail = sum(s[0] + s[2] for s in shapes) + (0 if more else e["final"])
        assert 200 <= tail <= 400
        # a "long" stream goes on with matches above 16 bytes, which take copy_match's loops:
        # at every offset class, the last one 1 mod 32 bytes at an offset >= 32
        assert bool(more) == ("long" in e["name"])
        if more:
            assert [(s[0], s[2]) for s in more] == [(n, ml) for n, _, ml in M.LONG_SEQUENCES]
            assert all(s[2] > 16 and s[0] <= 16 for s in more)
            for (lo, hi), s in zip((M.OFFSET_CLASSES[c] for _, c, _ in M.LONG_SEQUENCES), more):
                assert lo <= s[1] <= hi
            assert {c for _, c, _ in M.LONG_SEQUENCES} == {0, 1, 2, 3}
            assert more[-1][1] >= 32 and more[-1][2] % 32 == 1
        # the plain's tail is those sequences: walk them backwards from its end
        at = len(plain) - e["final"]
        for nlit, off, ml in reversed(e["shapes"]):
            for j in range(at - ml, at):
                assert plain[j] == plain[j - off], (e["name"], j, off)
            at -= ml + nlit
        if codec == O.CODEC_LZ4:
            seqs = _lz4_sequences(e["stream"])
            count = len(e["shapes"])
            assert seqs[-1] == (e["final"], 0, 0)
            assert seqs[-count:-1] == [tuple(s) for s in e["shapes"][1:]]
            head = len(seqs) - count - 1  # (sequences inside the body)
            assert head == (2 if e["name"] == "lz4-deferred" else 0)
            assert seqs[head][1:] == shapes[0][1:] and seqs[head][0] >= shapes[0][0]
            if head:  # a short match from far behind, most of the block still ahead of it
                assert seqs[1] == (3, 11000, 8) and seqs[2][0] > 8000
            assert e["final"] >= 5 and e["shapes"][-1][2] + e["final"] >= 12


def _lz4_sequences(block):
    """(literal count, offset, match length) of every sequence of an LZ4 block; the last one
    has no match"""
    seqs, at = [], 0
    while at < len(block):
        tok = block[at]
        at += 1
        ll, ml = tok >> 4, tok & 15
        if ll == 15:
            while True:
                ll += block[at]
                at += 1
                if block[at - 1] != 255:
                    break
        at += ll
        if at == len(block):
            seqs.append((ll, 0, 0))
            break
        off = block[at] | block[at + 1] << 8
        at += 2
        if ml == 15:
            while True:
                ml += block[at]
                at += 1
                if block[at - 1] != 255:
                    break
        seqs.append((ll, off, ml + 4))
    return seqs


def test_end_room_zstd_literal_sections_and_headers():
    """one frame with Huffman literals in its last block (they sit at the slot's tail in the
    lane decoder), one with raw literals, one without a content size; the lane decoder's
    scope (tests/zstd_routing.py) holds some of them, one without a content size included, and
    leaves others to the wave decoder"""
    import zstd_routing
    streams = M.end_room_streams(O.CODEC_ZSTD)
    lanes = {e["name"] for e in streams if zstd_routing.route(e["stream"], 1)["lanes"]}
    assert lanes and len(lanes) < len(streams)
    assert any("nofcs" in name for name in lanes), lanes
    assert any("long" in name for name in lanes), lanes  # long matches in the lane decoder
    assert zstd_routing.route(M.spacer(O.CODEC_ZSTD), 1)["lanes"]
    last = {e["name"]: M.zstd_literal_types(e["stream"])[-1:] for e in streams}
    assert any(t and t[0] in (2, 3) for t in last.values()), last
    assert any(t == [0] for t in last.values()), last
    nofcs = [e for e in streams if "nofcs" in e["name"]]
    assert nofcs
    for e in nofcs:
        fhd = e["stream"][4]
        assert fhd >> 6 == 0 and not fhd & 0x20  # no Frame_Content_Size field at all


def test_end_room_deflate_block_types():
    """a fixed-Huffman stream (the lane inflater's scope) and a dynamic one (the wave
    inflater's) of every plain, ours and zlib's"""
    streams = M.end_room_streams(O.CODEC_DEFLATE)
    for e in streams:
        btype = e["stream"][0] >> 1 & 3
        assert btype == (1 if "fixed" in e["name"] else 2), e["name"]
    assert {e["name"].split("-")[1] for e in streams} == {"fixed", "dynamic", "zlib"}
    assert any("fixed-long" in e["name"] for e in streams)  # long matches in the lane inflater
