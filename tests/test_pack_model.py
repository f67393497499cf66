"""CPU tests of the frame packing model (tests/pack_model.py): hand-worked cases of every
function as literals, and LZ4 frames built from the oracle's blocks by the model's rules that
the stock decoders (pyarrow's LZ4_FRAME codec, liblz4's LZ4F_decompress) must accept and
decode to the input -- so the raw-block rule, the size fields and the header checksum byte
are judged by code the project did not write."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as O
import pack_model as P

ERR = P.SEGMENT_ERROR


def test_xxh32_known_answers():
    # the xxHash specification's own vectors, and an input that runs the 16-byte lanes
    assert P.xxh32(b"") == 0x02CC5D05
    assert P.xxh32(b"", 1) == 0x0B2CB792
    assert P.xxh32(b"abc") == 0x32D153FF
    assert P.xxh32(b"Nobody inspects the spammish repetition") == 0xE2293B2F


def test_offsets_by_hand():
    off, flagged = P.offsets([], 256)
    assert off.dtype == np.uint64 and off.tolist() == [0] and not flagged
    off, flagged = P.offsets([7], 256)
    assert off.tolist() == [0, 7] and not flagged
    off, flagged = P.offsets([0], 256)
    assert off.tolist() == [0, 0] and not flagged
    # a size at the limit counts, one above it counts 0 and flags
    off, flagged = P.offsets([10, 256, 20], 256)
    assert off.tolist() == [0, 10, 266, 286] and not flagged
    off, flagged = P.offsets([10, 257, 20], 256)
    assert off.tolist() == [0, 10, 10, 30] and flagged
    off, flagged = P.offsets([10, ERR, 20, 0, 5], 256)
    assert off.tolist() == [0, 10, 10, 30, 30, 35] and flagged
    # no stride: every size but SEGMENT_ERROR counts
    off, flagged = P.offsets([5, ERR - 1, ERR, 1], P.NO_STRIDE_LIMIT)
    assert off.tolist() == [0, 5, 0x100000003, 0x100000003, 0x100000004] and flagged
    # a total above 2^32
    off, flagged = P.offsets([0x80000000, 0x80000000, 0x80000001, 3], P.NO_STRIDE_LIMIT)
    assert off.tolist() == [0, 0x80000000, 0x100000000, 0x180000001, 0x180000004]
    assert not flagged


def test_pack_by_hand():
    slab = np.arange(32, dtype=np.uint8)  # four slots of 8 bytes
    assert P.pack(slab, 8, []).tolist() == []
    assert P.pack(slab, 8, [3]).tolist() == [0, 1, 2]
    assert P.pack(slab, 8, [2, 0, 8, 1]).tolist() == [0, 1, 16, 17, 18, 19, 20, 21, 22, 23, 24]
    # a flagged size in the middle packs nothing
    assert P.pack(slab, 8, [2, 9, 3]).tolist() == [0, 1, 16, 17, 18]
    assert P.pack(slab, 8, [2, ERR, 3]).tolist() == [0, 1, 16, 17, 18]


def test_lz4f_blocks_by_hand():
    data = np.frombuffer(b"ABCDEFGHIJ", np.uint8)  # seg 4: blocks ABCD, EFGH, IJ
    slab = np.frombuffer(b"abcdefgh" b"ijklmnop" b"qrstuvwx", np.uint8)  # stride 8
    framed, off, body = P.lz4f_blocks(np.zeros(0, np.uint8), 4, slab, 8, [])
    assert (framed.tolist(), off.tolist(), body) == ([], [0], b"")
    # one block, smaller than its input: the slot's bytes under their size
    framed, off, body = P.lz4f_blocks(data[:4], 4, slab, 8, [3])
    assert (framed.tolist(), off.tolist()) == ([7], [0, 7])
    assert body == b"\x03\x00\x00\x00abc"
    # size < len, == len (raw: a block that did not shrink), then the short last block at
    # its own length (2: raw)
    framed, off, body = P.lz4f_blocks(data, 4, slab, 8, [1, 4, 2])
    assert (framed.tolist(), off.tolist()) == ([5, 8, 6], [0, 5, 13, 19])
    assert body == b"\x01\x00\x00\x00a" b"\x04\x00\x00\x80EFGH" b"\x02\x00\x00\x80IJ"
    # == len + 1, a failed segment (both raw), and the last block one below its length
    framed, off, body = P.lz4f_blocks(data, 4, slab, 8, [5, ERR, 1])
    assert (framed.tolist(), off.tolist()) == ([8, 8, 5], [0, 8, 16, 21])
    assert body == b"\x04\x00\x00\x80ABCD" b"\x04\x00\x00\x80EFGH" b"\x01\x00\x00\x00q"
    # an empty compressed block is a size field of 0 (never written by the codec)
    framed, off, body = P.lz4f_blocks(data[:4], 4, slab, 8, [0])
    assert (framed.tolist(), body) == ([4], b"\x00\x00\x00\x00")


def test_lz4f_frame_by_hand():
    assert P.lz4f_header()[:6] == b"\x04\x22\x4d\x18\x60\x40" and len(P.lz4f_header()) == 7
    assert P.lz4f_frame(b"") == P.lz4f_header() + b"\x00\x00\x00\x00"
    assert P.lz4f_frame(b"\x01\x00\x00\x80x") == P.lz4f_header() + b"\x01\x00\x00\x80x" + bytes(4)


# ---- real frames under the stock decoders ---------------------------------------------------

# one 4-byte match between two short literal runs: a match of m bytes saves m and costs its
# 2-byte offset and the next token, so the block is exactly as long as its input
EQUAL = b"abcdWXYZabcd0123456789:;"
NAMES = ("kind 0, all raw", "kind 6, all compressed", "kind 6, 1-byte tail",
         "kind 1 across a border", "size == length")


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (input bytes, seg)}"""
    mixed = O.fill(1, 3, (2 << 20) + 8192 + 1)[(2 << 20) - 8192:]  # text | random, 1-byte tail
    return {
        "kind 0, all raw": (O.fill(0, 3, 2 * 65536 + 1).tobytes(), 65536),
        "kind 6, all compressed": (O.fill(6, 3, 2 * 65536 + 4321).tobytes(), 65536),
        "kind 6, 1-byte tail": (O.fill(6, 3, 2 * 65536 + 1).tobytes(), 65536),
        "kind 1 across a border": (mixed.tobytes(), 2048),
        "size == length": (b"a" * 24 + EQUAL + b"b" * 24 + b"z", 24),
    }


@functools.lru_cache(maxsize=None)
def framed_case(name):
    """the oracle's block of every segment in a slab -> (data, seg, slab, stride, sizes)"""
    data, seg = cases()[name]
    stride = O.lz4_bound(seg) + 7
    nseg = (len(data) + seg - 1) // seg
    slab = np.full(nseg * stride, 0xEE, np.uint8)
    sizes = np.zeros(nseg, np.uint32)
    for i in range(nseg):
        r, c = O.lz4_compress(data[i * seg:(i + 1) * seg])
        assert r == 0
        slab[i * stride:i * stride + len(c)] = np.frombuffer(c, np.uint8)
        sizes[i] = len(c)
    return np.frombuffer(data, np.uint8), seg, slab, stride, sizes


def block_forms(name):
    """per block: True where the model ships it raw (read from the size fields)"""
    data, seg, slab, stride, sizes = framed_case(name)
    _, off, body = P.lz4f_blocks(data, seg, slab, stride, sizes)
    return [body[int(o) + 3] >> 7 == 1 for o in off[:-1]]


def test_cases_have_the_forms_they_are_named_for():
    assert all(block_forms("kind 0, all raw"))
    assert not any(block_forms("kind 6, all compressed"))
    assert block_forms("kind 6, 1-byte tail") == [False, False, True]
    forms = block_forms("kind 1 across a border")
    assert forms == [False] * 4 + [True] * 5  # text, random, the 1-byte tail
    data, seg, slab, stride, sizes = framed_case("size == length")
    assert sizes.tolist()[1] == len(EQUAL) == seg
    assert block_forms("size == length") == [False, True, False, True]


def lz4f_decompress(frame, n):
    """liblz4's LZ4F_decompress of one whole frame -> bytes, or None where liblz4 is missing"""
    try:
        L = ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None
    sz = ctypes.c_size_t
    L.LZ4F_createDecompressionContext.restype = sz
    L.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    L.LZ4F_freeDecompressionContext.restype = sz
    L.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
    L.LZ4F_decompress.restype = sz
    L.LZ4F_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(sz),
                                  ctypes.c_void_p, ctypes.POINTER(sz), ctypes.c_void_p]
    L.LZ4F_isError.restype = ctypes.c_uint
    L.LZ4F_isError.argtypes = [sz]
    ctx = ctypes.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100))
    try:
        src = ctypes.create_string_buffer(frame, len(frame))
        dst = ctypes.create_string_buffer(n + 1)
        at, out = 0, 0
        while True:
            dn, sn = sz(n + 1 - out), sz(len(frame) - at)
            hint = L.LZ4F_decompress(ctx, ctypes.byref(dst, out), ctypes.byref(dn),
                                     ctypes.byref(src, at), ctypes.byref(sn), None)
            if L.LZ4F_isError(hint):
                raise ValueError(f"LZ4F_decompress: error {hint - (1 << 64)}")
            at += sn.value
            out += dn.value
            if hint == 0:
                break
            if sn.value == 0 and dn.value == 0:
                raise ValueError("LZ4F_decompress: the frame ends early")
        if at != len(frame):
            raise ValueError("LZ4F_decompress: bytes behind the EndMark")
        return dst.raw[:out]
    finally:
        L.LZ4F_freeDecompressionContext(ctx)


@pytest.mark.parametrize("name", NAMES)
def test_stock_decoders_accept_the_models_frames(name):
    pa = pytest.importorskip("pyarrow")
    data, seg, slab, stride, sizes = framed_case(name)
    framed, off, body = P.lz4f_blocks(data, seg, slab, stride, sizes)
    assert len(body) == int(off[-1]) == int(framed.sum(dtype=np.uint64))
    frame = P.lz4f_frame(body)
    plain = data.tobytes()
    assert pa.Codec("lz4").decompress(frame, decompressed_size=len(plain)).to_pybytes() == plain
    got = lz4f_decompress(frame, len(plain))
    assert got is None or got == plain


def test_stock_decoders_reject_another_header_checksum():
    """the byte lz4f_header computes is the only one the stock decoders take"""
    pa = pytest.importorskip("pyarrow")
    data, seg, slab, stride, sizes = framed_case("size == length")
    frame = bytearray(P.lz4f_frame(P.lz4f_blocks(data, seg, slab, stride, sizes)[2]))
    for delta in (1, 0x80, 0xFF):
        bad = bytearray(frame)
        bad[6] = (bad[6] + delta) & 0xFF
        with pytest.raises(Exception):
            pa.Codec("lz4").decompress(bytes(bad), decompressed_size=data.size)
        if lz4f_decompress(bytes(frame), data.size) is not None:
            with pytest.raises(ValueError):
                lz4f_decompress(bytes(bad), data.size)


def test_a_failed_segment_ships_raw_and_decodes():
    """SEGMENT_ERROR in sizes: that block is the input slice, and the frame still decodes"""
    pa = pytest.importorskip("pyarrow")
    data, seg, slab, stride, sizes = framed_case("kind 6, 1-byte tail")
    failed = sizes.copy()
    failed[1] = ERR
    framed, off, body = P.lz4f_blocks(data, seg, slab, stride, failed)
    assert framed.tolist() == [4 + int(sizes[0]), 4 + seg, 5]
    frame = P.lz4f_frame(body)
    assert pa.Codec("lz4").decompress(frame, decompressed_size=data.size).to_pybytes() == \
        data.tobytes()
