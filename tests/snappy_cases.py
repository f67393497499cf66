"""Inputs shared by the Snappy tests (tests/test_snappy_model.py on the CPU,
tests/test_gpu_snappy.py on the GPU): the model's streams of the oracle's input kinds, stock
Snappy through pyarrow, and the seeded mutation corpus.  Test infrastructure only."""
import functools

import numpy as np

import oracle_lib as O
import snappy_model as M

SEED = 2000


def pa_codec():
    import pyarrow as pa
    return pa.Codec("snappy")


def pa_decode(stream, size):
    """pyarrow's verdict on a raw stream whose declared length is `size`: bytes or None"""
    import pyarrow as pa
    try:
        return pa_codec().decompress(bytes(stream), decompressed_size=size).to_pybytes()
    except (pa.ArrowException, OSError, ValueError):
        return None


def pa_encode(data):
    return pa_codec().compress(bytes(data)).to_pybytes()


def model_streams(data, seg):
    """the model's stream of every segment of data: the oracle's LZ4 block, re-emitted"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if data.size == 0:
        return []
    stride = (O.lz4_bound(seg) + 15) & ~15
    r, slab, sizes = O.compress_segments(O.CODEC_LZ4, data, seg, stride)
    assert r == 0
    return [M.from_lz4_block(part.tobytes(), slab[i * stride:i * stride + int(sizes[i])].tobytes())
            for i, part in enumerate(M.segments(data, seg))]


@functools.lru_cache(maxsize=None)
def base_stream(kind, seg):
    """(segment bytes, model stream) of the first whole segment of input kind `kind`"""
    data = O.fill(kind, SEED, seg)
    (stream,) = model_streams(data, seg)
    return data.tobytes(), stream


@functools.lru_cache(maxsize=None)
def mutation_corpus():
    """420 seeded mutations of the model's streams of kinds 1, 5 and 6 at segments of 4099 and
    65536 bytes -> [(stream, capacity)]: per base 25 single bit flips, 20 bytes set within the
    first 64, 10 truncations and 15 triple bit flips"""
    out = []
    for kind in (1, 5, 6):
        for seg in (4099, 65536):
            _, s = base_stream(kind, seg)
            rng = np.random.default_rng(SEED + 31 * kind + seg)
            assert len(s) > 64
            for _ in range(25):
                t = bytearray(s)
                t[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
                out.append((bytes(t), seg))
            for _ in range(20):
                t = bytearray(s)
                t[int(rng.integers(0, 64))] = int(rng.integers(0, 256))
                out.append((bytes(t), seg))
            for _ in range(10):
                out.append((s[:int(rng.integers(1, len(s)))], seg))
            for _ in range(15):
                t = bytearray(s)
                for _ in range(3):
                    t[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
                out.append((bytes(t), seg))
    assert len(out) == 420
    return out


def census(streams):
    """the classes a set of streams shows, as names"""
    seen = set()
    for s in streams:
        els = M.elements(s)
        n = M.preamble(s)[0]
        if len(els) == 1 and els[0][0] == M.LITERAL and els[0][1] == n:
            seen.add("stored")
        for k, length, offset, code in els:
            if k == M.LITERAL:
                seen.add("literal inline" if code < 60 else f"literal {code - 59}-byte length")
            else:
                seen.add({M.COPY1: "copy-1", M.COPY2: "copy-2", M.COPY4: "copy-4"}[k])
        # a split match: two copies of one offset in a row, the first of 64 or 60 bytes
        for a, b in zip(els, els[1:]):
            if a[0] != M.LITERAL and b[0] != M.LITERAL and a[2] == b[2] and a[1] in (64, 60):
                seen.add("split match")
    return seen


def hand_built():
    """[(stream, capacity, expected bytes or None)]: every format class a decoder must take and
    every way a stream must be refused"""
    abc = b"abcdefgh"
    out = []
    for code in (60, 61, 62, 63):  # long length codes on a short literal
        out.append((bytes([8]) + bytes([code << 2]) + (7).to_bytes(code - 59, "little") + abc,
                    64, abc))
    # copy-4
    out.append((bytes([16, 7 << 2]) + abc + bytes([3 | 7 << 2]) + (8).to_bytes(4, "little"),
                64, abc + abc))
    # a 5-byte varint, not minimal
    out.append((bytes([0x88, 0x80, 0x80, 0x80, 0x00, 7 << 2]) + abc, 64, abc))
    out.append((bytes([0x88, 0x80, 0x80, 0x80, 0x10, 7 << 2]) + abc, 64, None))  # fifth >= 16
    out.append((bytes([0x88, 0x80, 0x80, 0x80, 0x80, 0x00, 7 << 2]) + abc, 64, None))  # six
    # offset equal to the bytes produced
    out.append((bytes([16, 7 << 2]) + abc + M.copy(8, 8), 64, abc + abc))
    # overlap at offsets 1, 2 and 3: the copy replicates
    for off in (1, 2, 3):
        want = abc + bytes(abc[8 - off + i % off] for i in range(20))
        out.append((bytes([28, 7 << 2]) + abc + M.copy(off, 20), 64, want))
    out.append((bytes([8]) + M.copy(1, 8), 64, None))                    # a copy first
    out.append((bytes([16, 7 << 2]) + abc + bytes([2 | 7 << 2, 0, 0]), 64, None))  # offset 0
    out.append((bytes([16, 7 << 2]) + abc + M.copy(9, 8), 64, None))     # beyond the output
    out.append((bytes([8, 7 << 2]) + abc + b"\x00z", 64, None))          # a trailing element
    out.append((bytes([9, 7 << 2]) + abc, 64, None))                     # short output
    out.append((bytes([8, 7 << 2]) + abc[:7], 64, None))                 # truncated literal
    out.append((bytes([8, 60 << 2]), 64, None))                          # truncated length
    out.append((bytes([16, 7 << 2]) + abc + bytes([2 | 7 << 2, 8]), 64, None))  # truncated copy
    out.append((bytes([65, 7 << 2]) + abc, 64, None))                    # above the capacity
    out.append((b"", 64, None))
    out.append((b"\x00", 64, b""))
    # the same elements at the head of a longer stream (four literals of 50 bytes behind them), so
    # that a decoder with a path for many short elements at once meets them there: the accepted
    # ones, and the three bad copies
    tail = bytes(range(50, 250))
    pad = b"".join(M.literal(tail[k:k + 50]) for k in range(0, 200, 50))
    for stream, cap, want in list(out):
        pre = M.preamble(stream)
        if pre is None or pre[0] > cap:
            continue
        bad_copy = want is None and stream[pre[1]:] in (
            M.copy(1, 8), bytes([7 << 2]) + abc + bytes([2 | 7 << 2, 0, 0]),
            bytes([7 << 2]) + abc + M.copy(9, 8))
        if want is not None or bad_copy:
            out.append((M.varint(pre[0] + 200) + stream[pre[1]:] + pad, 512,
                        None if want is None else want + tail))
    # a copy from 4990 back -- beyond a 4 KiB history ring -- and right behind it a copy that
    # overlaps the first one's bytes, then the four literals; and the same with the first copy
    # reaching one byte before the output's start
    body = bytes(np.random.default_rng(SEED).integers(0, 256, 5000, dtype=np.uint8))
    for off in (4990, 5001):
        stream = M.varint(5218) + M.literal(body) + M.copy(off, 10) + M.copy(5, 8) + pad
        want = bytearray(body)
        if off <= 5000:
            want += want[5000 - off:5010 - off]
            for _ in range(8):
                want.append(want[-5])
            want += tail
        out.append((stream, 8192, bytes(want) if off <= 5000 else None))
    return out
