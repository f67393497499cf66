"""The Snappy segment format (tests/snappy_model.py) on the CPU: worked examples byte for byte,
stock Snappy (pyarrow) as the reader of every model stream and as the judge of the model's
decoder on a mutation corpus, the size bound, and the library's surface for the new id."""
import numpy as np
import pytest

import oracle_lib as O
import snappy_cases as C
import snappy_model as M

pa = pytest.importorskip("pyarrow")

KINDS = (0, 1, 2, 5, 6)
SEGS = (65536, 4099)


def test_varint_and_literal_tag_boundaries():
    assert M.varint(0) == b"\x00" and M.varint(127) == b"\x7f"
    assert M.varint(128) == b"\x80\x01" and M.varint(16383) == b"\xff\x7f"
    assert M.varint(16384) == b"\x80\x80\x01" and M.varint(65536) == b"\x80\x80\x04"
    body = bytes(range(256)) * 2
    assert M.literal(body[:1]) == b"\x00" + body[:1]
    assert M.literal(body[:60]) == bytes([59 << 2]) + body[:60]
    assert M.literal(body[:61]) == bytes([60 << 2, 60]) + body[:61]
    assert M.literal(body[:256]) == bytes([60 << 2, 255]) + body[:256]
    assert M.literal(body[:257]) == bytes([61 << 2, 0, 1]) + body[:257]
    assert M.literal(bytes(65536))[:3] == bytes([61 << 2, 0xFF, 0xFF])


def test_match_pieces_and_copy_elements():
    assert M.pieces(11) == [11] and M.pieces(12) == [12] and M.pieces(64) == [64]
    assert M.pieces(65) == [60, 5] and M.pieces(67) == [60, 7] and M.pieces(68) == [64, 4]
    assert M.pieces(130) == [64, 60, 6] and M.pieces(131) == [64, 60, 7]
    assert M.pieces(132) == [64, 64, 4]
    # copy-1: tag 01 | (len - 4) << 2 | (offset >> 8) << 5, then the offset's low byte
    assert M.copy(1, 4) == bytes([0x01, 0x01])
    assert M.copy(2047, 11) == bytes([0x01 | 7 << 2 | 7 << 5, 0xFF])
    # copy-2: tag 10 | (len - 1) << 2, then the offset, little-endian
    assert M.copy(2048, 11) == bytes([0x02 | 10 << 2, 0x00, 0x08])
    assert M.copy(2047, 12) == bytes([0x02 | 11 << 2, 0xFF, 0x07])
    assert M.copy(2560, 64) == bytes([0xFE, 0x00, 0x0A])


def _ramp(n):
    return bytes((7 * i + (i >> 8)) & 255 for i in range(n))


@pytest.mark.parametrize("lit", (60, 61, 256, 257))
@pytest.mark.parametrize("mlen", (11, 12, 64, 65, 67, 68, 130))
@pytest.mark.parametrize("offset", (2047, 2048))
def test_worked_sequences(lit, mlen, offset):
    """3000 stored-size-defeating bytes, then `lit` literals, a match and a 5-byte tail"""
    head = _ramp(3000)
    src = bytearray(head + bytes(200 + i % 50 for i in range(lit)))
    start = len(src)
    for i in range(mlen):
        src.append(src[start - offset + i])
    src += b"\x01\x02\x03\x04\x05"
    # (a second, long match, so that the stream beats the stored form)
    src += src[:1500]
    seqs = [(3000 + lit, offset, mlen), (5, len(src) - 1500, 1500)]
    got = M.encode(bytes(src), seqs)
    want = bytearray(M.varint(len(src)))
    want += M.literal(src[:3000 + lit])
    for p in M.pieces(mlen):
        want += M.copy(offset, p)
    want += M.literal(b"\x01\x02\x03\x04\x05")
    for p in M.pieces(1500):
        want += M.copy(len(src) - 1500, p)
    assert got == bytes(want)
    assert M.decode(got, len(src)) == bytes(src)
    assert C.pa_decode(got, len(src)) == bytes(src)
    kinds = [e[0] for e in M.elements(got)]
    first = M.COPY1 if 4 <= M.pieces(mlen)[0] <= 11 and offset < 2048 else M.COPY2
    assert kinds[0] == M.LITERAL and kinds[1] == first


def test_lz4_block_as_sequences():
    src = b"abcdabcdabcdabcdabcdXYZ-tail-bytes"
    r, block = O.lz4_compress(np.frombuffer(src, np.uint8))
    assert r == 0
    seqs = M.lz4_sequences(block)
    assert sum(a + c for a, _, c in seqs) == len(src) and seqs[-1][2] == 0
    s = M.from_lz4_block(src, block)
    assert M.decode(s, len(src)) == src and C.pa_decode(s, len(src)) == src
    assert M.from_lz4_block(b"", b"\x00") == b"\x00" and M.decode(b"\x00", 0) == b""


def test_stored_form_and_the_size_bound():
    for n in (1, 13, 60, 61, 127, 128, 256, 257, 4099, 16383, 16384, 65536):
        src = O.fill(0, n, n).tobytes()
        r, block = O.lz4_compress(np.frombuffer(src, np.uint8))
        s = M.from_lz4_block(src, block)
        assert s == M.stored(src) and len(s) == M.slot_bound(n) <= n + 6
        assert C.pa_decode(s, n) == src
    # the tie goes to the stored form: 2048 literals, a far 4-byte match, one literal, the same
    # match again and a 1-byte tail code to 2063 bytes, and so does the stored form; without the
    # tail the stream is one byte smaller and is kept
    head = _ramp(2048)
    src = head + head[:4] + b"!" + head[5:9] + b"?"
    seqs = [(2048, 2048, 4), (1, 2048, 4), (1, 0, 0)]
    coded = M.varint(2058) + M.literal(head) + M.copy(2048, 4) + M.literal(b"!") + \
        M.copy(2048, 4) + M.literal(b"?")
    assert len(coded) == len(M.stored(src)) == 2063
    assert M.encode(src, seqs) == M.stored(src)
    assert M.encode(src[:-1], seqs[:2]) == M.varint(2057) + coded[2:-2]
    assert M.decode(M.varint(2057) + coded[2:-2], 4096) == src[:-1]


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("kind", KINDS)
def test_pyarrow_decodes_every_model_stream(kind, seg):
    data = O.fill(kind, C.SEED, 4 * seg + 1234)
    streams = C.model_streams(data, seg)
    for part, s in zip(M.segments(data, seg), streams):
        assert len(s) <= part.size + 6
        assert C.pa_decode(s, part.size) == part.tobytes()
        assert M.decode(s, seg) == part.tobytes()
    if kind == 0:
        assert C.census(streams) == {"stored", "literal 2-byte length"}
    elif seg == 65536:
        assert {"literal inline", "copy-1", "copy-2"} <= C.census(streams)


def test_model_decoder_agrees_with_pyarrow_on_the_mutation_corpus():
    corpus = C.mutation_corpus()
    rejects = changed = same = over = 0
    bases = {C.base_stream(k, seg)[0] for k in (1, 5, 6) for seg in (4099, 65536)}
    for stream, cap in corpus:
        mine = M.decode(stream, cap)
        pre = M.preamble(stream)
        if pre is not None and pre[0] > cap:
            # a declared length above the capacity: a reject by the engine's rule (pyarrow
            # would allocate the declared size)
            assert mine is None
            over += 1
            continue
        theirs = C.pa_decode(stream, pre[0]) if pre is not None else C.pa_decode(stream, cap)
        assert mine == theirs, (len(stream), cap, pre)
        if theirs is None:
            rejects += 1
        elif theirs in bases:
            same += 1
        else:
            changed += 1
    print(f"mutation corpus: {rejects} rejects, {changed} accepted with changed output, "
          f"{same} accepted unchanged, {over} preambles above the capacity")
    assert rejects + changed + same + over == 420
    assert rejects >= 105 and changed >= 105


def test_hand_built_streams_model_against_pyarrow():
    for stream, cap, want in C.hand_built():
        assert M.decode(stream, cap) == want, stream[:16].hex()
        pre = M.preamble(stream)
        if pre is not None and pre[0] <= cap:
            assert C.pa_decode(stream, pre[0]) == want, stream[:16].hex()


def test_library_surface():
    import bitar_amd as B
    assert B.CODEC_SNAPPY == 6
    assert B.slot_size(B.CODEC_SNAPPY, 65536) == 65792
    assert B.slot_size(B.CODEC_SNAPPY, 1) == 256 and B.slot_size(B.CODEC_SNAPPY, 250) == 256
    assert B.slot_size(B.CODEC_SNAPPY, 251) == 512
    for seg in (1, 60, 61, 127, 128, 256, 257, 16383, 16384, 65536):
        assert B.slot_size(B.CODEC_SNAPPY, seg) >= M.slot_bound(seg)
    assert B.max_distance(B.CODEC_SNAPPY) == 2560
    assert B.lib().bitar_hip_abi_version() == 3
    for bad in (7, 12, 99):
        assert B.slot_size(bad, 65536) == 0 and B.max_distance(bad) == 0
