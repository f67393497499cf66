"""The linked-block LZ4 model and its corpus (lz4_linked_model.py) against liblz4: every case
is wrapped in a real linked-block frame and decoded by LZ4F_decompress.  What the model
accepts liblz4 decodes to the same bytes, what it rejects for a reason a frame can express
liblz4 rejects, and the only differences are the lenient ones of M.DIVERGENCES.  The corpus
holds every class of M.CLASSES, read back from the blocks of its cases.  No device."""
import pytest

import lz4_linked_model as M

# reasons a frame cannot express: the table and the capacity are the caller's, not the frame's
NOT_IN_A_FRAME = ("entry_past_src", "entry_wraps", "cap_literals", "cap_match", "cap_stored")


@pytest.fixture(scope="module")
def corpus():
    return M.cases()


def test_xxh32_and_the_writers():
    assert M.xxh32(b"") == 0x02CC5D05 and M.xxh32(b"abc") == 0x32D153FF
    assert M.xxh32(bytes(range(100))) == M.xxh32(bytearray(range(100)))
    assert M.xxh32(b"abc", 1) != M.xxh32(b"abc")
    # token: 3 literals, match of 4 + 5; offset little-endian; the closing run
    assert M.emit_block([(b"abc", 0x0102, 9)], b"xy") == b"\x35abc\x02\x01\x20xy"
    assert M.emit_block([], b"") == b"\x00"
    assert M.emit_block([(b"", 1, 4)], None) == b"\x00\x01\x00"
    blk = M.emit_block([(b"a" * 15, 7, 19), (b"b" * 270, 7, 19 + 255)], b"c" * 14)
    assert M.walk_block(blk) == ([(15, 7, 19, 0, 0), (270, 7, 274, 1, 1)], (14, 0))
    # a frame liblz4 reads, with every optional field
    blocks = [(M.emit_block([(b"hello ", 6, 30)], b"world"), False), (b"stored", True)]
    plain = b"hello " * 6 + b"world" + b"stored"
    for linked in (True, False):
        f = M.frame(blocks, linked=linked, block_checksum=True, content_size=len(plain),
                    content_checksum=True)
        assert M.lz4f_decompress(f) == plain
    assert M.lz4f_decompress(M.frame(blocks, content_checksum=M.xxh32(plain) ^ 1)) is None
    assert M.lz4f_decompress(M.frame(blocks)[:-1]) is None


def test_the_decoder_on_hand_counted_streams():
    src, table = M.layout([(b"\x35abc\x02\x00\x20xy", False), (b"\x0f\x02\x00\x00\x00", False)])
    # abc, 9 bytes at offset 2 (overlapping: bcbcbcbcb), xy; then 19 bytes at offset 2 (xyxy...)
    want = b"abc" + b"bcbcbcbcb" + b"xy" + b"xy" * 9 + b"x"
    assert M.decode(src, table, len(want)) == want
    assert M.decode(src, table, len(want) - 1) is None
    assert M.decode_why(src, table[1:], 100) == (None, "offset_past_produced_first_block")
    assert M.decode(src, [(0, 3 | M.STORED)], 3) == src[:3]
    assert M.decode(src, [], 0) == b""
    assert M.decode_why(src, [(len(src) - 1, 2 | M.STORED)], 9) == (None, "entry_past_src")


def test_verdicts_of_the_corpus_are_what_their_names_say(corpus):
    names = [c.name for c in corpus]
    assert len(set(names)) == len(names)
    for c in corpus:
        rejected = c.name.startswith("rej_") or c.name.startswith("cap_short")
        assert (c.expected is None) == rejected, c.name
        assert c.expected == M.decode(c.src, c.table, c.cap), c.name
        assert c.cap < (1 << 19) and (c.expected is None or len(c.expected) < (1 << 19)), c.name
        assert c.diverges is None or c.diverges in M.DIVERGENCES, c.name


def test_liblz4_agrees_on_every_case_a_frame_can_express(corpus):
    hit, framed = set(), 0
    for c in corpus:
        blocks = M.blocks_of(c.src, c.table)
        if c.expected is not None:
            assert blocks is not None, c.name
            got = M.lz4f_decompress(M.frame(blocks, linked=True))
            if c.diverges:  # model accepts, liblz4 rejects
                assert got is None, c.name
                hit.add(c.diverges)
            else:
                assert got == c.expected, c.name
            framed += 1
            continue
        why = M.decode_why(c.src, c.table, c.cap)[1]
        if why in NOT_IN_A_FRAME:
            if why.startswith("cap_"):  # with room, the same bytes; they do not fit cap
                full = M.decode(c.src, c.table, 1 << 31)
                assert len(full) > c.cap, c.name
                got = M.lz4f_decompress(M.frame(blocks, linked=True))
                assert got in (full, None), c.name
                assert got == full or "match" in c.name, c.name  # (the end margins again)
            continue
        assert blocks is not None, c.name
        if why in M.FORMAT_ERRORS_OLD_LIBLZ4_TAKES:
            continue
        assert M.lz4f_decompress(M.frame(blocks, linked=True)) is None, (c.name, why)
        framed += 1
    # every divergence is of the allowed kind and is hit; nothing the model rejects is
    # accepted by liblz4 (asserted case by case above)
    assert hit == set(M.DIVERGENCES)
    assert framed > 150


def test_corpus_holds_every_class(corpus):
    have = set()
    for c in corpus:
        tags = M.describe(c)
        if c.diverges == "block_over_64k":
            assert "block_over_64k" in tags, c.name
        elif c.expected is not None:
            assert "block_over_64k" not in tags, c.name
        have |= tags
    missing = [k for k in M.CLASSES if k not in have]
    assert not missing, missing


def test_constants_are_the_default_build_of_the_ring():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "bitar_amd", "csrc", "stream_ring.hip.h")) as f:
        text = f.read()
    assert int(re.search(r"#define BITAR_DEC_RING (\d+)", text).group(1)) == M.RING
    assert int(re.search(r"#define BITAR_DEC_WIN (\d+)", text).group(1)) == M.WIN
    assert int(re.search(r"kLongLit = (\d+);", text).group(1)) == M.LONG_LIT
    assert "kFlushAt = kRing / 2;" in text and M.FLUSH_AT == 2048
    assert "kNearOff = kRing - 2 * kWave - 16;" in text and M.NEAR == 3952 and M.WAVE == 64
    assert M.FORMAT_ERRORS_OLD_LIBLZ4_TAKES == ("offset_0",)


def test_cases_stay_small(corpus):
    total = sum(len(c.src) + c.cap for c in corpus)
    assert total < 24 << 20, total
