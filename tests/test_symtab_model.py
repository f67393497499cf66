"""The SYMTAB format on the CPU: the Python model (symtab_model.py) against streams worked by hand
from the format's and the encoder's rules, the tie at 4 + L, every reject and accept rule on its
own, round trips, the slot rule, the threshold tie, the sample switch, the sizes against the
oracle's LZ4, and the library's surface (ids, slots, reach)."""
import numpy as np
import pytest

import symtab_cases as C
import symtab_model as M


def u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


# ---- worked examples ---------------------------------------------------------------------------

def test_golden_pair_promoted_across_generations():
    """b"abababab": the tables of the five generations as the docstring derives them"""
    assert M.slot_of(0x61 * 512 + 0x62) == 2487 and M.slot_of(0x62 * 512 + 0x61) == 1731
    want = ([b"a", b"b", b"ba", b"ab"], [b"ab", b"abab"], [b"abab", b"abababab"], [b"abababab"],
            [b"abababab"])
    for g, table in enumerate(want, 1):
        assert M.build_table(b"abababab", g) == table
        assert M.build_table(b"ab" * 64, g) == table
    assert M.coded_form(u8(b"abababab")) == bytes.fromhex("c0010700010008") + b"abababab" + b"\0"
    assert M.encode_segment(u8(b"abababab")) == bytes.fromhex("c1000700") + b"abababab"
    s = M.encode_segment(u8(b"ab" * 64))
    assert s == bytes.fromhex("c0017f00100008") + b"abababab" + bytes(16) and len(s) == 31
    assert M.decode(s, 128) == b"ab" * 64


def test_golden_escape_of_0xff():
    a = np.full(16390, 0x61, np.uint8)
    a[300] = 0xFF
    want = ([b"a", b"aa"], [b"aa", b"aaaa"], [b"aa", b"aaaa", b"a" * 8, b"a" * 6],
            [b"a" * 8, b"a" * 6], [b"a" * 8, b"a" * 6])
    for g, table in enumerate(want, 1):
        assert M.build_table(a.tobytes(), g) == table
    s = M.encode_segment(a)
    assert s == bytes.fromhex("c0020540" "0608" "0806") + b"a" * 14 + \
        bytes(37) + b"\xff" * 5 + bytes(2011) + b"\xff" + bytes.fromhex("61616161ff61")
    assert len(s) == 2082 and M.decode(s, 65536) == a.tobytes()
    # the same byte inside the sample is a symbol, not an escape
    a[300], a[1024 + 44] = 0x61, 0xFF
    lens, syms, codes, lits = M.parts_of(M.encode_segment(a))
    assert any(0xFF in s for s in syms) and 0xFF not in lits


def test_tie_at_4_plus_L():
    """b"abc" * k to 32 bytes: the coded form is one byte over; 17 a's: one byte under; the stream
    built by hand at exactly 4 + L is not what the encoder takes"""
    d = u8((b"abc" * 11)[:32])
    assert len(M.coded_form(d)) == 4 + 32 + 1 and M.encode_segment(d)[0] == 0xC1
    d = u8(b"a" * 17)
    s = M.coded_form(d)
    assert s == bytes.fromhex("c002100003000108") + b"a" * 9 + bytes.fromhex("010100")
    assert len(s) == 4 + 17 - 1 and M.encode_segment(d) == s
    # equal sizes: stored.  57 bytes of abcde: six symbols of 35 bytes, 8 codes, 61 = 4 + 57
    d = u8((b"abcde" * 12)[:57])
    s = M.coded_form(d)
    assert len(s) == 4 + 57 and s[1] == 6 and (s[4] | s[5] << 8) == 8 and M.decode(s, 57) == d.tobytes()
    assert M.encode_segment(d) == bytes.fromhex("c1003800") + d.tobytes()
    # (a stream of exactly 4 + L built by hand decodes all the same)
    tie = M.coded_stream(14, [b"xyxy", b"xy"], [0, 0, 0, 1], b"")
    assert len(tie) == 4 + 14 and M.decode(tie, 14) == b"xy" * 7


# ---- the decoder's rules, each alone ---------------------------------------------------------------

GOOD = M.coded_stream(12, [b"ab", b"cde"], [0, 1, 255, 0, 1, 255], b"xy")


def test_good_stream():
    assert GOOD == bytes.fromhex("c0020b00" "0600" "0203") + b"abcde" + bytes([0, 1, 255, 0, 1, 255]) + b"xy"
    assert len(GOOD) == 6 + 2 + 5 + 6 + 2 and M.decode(GOOD, 12) == b"abcdexabcdey"
    assert M.decode(GOOD, 4096) == b"abcdexabcdey"


def put(s, at, *vals):
    m = bytearray(s)
    m[at:at + len(vals)] = bytes(vals)
    return bytes(m)


def test_decode_rejects_the_tag_and_mode():
    for tag in (0x00, 0xA0, 0xB0, 0xD0, 0x0C, 0xC2, 0xC3, 0xCF):
        assert M.decode(put(GOOD, 0, tag), 4096) is None
    stored = bytes.fromhex("c1000200") + b"xyz"
    assert M.decode(stored, 3) == b"xyz"
    assert M.decode(put(stored, 0, 0xC0), 3) is None and M.decode(put(stored, 0, 0xD1), 3) is None


def test_decode_rejects_byte_one_of_a_stored_stream():
    stored = bytes.fromhex("c1000200") + b"xyz"
    for v in (1, 3, 255):
        assert M.decode(put(stored, 1, v), 3) is None


def test_decode_rejects_length_above_the_segment():
    assert M.decode(GOOD, 12) is not None and M.decode(GOOD, 11) is None
    stored = bytes.fromhex("c1000200") + b"xyz"
    assert M.decode(stored, 2) is None


def test_decode_rejects_no_symbols_and_no_codes():
    assert M.decode(put(GOOD, 1, 0), 4096) is None
    assert M.decode(put(GOOD, 4, 0, 0), 4096) is None
    # (not even for the sizes that would fit: nsym = 0 with one escape code)
    s = bytes.fromhex("c0000000" "0100") + b"\xff" + b"q"
    assert M.decode(s, 4096) is None
    assert M.decode(put(s, 1, 1)[:6] + b"\x01" + b"z" + b"\xff" + b"q", 4096) == b"q"


def test_decode_rejects_lengths():
    for v in (0, 9, 255):
        assert M.decode(put(GOOD, 6, v), 4096) is None
        assert M.decode(put(GOOD, 7, v), 4096) is None


def test_decode_rejects_codes_out_of_range():
    for v in (2, 3, 128, 254):
        assert M.decode(put(GOOD, 13, v), 4096) is None
    assert M.decode(put(GOOD, 13, 1), 4096) is None  # (in range, but the lengths no longer sum)


def test_decode_rejects_sizes():
    assert M.decode(GOOD[:-1], 4096) is None and M.decode(GOOD + b"z", 4096) is None
    for k in range(len(GOOD)):
        assert M.decode(GOOD[:k], 4096) is None
    # nc off by one with the size unchanged, a 255 added without its literal and one removed
    assert M.decode(put(GOOD, 4, 5), 4096) is None and M.decode(put(GOOD, 4, 7), 4096) is None
    assert M.decode(put(GOOD, 13, 255), 4096) is None
    assert M.decode(put(GOOD, 15, 0), 4096) is None


def test_decode_rejects_lengths_that_do_not_sum_to_L():
    assert M.decode(put(GOOD, 2, 12), 4096) is None and M.decode(put(GOOD, 2, 10), 4096) is None
    assert M.decode(put(GOOD, 13, 1), 4096) is None
    # the right sum by other codes is accepted
    s = M.coded_stream(13, [b"ab", b"cde"], [0, 1, 255, 0, 1, 255], b"xy")
    assert M.decode(s, 4096) is None  # (12 bytes decoded, 13 named)
    s = M.coded_stream(12, [b"ab", b"cde"], [1, 1, 1, 1], b"")
    assert M.decode(s, 4096) == b"cde" * 4


def test_decode_accepts_streams_no_encoder_writes():
    # duplicate symbols, a symbol no code uses, symbols out of any order, a stream above 4 + L
    s = M.coded_stream(4, [b"ab", b"ab", b"zzzzzzzz"], [0, 1], b"")
    assert M.decode(s, 4) == b"abab" and len(s) > 8
    # 255 symbols, code 254 the last of them, and an escape beside it
    table = [bytes([i]) for i in range(255)]
    s = M.coded_stream(3, table, [254, 255, 0], b"\xfe")
    assert M.decode(s, 3) == b"\xfe\xfe\x00"
    # escapes alone
    s = M.coded_stream(3, [b"q"], [255, 255, 255], b"abc")
    assert M.decode(s, 3) == b"abc"
    # an 8-byte symbol with zero bytes
    s = M.coded_stream(16, [bytes(8)], [0, 0], b"")
    assert M.decode(s, 16) == bytes(16)


def test_every_mutant_has_a_verdict():
    for data in (C.text(4096, 1), C.all_bytes(4000, 2), C.rnd(300, 3)):
        base = M.coded_form(data)
        muts = C.mutants(base)
        verdicts = [M.decode(t[:n], 4096) for t, n in muts]
        assert verdicts[0] == data.tobytes()
        assert 0.5 < sum(v is None for v in verdicts) / len(muts) < 1
        assert len({v for v in verdicts if v is not None}) > 1
        for (t, n), v in zip(muts, verdicts):
            L = 1 + t[2] + (t[3] << 8) if n >= 4 else 0
            assert v is None or len(v) == L


# ---- round trips -------------------------------------------------------------------------------

@pytest.mark.parametrize("seg", (65536, 20000, 4096, 1000, 257, 256, 255, 9, 8, 7, 1))
def test_round_trips(seg):
    n = min(3 * seg + 17, 70000)
    for data in (C.text(n, seg), C.names(n, seg), C.mixed(n, seg), C.all_bytes(n, seg),
                 C.alphabet64(n, seg), C.symbol_at_ends(min(n, seg)), np.full(n, 7, np.uint8)):
        streams = M.encode(data, seg)
        assert len(streams) == (data.size + seg - 1) // seg
        back = b"".join(M.decode(s, seg) for s in streams)
        assert back == data.tobytes()
        for i, s in enumerate(streams):
            L = min(seg, data.size - i * seg)
            assert len(s) <= 4 + L and (s[0] == 0xC1) == (len(s) == 4 + L)


def test_noise_is_stored():
    data = C.rnd(2 * 65536, 1)
    streams = M.encode(data, 65536)
    assert [len(s) for s in streams] == [65540, 65540] and all(s[0] == 0xC1 for s in streams)
    assert M.coded_form(data[:65536]) is None  # (more than 65535 codes)
    assert len(M.coded_form(data[:60000])) > 60004


# ---- the encoder's rules -----------------------------------------------------------------------

def test_the_smallest_key_of_a_slot_is_counted_alone():
    data, groups = C.collide()
    c1, slots = M.count_generation(data.tobytes(), M.sample_chunks(data.size), [])
    assert len(groups) == 8
    for group in groups:
        keys = sorted(a * 512 + b for a, b in group)
        assert len(keys) >= 2 and len({M.slot_of(k) for k in keys}) == 1
        key, count, n = slots[M.slot_of(keys[0])]
        assert key == keys[0] and n == 2 and count > 16
        # the pair of the larger key is seen as often and is no candidate of this generation
        loser = bytes([keys[1] >> 9, keys[1] & 511])
        assert data.tobytes().count(loser) > 16
        assert loser not in [s for _, _, s in M.candidates(c1, slots, [])]
    # ... and the next generation's table holds the winners' strings only
    table = M.build_table(data.tobytes(), 1)
    for group in groups:
        keys = sorted(a * 512 + b for a, b in group)
        assert bytes([keys[0] >> 9, keys[0] & 511]) in table
        assert bytes([keys[1] >> 9, keys[1] & 511]) not in table


def test_the_threshold_tie_goes_by_index():
    data = C.equal_gains(8192)
    c1, slots = M.count_generation(data.tobytes(), M.sample_chunks(data.size), [])
    cands = M.candidates(c1, slots, [])
    # 32 of every byte, 16 of every pair of two bytes: one gain (but for the pairs that lost
    # their slot to a smaller key, which are no candidates)
    assert {g for _, g, _ in cands} == {32} and 700 < len(cands) <= 766
    taken = M.select(cands)
    assert [c[0] for c in taken] == list(range(255))
    assert M.build_table(data.tobytes(), 1) == [bytes([i]) for i in range(255)]
    # all gains equal: the first 255 by index
    flat = [(i, 5, b"x") for i in range(0, 600, 2)]
    assert M.select(flat) == flat[:255]
    assert M.select(flat[:255]) == flat[:255] and M.select(flat[:7]) == flat[:7]
    # one above the rest
    assert M.select(flat + [(700, 6, b"y")]) == flat[:254] + [(700, 6, b"y")]


def test_both_sides_of_the_sample_switch():
    assert len(M.sample_chunks(16384)) == 64 and M.sample_chunks(16384)[1] == (256, 512)
    assert len(M.sample_chunks(16385)) == 17 and M.sample_chunks(16385)[1] == (1024, 1280)
    assert M.sample_chunks(16385)[-1] == (16384, 16385)
    assert len(M.sample_chunks(65536)) == 64 and M.sample_chunks(65536)[-1] == (64512, 64768)
    assert M.sample_chunks(1) == [(0, 1)] and M.sample_chunks(257) == [(0, 256), (256, 257)]
    # a word in chunk 1 alone: in the table at 16384 bytes, escaped at 16385
    a = np.full(16385, 0x2E, np.uint8)
    a[300:308] = np.frombuffer(b"ABCDEFGH", np.uint8)
    lens, syms, codes, lits = M.parts_of(M.encode_segment(a[:16384]))
    assert any(b"ABCD" in s for s in syms) and any(b"EFGH" in s for s in syms) and lits == b""
    lens, syms, codes, lits = M.parts_of(M.encode_segment(a))
    assert lits == b"ABCDEFGH" and all(set(s) == {0x2E} for s in syms)


def test_nothing_pairs_across_a_chunk():
    """'xy' astride the chunks 0 and 1 only: no symbol xy"""
    a = np.full(1024, 0x2E, np.uint8)
    a[255], a[256] = ord("x"), ord("y")
    table = M.build_table(a.tobytes())
    assert b"xy" not in table and not any(b"xy" in s for s in table)
    a[100], a[101] = ord("x"), ord("y")
    assert any(b"xy" in s for s in M.build_table(a.tobytes()))


# ---- sizes ---------------------------------------------------------------------------------------

def test_sizes_against_the_oracle_lz4():
    import oracle_lib as O
    seg = 65536
    log = O.fill(6, 1, 4 * seg)
    names = C.names(4 * seg)
    want = {"log": [16707, 17153, 16012, 17129], "names": [31568, 30907, 31490, 32087]}
    for name, data in (("log", log), ("names", names)):
        sizes = [len(s) for s in M.encode(data, seg)]
        lz4 = sum(len(O.lz4_compress(data[o:o + seg])[1]) for o in range(0, data.size, seg))
        assert sizes == want[name]
        assert sum(sizes) < lz4, (name, sum(sizes), lz4)
    # the ratios the table of DESIGN.md 4.27 quotes: 3.91 and 2.08
    assert round(4 * seg / sum(want["log"]), 2) == 3.91
    assert round(4 * seg / sum(want["names"]), 2) == 2.08
    assert [len(s) for s in M.encode(C.rnd(seg + 100, 9), seg)] == [4 + seg, 104]


# ---- the library's surface -----------------------------------------------------------------------

def test_library_surface():
    import bitar_amd as B
    import test_abi
    assert B.CODEC_SYMTAB == 88
    assert tuple(B.slot_size(B.CODEC_SYMTAB, seg) for seg in test_abi.SLOT_SEGS) == \
        (256, 256, 4352, 59648, 65792)
    assert B.max_distance(B.CODEC_SYMTAB) == 0
    for unknown in (84, 85, 86, 87, 89, 90, 99):
        assert B.slot_size(unknown, 100) == 0 and B.max_distance(unknown) == 0


def test_abi_is_untouched():
    import bitar_amd as B
    import test_abi
    assert B.lib().bitar_hip_abi_version() == 3
    assert sorted(B.ABI_SYMBOLS) == test_abi.header_symbols() and len(B.ABI_SYMBOLS) == 39
    assert not [s for s in B.ABI_SYMBOLS if "symtab" in s]
