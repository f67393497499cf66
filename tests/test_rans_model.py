"""The RANS format on the CPU: the numpy model (rans_model.py) against worked examples done by
hand from the format's rules, the normalisation, every reject and accept rule on its own, round
trips, the sizes against the order-0 entropy, and the library's surface (ids, slots, reach)."""
import numpy as np
import pytest

import rans_cases as C
import rans_model as M

STATES0 = bytes.fromhex("00000100") * 64  # 64 states of 2^16


# ---- worked examples ---------------------------------------------------------------------------

def test_golden_constant_segment():
    """291 zero bytes: one symbol with f = 4096 (f - 1 = 0xFFF, padded to two bytes), no lane
    ever emits (x >> 20 is below 4096) and x = (x div 4096) * 4096 + x mod 4096 + 0 = x"""
    s = M.encode_segment(np.zeros(291, np.uint8))
    assert s == bytes.fromhex("a0002201") + b"\x01" + bytes(31) + b"\xff\x0f" + STATES0
    assert len(s) == 294 and M.decode(s, 291) == bytes(291)
    t = M.encode_segment(np.zeros(290, np.uint8))  # a tie at 294: stored
    assert t == bytes.fromhex("a1002101") + bytes(290)


def test_golden_two_symbols_by_hand():
    """L = 512: 448 x 'a' then 64 x 'b'.  nsym = 2, f = 1 + floor(c * 4094 / 512) = 3583 and 512,
    the deficit 1 to 'a': 3584, 512; cum 0, 3584.  The last step (all 'b') runs first: x = 2^16,
    2^16 div 512 = 128, so x = 128 * 4096 + 0 + 3584 = 527872 in every lane.  Then seven steps of
    'a' with f = 3584: a lane emits when x >= 3584 << 20, which 527872 and its successors never
    reach within seven steps (each step multiplies x by about 8/7)"""
    data = np.array([97] * 448 + [98] * 64, np.uint8)
    f = M.normalise(np.bincount(data, minlength=256))
    assert (f[97], f[98]) == (3584, 512)
    x = 527872
    for _ in range(7):
        assert x < 3584 << 20
        x = (x // 3584) * 4096 + x % 3584
    s = M.rans_form(data)
    bitmap = bytearray(32)
    bitmap[97 >> 3] |= 1 << (97 & 7)
    bitmap[98 >> 3] |= 1 << (98 & 7)
    freqs = (3583 | 511 << 12).to_bytes(4, "little")  # 24 bits, padded to an even size
    assert s == bytes.fromhex("a000ff01") + bytes(bitmap) + freqs + x.to_bytes(4, "little") * 64
    assert M.decode(s, 512) == data.tobytes()
    assert M.encode_segment(data) == s  # 296 bytes against 516


def test_golden_emission_order():
    """L = 128 of one symbol among two: step 1 runs first, step 0 second; with f small enough to
    emit, a step's words are the emitting lanes' low halves in lane order"""
    f = np.zeros(256, np.int64)
    f[0], f[1] = 1, 4095
    data = np.zeros(128, np.uint8)
    words, states = M.encode_words(data, f)
    # step 1: x = 2^16 >= 1 << 20 is false: x = 2^16 * 4096 = 2^28.  Step 0: 2^28 >= 2^20: every
    # lane emits 0, x = 2^12, then x = 2^12 * 4096 = 2^24
    assert words.tolist() == [0] * 64 and states.tolist() == [1 << 24] * 64
    assert M.decode(M.rans_stream(128, f, words, states), 128) == bytes(128)


@pytest.mark.parametrize("L,delta", ((438, 2), (440, 0), (442, -2)))
def test_tie_cases(L, delta):
    data = C.tie_input(L)
    assert len(M.rans_form(data)) - (4 + L) == delta
    s = M.encode_segment(data)
    assert s[0] == (0xA0 if delta < 0 else 0xA1) and len(s) == 4 + L + min(delta, 0)
    assert M.decode(s, L) == data.tobytes()


# ---- normalisation -----------------------------------------------------------------------------

def counts_of(pairs):
    c = np.zeros(256, np.int64)
    for s, n in pairs:
        c[s] = n
    return c


def test_normalisation():
    f = M.normalise(counts_of([(77, 5)]))  # nsym = 1
    assert f[77] == 4096 and f.sum() == 4096
    f = M.normalise(counts_of([(3, 1), (200, 65535)]))  # nsym = 2, one a singleton
    assert (f[3], f[200]) == (1, 4095)
    f = M.normalise(np.r_[np.full(255, 257), 1])  # nsym = 256 (65536 bytes)
    assert f.min() == 1 and f.sum() == 4096 and np.count_nonzero(f) == 256
    f = M.normalise(np.r_[np.full(255, 3), 0])  # nsym = 255
    assert f[255] == 0 and f.sum() == 4096 and f[:255].min() >= 1
    # 127 x 512, one x 384, 128 singletons: "floor, bump zeros, take from the largest" would
    # take 128 - (4096 - 127 * 32 - 24) = 120 from a frequency of 32
    c = np.array([512] * 127 + [384] + [1] * 128)
    f = M.normalise(c)
    assert f.sum() == 4096 and f.min() == 1
    assert f[0] == 1 + 512 * 3840 // 65536 + (4096 - int((1 + c * 3840 // 65536).sum()))
    assert (f[1:127] == 31).all() and f[127] == 23 and (f[128:] == 1).all()
    # a most-frequent tie: the deficit goes to the lowest value
    f = M.normalise(counts_of([(9, 100), (4, 100), (250, 100), (30, 7)]))
    base = 1 + 100 * 4092 // 307
    assert f[9] == base and f[250] == base and f[4] > base and f.sum() == 4096
    rng = np.random.default_rng(5)
    for _ in range(200):  # 0 <= deficit < nsym is asserted inside
        nsym = int(rng.integers(1, 257))
        c = np.zeros(256, np.int64)
        c[rng.permutation(256)[:nsym]] = rng.integers(1, 2000, nsym) ** int(rng.integers(1, 3))
        if c.sum() <= 65536:
            M.normalise(c)


def test_table_layout():
    f = counts_of([(0, 1), (1, 0xABC + 1), (255, 4096 - 1 - 0xABD)])
    t = M.pack_table(f)
    assert t[:32] == b"\x03" + bytes(30) + b"\x80"
    v = 0 | 0xABC << 12 | (4096 - 2 - 0xABD) << 24
    assert t[32:] == v.to_bytes(6, "little") and M.table_size(3) == 6
    assert [M.table_size(n) for n in (1, 2, 4, 5, 255, 256)] == [2, 4, 6, 8, 384, 384]


# ---- the decoder's rules, each alone -------------------------------------------------------------

def example():
    data = C.alphabet(1500, 5, 1)
    s = M.encode_segment(data)
    assert s[0] == 0xA0 and C.parts_of(s)[0] == 5 and C.parts_of(s)[2] > 64
    return s, data.tobytes()


def poke(s, at, value):
    t = bytearray(s)
    t[at] = value & 255
    return bytes(t)


def test_decode_rejects_the_tag_and_byte_one():
    s, data = example()
    for nib in range(16):
        assert (M.decode(poke(s, 0, nib << 4), 4096) == data) == (nib == 0xA)
    for mode in range(2, 16):
        assert M.decode(poke(s, 0, 0xA0 | mode), 4096) is None
    for b1 in range(1, 256):
        assert M.decode(poke(s, 1, b1), 4096) is None
    stored = M.encode_segment(C.rnd(500, 1))
    assert stored[0] == 0xA1 and M.decode(poke(stored, 1, 1), 4096) is None


def test_decode_rejects_length_above_the_segment():
    s, data = example()
    assert M.decode(s, len(data)) == data
    assert M.decode(s, len(data) - 1) is None
    stored = M.encode_segment(C.rnd(500, 1))
    assert M.decode(stored, 500) is not None and M.decode(stored, 499) is None


def test_decode_rejects_sizes():
    s, data = example()
    for t in (s + b"\0", s[:-1], s[:-3], s[:3], b"", s[:293], s[:292]):
        assert M.decode(t, 4096) is None  # odd 2 * nw, a negative one, too short
    assert M.decode(s + b"\0\0", 4096) is None and M.decode(s[:-2], 4096) is None  # nw +- 1
    stored = M.encode_segment(C.rnd(500, 1))
    for t in (stored + b"\0", stored[:-1], stored[:4]):
        assert M.decode(t, 4096) is None
    # a rans form of fewer than 36 + 2 + 256 bytes: nothing fits in it
    one = M.rans_form(np.zeros(10, np.uint8))
    assert len(one) == 294 and M.decode(one, 10) == bytes(10)
    assert M.decode(one[:293], 10) is None and M.decode(one[:36] + one[38:], 10) is None


def test_decode_rejects_tables():
    s, data = example()
    assert M.decode(s[:4] + bytes(32) + s[36:], 4096) is None  # an empty bitmap
    f = C.frequencies_of(s)
    present = np.flatnonzero(f)
    for d in (1, -1):  # the sum is 4097 and 4095
        g = f.copy()
        g[present[0]] += d
        assert M.decode(s[:4] + M.pack_table(g) + s[36 + 8:], 4096) is None
    nsym, tsize, _ = C.parts_of(s)  # 5 symbols: 60 bits in 8 bytes, 4 pad bits
    assert (nsym, tsize) == (5, 8)
    for bit in range(4, 8):
        assert M.decode(poke(s, 36 + 7, s[36 + 7] | 1 << bit), 4096) is None
    # one bit more in the bitmap: a sixth symbol, the table is read differently
    absent = int(np.flatnonzero(f == 0)[0])
    assert M.decode(poke(s, 4 + (absent >> 3), s[4 + (absent >> 3)] | 1 << (absent & 7)), 4096) is None


def test_decode_rejects_states_and_words():
    s, data = example()
    nsym, tsize, nw = C.parts_of(s)
    at = 36 + tsize + 2 * nw
    for lane in (0, 17, 63):  # an initial state below 2^16
        t = s[:at + 4 * lane] + (0xFFFF).to_bytes(4, "little") + s[at + 4 * lane + 4:]
        assert M.decode(t, 4096) is None
    body = s[36 + tsize:at]
    for k in (0, nw // 2, nw - 1):  # a word less: some refill finds none left; a word more: p != 0
        assert M.decode(s[:36 + tsize] + body[:2 * k] + body[2 * k + 2:] + s[at:], 4096) is None
        assert M.decode(s[:36 + tsize] + body[:2 * k] + b"\1\2" + body[2 * k:] + s[at:], 4096) is None
    # an altered word or state: the decoder does not land on 2^16
    assert M.decode(poke(s, 36 + tsize, s[36 + tsize] ^ 1), 4096) is None
    assert M.decode(poke(s, at + 2, s[at + 2] ^ 1), 4096) is None
    # no words at all although the states need some
    assert M.decode(s[:36 + tsize] + s[at:], 4096) is None


def test_decode_accepts_non_canonical_streams():
    s, data = example()
    f = C.frequencies_of(s)
    present = np.flatnonzero(f)
    g = f.copy()  # any table that sums to 4096
    g[present[0]] += 5
    g[present[1]] -= 5
    arr = np.frombuffer(data, np.uint8)
    t = M.rans_stream(arr.size, g, *M.encode_words(arr, g))
    assert t != s and M.decode(t, 4096) == data
    h = np.full(256, 16, np.int64)  # a table with symbols the segment does not have
    t = M.rans_stream(arr.size, h, *M.encode_words(arr, h))
    assert M.decode(t, 4096) == data
    noise = C.rnd(300, 3)  # a rans form larger than 4 + L
    t = M.rans_form(noise)
    assert len(t) > 304 and M.decode(t, 300) == noise.tobytes()
    assert M.encode_segment(noise)[0] == 0xA1


def test_every_mutant_has_a_verdict():
    """the corpus of the GPU test: the model neither raises nor accepts a damaged stream with the
    original's bytes unless the stream says the same"""
    s, data = example()
    muts = C.mutants(s)
    assert len(muts) > 400
    verdicts = [M.decode(t[:size] if size <= len(t) else t + b"\x5a" * (size - len(t)), 4096)
                for t, size in muts]
    assert verdicts[0] == data
    assert sum(v is None for v in verdicts) > 400 and sum(v is not None for v in verdicts) >= 3


# ---- round trips and sizes -----------------------------------------------------------------------

@pytest.mark.parametrize("seg", (65536, 59460, 4096, 1000, 999, 72, 7, 1))
def test_round_trips(seg):
    for tail in (0, 1, 63, 64, 65):
        data = C.mixed(3 * seg + tail, seg + tail)
        streams = M.encode(data, seg)
        assert len(streams) == (data.size + seg - 1) // seg
        for i, s in enumerate(streams):
            part = data[i * seg:(i + 1) * seg]
            assert len(s) <= 4 + part.size and (s[0] == 0xA1) == (len(s) == 4 + part.size)
            assert M.decode(s, seg) == part.tobytes()


@pytest.mark.parametrize("L", (63, 64, 65, 127, 128, 129, 1087, 1088, 1089))
@pytest.mark.parametrize("nsym", (1, 2, 16, 255, 256))
def test_round_trips_of_the_coder_alone(L, nsym):
    data = C.alphabet(L, nsym, L + nsym)
    s = M.rans_form(data)
    assert len(s) % 2 == 0 and M.decode(s, L) == data.tobytes()


def test_sizes_against_the_entropy():
    """64 KiB segments of the inputs of DESIGN 4.25's table: within 1.5 % + 300 bytes of the
    order-0 entropy"""
    rng = np.random.default_rng(11)
    inputs = {
        "text": M.text_like(rng, 65536),
        "walk": C.smooth_walk_shuffled(65536, 1),
        "normal": C.normal_shuffled(65536, 2),
        "two symbols": C.two_symbols(65536, 3),
        "constant": np.full(65536, 65, np.uint8),
    }
    for name, data in inputs.items():
        s = M.encode_segment(data)
        h = M.entropy_bytes(data)
        assert s[0] == 0xA0, name
        assert len(s) <= 1.015 * h + 300, (name, len(s), h)
        assert M.decode(s, 65536) == data.tobytes()
    assert len(M.encode_segment(inputs["constant"])) == 294  # ratio 223
    noise = C.rnd(65536, 4)
    assert len(M.encode_segment(noise)) == 65540 and len(M.rans_form(noise)) > 66000


# ---- the library's surface -----------------------------------------------------------------------

def test_library_surface():
    import bitar_amd as B
    import test_abi
    assert B.CODEC_RANS == 72
    assert tuple(B.slot_size(B.CODEC_RANS, seg) for seg in test_abi.SLOT_SEGS) == \
        (256, 256, 4352, 59648, 65792)
    assert B.max_distance(B.CODEC_RANS) == 0
    for unknown in (68, 71, 73, 99):
        assert B.slot_size(unknown, 100) == 0 and B.max_distance(unknown) == 0


def test_abi_is_untouched():
    import bitar_amd as B
    import test_abi
    assert B.lib().bitar_hip_abi_version() == 3
    assert sorted(B.ABI_SYMBOLS) == test_abi.header_symbols() and len(B.ABI_SYMBOLS) == 39
    assert not [s for s in B.ABI_SYMBOLS if "rans" in s]
