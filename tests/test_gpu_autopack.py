"""GPU tests of AUTOPACK (csrc/autopack.hip and the dispatch in csrc/runtime.hip) through the C
ABI: the slots and sizes of a compress equal the numpy model's streams (autopack_model.py) byte
for byte -- the smallest candidate's, the earlier one's at a tie -- the decoder returns the input,
and on mutated streams its verdict is the model's, with canaries around every buffer a call
writes.

Candidate 0 (RUNPACK) writes its stream into the slot before the winner is copied over it, so
inside a slot the canary is checked past the larger of the two streams.

Shapes: segments of 65536, 59460 (the reference's segment), 4096, 1000 (odd base for the wide
elements), 72 and 7; inputs of one segment per kind (runs, narrow integers, few wide values,
decimal floats, random bytes: autopack_cases.py), so that each applicable format wins a segment;
the ties the model test holds; 70 000 small segments, which crosses the chunk borders of both
directions."""
import numpy as np
import pytest

import autopack_cases as C
import autopack_model as M
import runpack_model as RM

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEGS = (65536, 59460, 4096, 1000, 72, 7)
CANARY = 0xA5
CANARY32 = np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]
PAD = 256
ERR = np.array([0xFFFFFFFF], np.uint32).view(np.int32)[0]


@pytest.fixture(scope="module")
def eng():
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0)
    yield e
    e.close()


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


class Buffers:
    """device buffers of one compress + decompress with canaries on both sides of each"""

    def __init__(self, nseg, stride, seg):
        self.nseg, self.stride, self.seg = nseg, stride, seg
        self.slab = torch.full((PAD + nseg * stride + PAD,), CANARY, dtype=torch.uint8,
                               device="cuda")
        self.sizes = torch.full((nseg + 16,), int(CANARY32), dtype=torch.int32, device="cuda")
        self.out = torch.full((PAD + nseg * seg + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        self.prod = torch.full((nseg + 16,), int(CANARY32), dtype=torch.int32, device="cuda")

    slab_ptr = property(lambda self: self.slab.data_ptr() + PAD)
    sizes_ptr = property(lambda self: self.sizes.data_ptr() + 32)
    out_ptr = property(lambda self: self.out.data_ptr() + PAD)
    prod_ptr = property(lambda self: self.prod.data_ptr() + 32)

    def check_streams(self, streams, first):
        """slots and sizes against the model's streams; past the larger of a segment's stream
        and candidate 0's (`first`) the slot is still the canary"""
        sizes = self.sizes.cpu().numpy()
        assert np.all(sizes[:8] == CANARY32) and np.all(sizes[8 + self.nseg:] == CANARY32)
        got = sizes[8:8 + self.nseg].view(np.uint32)
        assert got.tolist() == [len(s) for s in streams]
        slab = self.slab.cpu().numpy()
        assert np.all(slab[:PAD] == CANARY) and np.all(slab[-PAD:] == CANARY)
        for i, s in enumerate(streams):
            slot = slab[PAD + i * self.stride:PAD + (i + 1) * self.stride]
            want = np.frombuffer(s, np.uint8)
            assert np.array_equal(slot[:want.size], want), \
                (i, s[0], np.flatnonzero(slot[:want.size] != want)[:8].tolist())
            assert np.all(slot[max(want.size, len(first[i])):] == CANARY), i

    def check_output(self, data):
        n = data.size
        prod = self.prod.cpu().numpy()
        assert np.all(prod[:8] == CANARY32) and np.all(prod[8 + self.nseg:] == CANARY32)
        want = [min(self.seg, n - i * self.seg) for i in range(self.nseg)]
        assert prod[8:8 + self.nseg].tolist() == want
        out = self.out.cpu().numpy()
        assert np.all(out[:PAD] == CANARY) and np.all(out[PAD + n:] == CANARY)
        assert np.array_equal(out[PAD:PAD + n], data), np.flatnonzero(out[PAD:PAD + n] != data)[:8]


def check_case(eng, w, seg, data, in_off=0):
    import bitar_amd as B
    codec = B.codec_autopack(w)
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec, seg)
    src = torch.zeros(in_off + n + PAD, dtype=torch.uint8, device="cuda")
    src[in_off:in_off + n] = dev(data)
    buf = Buffers(nseg, stride, seg)
    eng.compress_into(codec, src.data_ptr() + in_off, seg, buf.slab_ptr, stride, buf.sizes_ptr, n=n)
    eng.decompress_slab_into(codec, buf.slab_ptr, stride, buf.sizes_ptr, nseg, seg, buf.out_ptr,
                             buf.prod_ptr, capacity=nseg * seg)
    eng.sync()
    streams = M.encode(data, w, seg)
    buf.check_streams(streams, RM.encode(data, w, seg))
    buf.check_output(data)
    return streams


# ---- exact bytes and round trip -------------------------------------------------------------------

@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("w", M.WIDTHS)
def test_exact_bytes_and_round_trip(eng, w, seg):
    data = C.stretches(w, seg)
    # the model first: every applicable format wins a segment, and one is stored
    kinds = set(C.formats(M.encode(data, w, seg)))
    if seg > 72:
        assert kinds == set(M.CANDIDATES[w]) | {"stored"}
    check_case(eng, w, seg, data)
    if seg == 72:
        for n in range(1, w):  # shorter than an element
            check_case(eng, w, seg, rnd(n, n))


@pytest.mark.parametrize("knob", ("BITAR_HIP_AUTOPACK_LISTS", "BITAR_HIP_AUTOPACK_STORELESS"))
@pytest.mark.parametrize("w", M.WIDTHS)
def test_knobs_off_give_the_same_bytes(eng, w, knob, monkeypatch):
    """the tag-peek decoders (LISTS=0) and the later candidates' storing kernels (STORELESS=0):
    the library reads either variable at every call"""
    monkeypatch.setenv(knob, "0")
    for seg in (4096, 72):
        check_case(eng, w, seg, C.stretches(w, seg))


def test_ties_go_to_the_earlier_candidate(eng):
    a = np.full(129, 0xAB, np.uint8)          # w = 1: RUNPACK = INTPACK = 8
    (s,) = check_case(eng, 1, 4096, a)
    assert C.formats([s]) == ["RUNPACK"] and len(s) == 8
    for w, size in ((8, 14), (4, 10)):        # INTPACK = DICTPACK, RUNPACK one above
        (s,) = check_case(eng, w, 4096, np.tile(rnd(w, 3), 65))
        assert C.formats([s]) == ["INTPACK"] and len(s) == size
    c = np.zeros(20, np.uint8)                # w = 4: RUNPACK = INTPACK = 21
    c[0:8:4], c[8:16:4], c[16] = 0, 1, 2
    (s,) = check_case(eng, 4, 4096, c)
    assert C.formats([s]) == ["RUNPACK"] and len(s) == 21
    one = np.full(4096, 7, np.uint8)          # the worked examples
    assert [len(check_case(eng, w, 4096, one)[0]) for w in (8, 1, 16)] == [14, 9, 22]


# ---- alignment and the other paths ----------------------------------------------------------------

@pytest.mark.parametrize("w", M.WIDTHS)
def test_input_at_every_alignment(eng, w):
    for seg in (59460, 4096):
        for in_off in (0, 1, 3, 15):
            check_case(eng, w, seg, C.stretches(w, seg, seed=in_off), in_off=in_off)


@pytest.mark.parametrize("w", M.WIDTHS)
def test_scattered_pointer_list_and_host_paths(eng, w):
    """one shape per width through bitar_hip_compress_scattered (the winner is copied into
    dsts[i]), bitar_hip_decompress with the streams at odd addresses, and the host-overlapped
    pair"""
    import bitar_amd as B
    codec = B.codec_autopack(w)
    seg = 59460
    data = C.stretches(w, seg, seed=9)
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec, seg)
    streams = M.encode(data, w, seg)
    first = RM.encode(data, w, seg)
    assert set(C.formats(streams)) == set(M.CANDIDATES[w]) | {"stored"}
    src = dev(data)

    # scattered: slot i of the call is slot perm[i] of the slab
    buf = Buffers(nseg, stride, seg)
    perm = [2, 0, 5, 3, 1, 4]
    assert nseg == len(perm)
    dsts = dev(np.array([buf.slab_ptr + p * stride for p in perm], np.int64))
    B.check(B.lib().bitar_hip_compress_scattered(eng.ctx, eng._stream(None), codec,
                                                 src.data_ptr(), n, seg, dsts.data_ptr(), stride,
                                                 buf.sizes_ptr))
    eng.sync()
    sizes = buf.sizes.cpu().numpy()[8:8 + nseg].view(np.uint32)
    assert sizes.tolist() == [len(s) for s in streams]
    by_slot, first_by_slot = [None] * nseg, [None] * nseg
    for i, p in enumerate(perm):
        by_slot[p], first_by_slot[p] = streams[i], first[i]
    buf.sizes[8:8 + nseg] = dev(np.array([len(s) for s in by_slot], np.int32))
    buf.check_streams(by_slot, first_by_slot)

    # pointer list: stream i at an odd address (1, 3, 5, ... past a 16-B boundary)
    room = (max(len(s) for s in streams) + 32) & ~15
    packed = np.full(nseg * room + 16, CANARY, np.uint8)
    ptrs = []
    for i, s in enumerate(streams):
        o = i * room + 2 * i + 1
        packed[o:o + len(s)] = np.frombuffer(s, np.uint8)
        ptrs.append(o)
    d_packed = dev(packed)
    d_ptrs = dev(np.array(ptrs, np.int64) + d_packed.data_ptr())
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    buf = Buffers(nseg, stride, seg)
    eng.decompress_into(codec, d_ptrs, d_sizes, nseg, seg, buf.out_ptr, buf.prod_ptr,
                        capacity=nseg * seg)
    eng.sync()
    buf.check_output(data)

    # host-overlapped: compress from host memory, decompress into host memory
    buf = Buffers(nseg, stride, seg)
    host = torch.from_numpy(data.copy())
    stage = torch.zeros(nseg * seg, dtype=torch.uint8, device="cuda")
    eng.compress_host_into(codec, host, n, seg, stage, buf.slab_ptr, stride, buf.sizes_ptr)
    eng.sync()
    buf.check_streams(streams, first)
    d_ptrs = dev(np.array([buf.slab_ptr + i * stride for i in range(nseg)], np.int64))
    back = torch.full((nseg * seg,), CANARY, dtype=torch.uint8)
    eng.decompress_host_into(codec, d_ptrs, buf.sizes_ptr, nseg, seg, stage, back, buf.prod_ptr)
    eng.sync()
    assert np.array_equal(back.numpy()[:n], data)
    assert buf.prod.cpu().numpy()[8:8 + nseg].tolist() == [min(seg, n - i * seg) for i in range(nseg)]


# ---- a call that crosses the chunk borders --------------------------------------------------------

def test_many_small_segments_cross_the_chunk_borders(eng):
    """70 000 segments of 72 bytes at w = 8: compress works in chunks of at most 8192 segments,
    decompress in chunks of at most 65536.  The data is a pattern of 16 segments tiled; the
    model encodes the 16 once and the expectation is tiled"""
    import bitar_amd as B
    w, seg, nseg = 8, 72, 70_000
    codec = B.codec_autopack(w)
    rng = np.random.default_rng(72)
    const = np.tile(rnd(8, 1), 9)
    two = rnd(16, 2).reshape(2, 8)[np.arange(9) & 1].reshape(-1)  # (a, b, a, b, ...)
    pattern = [C.segment(k, seg, w, rng) for k in C.KINDS] + [const, two] + \
        [C.segment(k, seg, w, rng) for k in ("runs", "random", "runs", "narrow", "few",
                                             "runs", "random", "decimal", "runs")]
    assert len(pattern) == 16
    streams = [M.encode_segment(p, w) for p in pattern]
    first = [RM.encode_segment(p, w) for p in pattern]
    kinds = C.formats(streams)
    assert {"RUNPACK", "INTPACK", "DICTPACK", "stored"} <= set(kinds), kinds
    stride = B.slot_size(codec, seg)
    rows = np.full((16, stride), CANARY, np.uint8)
    care = np.ones((16, stride), bool)
    for i, s in enumerate(streams):
        rows[i, :len(s)] = np.frombuffer(s, np.uint8)
        care[i, len(s):max(len(s), len(first[i]))] = False
    reps = -(-nseg // 16)
    data = np.tile(np.concatenate(pattern), reps)[:nseg * seg]
    want_slab = np.tile(rows, (reps, 1))[:nseg]
    want_care = np.tile(care, (reps, 1))[:nseg]
    want_sizes = np.tile(np.array([len(s) for s in streams], np.uint32), reps)[:nseg]

    src = dev(data)
    buf = Buffers(nseg, stride, seg)
    eng.compress_into(codec, src, seg, buf.slab_ptr, stride, buf.sizes_ptr, n=data.size)
    eng.decompress_slab_into(codec, buf.slab_ptr, stride, buf.sizes_ptr, nseg, seg, buf.out_ptr,
                             buf.prod_ptr, capacity=nseg * seg)
    eng.sync()
    sizes = buf.sizes.cpu().numpy()
    assert np.all(sizes[:8] == CANARY32) and np.all(sizes[8 + nseg:] == CANARY32)
    assert np.array_equal(sizes[8:8 + nseg].view(np.uint32), want_sizes)
    slab = buf.slab.cpu().numpy()
    assert np.all(slab[:PAD] == CANARY) and np.all(slab[-PAD:] == CANARY)
    got = slab[PAD:-PAD].reshape(nseg, stride)
    bad = np.flatnonzero(((got != want_slab) & want_care).any(axis=1))
    assert bad.size == 0, bad[:8].tolist()
    buf.check_output(data)
    census = eng.autopack_census(buf.slab[PAD:], stride, buf.sizes[8:], nseg)
    tiled = (kinds * reps)[:nseg]
    assert census == {**{k: tiled.count(k) for k in ("INTPACK", "FLTPACK", "DICTPACK", "RUNPACK",
                                                     "stored")}, "other": 0}


# ---- hostile streams --------------------------------------------------------------------------------

def base_streams(seg):
    """one packed stream per format, of a segment that ends inside a chunk and has a tail"""
    rng = np.random.default_rng(seg)
    out = {}
    for kind, name in C.BUILT_FOR.items():
        s = M.MODELS[name].encode_segment(C.segment(kind, seg - 43, 8, rng), 8)
        assert M.format_of(s) == name and C.formats([s]) == [name]
        out[name] = s
    return out


def mutants(s):
    """deterministic mutations of the stream s -> [(bytes, size given to the decoder)]"""
    out = [(s, len(s))]

    def poke(at, value):
        if s[at] != value & 255:
            t = bytearray(s)
            t[at] = value & 255
            out.append((bytes(t), len(s)))

    for bit in range(8):  # the first six bytes, bit by bit
        for at in range(6):
            poke(at, s[at] ^ (1 << bit))
    for nib in range(16):  # the tag through all 16 nibbles
        poke(0, nib << 4 | s[0] & 15)
    out += [(s, len(s) + 1), (s, len(s) - 1), (s, len(s) + 3), (s, len(s) - 3), (s, 3), (s, 0)]
    return out


@pytest.mark.parametrize("seg", (4096, 65536))
@pytest.mark.parametrize("name", ("INTPACK", "FLTPACK", "DICTPACK", "RUNPACK"))
def test_hostile_streams_get_the_model_verdict(eng, name, seg):
    """every mutant is accepted with the model's bytes or rejected with SEGMENT_ERROR; a segment
    rejected for its nibble or an empty stream, and every rejected RUNPACK stream, leaves its
    whole range as it was, and no rejected segment writes outside its own range; the sync reports IOError exactly when one was rejected; the engine works afterwards"""
    import bitar_amd as B
    codec = B.codec_autopack(2)
    base = base_streams(seg)[name]
    muts = mutants(base)
    nseg = len(muts)
    stride = (max(len(t) for t, _ in muts) + 3 + 255) & ~255
    slab = np.full((nseg, stride), 0x5A, np.uint8)
    for i, (t, _) in enumerate(muts):
        slab[i, :len(t)] = np.frombuffer(t, np.uint8)
    given = [slab[i, :size].tobytes() for i, (_, size) in enumerate(muts)]
    verdicts = [M.decode(g, seg) for g in given]
    assert verdicts[0] is not None and any(v is None for v in verdicts)
    assert sum(M.format_of(g) is None for g in given) >= 13  # 12 foreign nibbles, one empty
    d_slab = dev(slab.reshape(-1))
    d_sizes = dev(np.array([size for _, size in muts], np.int32))
    out = torch.full((PAD + nseg * seg + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    prod = torch.full((nseg + 16,), int(CANARY32), dtype=torch.int32, device="cuda")
    eng.decompress_slab_into(codec, d_slab, stride, d_sizes, nseg, seg, out.data_ptr() + PAD,
                             prod.data_ptr() + 32, capacity=nseg * seg)
    with pytest.raises(B.BitarError) as e:
        eng.sync()
    assert e.value.code == -5
    got = prod.cpu().numpy()
    assert np.all(got[:8] == CANARY32) and np.all(got[8 + nseg:] == CANARY32)
    want = [ERR if v is None else len(v) for v in verdicts]
    assert got[8:8 + nseg].tolist() == want
    assert bool((out[:PAD] == CANARY).all()) and bool((out[PAD + nseg * seg:] == CANARY).all())
    host = out.cpu().numpy()
    for i, v in enumerate(verdicts):
        seg_out = host[PAD + i * seg:PAD + (i + 1) * seg]
        if v is not None:
            assert seg_out[:len(v)].tobytes() == v, i
            assert np.all(seg_out[len(v):] == CANARY), i
        elif M.format_of(given[i]) in (None, "RUNPACK", "FLTPACK"):
            assert np.all(seg_out == CANARY), i  # (FLTPACK's decoder writes nothing either)
        elif M.format_of(given[i]) == "DICTPACK":  # never past the length its header gives
            L = 1 + given[i][2] + (given[i][3] << 8) if len(given[i]) >= 4 else 0
            assert np.all(seg_out[min(L, seg):] == CANARY), i
        # (a rejected INTPACK stream may have written inside its own range: the neighbours'
        # ranges are checked by their own turns of this loop)
    # only accepted streams: no error at the sync, and the error above was reported once
    keep = [i for i, v in enumerate(verdicts) if v is not None]
    d_slab2 = dev(slab[keep].reshape(-1))
    d_sizes2 = dev(np.array([muts[i][1] for i in keep], np.int32))
    buf = Buffers(len(keep), stride, seg)
    eng.decompress_slab_into(codec, d_slab2, stride, d_sizes2, len(keep), seg, buf.out_ptr,
                             buf.prod_ptr, capacity=len(keep) * seg)
    eng.sync()
    assert buf.prod.cpu().numpy()[8:8 + len(keep)].tolist() == [len(verdicts[i]) for i in keep]


# ---- ids and empty input ------------------------------------------------------------------------------

def test_every_id_decodes_all_formats_at_mixed_widths(eng):
    import bitar_amd as B
    seg = 4096
    datas, streams = [], []
    for w in M.WIDTHS:
        d = C.stretches(w, seg)[:5 * seg]
        datas.append(d)
        streams += M.encode(d, w, seg)
    assert set(C.formats(streams)) == {"INTPACK", "FLTPACK", "DICTPACK", "RUNPACK", "stored"}
    assert {(M.format_of(s), s[0] & 3) for s in streams} >= {("RUNPACK", 0), ("INTPACK", 1),
                                                             ("DICTPACK", 2), ("FLTPACK", 3)}
    nseg = len(streams)
    stride = B.slot_size(B.CODEC_AUTOPACK8, seg)
    slab = np.zeros((nseg, stride), np.uint8)
    for i, s in enumerate(streams):
        slab[i, :len(s)] = np.frombuffer(s, np.uint8)
    d_slab = dev(slab.reshape(-1))
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    for w in M.WIDTHS:
        buf = Buffers(nseg, stride, seg)
        eng.decompress_slab_into(B.codec_autopack(w), d_slab, stride, d_sizes, nseg, seg,
                                 buf.out_ptr, buf.prod_ptr, capacity=nseg * seg)
        eng.sync()
        buf.check_output(np.concatenate(datas))
    kinds = C.formats(streams)
    assert eng.autopack_census(d_slab, stride, d_sizes, nseg) == \
        {**{k: kinds.count(k) for k in ("INTPACK", "FLTPACK", "DICTPACK", "RUNPACK", "stored")},
         "other": 0}
    d_sizes[3] = 0
    d_slab[5 * stride] = 0x33
    census = eng.autopack_census(d_slab, stride, d_sizes, nseg)
    assert census["other"] == 2 and sum(census.values()) == nseg
    assert eng.autopack_census(d_slab, stride, d_sizes, 0)["other"] == 0


def test_empty_input_launches_nothing(eng):
    import bitar_amd as B
    buf = Buffers(1, 4352, 4096)
    src = torch.zeros(PAD, dtype=torch.uint8, device="cuda")
    for w in M.WIDTHS:
        eng.compress_into(B.codec_autopack(w), src, 4096, buf.slab_ptr, 4352, buf.sizes_ptr, n=0)
        eng.decompress_slab_into(B.codec_autopack(w), buf.slab_ptr, 4352, buf.sizes_ptr, 0, 4096,
                                 buf.out_ptr, buf.prod_ptr, capacity=0)
    eng.sync()
    for t in (buf.slab, buf.out):
        assert bool((t == CANARY).all())
    for t in (buf.sizes, buf.prod):
        assert bool((t == int(CANARY32)).all())


def test_compress_bits_refuses_autopack(eng):
    import bitar_amd as B
    src = dev(C.stretches(4, 4096)[:8192])
    buf = Buffers(2, 4352, 4096)
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    for w in M.WIDTHS:
        with pytest.raises(B.BitarError) as e:
            eng.compress_bits_into(B.codec_autopack(w), src, 4096, buf.slab_ptr, 4352,
                                   buf.sizes_ptr, bits)
        assert e.value.code == -4
    eng.sync()
    assert bool((buf.slab == CANARY).all()) and bool((bits == 0).all())
