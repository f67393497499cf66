"""GPU tests of the RANS codec (csrc/rans.hip) through the C ABI: the slots and sizes of a
compress equal the numpy model's streams (rans_model.py) byte for byte, the decoder returns the
input, and on mutated streams its verdict is the model's, with canaries around every buffer a
call writes.

Shapes: segments of 65536, 59460 (segment starts at every residue mod 4), 4096, 1000 / 999, 72,
7 and 1; lengths on both sides of one and two steps of 64 symbols; the lengths at which the rans
form, the stored form and their tie meet; alphabets of 1, 2, 16, 255 and 256 symbols."""
import numpy as np
import pytest

import rans_cases as C
import rans_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEGS = (65536, 59460, 4096, 1000, 999, 72, 7, 1)
CANARY = 0xA5
CANARY32 = np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]
PAD = 256
ERR = np.array([0xFFFFFFFF], np.uint32).view(np.int32)[0]


@pytest.fixture(scope="module")
def eng():
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0, num_streams=2)
    yield e
    e.close()


def codec():
    import bitar_amd as B
    return B.CODEC_RANS


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

    def check_streams(self, streams):
        """slots and sizes against the model's streams; whatever a stream does not cover is
        still the canary (for a stored stream that is the slot from 4 + L on)"""
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
            assert np.all(slot[want.size:] == CANARY), i

    def check_output(self, data):
        n = data.size
        prod = self.prod.cpu().numpy()
        assert np.all(prod[:8] == CANARY32) and np.all(prod[8 + self.nseg:] == CANARY32)
        want = [min(self.seg, n - i * self.seg) for i in range(self.nseg)]
        assert prod[8:8 + self.nseg].tolist() == want
        out = self.out.cpu().numpy()
        assert np.all(out[:PAD] == CANARY) and np.all(out[PAD + n:] == CANARY)
        assert np.array_equal(out[PAD:PAD + n], data), np.flatnonzero(out[PAD:PAD + n] != data)[:8]


def check_case(eng, seg, data, in_off=0):
    import bitar_amd as B
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec(), seg)
    src = torch.zeros(in_off + n + PAD, dtype=torch.uint8, device="cuda")
    src[in_off:in_off + n] = dev(data)
    buf = Buffers(nseg, stride, seg)
    eng.compress_into(codec(), src.data_ptr() + in_off, seg, buf.slab_ptr, stride, buf.sizes_ptr,
                      n=n)
    eng.decompress_slab_into(codec(), buf.slab_ptr, stride, buf.sizes_ptr, nseg, seg, buf.out_ptr,
                             buf.prod_ptr, capacity=nseg * seg)
    eng.sync()
    streams = M.encode(data, seg)
    buf.check_streams(streams)
    buf.check_output(data)
    return streams


@pytest.mark.parametrize("seg", SEGS)
def test_exact_bytes_and_round_trip(eng, seg):
    """whole segments and a short last one; from 1000 bytes up the segments take both forms"""
    tails = (0, 777) if seg > 4096 else sorted({0, 1, 63, 64, 65} & set(range(seg)))
    for r in tails:
        streams = check_case(eng, seg, C.mixed(5 * seg + r, seg + r))
        if seg >= 999:
            assert {s[0] for s in streams} == {0xA0, 0xA1}
        if seg <= 72:
            assert {s[0] for s in streams} == {0xA1}


@pytest.mark.parametrize("L", (63, 64, 65, 127, 128, 129))
def test_one_and_two_steps(eng, L):
    """a partial first-processed step, one whole step, two: as the only and as the last segment.
    Lengths this short are stored (the states alone are 256 bytes); the same lengths as the tail
    of a rans-coded segment size go through the coder"""
    (s,) = check_case(eng, 65536, np.full(L, 5, np.uint8))
    assert s[0] == 0xA1
    streams = check_case(eng, 1024 + L, np.full(3 * (1024 + L), 5, np.uint8))
    assert all(s[0] == 0xA0 for s in streams)
    streams = check_case(eng, 1024 + L, C.alphabet(2 * (1024 + L) + 512 + L, 4, L))
    assert all(s[0] == 0xA0 for s in streams)


def test_worked_example_and_ties(eng):
    (s,) = check_case(eng, 4096, np.zeros(291, np.uint8))
    assert s == bytes.fromhex("a0002201" + "01" + "00" * 31 + "ff0f") + bytes.fromhex("00000100") * 64
    (s,) = check_case(eng, 4096, np.zeros(290, np.uint8))
    assert s[0] == 0xA1 and len(s) == 294
    for L, mode in ((438, 1), (440, 1), (442, 0)):
        (s,) = check_case(eng, 4096, C.tie_input(L))
        assert s[0] == 0xA0 | mode, L
        assert len(M.rans_form(C.tie_input(L))) - (4 + L) == {438: 2, 440: 0, 442: -2}[L]


@pytest.mark.parametrize("nsym", (1, 2, 16, 255, 256))
def test_alphabets(eng, nsym):
    for seg in (65536, 4096):
        streams = check_case(eng, seg, C.alphabet(2 * seg + 1000, nsym, nsym))
        if nsym <= 16 or seg == 65536:
            assert all(s[0] == 0xA0 and C.parts_of(s)[0] == nsym for s in streams[:2])


def test_stress_histogram_random_and_near_empty(eng):
    """the 127 x 512 + 384 + 128 singletons histogram; random bytes, stored, with the canary
    just past 4 + L; one symbol but for a handful, hardly a word"""
    (s,) = check_case(eng, 65536, C.stress_histogram())
    f = C.frequencies_of(s)
    assert s[0] == 0xA0 and f.sum() == 4096 and f.min() >= 1
    streams = check_case(eng, 65536, C.rnd(2 * 65536 + 100, 3))
    assert all(s[0] == 0xA1 for s in streams)
    streams = check_case(eng, 59460, C.rnd(59460 + 4093, 4), in_off=3)
    assert all(s[0] == 0xA1 for s in streams)
    streams = check_case(eng, 65536, C.mostly_one(2 * 65536, 5))
    assert all(s[0] == 0xA0 and C.parts_of(s)[2] < 64 for s in streams)
    (s,) = check_case(eng, 65536, np.full(65536, 200, np.uint8))
    assert s[0] == 0xA0 and C.parts_of(s) == (1, 2, 0)


@pytest.mark.parametrize("seg", (59460, 4096))
def test_input_at_every_alignment(eng, seg):
    data = C.mixed(3 * seg + 65, seg)
    for in_off in range(16):
        check_case(eng, seg, data, in_off=in_off)


def test_mixed_segments_in_one_call(eng):
    seg = 4096
    rng = np.random.default_rng(1)
    a, b, c = M.text_like(rng, seg), C.rnd(seg, 2), C.alphabet(seg, 16, 3)
    data = np.concatenate([a, b, c, b, np.full(seg, 1, np.uint8), c[:300], C.rnd(7, 4)])
    streams = check_case(eng, seg, data)
    assert [s[0] & 1 for s in streams] == [0, 1, 0, 1, 0, 1]


def test_empty_input_launches_nothing(eng):
    buf = Buffers(1, 4352, 4096)
    src = torch.zeros(PAD, dtype=torch.uint8, device="cuda")
    eng.compress_into(codec(), src, 4096, buf.slab_ptr, 4352, buf.sizes_ptr, n=0)
    eng.decompress_slab_into(codec(), buf.slab_ptr, 4352, buf.sizes_ptr, 0, 4096, buf.out_ptr,
                             buf.prod_ptr, capacity=0)
    eng.sync()
    for t in (buf.slab, buf.out):
        assert bool((t == CANARY).all())
    for t in (buf.sizes, buf.prod):
        assert bool((t == int(CANARY32)).all())


def test_scattered_pointer_list_and_host_paths(eng):
    """bitar_hip_compress_scattered, bitar_hip_decompress with the streams at odd addresses
    (words and states unaligned), and the host-overlapped pair"""
    import bitar_amd as B
    seg = 59460
    data = C.mixed(3 * seg + 65, 77)
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec(), seg)
    streams = M.encode(data, seg)
    assert {s[0] for s in streams} == {0xA0, 0xA1}
    src = dev(data)

    # scattered: slot i of the call is slot perm[i] of the slab
    buf = Buffers(nseg, stride, seg)
    perm = [2, 0, 3, 1]
    assert nseg == len(perm)
    dsts = dev(np.array([buf.slab_ptr + p * stride for p in perm], np.int64))
    B.check(B.lib().bitar_hip_compress_scattered(eng.ctx, eng._stream(None), codec(),
                                                 src.data_ptr(), n, seg, dsts.data_ptr(), stride,
                                                 buf.sizes_ptr))
    eng.sync()
    sizes = buf.sizes.cpu().numpy()[8:8 + nseg].view(np.uint32)
    assert sizes.tolist() == [len(s) for s in streams]
    by_slot = [None] * nseg
    for i, p in enumerate(perm):
        by_slot[p] = streams[i]
    buf.sizes[8:8 + nseg] = dev(np.array([len(s) for s in by_slot], np.int32))
    buf.check_streams(by_slot)

    # pointer list: stream i at an odd address (1, 3, 5, 7 past a 16-B boundary)
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
    eng.decompress_into(codec(), d_ptrs, d_sizes, nseg, seg, buf.out_ptr, buf.prod_ptr,
                        capacity=nseg * seg)
    eng.sync()
    buf.check_output(data)

    # host-overlapped: compress from host memory, decompress into host memory
    buf = Buffers(nseg, stride, seg)
    host = torch.from_numpy(data.copy())
    stage = torch.zeros(nseg * seg, dtype=torch.uint8, device="cuda")
    eng.compress_host_into(codec(), host, n, seg, stage, buf.slab_ptr, stride, buf.sizes_ptr)
    eng.sync()
    buf.check_streams(streams)
    d_ptrs = dev(np.array([buf.slab_ptr + i * stride for i in range(nseg)], np.int64))
    back = torch.full((nseg * seg,), CANARY, dtype=torch.uint8)
    eng.decompress_host_into(codec(), d_ptrs, buf.sizes_ptr, nseg, seg, stage, back, buf.prod_ptr)
    eng.sync()
    assert np.array_equal(back.numpy()[:n], data)
    assert buf.prod.cpu().numpy()[8:8 + nseg].tolist() == [min(seg, n - i * seg) for i in range(nseg)]


# ---- hostile streams ----------------------------------------------------------------------------

def base_streams(seg):
    """a rans stream of text-like bytes, one of a small alphabet that ends inside a step, one of
    a single symbol, a rans form no encoder writes (larger than 4 + L) and a stored one"""
    rng = np.random.default_rng(seg)
    out = []
    for data in (M.text_like(rng, seg), C.alphabet(seg - 37, 5, seg), np.full(seg - 1, 7, np.uint8)):
        (s,) = M.encode(data, seg)
        assert s[0] == 0xA0 and M.decode(s, seg) == data.tobytes()
        out.append(s)
    data = C.rnd(300, seg)
    s = M.rans_form(data)
    assert len(s) > 4 + 300 and M.decode(s, seg) == data.tobytes()
    out.append(s)
    (s,) = M.encode(C.rnd(seg - 3, seg + 1), seg)
    assert s[0] == 0xA1
    out.append(s)
    return out


@pytest.mark.parametrize("seg", (4096, 1000))
def test_hostile_streams_get_the_model_verdict(eng, seg):
    """every mutant is accepted with the model's bytes or rejected with SEGMENT_ERROR, nothing
    outside a segment's own seg output bytes is written (a reject that rANS's own check finds
    comes after part of that range was written), the sync of its queue pair reports IOError
    exactly once, a good stream decodes on the other queue pair at the same time, and the engine
    works afterwards"""
    import bitar_amd as B
    q0, q1 = eng.queue_pair_stream(0), eng.queue_pair_stream(1)
    for base in base_streams(seg):
        muts = C.mutants(base)
        nseg = len(muts)
        stride = (max(len(t) for t, _ in muts) + 1 + 255) & ~255
        slab = np.full((nseg, stride), 0x5A, np.uint8)
        for i, (t, _) in enumerate(muts):
            slab[i, :len(t)] = np.frombuffer(t, np.uint8)
        verdicts = [M.decode(slab[i, :size].tobytes(), seg) for i, (_, size) in enumerate(muts)]
        assert verdicts[0] is not None and any(v is None for v in verdicts)
        if base[0] == 0xA0 and C.parts_of(base)[0] > 1:  # (accepted with other bytes too)
            assert len({v for v in verdicts if v is not None}) > 1
            assert sum(v is not None for v in verdicts) >= 3
        d_slab = dev(slab.reshape(-1))
        d_sizes = dev(np.array([size for _, size in muts], np.int32))
        out = torch.full((PAD + nseg * seg + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        prod = torch.full((nseg + 16,), int(CANARY32), dtype=torch.int32, device="cuda")
        g_out = torch.full((PAD + seg + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        g_prod = torch.full((1 + 16,), int(CANARY32), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # (the buffers were filled on torch's stream)
        eng.decompress_slab_into(codec(), d_slab, stride, d_sizes, nseg, seg, out.data_ptr() + PAD,
                                 prod.data_ptr() + 32, capacity=nseg * seg, stream=q0)
        eng.decompress_slab_into(codec(), d_slab, stride, d_sizes, 1, seg, g_out.data_ptr() + PAD,
                                 g_prod.data_ptr() + 32, capacity=seg, stream=q1)
        eng.sync(stream=q1)  # the good stream on the other queue pair: nothing to report
        with pytest.raises(B.BitarError) as e:
            eng.sync(stream=q0)
        assert e.value.code == -5
        eng.sync(stream=q0)  # reported once
        g = g_out.cpu().numpy()
        assert g_prod.cpu().numpy()[8] == len(verdicts[0])
        assert g[PAD:PAD + len(verdicts[0])].tobytes() == verdicts[0]
        assert np.all(g[:PAD] == CANARY) and np.all(g[PAD + len(verdicts[0]):] == CANARY)
        got = prod.cpu().numpy()
        assert np.all(got[:8] == CANARY32) and np.all(got[8 + nseg:] == CANARY32)
        want = [ERR if v is None else len(v) for v in verdicts]
        assert got[8:8 + nseg].tolist() == want
        host = out.cpu().numpy()
        assert np.all(host[:PAD] == CANARY) and np.all(host[PAD + nseg * seg:] == CANARY)
        for i, v in enumerate(verdicts):
            seg_out = host[PAD + i * seg:PAD + (i + 1) * seg]
            if v is None:  # at most the L bytes the header names were written
                L = 1 + int(slab[i, 2]) + (int(slab[i, 3]) << 8)
                assert np.all(seg_out[min(L, seg):] == CANARY), i
            else:
                assert seg_out[:len(v)].tobytes() == v, i
                assert np.all(seg_out[len(v):] == CANARY), i
        # the engine works afterwards
        eng.decompress_slab_into(codec(), d_slab, stride, d_sizes, 1, seg, out.data_ptr() + PAD,
                                 prod.data_ptr() + 32, capacity=seg)
        eng.sync()
        assert out[PAD:PAD + len(verdicts[0])].cpu().numpy().tobytes() == verdicts[0]


def test_compress_bits_refuses_rans(eng):
    import bitar_amd as B
    src = dev(C.mixed(8192, 1))
    buf = Buffers(2, 4352, 4096)
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(B.BitarError) as e:
        eng.compress_bits_into(codec(), src, 4096, buf.slab_ptr, 4352, buf.sizes_ptr, bits)
    assert e.value.code == -4
    eng.sync()
    assert bool((buf.slab == CANARY).all())
