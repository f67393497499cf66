"""GPU tests of the DECPACK codec (csrc/decpack.hip) through the C ABI: the slots and sizes of a
compress equal the Python model's streams (decpack_model.py) byte for byte, the decoder returns
the input, and on mutated streams its verdict is the model's, with canaries around every buffer
a call writes.

Shapes: segments of 65536 (16 blocks, 16-B aligned everywhere), 59460 (segments start 4 bytes
into an element: every element is split), 4096 (one block), 1040 (a miniblock and one lane),
1000 / 999, 72 and 7 (shorter than an element).  A value is four dwords on the wave and a field
lies in up to five dwords of the bit string: widths on both sides of every dword edge with the
largest residual in lane 0, lane 63 and the last element of a partial miniblock, references on
both sides of 0 and at the most negative value, running sums that carry out of the low 64 bits
inside a miniblock and across its edge."""
import numpy as np
import pytest

import decpack_cases as C
import decpack_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEGS = (65536, 59460, 4096, 1040, 1000, 999, 72, 7)
TAILS = (0, 1, 15, 16, 63 * 16, 64 * 16, 64 * 16 + 1)
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
        still the canary"""
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
    """compress and decompress `data` -> the model's streams, which the slots equal"""
    import bitar_amd as B
    codec = B.codec_decpack(16)
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
    streams = M.encode(data, seg)
    buf.check_streams(streams)
    buf.check_output(data)
    return streams


def decode_forced(eng, seg, cases):
    """decode the streams of cases = [(data, stream)] from a slab: each gives its data and
    nothing past it"""
    import bitar_amd as B
    stride = (max(len(s) for _, s in cases) + 255) & ~255  # (a packed form may be above 4 + L)
    slab = np.full((len(cases), stride), 0x5A, np.uint8)
    for i, (data, s) in enumerate(cases):
        assert M.decode(s, seg) == data.tobytes()
        slab[i, :len(s)] = np.frombuffer(s, np.uint8)
    buf = Buffers(len(cases), stride, seg)
    eng.decompress_slab_into(B.codec_decpack(16), dev(slab.reshape(-1)), stride,
                             dev(np.array([len(s) for _, s in cases], np.int32)), len(cases), seg,
                             buf.out_ptr, buf.prod_ptr, capacity=len(cases) * seg)
    eng.sync()
    prod = buf.prod.cpu().numpy()[8:8 + len(cases)]
    out = buf.out.cpu().numpy()
    assert np.all(out[:PAD] == CANARY) and np.all(out[PAD + len(cases) * seg:] == CANARY)
    for i, (data, _) in enumerate(cases):
        assert prod[i] == data.size
        got = out[PAD + i * seg:PAD + (i + 1) * seg]
        assert np.array_equal(got[:data.size], data), (i, np.flatnonzero(got[:data.size] != data)[:8])
        assert np.all(got[data.size:] == CANARY), i


@pytest.mark.parametrize("seg", SEGS)
def test_exact_bytes_and_round_trip(eng, seg):
    for r in TAILS:
        data = C.column(8, seg, seg * 31 + r, extra=r)
        streams = check_case(eng, seg, data)
        if seg >= 999:  # where a segment has room, every mode is chosen
            assert {M.mode_of(s) for s in streams} == {0, 1, 2}
    if seg == 72:
        for n in range(1, 16):  # shorter than an element: stored
            check_case(eng, seg, C.noise_segment(n, n))


def test_input_at_every_alignment(eng):
    for seg in (59460, 4096):
        for in_off in (0, 1, 3, 4, 8, 15):
            check_case(eng, seg, C.column(4, seg, in_off, extra=64 * 16 + 1), in_off=in_off)


def test_the_case_columns(eng):
    """the columns of DESIGN.md 4.30's table"""
    for name, col in C.table_columns(n=2 * 65536):
        check_case(eng, 65536, col)


@pytest.mark.parametrize("place", (0, -1))
def test_widths_across_every_dword_edge(eng, place):
    """miniblocks of widths 0, 1, 31, ..., 128 with the largest residual in lane 0, in lane 63
    and in the last element of a partial miniblock; the widths are read back from the model's
    streams"""
    n = len(C.EDGE_WIDTHS)
    for seg in (65536, 65536 - 59 * 16 + 5):  # (the second: a last miniblock of 5 elements)
        segs = [C.width_segment(seg, place, 10 + shift, shift=shift) for shift in (0, 5)]
        streams = check_case(eng, seg, np.concatenate(segs))
        nmb = (seg // 16 + 63) // 64
        for s, shift in zip(streams, (0, 5)):
            assert M.mode_of(s) == 0
            assert M.widths_of(s) == [C.EDGE_WIDTHS[(k + shift) % n] for k in range(nmb)]
        # the block that holds a miniblock of 127 or 128 bits: the most negative reference
        refs_at = 4 + nmb
        refs = {int.from_bytes(streams[0][refs_at + 16 * i:refs_at + 16 * i + 16], "little")
                for i in range((nmb + 3) // 4)}
        assert C.MOST_NEGATIVE in refs
        assert any(r >> 127 and r != C.MOST_NEGATIVE for r in refs) and any(r >> 127 == 0 for r in refs)


def test_delta_carries_and_signs(eng):
    """ascending sums that carry out of the low 64 bits inside a miniblock and across its edge,
    descending columns, a step at element 1"""
    seg = 4096
    segs = [C.delta_segment(seg, kind, 3) for kind in ("asc", "desc", "step")]
    lo = np.concatenate(segs[:1]).view("<u8")[0::2]
    wraps = np.flatnonzero(lo[1:] < lo[:-1]) + 1  # elements whose low half wrapped
    assert np.any(wraps % 64 == 0) and np.any(wraps % 64 != 0)
    streams = check_case(eng, seg, np.concatenate(segs))
    assert [M.mode_of(s) for s in streams] == [1, 1, 1]
    for seg in (59460, 1040):
        data = np.concatenate([C.delta_segment(seg, k, 4) for k in ("asc", "desc", "step")])
        streams = check_case(eng, seg, data)
        assert M.mode_of(streams[0]) == 1 and M.mode_of(streams[2]) == 1


def test_one_and_two_elements(eng):
    """m = 1 and m = 2: the encoder stores them; the decoder takes their packed forms in both
    modes (x_0 = 0 when m = 1)"""
    for L in (16, 17, 31, 32, 47):
        data = C.delta_segment(L, "asc", L)
        streams = check_case(eng, L, np.concatenate([data, data]))
        assert all(M.mode_of(s) == 2 for s in streams)
        decode_forced(eng, 48, [(data, M.packed_stream(data, mode)) for mode in (0, 1)])


def test_streams_no_encoder_writes(eng):
    """all widths 128 (a packed form above 4 + L), mode 1 where mode 0 is smaller and mode 0 where
    mode 1 is"""
    for seg in (65536, 4096):
        L = seg - 5 * 16 - 3
        nmb = (L // 16 + 63) // 64
        plain, asc = C.width_segment(L, -1, 5), C.delta_segment(L, "asc", 6)
        cases = [(plain, M.packed_stream(plain, 0, [128] * nmb)),
                 (asc, M.packed_stream(asc, 1, [128] * nmb)),
                 (plain, M.packed_stream(plain, 1)), (asc, M.packed_stream(asc, 0))]
        assert len(cases[0][1]) > 4 + L and len(cases[1][1]) > 4 + L
        assert len(cases[2][1]) > len(M.packed_stream(plain, 0))
        decode_forced(eng, seg, cases)


def test_mixed_segments_in_one_call(eng):
    """plain, stored, delta, stored and a short last segment without and with a tail, in one
    call"""
    seg = 4096
    a, c = C.width_segment(seg, 0, 3), C.delta_segment(seg, "desc", 4)
    b = C.noise_segment(seg, 2)
    for tail in (0, 15):
        data = np.concatenate([a, b, c, b, a[:100 * 16], C.noise_segment(tail, 4)])
        streams = check_case(eng, seg, data)
        assert [M.mode_of(s) for s in streams] == [0, 2, 1, 2, 0]


def test_empty_input_launches_nothing(eng):
    import bitar_amd as B
    buf = Buffers(1, 4352, 4096)
    src = torch.zeros(PAD, dtype=torch.uint8, device="cuda")
    eng.compress_into(B.codec_decpack(16), src, 4096, buf.slab_ptr, 4352, buf.sizes_ptr, n=0)
    eng.decompress_slab_into(B.codec_decpack(16), buf.slab_ptr, 4352, buf.sizes_ptr, 0, 4096,
                             buf.out_ptr, buf.prod_ptr, capacity=0)
    eng.sync()
    for t in (buf.slab, buf.out):
        assert bool((t == CANARY).all())
    for t in (buf.sizes, buf.prod):
        assert bool((t == int(CANARY32)).all())


def test_more_segments_than_a_chunk(eng):
    """32800 segments of 64 bytes in one call: beyond the runtime's 32768-segment chunk"""
    seg, nseg = 64, 32800
    rng = np.random.default_rng(9)
    v = rng.integers(-16, 16, nseg * 4)  # (4 elements a segment: at most 5 bits each pack)
    v[::7] = rng.integers(-2**62, 2**62, v[::7].size)  # (these segments are stored)
    data = C.from_int64(v)
    streams = check_case(eng, seg, data)
    assert {M.mode_of(s) for s in streams} >= {0, 2}


def test_pointer_list_at_odd_addresses(eng):
    """bitar_hip_decompress with the streams at odd addresses: every load of the header arrays,
    the references and the payload is unaligned"""
    import bitar_amd as B
    seg = 59460
    data = C.column(8, seg, 77, extra=64 * 16 + 1)
    streams = M.encode(data, seg)
    nseg = len(streams)
    room = (max(len(s) for s in streams) + 32) & ~15
    packed = np.full(nseg * room + 32, CANARY, np.uint8)
    ptrs = []
    for i, s in enumerate(streams):
        o = i * room + 2 * i + 1
        packed[o:o + len(s)] = np.frombuffer(s, np.uint8)
        ptrs.append(o)
    d_packed = dev(packed)
    d_ptrs = dev(np.array(ptrs, np.int64) + d_packed.data_ptr())
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    buf = Buffers(nseg, B.slot_size(B.codec_decpack(16), seg), seg)
    eng.decompress_into(B.codec_decpack(16), d_ptrs, d_sizes, nseg, seg, buf.out_ptr,
                        buf.prod_ptr, capacity=nseg * seg)
    eng.sync()
    buf.check_output(data)


# ---- hostile streams (the mutants: decpack_cases.py; their split: test_decpack_model.py) ---------

@pytest.mark.parametrize("seg", (4096, 65536))
def test_hostile_streams_get_the_model_verdict(eng, seg):
    """every mutant is accepted with the model's bytes or rejected with SEGMENT_ERROR and its
    whole output range left as it was, the sync of its queue pair reports IOError exactly once, a
    good stream decodes on the other queue pair at the same time, nothing outside the output is
    written and the engine works afterwards"""
    import bitar_amd as B
    codec = B.codec_decpack(16)
    q0, q1 = eng.queue_pair_stream(0), eng.queue_pair_stream(1)
    count = 0
    for base in C.base_streams(M, seg):
        muts = C.mutants(base)
        count += len(muts)
        nseg = len(muts)
        stride = (max(max(len(t), size) for t, size in muts) + 1 + 255) & ~255
        slab = np.full((nseg, stride), 0x5A, np.uint8)
        for i, (t, _) in enumerate(muts):
            slab[i, :len(t)] = np.frombuffer(t, np.uint8)
        verdicts = [M.decode(slab[i, :size].tobytes(), seg) for i, (_, size) in enumerate(muts)]
        assert verdicts == [M.decode(C.given(t, size), seg) for t, size in muts]
        assert verdicts[0] is not None and any(v is None for v in verdicts)
        d_slab = dev(slab.reshape(-1))
        d_sizes = dev(np.array([size for _, size in muts], np.int32))
        out = torch.full((PAD + nseg * seg + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        prod = torch.full((nseg + 16,), int(CANARY32), dtype=torch.int32, device="cuda")
        g_out = torch.full((PAD + seg + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        g_prod = torch.full((1 + 16,), int(CANARY32), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # (the buffers were filled on torch's stream)
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, nseg, seg, out.data_ptr() + PAD,
                                 prod.data_ptr() + 32, capacity=nseg * seg, stream=q0)
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, 1, seg, g_out.data_ptr() + PAD,
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
        assert bool((out[:PAD] == CANARY).all()) and bool((out[PAD + nseg * seg:] == CANARY).all())
        host = out.cpu().numpy()
        for i, v in enumerate(verdicts):
            seg_out = host[PAD + i * seg:PAD + (i + 1) * seg]
            n = 0 if v is None else len(v)  # a rejected segment writes nothing at all
            assert seg_out[:n].tobytes() == (v or b""), i
            assert np.all(seg_out[n:] == CANARY), i
        # the engine works afterwards
        eng.decompress_slab_into(codec, d_slab, stride, d_sizes, 1, seg, out.data_ptr() + PAD,
                                 prod.data_ptr() + 32, capacity=seg)
        eng.sync()
        assert out[PAD:PAD + len(verdicts[0])].cpu().numpy().tobytes() == verdicts[0]
    assert count >= 80


def test_compress_bits_refuses_decpack(eng):
    import bitar_amd as B
    src = dev(C.column(2, 4096, 1))
    buf = Buffers(2, 4352, 4096)
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(B.BitarError) as e:
        eng.compress_bits_into(B.codec_decpack(16), src, 4096, buf.slab_ptr, 4352, buf.sizes_ptr,
                               bits)
    assert e.value.code == -4
    eng.sync()
    assert bool((buf.slab == CANARY).all())


def test_other_families_reject_the_nibble(eng):
    """DECPACK is no candidate of AUTOPACK, whose decoder goes on rejecting tag nibble 0xD, and
    the INTPACK, PATCHPACK and RUNPACK ids reject the stream too: the range stays untouched"""
    import bitar_amd as B
    seg = 4096
    (s,) = M.encode(C.width_segment(seg, 0, 9), seg)
    assert s[0] >> 4 == 0xD
    for codec in (B.CODEC_AUTOPACK128, B.CODEC_INTPACK64, B.CODEC_PATCHPACK64, B.CODEC_RUNPACK128):
        stride = B.slot_size(codec, seg)
        slab = np.zeros(stride, np.uint8)
        slab[:len(s)] = np.frombuffer(s, np.uint8)
        buf = Buffers(1, stride, seg)
        eng.decompress_slab_into(codec, dev(slab), stride, dev(np.array([len(s)], np.int32)), 1,
                                 seg, buf.out_ptr, buf.prod_ptr, capacity=seg)
        with pytest.raises(B.BitarError) as e:
            eng.sync()
        assert e.value.code == -5
        assert buf.prod.cpu().numpy()[8] == ERR and bool((buf.out == CANARY).all())
