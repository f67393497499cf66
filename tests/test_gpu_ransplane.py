"""GPU tests of the RANSPLANE codec (csrc/ransplane.hip) through the C ABI, for the element
widths 2, 4 and 8: the slots and sizes of a compress equal the numpy model's streams
(ransplane_model.py) byte for byte, the decoder returns the input, and on mutated streams its
verdict is the model's.  Every buffer a call writes is a guarded view (gpu_canary.py): nothing
past a stream's last byte -- so nothing past 4 + L of a slot -- and nothing outside a segment's L
output bytes is written, on accepted and on rejected streams.

Shapes: segments of 65536, 59460 (no multiple of 8: the planes of odd segments are rotated),
4096, 129 and 64, three of them and a short last one whose length is no multiple of the width;
lengths on both sides of one and two steps of 64 symbols and of the width; planes of every shape
in one segment; a segment whose words pass 4 + L in the coder's last steps."""
import numpy as np
import pytest

import gpu_canary as G
import ransplane_cases as C
import ransplane_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WIDTHS = M.WIDTHS
SEGS = (65536, 59460, 4096, 129, 64)
ERR = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0, num_streams=2)
    yield e
    e.close()


def codec(w):
    import bitar_amd as B
    return B.codec_ransplane(w)


def stored(w):
    return 0xB8 | M.lg_of(w)


def planes(w):
    return 0xB0 | M.lg_of(w)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


class Buffers:
    """guarded device buffers of one compress + decompress"""

    def __init__(self, nseg, stride, seg):
        self.nseg, self.stride, self.seg = nseg, stride, seg
        self.slab = G.GuardedBytes(nseg * stride, 0, "cuda", "slab")
        self.sizes = G.GuardedWords(nseg, "cuda", "sizes")
        self.out = G.GuardedBytes(nseg * seg, 0, "cuda", "out")
        self.prod = G.GuardedWords(nseg, "cuda", "produced")

    def check_streams(self, streams):
        """slots and sizes against the model's streams; whatever a stream does not cover still
        holds the fill byte (for a stored stream that is the slot from 4 + L on)"""
        self.sizes.check()
        assert self.sizes.values().tolist() == [len(s) for s in streams]
        whole = self.slab.host()
        self.slab.check(whole)
        slab = self.slab.payload(whole)
        for i, s in enumerate(streams):
            slot = slab[i * self.stride:(i + 1) * self.stride]
            want = np.frombuffer(s, np.uint8)
            assert np.array_equal(slot[:want.size], want), \
                (i, s[0], np.flatnonzero(slot[:want.size] != want)[:8].tolist())
            self.slab.check_fill(i * self.stride + want.size, (i + 1) * self.stride,
                                 f"slot {i} past its stream", whole)

    def check_output(self, data):
        n = data.size
        self.prod.check()
        want = [min(self.seg, n - i * self.seg) for i in range(self.nseg)]
        assert self.prod.values().tolist() == want
        whole = self.out.host()
        self.out.check(whole)
        out = self.out.payload(whole)
        assert np.array_equal(out[:n], data), np.flatnonzero(out[:n] != data)[:8]
        self.out.check_fill(n, self.nseg * self.seg, "the last segment past its length", whole)


def check_case(eng, w, seg, data, in_off=0):
    import bitar_amd as B
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec(w), seg)
    src = torch.zeros(in_off + n + 256, dtype=torch.uint8, device="cuda")
    src[in_off:in_off + n] = dev(data)
    buf = Buffers(nseg, stride, seg)
    eng.compress_into(codec(w), src.data_ptr() + in_off, seg, buf.slab.ptr, stride, buf.sizes.ptr,
                      n=n)
    eng.decompress_slab_into(codec(w), buf.slab.ptr, stride, buf.sizes.ptr, nseg, seg, buf.out.ptr,
                             buf.prod.ptr, capacity=nseg * seg)
    eng.sync()
    streams = M.encode(data, seg, w)
    buf.check_streams(streams)
    buf.check_output(data)
    return streams


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("w", WIDTHS)
def test_exact_bytes_and_round_trip(eng, w, seg):
    """three whole segments, the third of noise, and a last one whose length is no multiple of
    the width; the large segments take both forms"""
    for tail in (w + 1, seg // 2 + 1) if seg > 129 else (1, w + 1, 63):
        assert tail % w and tail < seg
        data = np.concatenate([C.mixed(2 * seg, w, seg + tail), C.rnd(seg, tail),
                               C.mixed(tail, w, tail)])
        streams = check_case(eng, w, seg, data)
        assert len(streams) == 4
        if seg >= 59460:
            assert {s[0] for s in streams} == {planes(w), stored(w)}
        elif seg <= 129:  # (at 4096 the tables of width 8 leave little to win)
            assert {s[0] for s in streams} == {stored(w)}


@pytest.mark.parametrize("w", WIDTHS)
def test_lengths_around_the_steps_and_the_width(eng, w):
    """a partial first-processed step, one whole step, two, and one byte around the width: as the
    only segment (stored: the states alone are 256 bytes) and as the tail of a segment size the
    coder takes"""
    for L in (1, w - 1, w, w + 1, 63, 64, 65, 127, 128, 129):
        (s,) = check_case(eng, w, 65536, C.sparse(L, w, L))
        assert s[0] == stored(w)
        streams = check_case(eng, w, 2048 + L, C.sparse(2 * (2048 + L) + 1024 + L, w, L))
        assert all(s[0] == planes(w) for s in streams)


@pytest.mark.parametrize("w", WIDTHS)
def test_cross_check_sizes_and_the_tie(eng, w):
    (s,) = check_case(eng, w, 65536, np.full(65536, 0x41, np.uint8))
    assert len(s) == 260 + 34 * w and C.parts_of(s, w) == ([1] * w, [2] * w, 0)
    near = 2 * (4 + 56 * w + 256)
    found = {}
    for L in range(near - 400, near + 200):
        d = len(M.planes_form(C.tie_alphabet(L, w), w)) - (4 + L)
        if d in (2, 0, -2) and d not in found:
            found[d] = L
    assert set(found) == {2, 0, -2}
    for d, L in found.items():
        (s,) = check_case(eng, w, 4096, C.tie_alphabet(L, w))
        assert s[0] == (planes(w) if d < 0 else stored(w)), (d, L)


@pytest.mark.parametrize("w", WIDTHS)
def test_plane_shapes_noise_and_a_late_bail_out(eng, w):
    """a constant plane (f = 4096, the lane never emits) beside planes of 2, 17 and 256 symbols and
    noise; noise everywhere, stored; near-noise in every plane, whose words pass 4 + L in the
    coder's last steps, stored too, with the fill byte just past 4 + L"""
    for seed in (2, 3):
        data = np.concatenate([C.plane_shapes(65536, w, seed), C.plane_shapes(65536 - 3, w, seed + 2)])
        streams = check_case(eng, w, 65536, data)
        assert all(s[0] == planes(w) for s in streams)
        assert max(C.parts_of(streams[0], w)[0]) == 256
    streams = check_case(eng, w, 59460, C.rnd(59460 + 4093, 4), in_off=3)
    assert all(s[0] == stored(w) for s in streams)
    data = C.near_noise(2 * 65536 - 5, w)
    assert len(M.planes_form(data[:65536], w)) < 1.06 * 65536
    streams = check_case(eng, w, 65536, data)
    assert all(s[0] == stored(w) for s in streams)


@pytest.mark.parametrize("w", WIDTHS)
def test_input_at_every_alignment(eng, w):
    for seg in (59460, 4096):
        data = C.mixed(2 * seg + 65, w, seg)
        for in_off in range(8):
            check_case(eng, w, seg, data, in_off=in_off)


@pytest.mark.parametrize("w", WIDTHS)
def test_mixed_segments_in_one_call(eng, w):
    seg = 4096
    a, b, c = C.plane_shapes(seg, w, 6), C.rnd(seg, 2), C.sparse(seg, w, 3)
    data = np.concatenate([a, b, c, b, np.full(seg, 1, np.uint8), c[:300], C.rnd(7, 4)])
    streams = check_case(eng, w, seg, data)
    assert [s[0] >> 3 & 1 for s in streams] == [0, 1, 0, 1, 0, 1]


def test_empty_input_launches_nothing(eng):
    for w in WIDTHS:
        buf = Buffers(1, 4352, 4096)
        src = torch.zeros(256, dtype=torch.uint8, device="cuda")
        eng.compress_into(codec(w), src, 4096, buf.slab.ptr, 4352, buf.sizes.ptr, n=0)
        eng.decompress_slab_into(codec(w), buf.slab.ptr, 4352, buf.sizes.ptr, 0, 4096, buf.out.ptr,
                                 buf.prod.ptr, capacity=0)
        eng.sync()
        for t in (buf.slab, buf.out):
            t.check()
            t.check_fill(0, t.n, "an empty call's buffer")
        for t in (buf.sizes, buf.prod):
            t.check()
            assert (t.values() == G.FILL_WORD).all()


@pytest.mark.parametrize("w", WIDTHS)
def test_scattered_pointer_list_and_host_paths(eng, w):
    """bitar_hip_compress_scattered, bitar_hip_decompress with the streams at odd addresses
    (tables, words and states unaligned), and the host-overlapped pair"""
    import bitar_amd as B
    seg = 59460
    data = C.mixed(3 * seg + 65, w, 77)
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec(w), seg)
    streams = M.encode(data, seg, w)
    assert {s[0] for s in streams} == {planes(w), stored(w)}
    src = dev(data)

    # scattered: slot i of the call is slot perm[i] of the slab
    buf = Buffers(nseg, stride, seg)
    perm = [2, 0, 3, 1]
    assert nseg == len(perm)
    dsts = dev(np.array([buf.slab.ptr + p * stride for p in perm], np.int64))
    B.check(B.lib().bitar_hip_compress_scattered(eng.ctx, eng._stream(None), codec(w),
                                                 src.data_ptr(), n, seg, dsts.data_ptr(), stride,
                                                 buf.sizes.ptr))
    eng.sync()
    assert buf.sizes.values().tolist() == [len(s) for s in streams]
    by_slot = [None] * nseg
    for i, p in enumerate(perm):
        by_slot[p] = streams[i]
    buf.sizes.load([len(s) for s in by_slot])
    buf.check_streams(by_slot)

    # pointer list: stream i at an odd address (1, 3, 5, 7 past a 16-B boundary)
    room = (max(len(s) for s in streams) + 32) & ~15
    packed = np.full(nseg * room + 16, G.GUARD_BYTE, np.uint8)
    ptrs = []
    for i, s in enumerate(streams):
        o = i * room + 2 * i + 1
        packed[o:o + len(s)] = np.frombuffer(s, np.uint8)
        ptrs.append(o)
    d_packed = dev(packed)
    d_ptrs = dev(np.array(ptrs, np.int64) + d_packed.data_ptr())
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    buf = Buffers(nseg, stride, seg)
    eng.decompress_into(codec(w), d_ptrs, d_sizes, nseg, seg, buf.out.ptr, buf.prod.ptr,
                        capacity=nseg * seg)
    eng.sync()
    buf.check_output(data)

    # host-overlapped: compress from host memory, decompress into host memory
    buf = Buffers(nseg, stride, seg)
    host = torch.from_numpy(data.copy())
    stage = torch.zeros(nseg * seg, dtype=torch.uint8, device="cuda")
    eng.compress_host_into(codec(w), host, n, seg, stage, buf.slab.ptr, stride, buf.sizes.ptr)
    eng.sync()
    buf.check_streams(streams)
    d_ptrs = dev(np.array([buf.slab.ptr + i * stride for i in range(nseg)], np.int64))
    back = torch.full((nseg * seg,), G.GUARD_BYTE, dtype=torch.uint8)
    eng.decompress_host_into(codec(w), d_ptrs, buf.sizes.ptr, nseg, seg, stage, back, buf.prod.ptr)
    eng.sync()
    assert np.array_equal(back.numpy()[:n], data)
    assert buf.prod.values().tolist() == [min(seg, n - i * seg) for i in range(nseg)]


# ---- hostile streams ----------------------------------------------------------------------------
# (the decoder's reads are bounded by csize and its writes by L by construction: the sizes are
# checked before the bitmaps, the fields and the states are read, a plane's frequencies before its
# slots are marked, the word ring is filled below nw alone, and an output index is below L)

def base_streams(w, seg):
    """a planes stream with 4 pad bits in a field and a length that ends inside a step, one of
    plane shapes that fills the segment, a planes form no encoder writes (larger than 4 + L) and
    a stored one"""
    out = [C.example(w, seg - 37)[0]]
    (s,) = M.encode(C.plane_shapes(seg, w, seg), seg, w)
    assert s[0] == planes(w)
    out.append(s)
    data = C.rnd(300, seg)
    s = M.planes_form(data, w)
    assert len(s) > 4 + 300 and M.decode(s, seg, w) == data.tobytes()
    out.append(s)
    (s,) = M.encode(C.rnd(seg - 3, seg + 1), seg, w)
    assert s[0] == stored(w)
    out.append(s)
    return out


@pytest.mark.parametrize("w", WIDTHS)
def test_hostile_streams_get_the_model_verdict(eng, w):
    """every mutant is accepted with the model's bytes or rejected with SEGMENT_ERROR, nothing
    outside a segment's own L output bytes is written (a reject that rANS's own check finds comes
    after part of that range was written), the sync of its queue pair reports IOError exactly
    once, a good stream decodes on the other queue pair at the same time, and the engine works
    afterwards"""
    import bitar_amd as B
    seg = 4096
    q0, q1 = eng.queue_pair_stream(0), eng.queue_pair_stream(1)
    total = 0
    for base in base_streams(w, seg):
        muts = C.mutants(base, w)
        nseg = len(muts)
        total += nseg
        stride = (max(len(t) for t, _ in muts) + 3 + 255) & ~255
        slab = np.full((nseg, stride), 0x5A, np.uint8)
        for i, (t, _) in enumerate(muts):
            slab[i, :len(t)] = np.frombuffer(t, np.uint8)
        verdicts = [M.decode(slab[i, :size].tobytes(), seg, w) for i, (_, size) in enumerate(muts)]
        assert verdicts[0] is not None and any(v is None for v in verdicts)
        if not base[0] & 8:  # (accepted with other bytes too)
            assert len({v for v in verdicts if v is not None}) > 1
        d_slab = dev(slab.reshape(-1))
        d_sizes = dev(np.array([size for _, size in muts], np.int32))
        out = G.GuardedBytes(nseg * seg, 0, "cuda", "out")
        prod = G.GuardedWords(nseg, "cuda", "produced")
        g_out = G.GuardedBytes(seg, 0, "cuda", "the good stream's out")
        g_prod = G.GuardedWords(1, "cuda", "the good stream's produced")
        torch.cuda.synchronize()  # (the buffers were filled on torch's stream)
        eng.decompress_slab_into(codec(w), d_slab, stride, d_sizes, nseg, seg, out.ptr, prod.ptr,
                                 capacity=nseg * seg, stream=q0)
        eng.decompress_slab_into(codec(w), d_slab, stride, d_sizes, 1, seg, g_out.ptr, g_prod.ptr,
                                 capacity=seg, stream=q1)
        eng.sync(stream=q1)  # the good stream on the other queue pair: nothing to report
        with pytest.raises(B.BitarError) as e:
            eng.sync(stream=q0)
        assert e.value.code == -5
        eng.sync(stream=q0)  # reported once
        n0 = len(verdicts[0])
        g_out.check()
        g_prod.check()
        assert g_prod.values().tolist() == [n0]
        assert g_out.payload()[:n0].tobytes() == verdicts[0]
        g_out.check_fill(n0, seg, "the good segment past its length")
        prod.check()
        assert prod.values().tolist() == [ERR if v is None else len(v) for v in verdicts]
        whole = out.host()
        out.check(whole)
        host = out.payload(whole)
        for i, v in enumerate(verdicts):
            if v is None:  # at most the L bytes the header names were written
                L = 1 + int(slab[i, 2]) + (int(slab[i, 3]) << 8) if muts[i][1] >= 4 else 0
                out.check_fill(i * seg + min(L, seg), (i + 1) * seg, f"rejected segment {i}", whole)
            else:
                assert host[i * seg:i * seg + len(v)].tobytes() == v, i
                out.check_fill(i * seg + len(v), (i + 1) * seg, f"segment {i} past its length", whole)
        # a stream of this width under the other widths' ids: rejected, its output untouched
        for other in WIDTHS:
            if other == w:
                continue
            o_out = G.GuardedBytes(seg, 0, "cuda", "out")
            o_prod = G.GuardedWords(1, "cuda", "produced")
            torch.cuda.synchronize()
            eng.decompress_slab_into(codec(other), d_slab, stride, d_sizes, 1, seg, o_out.ptr,
                                     o_prod.ptr, capacity=seg, stream=q0)
            with pytest.raises(B.BitarError):
                eng.sync(stream=q0)
            assert o_prod.values().tolist() == [ERR]
            o_out.check()
            o_out.check_fill(0, seg, "the output of a stream of another width")
        # the engine works afterwards
        eng.decompress_slab_into(codec(w), d_slab, stride, d_sizes, 1, seg, g_out.ptr, g_prod.ptr,
                                 capacity=seg)
        eng.sync()
        assert g_out.payload()[:n0].tobytes() == verdicts[0]
    assert 300 < total < 2500


def test_compress_bits_refuses_ransplane(eng):
    import bitar_amd as B
    src = dev(C.mixed(8192, 4, 1))
    buf = Buffers(2, 4352, 4096)
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(B.BitarError) as e:
        eng.compress_bits_into(codec(4), src, 4096, buf.slab.ptr, 4352, buf.sizes.ptr, bits)
    assert e.value.code == -4
    eng.sync()
    buf.slab.check()
    buf.slab.check_fill(0, buf.slab.n, "the slab of a refused call")
