"""GPU tests of the SYMTAB codec (csrc/symtab.hip) through the C ABI: the slots and sizes of a
compress equal the Python model's streams (symtab_model.py) byte for byte, the decoder returns
the input, and on mutated streams its verdict is the model's; every buffer a call writes is a
guarded view (gpu_canary.py), and what a stream does not cover of its slot keeps the fill byte.

Shapes: segments of 1, 7, 8, 9, 255, 256, 257 and 1023 bytes (below, at and above one symbol and
one sample chunk), 16384 and 16385 (the two sides of the sample switch), 59460 and 65536, each
with a short last segment; 64, 512 and 513 codes and their neighbours (one step and one group of
the decoder)."""
import numpy as np
import pytest

import gpu_canary as G
import symtab_cases as C
import symtab_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR = 0xFFFFFFFF


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
    return B.CODEC_SYMTAB


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


class Buffers:
    """guarded device buffers of one compress + decompress"""

    def __init__(self, nseg, stride, seg, residue=0):
        self.nseg, self.stride, self.seg = nseg, stride, seg
        self.slab = G.GuardedBytes(nseg * stride, 0, "cuda", "slab")
        self.sizes = G.GuardedWords(nseg, "cuda", "sizes")
        self.out = G.GuardedBytes(nseg * seg, residue, "cuda", "out")
        self.prod = G.GuardedWords(nseg, "cuda", "produced")

    def check_streams(self, streams):
        """slots and sizes against the model's streams; what a stream does not cover of its slot
        still holds the fill byte"""
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
            assert np.all(slot[want.size:] == G.FILL), i

    def check_output(self, data):
        n = data.size
        self.prod.check()
        want = [min(self.seg, n - i * self.seg) for i in range(self.nseg)]
        assert self.prod.values().tolist() == want
        whole = self.out.host()
        self.out.check(whole)
        out = self.out.payload(whole)
        assert np.array_equal(out[:n], data), np.flatnonzero(out[:n] != data)[:8]
        assert np.all(out[n:] == G.FILL)


def check_case(eng, seg, data, in_off=0, streams=None):
    import bitar_amd as B
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec(), seg)
    src = G.GuardedBytes(n, in_off, "cuda", "input")
    src.load(data)
    buf = Buffers(nseg, stride, seg, residue=(5 * in_off) % 16)
    eng.compress_into(codec(), src.ptr, seg, buf.slab.ptr, stride, buf.sizes.ptr, n=n)
    eng.decompress_slab_into(codec(), buf.slab.ptr, stride, buf.sizes.ptr, nseg, seg, buf.out.ptr,
                             buf.prod.ptr, capacity=nseg * seg)
    eng.sync()
    streams = M.encode(data, seg) if streams is None else streams
    buf.check_streams(streams)
    buf.check_output(data)
    src.check()
    return streams


@pytest.mark.parametrize("L", (1, 7, 8, 9, 255, 256, 257, 1023, 16384, 16385, 59460, 65536))
def test_exact_bytes_and_round_trip(eng, L):
    """text, and one line over and over: two whole segments and a short last one"""
    tail = 0 if L == 1 else min(L - 1, 777)
    streams = check_case(eng, L, C.text(2 * L + tail, L))
    if L >= 16384:
        assert all(s[0] == 0xC0 for s in streams[:2])
    if L <= 9:
        assert all(s[0] == 0xC1 for s in streams)
    if L < 16384:
        streams = check_case(eng, L, C.phrases(2 * L + tail, L))
        assert all(s[0] == (0xC0 if L >= 255 else 0xC1) for s in streams[:2])


def test_worked_examples(eng):
    (s,) = check_case(eng, 4096, np.frombuffer(b"abababab", np.uint8).copy())
    assert s == bytes.fromhex("c1000700") + b"abababab"
    (s,) = check_case(eng, 4096, np.frombuffer(b"ab" * 64, np.uint8).copy())
    assert s == bytes.fromhex("c0017f00100008") + b"abababab" + bytes(16)
    a = np.full(16390, 0x61, np.uint8)
    a[300] = 0xFF
    (s,) = check_case(eng, 65536, a)
    assert s == bytes.fromhex("c0020540060808066161616161616161616161616161") + \
        bytes(37) + b"\xff" * 5 + bytes(2011) + b"\xff" + bytes.fromhex("61616161ff61")


@pytest.mark.parametrize("name", ("constant", "alphabet64", "all_bytes", "symbol_at_ends", "noise",
                                  "collide", "equal_gains", "names"))
def test_inputs(eng, name):
    if name == "constant":
        for L in (4096, 65536):
            (s,) = check_case(eng, 65536, np.full(L, 0x41, np.uint8))
            assert s[0] == 0xC0 and len(s) < 32 + L // 8
    elif name == "alphabet64":
        for seg in (4096, 20000):
            streams = check_case(eng, seg, C.alphabet64(2 * seg + 100, seg))
            # (6 bits a byte: at 4096 bytes the table costs more than it saves)
            want = (0xC0, 255) if seg == 20000 else (0xC1, 0)
            assert all((s[0], s[1]) == want for s in streams[:2])
    elif name == "all_bytes":
        for seg in (4096, 65536):
            streams = check_case(eng, seg, C.all_bytes(seg + 1000, seg))
            lens, syms, codes, lits = M.parts_of(streams[0])
            assert streams[0][0] == 0xC0 and len(lits) > 16
            assert any(0 in s[1:] for s in syms) and any(s[0] == 0xFF for s in syms)
    elif name == "symbol_at_ends":
        for L in (256, 512, 1000, 1027, 16385 + 7):
            (s,) = check_case(eng, 65536, C.symbol_at_ends(L))
            lens, syms, codes, lits = M.parts_of(s)
            assert b"ABCDEFGH" in syms
            assert L % 8 or syms[codes[-1]] == b"ABCDEFGH"
    elif name == "noise":
        streams = check_case(eng, 65536, C.rnd(65536 + 100, 3))
        assert all(s[0] == 0xC1 for s in streams)
        streams = check_case(eng, 59460, C.rnd(59460 + 4093, 4), in_off=3)
        assert all(s[0] == 0xC1 for s in streams)
    elif name == "collide":
        data, groups = C.collide()
        check_case(eng, 4096, data)
    elif name == "equal_gains":
        check_case(eng, 8192, C.equal_gains(8192 + 300))
    else:
        streams = check_case(eng, 65536, C.names(65536 + 5000))
        assert all(s[0] == 0xC0 for s in streams)


@pytest.mark.parametrize("nc", (63, 64, 65, 511, 512, 513, 1024))
def test_code_counts_around_the_decoder_step(eng, nc):
    """nc codes of the 8-byte symbol, and the same with a one-byte symbol in front"""
    (s,) = check_case(eng, 65536, np.full(8 * nc, 0x41, np.uint8))
    assert s[0] == 0xC0 and (s[4] | s[5] << 8) == nc
    a = np.full(8 * (nc - 1) + 1, 0x41, np.uint8)
    a[0] = 0xFF
    (s,) = check_case(eng, 65536, a)
    assert s[0] == 0xC0 and (s[4] | s[5] << 8) == nc


def test_input_at_every_alignment(eng):
    for seg in (1023, 4100):
        data = C.mixed(3 * seg + 65, seg)
        streams = M.encode(data, seg)
        assert {s[0] for s in streams} == {0xC0, 0xC1}
        for in_off in range(16):
            check_case(eng, seg, data, in_off=in_off, streams=streams)


def test_mixed_segments_in_one_call(eng):
    seg = 4096
    data = np.concatenate([C.text(seg, 1), C.rnd(seg, 2), C.names(seg, 3), C.rnd(seg, 4),
                           np.full(seg, 1, np.uint8), C.text(300, 5), C.rnd(7, 6)])
    streams = check_case(eng, seg, data)
    assert [s[0] & 1 for s in streams] == [0, 1, 0, 1, 0, 1]


def test_empty_input_launches_nothing(eng):
    buf = Buffers(1, 4352, 4096)
    src = torch.zeros(256, dtype=torch.uint8, device="cuda")
    eng.compress_into(codec(), src, 4096, buf.slab.ptr, 4352, buf.sizes.ptr, n=0)
    eng.decompress_slab_into(codec(), buf.slab.ptr, 4352, buf.sizes.ptr, 0, 4096, buf.out.ptr,
                             buf.prod.ptr, capacity=0)
    eng.sync()
    for b in (buf.slab, buf.out):
        b.check()
        b.check_fill(0, b.n, "payload")
    for w in (buf.sizes, buf.prod):
        w.check()
        assert np.all(w.values() == G.FILL_WORD)


def test_scattered_pointer_list_and_host_paths(eng):
    """bitar_hip_compress_scattered, bitar_hip_decompress with the streams at odd addresses, and
    the host-overlapped pair"""
    import bitar_amd as B
    seg = 20000
    data = C.mixed(3 * seg + 65, 77)
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec(), seg)
    streams = M.encode(data, seg)
    assert 0xC0 in {s[0] for s in streams}
    src = dev(data)

    # scattered: slot i of the call is slot perm[i] of a set of slots with guards between them
    slots = G.GuardedSlots(nseg, stride, "cuda", "scattered slots")
    sizes = G.GuardedWords(nseg, "cuda", "sizes")
    perm = [2, 0, 3, 1]
    assert nseg == len(perm)
    dsts = torch.tensor([slots.ptrs[p] for p in perm], dtype=torch.int64).cuda()
    B.check(B.lib().bitar_hip_compress_scattered(eng.ctx, eng._stream(None), codec(),
                                                 src.data_ptr(), n, seg, dsts.data_ptr(), stride,
                                                 sizes.ptr))
    eng.sync()
    sizes.check()
    assert sizes.values().tolist() == [len(s) for s in streams]
    whole = slots.host()
    slots.check(whole)
    for i, p in enumerate(perm):
        slot = slots.slot(p, whole)
        assert slot[:len(streams[i])].tobytes() == streams[i], i
        assert np.all(slot[len(streams[i]):] == G.FILL), i

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
    buf = Buffers(nseg, stride, seg, residue=7)
    eng.decompress_into(codec(), d_ptrs, d_sizes, nseg, seg, buf.out.ptr, buf.prod.ptr,
                        capacity=nseg * seg)
    eng.sync()
    buf.check_output(data)

    # host-overlapped: compress from host memory, decompress into host memory
    buf = Buffers(nseg, stride, seg)
    host = torch.from_numpy(data.copy())
    stage = torch.zeros(nseg * seg, dtype=torch.uint8, device="cuda")
    eng.compress_host_into(codec(), host, n, seg, stage, buf.slab.ptr, stride, buf.sizes.ptr)
    eng.sync()
    buf.check_streams(streams)
    d_ptrs = dev(np.array([buf.slab.ptr + i * stride for i in range(nseg)], np.int64))
    back = torch.full((nseg * seg,), G.FILL, dtype=torch.uint8)
    eng.decompress_host_into(codec(), d_ptrs, buf.sizes.ptr, nseg, seg, stage, back, buf.prod.ptr)
    eng.sync()
    assert np.array_equal(back.numpy()[:n], data)
    buf.prod.check()
    assert buf.prod.values().tolist() == [min(seg, n - i * seg) for i in range(nseg)]


# ---- hostile streams ----------------------------------------------------------------------------

def base_streams(seg):
    """coded streams of text, of all byte values (escapes, 255 symbols), of a constant with
    one other byte; a coded form no encoder writes (larger than 4 + L); a stored one"""
    out = []
    a = np.full(seg - 5, 0x41, np.uint8)
    a[seg // 2] = 0xFF
    for data in (C.text(seg, seg), C.all_bytes(seg - 37, seg), a):
        s = M.coded_form(data)  # (whatever its size: at 1000 bytes the first two are stored)
        assert s[0] == 0xC0 and M.decode(s, seg) == data.tobytes()
        out.append(s)
    assert M.encode(a, seg) == [out[-1]] and len(M.parts_of(out[1])[3]) > 2
    data = C.rnd(300, seg)
    s = M.coded_form(data)
    assert len(s) > 4 + 300 and M.decode(s, seg) == data.tobytes()
    out.append(s)
    (s,) = M.encode(C.rnd(seg - 3, seg + 1), seg)
    assert s[0] == 0xC1
    out.append(s)
    return out


@pytest.mark.parametrize("seg", (4096, 1000))
def test_hostile_streams_get_the_model_verdict(eng, seg):
    """every mutant is accepted with the model's bytes or rejected with SEGMENT_ERROR, a rejected
    stream writes nothing at all and an accepted one its L bytes alone, the sync of its queue
    pair reports IOError exactly once, a good stream decodes on the other queue pair at the same
    time, and the engine works afterwards"""
    import bitar_amd as B
    q0, q1 = eng.queue_pair_stream(0), eng.queue_pair_stream(1)
    total = 0
    for base in base_streams(seg):
        muts = C.mutants(base)
        nseg = len(muts)
        total += nseg
        stride = (max(len(t) for t, _ in muts) + 1 + 255) & ~255
        slab = np.full((nseg, stride), 0x5A, np.uint8)
        for i, (t, _) in enumerate(muts):
            slab[i, :len(t)] = np.frombuffer(t, np.uint8)
        verdicts = [M.decode(slab[i, :size].tobytes(), seg) for i, (_, size) in enumerate(muts)]
        assert verdicts[0] is not None and any(v is None for v in verdicts)
        if base[0] == 0xC0:  # (accepted with other bytes too)
            assert len({v for v in verdicts if v is not None}) > 1
        d_slab = dev(slab.reshape(-1))
        d_sizes = dev(np.array([size for _, size in muts], np.int32))
        out = G.GuardedBytes(nseg * seg, 3, "cuda", "out")
        prod = G.GuardedWords(nseg, "cuda", "produced")
        g_out = G.GuardedBytes(seg, 9, "cuda", "good out")
        g_prod = G.GuardedWords(1, "cuda", "good produced")
        torch.cuda.synchronize()  # (the buffers were filled on torch's stream)
        eng.decompress_slab_into(codec(), d_slab, stride, d_sizes, nseg, seg, out.ptr, prod.ptr,
                                 capacity=nseg * seg, stream=q0)
        eng.decompress_slab_into(codec(), d_slab, stride, d_sizes, 1, seg, g_out.ptr, g_prod.ptr,
                                 capacity=seg, stream=q1)
        eng.sync(stream=q1)  # the good stream on the other queue pair: nothing to report
        with pytest.raises(B.BitarError) as e:
            eng.sync(stream=q0)
        assert e.value.code == -5
        eng.sync(stream=q0)  # reported once
        g_out.check()
        g_prod.check()
        assert g_prod.values().tolist() == [len(verdicts[0])]
        assert g_out.payload()[:len(verdicts[0])].tobytes() == verdicts[0]
        g_out.check_fill(len(verdicts[0]), seg, "behind the good segment")
        prod.check()
        assert prod.values().tolist() == [ERR if v is None else len(v) for v in verdicts]
        whole = out.host()
        out.check(whole)
        host = out.payload(whole)
        for i, v in enumerate(verdicts):
            seg_out = host[i * seg:(i + 1) * seg]
            k = 0 if v is None else len(v)
            assert seg_out[:k].tobytes() == (v or b""), i
            assert np.all(seg_out[k:] == G.FILL), i
        # the engine works afterwards
        eng.decompress_slab_into(codec(), d_slab, stride, d_sizes, 1, seg, out.ptr, prod.ptr,
                                 capacity=seg)
        eng.sync()
        assert out.payload()[:len(verdicts[0])].tobytes() == verdicts[0]
    assert total >= 1000


def test_compress_bits_refuses_symtab(eng):
    import bitar_amd as B
    src = dev(C.text(8192, 1))
    buf = Buffers(2, 4352, 4096)
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(B.BitarError) as e:
        eng.compress_bits_into(codec(), src, 4096, buf.slab.ptr, 4352, buf.sizes.ptr, bits)
    assert e.value.code == -4
    eng.sync()
    buf.slab.check()
    buf.slab.check_fill(0, buf.slab.n, "slab")
