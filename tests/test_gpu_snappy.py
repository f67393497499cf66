"""GPU tests of the Snappy codec (csrc/snappy.hip) through the C ABI: a compress writes the
model's streams (tests/snappy_model.py: the oracle's LZ4 block of each segment re-emitted as
Snappy elements) byte for byte, stock Snappy (pyarrow) reads them, the decoder returns the input
from them and from stock streams, and on hand-built and mutated streams its verdict and bytes
are the model's -- with guards (tests/gpu_canary.py) around every buffer a call writes.

Shapes: segments of 65536, 59460 (the reference's), 4099 and 2561 (odd, just past the ring and
the distance cap), 255, 65, 13 (the parse's shortest segment with a window) and 1, each call with
a short last segment; inputs and outputs at address residues 0, 1, 5 and 15.  The compressor takes
another path for a literal run above 256 bytes, for one below its input ring and for a match
above 64 bytes; the decoder for a literal above 64 bytes, from 1 KiB, for an offset past 3952 and
in a stream's last 144 bytes."""
import numpy as np
import pytest

import gpu_canary as G
import oracle_lib as O
import snappy_cases as C
import snappy_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")

KINDS = (0, 1, 2, 3, 5, 6)
SEGS = (65536, 59460, 4099, 2561, 255, 65, 13, 1)
RESIDUES = (0, 1, 5, 15)
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
    return B.CODEC_SNAPPY


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def compress_guarded(eng, data, seg, residue=0):
    """one compress into a guarded slab -> (streams, slab, sizes): the guards and every entry
    checked, the streams as bytes"""
    import bitar_amd as B
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec(), seg)
    src = G.GuardedBytes(n, residue, "cuda", "input")
    src.load(data)
    slab = G.GuardedBytes(nseg * stride, 0, "cuda", "slab")
    sizes = G.GuardedWords(nseg, "cuda", "sizes")
    eng.compress_into(codec(), src.ptr, seg, slab.ptr, stride, sizes.ptr, n=n)
    eng.sync()
    slab.check()
    sizes.check()
    assert np.array_equal(src.payload(), data)
    got = sizes.values().tolist()
    body = slab.payload()
    assert all(0 < g <= stride for g in got), got[:8]
    return [body[i * stride:i * stride + g].tobytes() for i, g in enumerate(got)], slab, sizes


def decode_guarded(eng, streams, seg, residue=0, spacer=True):
    """the streams through bitar_hip_decompress_slab into a guarded output at `residue`, a
    spacer segment nothing may write after every segment -> (produced, [segment bytes]); the
    error word is read by the caller's sync"""
    nseg = len(streams)
    k = 2 if spacer else 1
    stride = (max(len(s) for s in streams) + 16 + 255) & ~255
    slab = np.full((k * nseg, stride), 0x5A, np.uint8)
    sizes = np.zeros(k * nseg, np.uint32)
    for i, s in enumerate(streams):
        slab[k * i, :len(s)] = np.frombuffer(s, np.uint8)
        sizes[k * i] = len(s)
    out = G.GuardedBytes(k * nseg * seg, residue, "cuda", "output")
    prod = G.GuardedWords(k * nseg, "cuda", "produced")
    state = (out, prod, k, nseg, seg)
    d_slab, d_sizes = dev(slab.reshape(-1)), dev(sizes.view(np.int32))
    # (a spacer is an empty stream: rejected, and its output range must stay untouched)
    eng.decompress_slab_into(codec(), d_slab, stride, d_sizes, k * nseg, seg, out.ptr, prod.ptr,
                             capacity=k * nseg * seg)
    return state


def decoded(state):
    out, prod, k, nseg, seg = state
    out.check()
    prod.check()
    got = prod.values()
    body = out.payload()
    res = []
    for i in range(nseg):
        p = int(got[k * i])
        res.append(None if p == ERR else body[k * i * seg:k * i * seg + p].tobytes())
        if p != ERR:
            out.check_fill(k * i * seg + p, (k * i + 1) * seg, f"segment {i} past its bytes")
        if k == 2:
            assert got[k * i + 1] == ERR
            out.check_fill((k * i + 1) * seg, (k * i + 2) * seg, f"spacer after segment {i}")
    return res


def sync_expect(eng, failed):
    import bitar_amd as B
    if failed:
        with pytest.raises(B.BitarError) as e:
            eng.sync()
        assert e.value.code == -5
    else:
        eng.sync()


def round_trip(eng, data, seg, residue=0):
    """compress against the model, pyarrow on every GPU stream, decode back with guards"""
    want = C.model_streams(data, seg)
    got, _, _ = compress_guarded(eng, data, seg, residue)
    assert [len(s) for s in got] == [len(s) for s in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, next(k for k in range(len(w)) if g[k] != w[k]))
    parts = [p.tobytes() for p in M.segments(data, seg)]
    for g, p in zip(got, parts):
        assert C.pa_decode(g, len(p)) == p
    state = decode_guarded(eng, got, seg, residue)
    sync_expect(eng, True)  # (the spacers are rejected streams)
    assert decoded(state) == parts
    return got


def sized(seg, kind):
    n = 4 * seg + min(1234, max(seg // 3, 1)) if seg >= 2561 else 33 * seg + max(seg // 2, 0)
    return O.fill(kind, C.SEED + seg, n)


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("kind", KINDS)
def test_compress_is_the_model_and_round_trips(eng, kind, seg):
    round_trip(eng, sized(seg, kind), seg, RESIDUES[(kind + seg) % 4])


def special_inputs():
    run = np.full(65536, 0x41, np.uint8)
    period3 = np.tile(np.array([1, 2, 3], np.uint8), 65536 // 3 + 1)[:65536]
    long_literals = np.concatenate([rnd(700, 1), np.zeros(300, np.uint8), rnd(70, 2),
                                    np.zeros(70, np.uint8), rnd(300, 3), np.zeros(130, np.uint8)])
    return [("run", run), ("period3", period3), ("literals", long_literals)]


def edge_inputs():
    """random segments with one run of a byte -> [(data, stored?)]: at the end, 100 bytes (the
    parse steps over incompressible input four positions at a time and walks past it: stored)
    and 200 (found); at the start, 5 bytes (a 4-byte match: one byte below the stored form) and
    4 (no match)"""
    out = []
    for at_end, r, stored in ((True, 100, True), (True, 200, False), (False, 5, False),
                              (False, 4, True)):
        e = rnd(65536, 5)
        e[(65536 - r if at_end else 0):(65536 if at_end else r)] = 0x20
        out.append((e, stored))
    return out


def test_runs_periods_and_the_stored_edge(eng):
    seen = set()
    for name, data in special_inputs():
        streams = round_trip(eng, data, 65536)
        seen |= C.census(streams)
        els = M.elements(streams[0])
        if name == "run":
            # one match of 65530 bytes at offset 1: 64-byte copies, then the LZ4 end rule's tail
            assert [e[:3] for e in els[:3]] == [(M.LITERAL, 1, 0), (M.COPY2, 64, 1),
                                                (M.COPY2, 64, 1)]
            assert sum(1 for e in els if e[0] == M.COPY2 and e[1] == 64) >= 1000
        if name == "period3":
            assert {e[2] for e in els if e[0] != M.LITERAL} == {3}
    for data, stored in edge_inputs():
        (s,) = round_trip(eng, data, 65536)
        assert (s == M.stored(data.tobytes())) == stored
        assert stored or len(s) < 65542
        seen |= C.census([s])
    for kind in (1, 5):
        seen |= C.census(round_trip(eng, O.fill(kind, 3, 2 * 65536), 65536))
    assert seen >= {"literal inline", "literal 1-byte length", "literal 2-byte length", "copy-1",
                    "copy-2", "split match", "stored"}, seen
    assert "copy-4" not in seen


def test_every_input_and_output_residue(eng):
    for residue in RESIDUES:
        for seg in (4099, 255):
            round_trip(eng, sized(seg, 1 if residue & 1 else 6), seg, residue)


def test_empty_input_launches_nothing(eng):
    slab = G.GuardedBytes(4352, 0, "cuda", "slab")
    sizes = G.GuardedWords(1, "cuda", "sizes")
    out = G.GuardedBytes(4096, 0, "cuda", "output")
    eng.compress_into(codec(), slab.ptr, 4096, slab.ptr, 4352, sizes.ptr, n=0)
    eng.decompress_slab_into(codec(), slab.ptr, 4352, sizes.ptr, 0, 4096, out.ptr, sizes.ptr,
                             capacity=0)
    eng.sync()
    for b in (slab, out):
        b.check()
        b.check_fill(0, b.n, "untouched payload")
    assert sizes.values().tolist() == [G.FILL_WORD]
    assert M.from_lz4_block(b"", b"\x00") == b"\x00"


def stock_segments():
    """[(segment bytes, pyarrow's stream)]: the oracle's kinds, and a 20 KiB random block three
    times over (copies from 20480 back, far past the decoder's 4 KiB ring)"""
    out = []
    for kind in KINDS:
        data = O.fill(kind, C.SEED, 2 * 65536 + 999)
        out += [(p.tobytes(), C.pa_encode(p.tobytes())) for p in M.segments(data, 65536)]
    block = rnd(20480, 9).tobytes()
    far = (block * 3)[:61440]
    out.append((far, C.pa_encode(far)))
    for n in (1, 13, 65, 4099):
        p = O.fill(1, n, n).tobytes()
        out.append((p, C.pa_encode(p)))
    return out


def test_stock_streams_decode(eng):
    segs = stock_segments()
    far = M.elements(segs[3 * len(KINDS)][1])
    assert max(e[2] for e in far) > 4096 and any(e[2] == 20480 for e in far)
    seen = C.census([s for _, s in segs])
    assert {"literal inline", "literal 2-byte length", "copy-1", "copy-2"} <= seen
    for residue in (0, 5):
        state = decode_guarded(eng, [s for _, s in segs], 65536, residue)
        sync_expect(eng, True)
        assert decoded(state) == [p for p, _ in segs]


def test_hand_built_streams(eng):
    cases = C.hand_built()
    for cap in (64, 512, 8192):
        group = [(s, w) for s, c, w in cases if c == cap]
        assert any(w is None for _, w in group) and any(w for _, w in group)
        state = decode_guarded(eng, [s for s, _ in group], cap, 1)
        sync_expect(eng, True)
        got = decoded(state)
        for (s, w), g in zip(group, got):
            assert g == w, s[:16].hex()
    # accepted streams alone raise nothing
    good = [(s, w) for s, c, w in cases if c == 64 and w]
    state = decode_guarded(eng, [s for s, _ in good], 64, 15, spacer=False)
    eng.sync()
    assert decoded(state) == [w for _, w in good]


@pytest.mark.parametrize("seg", (4099, 65536))
def test_mutation_corpus_gets_the_model_verdict(eng, seg):
    """the CPU test's corpus (there the model's verdicts are pyarrow's): per segment the model's
    verdict and bytes, good segments between the mutants unaffected, and the error on the stream
    that decoded them only"""
    import bitar_amd as B
    muts = [s for s, c in C.mutation_corpus() if c == seg]
    assert len(muts) == 210
    good = [C.base_stream(k, seg) for k in (1, 5, 6)]
    streams, want = [], []
    for i, s in enumerate(muts):
        streams.append(s)
        want.append(M.decode(s, seg))
        if i % 10 == 0:
            streams.append(good[i // 10 % 3][1])
            want.append(good[i // 10 % 3][0])
    assert sum(w is None for w in want) >= 50
    nseg = len(streams)
    stride = (max(len(s) for s in streams) + 16 + 255) & ~255
    slab = np.full((nseg, stride), 0x5A, np.uint8)
    for i, s in enumerate(streams):
        slab[i, :len(s)] = np.frombuffer(s, np.uint8)
    d_slab = dev(slab.reshape(-1))
    d_sizes = dev(np.array([len(s) for s in streams], np.int32))
    out = G.GuardedBytes(nseg * seg, 5, "cuda", "output")
    prod = G.GuardedWords(nseg, "cuda", "produced")
    q0, q1 = eng.queue_pair_stream(0), eng.queue_pair_stream(1)
    # a good call on the other queue pair: its sync reports nothing
    gs = good[0][1]
    g_slab = dev(np.frombuffer(gs + bytes(-len(gs) % 16 + 16), np.uint8))
    g_sizes = dev(np.array([len(gs)], np.int32))
    g_out = G.GuardedBytes(seg, 0, "cuda", "good output")
    g_prod = G.GuardedWords(1, "cuda", "good produced")
    torch.cuda.synchronize()  # (the buffers were filled on torch's stream)
    eng.decompress_slab_into(codec(), d_slab, stride, d_sizes, nseg, seg, out.ptr, prod.ptr,
                             capacity=nseg * seg, stream=q0)
    eng.decompress_slab_into(codec(), g_slab, g_slab.numel(), g_sizes, 1, seg, g_out.ptr,
                             g_prod.ptr, capacity=seg, stream=q1)
    eng.sync(stream=q1)
    with pytest.raises(B.BitarError) as e:
        eng.sync(stream=q0)
    assert e.value.code == -5
    eng.sync(stream=q0)  # reported once
    assert g_prod.values().tolist() == [seg] and g_out.payload().tobytes() == good[0][0]
    g_out.check()
    out.check()
    prod.check()
    got = prod.values()
    body = out.payload()
    for i, w in enumerate(want):
        if w is None:
            assert got[i] == ERR, i
        else:
            assert got[i] == len(w) and body[i * seg:i * seg + len(w)].tobytes() == w, i
            out.check_fill(i * seg + len(w), (i + 1) * seg, f"segment {i} past its bytes")


def test_scattered_pointer_list_and_host_paths(eng):
    import bitar_amd as B
    seg = 59460
    data = np.concatenate([O.fill(1, 4, 2 * seg), rnd(seg, 8), O.fill(6, 4, 777)])
    n = data.size
    nseg = (n + seg - 1) // seg
    stride = B.slot_size(codec(), seg)
    want = C.model_streams(data, seg)
    assert "stored" in C.census(want[2:3]) and "stored" not in C.census(want[:2])
    src = dev(data)
    sizes = G.GuardedWords(nseg, "cuda", "sizes")

    # scattered: slot i of the call is slot perm[i], each slot with guards of its own
    slots = G.GuardedSlots(nseg, stride, "cuda", "scattered slots")
    perm = [2, 0, 3, 1]
    ptrs = slots.ptr_tensor()[perm]
    B.check(B.lib().bitar_hip_compress_scattered(eng.ctx, eng._stream(None), codec(),
                                                 src.data_ptr(), n, seg, ptrs.data_ptr(), stride,
                                                 sizes.ptr))
    eng.sync()
    slots.check()
    sizes.check()
    assert sizes.values().tolist() == [len(s) for s in want]
    for i, p in enumerate(perm):
        assert slots.slot(p)[:len(want[i])].tobytes() == want[i], i

    # pointer list: stream i at an odd address
    room = (max(len(s) for s in want) + 32) & ~15
    packed = np.full(nseg * room + 16, 0x5A, np.uint8)
    offs = []
    for i, s in enumerate(want):
        o = i * room + 2 * i + 1
        packed[o:o + len(s)] = np.frombuffer(s, np.uint8)
        offs.append(o)
    d_packed = dev(packed)
    d_ptrs = dev(np.array(offs, np.int64) + d_packed.data_ptr())
    d_sizes = dev(np.array([len(s) for s in want], np.int32))
    out = G.GuardedBytes(nseg * seg, 15, "cuda", "output")
    prod = G.GuardedWords(nseg, "cuda", "produced")
    eng.decompress_into(codec(), d_ptrs, d_sizes, nseg, seg, out.ptr, prod.ptr, capacity=nseg * seg)
    eng.sync()
    out.check()
    prod.check()
    assert prod.values().tolist() == [min(seg, n - i * seg) for i in range(nseg)]
    assert np.array_equal(out.payload()[:n], data)

    # host-overlapped: compress from host memory, decompress into host memory
    slab = G.GuardedBytes(nseg * stride, 0, "cuda", "slab")
    sizes = G.GuardedWords(nseg, "cuda", "sizes")
    stage = torch.zeros(nseg * seg, dtype=torch.uint8, device="cuda")
    host = torch.from_numpy(data.copy())
    eng.compress_host_into(codec(), host, n, seg, stage, slab.ptr, stride, sizes.ptr)
    eng.sync()
    slab.check()
    sizes.check()
    assert sizes.values().tolist() == [len(s) for s in want]
    body = slab.payload()
    for i, s in enumerate(want):
        assert body[i * stride:i * stride + len(s)].tobytes() == s
    d_ptrs = dev(np.array([slab.ptr + i * stride for i in range(nseg)], np.int64))
    back = torch.full((nseg * seg,), 0x3C, dtype=torch.uint8)
    prod = G.GuardedWords(nseg, "cuda", "produced")
    eng.decompress_host_into(codec(), d_ptrs, sizes.ptr, nseg, seg, stage, back, prod.ptr)
    eng.sync()
    prod.check()
    assert np.array_equal(back.numpy()[:n], data)


def test_plain_and_cost_ordered_dispatch_agree():
    """4001 segments of 512 bytes (the ordered dispatch starts at 2048 segments): a context with
    plain order and one with cost order write the same slab and sizes and decode the same"""
    import bitar_amd as B
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    seg = 512
    data = np.concatenate([O.fill(1, 5, 1000 * seg), rnd(1000 * seg, 3), O.fill(6, 5, 2000 * seg),
                           O.fill(5, 5, 300)])
    src = dev(data)
    results = []
    for flags in (B.FLAG_PLAIN_ORDER, 0):
        e = B.Engine(0, flags=flags)
        slab, stride, sizes = e.compress(codec(), src, seg)
        slab.fill_(0)
        e.compress_into(codec(), src, seg, slab, stride, sizes)
        out, prod = e.decompress(codec(), slab, stride, sizes, seg)
        e.sync()
        results.append((slab.cpu().numpy(), sizes.cpu().numpy(), out.cpu().numpy()[:data.size],
                        prod.cpu().numpy()))
        e.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    assert np.array_equal(results[0][2], data)
    sizes = results[0][1]
    want = C.model_streams(data[:64 * seg], seg)
    assert sizes[:64].tolist() == [len(s) for s in want]
    assert sizes[1000:2000].min() == seg + 5  # the stored form: 2 + 3 + 512


def test_seventy_thousand_tiny_segments(eng):
    """one call of 70 000 segments of 16 bytes, past the 32768 and 65536 segment borders"""
    seg, nseg = 16, 70000
    data = O.fill(3, 1, nseg * seg).copy()
    data[::3 * seg] = np.arange(data[::3 * seg].size, dtype=np.uint8)  # (not all alike)
    noise = rnd(nseg * seg, 2)
    data[seg * 40000:] = noise[seg * 40000:]
    slab, stride, sizes = eng.compress(codec(), dev(data), seg)
    out, prod = eng.decompress(codec(), slab, stride, sizes, seg)
    eng.sync()
    assert np.array_equal(out.cpu().numpy(), data)
    assert bool((prod == seg).all())
    got = sizes.cpu().numpy()
    host = slab.cpu().numpy().reshape(nseg, stride)
    want = C.model_streams(data, seg)
    assert got.tolist() == [len(s) for s in want]
    for i in list(range(0, nseg, 97)) + list(range(32760, 32776)) + list(range(65528, 65544)):
        assert host[i, :len(want[i])].tobytes() == want[i], i
    assert got[:40000].min() == 11 and got[40000:].min() == seg + 2  # coded; the stored form


def test_compress_bits_refuses_snappy(eng):
    import bitar_amd as B
    src = dev(rnd(8192, 1))
    slab = G.GuardedBytes(2 * 4352, 0, "cuda", "slab")
    sizes = G.GuardedWords(2, "cuda", "sizes")
    bits = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(B.BitarError) as e:
        eng.compress_bits_into(codec(), src, 4096, slab.ptr, 4352, sizes.ptr, bits)
    assert e.value.code == -4
    eng.sync()
    slab.check_fill(0, slab.n, "untouched slab")
