"""GPU tests of whole-buffer raw Snappy streams through the C ABI (csrc/snappy.hip, DESIGN.md
4.23): bitar_hip_snappy_join writes the model's stream byte for byte, bitar_hip_snappy_split
finds the model's fragment starts, status, rounds and tile walks on the engine's own and on
pyarrow's streams, and bitar_hip_snappy_decompress_joined returns the input -- with guards
(tests/gpu_canary.py) around every buffer a call touches.

Shapes: inputs of 0, 1, 65535, 65536, 65537 and 3 * 65536 + 1 bytes (no, one, two and four
fragments, a 1-byte last one), 4 MiB + 1 for the round trip; streams of T - 1, T, T + 1 and 2T + 1
bytes at the shipped tile T = 4096; an element of every header size beginning in each of a tile's
last 5 bytes; a 64 KiB literal from mid-tile to mid-tile; stored fragments in a row; a stream
that needs one round per tile; every one again with max_rounds = 1 (the serial finish)."""
import functools

import numpy as np
import pytest

import gpu_canary as G
import oracle_lib as O
import snappy_cases as C
import snappy_model as M
import snappy_stream_model as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")

ERR = 0xFFFFFFFF
SIZES = (0, 1, 65535, 65536, 65537, 3 * 65536 + 1)
KINDS = (0, 1, 2, 5, 6)
RESIDUES = (0, 1, 5, 15)
T = S.TILE


@pytest.fixture(scope="module")
def eng():
    import bitar_amd
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = bitar_amd.Engine(0, num_streams=2)
    assert bitar_amd.SNAPPY_BLOCK == S.BLOCK
    assert (bitar_amd.SNAPPY_SPLIT_OK, bitar_amd.SNAPPY_SPLIT_UNSUPPORTED,
            bitar_amd.SNAPPY_SPLIT_INVALID, bitar_amd.SNAPPY_SPLIT_INCOMPLETE) == \
        (S.OK, S.UNSUPPORTED, S.INVALID, S.INCOMPLETE)
    assert bitar_amd.SNAPPY_NO_SERIAL_FINISH == S.NO_SERIAL_FINISH
    yield e
    e.close()


def codec():
    import bitar_amd as B
    return B.CODEC_SNAPPY


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """(input bytes, the model's joined stream, pyarrow's stream)"""
    data = O.fill(kind, C.SEED, n) if n else np.zeros(0, np.uint8)
    own = S.join(C.model_streams(data, S.BLOCK), n)
    return data.tobytes(), own, C.pa_encode(data.tobytes())


class Longs:
    """n uint64 entries with guard words on both sides"""

    def __init__(self, n):
        self.w = G.GuardedWords(2 * n, "cuda", "uint64 entries")
        assert self.w.ptr % 8 == 0
        self.ptr = self.w.ptr

    def values(self):
        self.w.check()
        return self.w.values().copy().view(np.uint64).tolist()


def join(eng, data, capacity=None, sizes_edit=None):
    """compress + join with guards -> (stream bytes or None, offsets, length)"""
    import bitar_amd as B
    n = len(data)
    nseg = S.nfrag(n)
    stride = B.slot_size(codec(), S.BLOCK)
    src = G.GuardedBytes(max(n, 1), 5, "cuda", "input")
    src.load(np.frombuffer(data, np.uint8).copy())
    slab = G.GuardedBytes(max(nseg, 1) * stride, 0, "cuda", "slab")
    sizes = G.GuardedWords(max(nseg, 1), "cuda", "sizes")
    eng.compress_into(codec(), src.ptr, S.BLOCK, slab.ptr, stride, sizes.ptr, n=n)
    if sizes_edit:
        eng.sync()
        v = sizes.values().copy()
        v[sizes_edit[0]] = sizes_edit[1]
        sizes.load(v)
    cap = n + 4 * nseg + 5 if capacity is None else capacity
    joined = G.GuardedBytes(max(cap, 1), 1, "cuda", "joined")
    offsets, length = Longs(nseg + 1), Longs(1)
    eng.snappy_join(slab.ptr, stride, sizes.ptr, n, offsets.ptr, joined.ptr, cap, length.ptr)
    return src, slab, sizes, joined, offsets, length


@pytest.mark.parametrize("n", SIZES)
def test_join_is_the_model(eng, n):
    kind = KINDS[SIZES.index(n) % len(KINDS)]
    data, want, _ = case(kind, n)
    src, slab, sizes, joined, offsets, length = join(eng, data)
    eng.sync()
    for b in (src, slab, sizes, joined):
        b.check()
    (total,) = length.values()
    assert total == len(want)
    assert joined.payload()[:total].tobytes() == want
    joined.check_fill(total, joined.n, "past the stream")
    pre = len(M.varint(n))
    bodies = [len(s) - M.preamble(s)[1] for s in C.model_streams(np.frombuffer(data, np.uint8),
                                                                  S.BLOCK)]
    assert offsets.values() == np.concatenate([[0], np.cumsum(bodies)]).astype(int).tolist()
    assert total == pre + sum(bodies) <= n + 4 * S.nfrag(n) + 5
    # sizes only
    offsets2, length2 = Longs(S.nfrag(n) + 1), Longs(1)
    import bitar_amd as B
    eng.snappy_join(None, B.slot_size(codec(), S.BLOCK), sizes.ptr, n, offsets2.ptr, None, 0,
                    length2.ptr)
    eng.sync()
    assert offsets2.values() == offsets.values() and length2.values() == [total]


def test_join_refusals(eng):
    import bitar_amd as B
    data, want, _ = case(1, 65537)
    # a capacity one byte short: nothing is written, the error is the stream's
    src, slab, sizes, joined, offsets, length = join(eng, data, capacity=len(want) - 1)
    with pytest.raises(B.BitarError) as e:
        eng.sync()
    assert e.value.code == -5
    joined.check()
    joined.check_fill(0, joined.n, "a stream that does not fit")
    assert length.values() == [len(want)]
    # a failed segment
    src, slab, sizes, joined, offsets, length = join(eng, data, sizes_edit=(0, ERR))
    with pytest.raises(B.BitarError) as e:
        eng.sync()
    assert e.value.code == -5
    joined.check()
    # another segment size
    with pytest.raises(B.BitarError) as e:
        eng.snappy_join(slab.ptr, 65792, sizes.ptr, 65537, offsets.ptr, joined.ptr, joined.n,
                        length.ptr, seg=59460)
    assert e.value.code == -4
    eng.sync()


def split(eng, stream, residue=0, max_rounds=0, queue=None):
    """-> (status, starts, (rounds, walks, tiles, serial)); guards checked"""
    pre = M.preamble(stream)
    n = pre[0] if pre else 0
    src = G.GuardedBytes(max(len(stream), 1), residue, "cuda", "stream")
    src.load(np.frombuffer(stream, np.uint8).copy())
    starts = Longs(S.nfrag(n) + 1)
    status, stats = G.GuardedWords(1, "cuda", "status"), G.GuardedWords(4, "cuda", "stats")
    torch.cuda.synchronize()
    eng.snappy_split(src.ptr, len(stream), n, starts.ptr, status.ptr, max_rounds, stats.ptr,
                     stream=queue)
    eng.sync(stream=queue)
    src.check()
    status.check()
    stats.check()
    assert src.payload()[:len(stream)].tobytes() == stream
    return int(status.values()[0]), starts.values(), tuple(int(v) for v in stats.values()), \
        (src, starts)


def check_split(eng, stream, residue=0, what=""):
    """the scan against the model: status, starts, rounds and walks; again with one round"""
    want = S.serial_split(stream)
    model = S.scan(stream, T)
    assert (model.status, model.starts) == want
    status, starts, stats, _ = split(eng, stream, residue)
    assert status == want[0], (what, S.STATUS[status])
    if status == S.OK:
        assert starts == want[1], what
    ntile = max((len(stream) + T - 1) // T, 1)
    if M.preamble(stream):
        assert stats == (model.rounds, model.walks, ntile, int(model.serial)), what
    one = S.scan(stream, T, max_rounds=1)
    status1, starts1, stats1, _ = split(eng, stream, residue, max_rounds=1)
    assert status1 == want[0], what
    if status1 == S.OK:
        assert starts1 == want[1], what
    if M.preamble(stream):
        assert stats1 == (1, ntile, ntile, int(one.serial)), what
    return model


def test_split_is_the_model_on_own_and_pyarrow_streams(eng):
    # every kind at four fragments, every size on kind 1
    for kind in KINDS:
        for n in SIZES if kind == 1 else SIZES[-1:]:
            _, own, stock = case(kind, n)
            r = RESIDUES[(kind + n) % 4]
            check_split(eng, own, r, ("own", kind, n))
            check_split(eng, stock, r, ("pyarrow", kind, n))


def test_the_smallest_shapes_where_the_scan_can_go_wrong(eng):
    for length in (T - 1, T, T + 1, 2 * T + 1):
        check_split(eng, S.sized_stream(length), 1, length)
    for kind in S.EDGE_ELEMENTS:
        for d in range(1, 6):
            check_split(eng, S.edge_stream(kind, T - d), d, (kind, d))
    _, tail, _ = case(6, 65537)
    m = check_split(eng, S.skipping_stream(tail), 5, "skipping literal")
    assert m.status == S.OK
    _, stored3, _ = case(0, 3 * 65536 + 1)
    assert check_split(eng, stored3, 15, "stored fragments").rounds == 1
    per = S.periodic_stream(6)
    m = check_split(eng, per, 0, "periodic")
    assert m.rounds > 2 and not m.serial  # the iteration ran, on the GPU too (check_split)
    # out of rounds: the serial finish gives the same starts, or the status says so
    import bitar_amd as B
    status, starts, stats, _ = split(eng, per, 0, max_rounds=2)
    assert (status, starts, stats[0], stats[3]) == (S.OK, m.starts, 2, 1)
    status, _, stats, _ = split(eng, per, 0, max_rounds=2 | B.SNAPPY_NO_SERIAL_FINISH)
    assert (status, stats[0], stats[3]) == (S.INCOMPLETE, 2, 0)


def test_hand_built_streams(eng):
    for name, stream, status, verdict, _ in S.hand_built():
        assert check_split(eng, stream, 1, name).status == status
        if status == S.OK:
            got, blocks, _ = decode(eng, stream, expect_error=verdict == "reject")
            want = S.decode_joined(stream, 1 << 20)
            assert (verdict, got) == (want[0], want[1]), name


def decode(eng, stream, residue=0, expect_error=False, queue=None):
    """split + joined decode with guards -> ([block bytes or None], output buffer, produced)"""
    import bitar_amd as B
    n = M.preamble(stream)[0]
    status, starts, _, (src, d_starts) = split(eng, stream, residue, queue=queue)
    assert status == S.OK
    out = G.GuardedBytes(max(n, 1), residue, "cuda", "output")
    prod = G.GuardedWords(max(S.nfrag(n), 1), "cuda", "produced")
    torch.cuda.synchronize()
    eng.decompress_joined_into(src.ptr, len(stream), n, d_starts.ptr, out.ptr, prod.ptr,
                               capacity=n, stream=queue)
    if expect_error:
        with pytest.raises(B.BitarError) as e:
            eng.sync(stream=queue)
        assert e.value.code == -5
    eng.sync(stream=queue)
    out.check()
    prod.check()
    src.check()
    body, got = out.payload(), prod.values()
    blocks = []
    for k in range(S.nfrag(n)):
        want = min(S.BLOCK, n - k * S.BLOCK)
        assert got[k] in (want, ERR), (k, got[k])
        blocks.append(None if got[k] == ERR else body[k * S.BLOCK:k * S.BLOCK + want].tobytes())
    if n == 0:
        assert got.tolist() == [G.FILL_WORD]
        out.check_fill(0, 1, "no output")
    return blocks, out, got


@pytest.mark.parametrize("n", (0, 1, 65537, 4 * 1048576 + 1))
def test_round_trip(eng, n):
    for residue in RESIDUES if n < 1 << 20 else (5,):
        kind = (1, 2, 5, 6)[RESIDUES.index(residue)]
        data, want, stock = case(kind, n)
        src, slab, sizes, joined, offsets, length = join(eng, data)
        eng.sync()
        (total,) = length.values()
        own = joined.payload()[:total].tobytes()
        assert own == want and C.pa_decode(own, n) == data
        for stream in (own, stock):
            blocks, _, _ = decode(eng, stream, residue)
            assert b"".join(blocks) == data


def test_join_past_one_scan_tile(eng):
    """1025 fragments: the join's prefix sum (scan_sizes_kernel, tiles of 1024 entries with a
    carried base) crosses a tile border.  The expected stream is the model's join of the
    engine's own 1025 slots, so the offsets, the length and every byte are pinned, and the
    split and the joined decode return the input."""
    n = 1024 * S.BLOCK + 1
    nseg = S.nfrag(n)
    assert nseg == 1025
    data = eng.empty(n)
    eng.fill(1, C.SEED, data)
    slab, stride, sizes = eng.compress(codec(), data, S.BLOCK)
    cap = n + 4 * nseg + 5
    joined = eng.empty(cap)
    offsets, length = Longs(nseg + 1), Longs(1)
    eng.snappy_join(slab, stride, sizes, n, offsets.ptr, joined, cap, length.ptr)
    eng.sync()
    h_sizes = sizes.cpu().numpy().astype(np.uint32)
    h_slab = slab.cpu().numpy()
    streams = [h_slab[i * stride:i * stride + h_sizes[i]].tobytes() for i in range(nseg)]
    want = S.join(streams, n)
    bodies = [len(s) - M.preamble(s)[1] for s in streams]
    assert [M.preamble(s)[0] for s in streams] == [S.BLOCK] * 1024 + [1]
    assert offsets.values() == np.concatenate([[0], np.cumsum(bodies)]).astype(int).tolist()
    (total,) = length.values()
    assert total == len(want) == len(M.varint(n)) + sum(bodies)
    assert joined[:total].cpu().numpy().tobytes() == want
    starts, status = Longs(nseg + 1), G.GuardedWords(1, "cuda", "status")
    eng.snappy_split(joined, total, n, starts.ptr, status.ptr)
    out = eng.empty(n)
    prod = eng.empty(nseg, dtype=torch.int32)
    eng.decompress_joined_into(joined, total, n, starts.ptr, out, prod, capacity=n)
    eng.sync()
    status.check()
    assert int(status.values()[0]) == S.OK
    assert starts.values() == [len(M.varint(n)) + o for o in offsets.values()]
    assert prod.cpu().tolist() == [S.BLOCK] * 1024 + [1]
    assert torch.equal(out, data)


def test_decode_refusals(eng):
    import bitar_amd as B
    data, own, _ = case(1, 65537)
    status, starts, _, (src, d_starts) = split(eng, own)
    out = G.GuardedBytes(65537, 0, "cuda", "output")
    prod = G.GuardedWords(2, "cuda", "produced")
    with pytest.raises(B.BitarError) as e:
        eng.decompress_joined_into(src.ptr, len(own), 65537, d_starts.ptr, out.ptr, prod.ptr,
                                   capacity=65536)
    assert e.value.code == -6
    # starts nobody wrote (all ones, as the split leaves them) reject every fragment
    blank = Longs(3)
    blank.w.view.fill_(-1)
    eng.decompress_joined_into(src.ptr, len(own), 65537, blank.ptr, out.ptr, prod.ptr,
                               capacity=65537)
    with pytest.raises(B.BitarError) as e:
        eng.sync()
    assert e.value.code == -5
    out.check()
    out.check_fill(0, out.n, "nothing decoded")
    assert prod.values().tolist() == [ERR, ERR]


@functools.lru_cache(maxsize=None)
def corpus():
    bases = [case(kind, 2 * 65536 + 777)[1] for kind in (1, 5, 6)]
    return bases, S.mutation_corpus(bases)


def test_mutation_corpus_gets_the_model_verdict(eng):
    """every mutant on queue pair 0, a good stream on queue pair 1 after every tenth: the
    verdict and every block are the model's, a rejected fragment leaves the other blocks and the
    guards alone, and the error is reported by the mutant's stream only"""
    bases, muts = corpus()
    q0, q1 = eng.queue_pair_stream(0), eng.queue_pair_stream(1)
    good_data = case(1, 2 * 65536 + 777)[0]
    census = {"ok": 0, "invalid": 0, "unsupported": 0, "reject": 0}
    for i, (t, b) in enumerate(muts):
        pre = M.preamble(t)
        verdict, want = S.decode_joined(t, 1 << 24)
        census[verdict] += 1
        if pre is None or pre[0] > 1 << 24:
            status, _, _, _ = split(eng, t, 1, queue=q0)
            assert status == S.INVALID, i
            continue
        status, _, _, _ = split(eng, t, i % 16, queue=q0)
        assert S.STATUS[status] == (verdict if verdict in ("invalid", "unsupported") else "ok"), i
        if status == S.OK:
            blocks, out, _ = decode(eng, t, i % 16, expect_error=verdict == "reject", queue=q0)
            assert blocks == want, i
        if i % 10 == 0:
            blocks, _, _ = decode(eng, bases[0], 0, queue=q1)
            assert b"".join(blocks) == good_data
    assert all(census.values()), census
