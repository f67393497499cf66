"""GPU tests of the segment filters (csrc/filter.hip) through the C ABI: exact bytes against
the numpy model (filter_model.py) in both directions, every alignment of the buffers, length
arrays with skipped segments, the invalid arguments, and the filters in front of the three
codec families against the oracle's encoders.

Shapes: 65536 (the largest segment, 16-B aligned everywhere), 59460 (the reference's segment:
every stream starts unaligned and three segments in four are only 4-B aligned), 4096 (one tile
exactly for width 4 and less than one for the others), 1000 / 999 (a remainder of elements,
odd bases), 72 and 7 (shorter than a plane group, shorter than an element)."""
import numpy as np
import pytest

import filter_model as F
import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEGS = (65536, 59460, 4096, 1000, 999, 72, 7)
CANARY = 0xA5
PAD = 256
FILTERS = (F.SHUFFLE, F.BITSHUFFLE)
IDS = ("shuffle", "bitshuffle")


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


def up(a, dtype=np.uint8):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros(1, dtype)
    return torch.from_numpy(a.copy()).cuda()


def run(eng, inverse, filt, w, data, seg, lens=None, in_off=0, out_off=0):
    """one call on the GPU -> (output bytes, the canaries in front of and behind them); the
    buffers start in_off / out_off bytes into their allocations"""
    n = data.size
    src = torch.zeros(in_off + n + PAD, dtype=torch.uint8, device="cuda")
    src[in_off:in_off + n] = torch.from_numpy(data.copy()).cuda()
    dst = torch.full((PAD + out_off + n + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    d_lens = None if lens is None else up(np.array(lens, np.uint32).view(np.int32), np.int32)
    nseg = None if lens is None else len(lens)
    fn = eng.unfilter_into if inverse else eng.filter_into
    fn(filt, w, src.data_ptr() + in_off, seg, dst.data_ptr() + PAD + out_off, n=n, lens=d_lens,
       nseg=nseg)
    eng.sync()
    host = dst.cpu().numpy()
    return (host[PAD + out_off:PAD + out_off + n], host[:PAD + out_off],
            host[PAD + out_off + n:])


def check_case(eng, filt, w, seg, n, seed, **kw):
    data = rnd(n, seed)
    for inverse, model in ((False, F.apply), (True, F.invert)):
        got, front, back = run(eng, inverse, filt, w, data, seg, **kw)
        assert np.all(front == CANARY) and np.all(back == CANARY), (seg, n, inverse)
        want = model(filt, data, w, seg)
        if seg >= 64 * w and n >= seg:  # (random bytes: the transposition is no identity)
            assert not np.array_equal(want, data)
        assert np.array_equal(got, want), \
            (seg, n, inverse, np.flatnonzero(got != want)[:8].tolist())


@pytest.mark.parametrize("w", F.WIDTHS)
@pytest.mark.parametrize("filt", FILTERS, ids=IDS)
def test_exact_bytes_both_directions(eng, filt, w):
    """apply and invert, each exact against the model on random input (the inverse on
    independent input, not as a round trip)"""
    for seg in SEGS:
        for r in (0, 1, w - 1, w, 8 * w - 1, 8 * w, 8 * w + 1, 64 * w + 3):
            check_case(eng, filt, w, seg, 3 * seg + r, seg * 31 + r)
    for n in (1, w - 1):  # shorter than an element
        check_case(eng, filt, w, 72, n, n)


@pytest.mark.parametrize("filt", FILTERS, ids=IDS)
def test_empty_input_launches_nothing(eng, filt):
    dst = torch.full((PAD,), CANARY, dtype=torch.uint8, device="cuda")
    src = torch.zeros(PAD, dtype=torch.uint8, device="cuda")
    eng.filter_into(filt, 8, src, 4096, dst, n=0)
    eng.unfilter_into(filt, 8, src, 4096, dst, n=0)
    eng.filter_into(filt, 8, src, 4096, dst, n=PAD, nseg=0)
    eng.sync()
    assert bool((dst == CANARY).all())


@pytest.mark.parametrize("seg", (65536, 59460))
@pytest.mark.parametrize("filt", FILTERS, ids=IDS)
def test_every_alignment(eng, filt, seg):
    for w in (4, 8):
        for k, (a, b) in enumerate(((1, 0), (0, 3), (4, 4), (8, 15), (15, 1), (3, 8))):
            check_case(eng, filt, w, seg, 2 * seg + 8 * w + 5, 100 * k + w, in_off=a, out_off=b)


@pytest.mark.parametrize("w", F.WIDTHS)
@pytest.mark.parametrize("filt", FILTERS, ids=IDS)
def test_length_array_and_skipped_segments(eng, filt, w):
    for seg in (59460, 1000):
        lens = [seg, 5, seg - 1, 0, F.SEGMENT_ERROR, 8 * w, 8 * w + 7, seg + 1]
        data = rnd(len(lens) * seg, seg + w)
        canary = np.full(data.size, CANARY, np.uint8)
        for inverse, model in ((False, F.apply), (True, F.invert)):
            got, front, back = run(eng, inverse, filt, w, data, seg, lens=lens)
            assert np.all(front == CANARY) and np.all(back == CANARY)
            # the model leaves what a call does not write as the canary: skipped segments
            # (SEGMENT_ERROR, seg + 1) and the bytes past each segment's length
            assert np.array_equal(got, model(filt, data, w, seg, lens=lens, out=canary)), \
                (seg, inverse)
            for i in (4, 7):
                assert np.all(got[i * seg:(i + 1) * seg] == CANARY)


def test_length_past_the_buffer_moves_nothing(eng):
    """n cuts the last segment short: a length that reaches past n is skipped, not clamped"""
    seg, w = 1000, 4
    data = rnd(2 * seg + 100, 5)
    lens = [seg, seg, 101]
    canary = np.full(data.size, CANARY, np.uint8)
    got, front, back = run(eng, False, F.SHUFFLE, w, data, seg, lens=lens)
    assert np.all(back == CANARY)
    assert np.array_equal(got, F.apply(F.SHUFFLE, data, w, seg, lens=lens, out=canary))
    assert np.all(got[2 * seg:] == CANARY)


def test_invalid_arguments_leave_the_engine_usable(eng):
    import bitar_amd as B
    n, seg = 8192, 4096
    src = up(rnd(n + 64, 1))
    dst = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    good = dict(filter=B.FILTER_SHUFFLE, width=8, data=src, seg=seg, out=dst, n=n)
    bad = [dict(filter=0), dict(filter=3), dict(width=1), dict(width=3), dict(width=32),
           dict(width=0), dict(seg=0), dict(seg=65537), dict(data=None), dict(out=None),
           dict(out=src), dict(out=src.data_ptr() + n - 1), dict(out=src.data_ptr() + 1),
           dict(data=dst.data_ptr() + 17, out=dst)]
    want = F.apply(F.SHUFFLE, src.cpu().numpy()[:n], 8, seg)
    for call in (eng.filter_into, eng.unfilter_into):
        for change in bad:
            with pytest.raises(B.BitarError) as e:
                call(**dict(good, **change))
            assert e.value.code == -4, change
            # ... and the next call on the same engine works
            dst.zero_()
            eng.filter_into(**good)
            eng.sync()
            assert np.array_equal(dst.cpu().numpy()[:n], want), change
    # buffers that touch without overlapping are fine
    both = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
    both[:n] = src[:n]
    eng.filter_into(B.FILTER_SHUFFLE, 8, both, seg, both.data_ptr() + n, n=n)
    eng.sync()
    assert np.array_equal(both.cpu().numpy()[n:], want)


@pytest.fixture(scope="module")
def kind5():
    return O.fill(5, 7, 4 << 20)


@pytest.fixture(scope="module")
def kind5_filtered(kind5):
    return {f: F.apply(f, kind5, 8, 65536) for f in FILTERS}


def codec_cases():
    import bitar_amd as B
    return [(B.CODEC_LZ4, O.CODEC_LZ4, B.CODEC_LZ4), (B.CODEC_ZSTD, O.CODEC_ZSTD, B.CODEC_ZSTD),
            (B.CODEC_DEFLATE_DYNAMIC, O.CODEC_DEFLATE_DYN, B.CODEC_DEFLATE)]


@pytest.mark.parametrize("case", range(3), ids=("lz4", "zstd", "deflate_dynamic"))
@pytest.mark.parametrize("filt", FILTERS, ids=IDS)
def test_filter_in_front_of_the_codecs(eng, kind5, kind5_filtered, filt, case):
    """kind 5 at 4 MiB, width 8: the slots of the filtered call are the oracle's encoding of the
    model-filtered bytes, bit for bit; decompress + invert returns the original"""
    import bitar_amd as B
    codec, ocodec, dcodec = codec_cases()[case]
    seg, n = 65536, kind5.size
    nseg = n // seg
    data = up(kind5)
    filtered = eng.empty(n)
    eng.filter_into(filt, 8, data, seg, filtered)
    slab, stride, sizes = eng.compress(codec, filtered, seg)
    out, prod = eng.decompress(dcodec, slab, stride, sizes, seg)
    back = torch.full((n,), CANARY, dtype=torch.uint8, device="cuda")
    eng.unfilter_into(filt, 8, out, seg, back, n=n, lens=prod, nseg=nseg)
    eng.sync()
    r, oslab, osizes = O.compress_segments(ocodec, kind5_filtered[filt], seg, stride, threads=4)
    assert r == 0
    gsz = sizes.cpu().numpy().astype(np.uint32)
    assert np.array_equal(gsz, osizes)
    g = slab.cpu().numpy()
    for i in range(nseg):
        assert np.array_equal(g[i * stride:i * stride + osizes[i]],
                              oslab[i * stride:i * stride + osizes[i]]), i
    assert np.array_equal(prod.cpu().numpy(), np.full(nseg, seg, np.int32))
    assert np.array_equal(back.cpu().numpy(), kind5)
