"""The hand-built RFC 1951 corpus (tests/deflate_streams.py) through the HIP inflaters, under
the three decoder configurations of tests/test_gpu_deflate.py and both hints of a call (the
FIXED hint: inflate_fixed_kernel with 9 / 8-bit fast tables, the DYNAMIC hint: inflate_kernel
with 10 / 9-bit ones -- either decodes whatever the stream holds): every stream gets the
oracle's verdict, size and bytes -- accepted and rejected streams interleaved in one call, at
exact capacity, one byte short of it, and with garbage instead of zeros behind each stream in
its slab slot -- and the path counters equal what a Python restatement of the routing
(tests/deflate_routing.py) predicts.

The CPU-side guards -- the oracle equals zlib and the writer's model on every stream, each
stream exercises what it claims, every route is fed -- are in tests/test_deflate_streams.py."""
import numpy as np
import pytest

import deflate_routing as R
import deflate_streams as DS
import oracle_lib as O

pytestmark = pytest.mark.gpu

SEG = DS.SEG
ERR = 0xFFFFFFFF

torch = pytest.importorskip("torch")
from test_gpu_lz4 import _decode_blobs, down, eng, up  # noqa: E402,F401  (fixture reuse)


@pytest.fixture(params=[4, 16, 0], ids=["lanes4", "lanes16", "wave"])
def inflate_decoder(request, eng):
    """(as tests/test_gpu_deflate.py's) the lane-per-segment inflater in front, 4 or 16
    segments per wave, or the wave inflater alone"""
    old = eng.set_decoder_options(inflate_lanes=request.param)
    yield request.param
    eng.set_decoder_options(**old)


@pytest.fixture(params=[O.CODEC_DEFLATE, O.CODEC_DEFLATE_DYN], ids=["fixed-hint", "dynamic-hint"])
def hint(request):
    return request.param


@pytest.fixture(scope="module")
def reference():
    """[(name, stream, the oracle's bytes or None)] in the interleaved order; computed once"""
    out = []
    for name, _, s, plain, _ in R.interleaved():
        r, ref = O.inflate(s, SEG)
        assert (ref if r == 0 else None) == plain, name  # (the writer's model)
        out.append((name, s, plain))
    return out


def _check(reference, ok, out, prod, seg):
    n_ok = 0
    for k, (name, _, ref) in enumerate(reference):
        if ref is None:
            assert prod[k] == ERR, (name, int(prod[k]))
        else:
            n_ok += 1
            assert prod[k] == len(ref), (name, int(prod[k]), len(ref))
            assert out[k * seg:k * seg + len(ref)].tobytes() == ref, name
    assert ok == (n_ok == len(reference))
    return n_ok


def test_whole_corpus_like_the_oracle(eng, reference, inflate_decoder, hint):
    ok, out, prod = _decode_blobs(eng, hint, [s for _, s, _ in reference], SEG)
    n_ok = _check(reference, ok, out, prod, SEG)
    assert 0 < n_ok < len(reference)  # (ok is false exactly because rejects are present)
    assert not ok


def test_path_counters_equal_the_routing_predicate(eng, reference, inflate_decoder, hint):
    streams = [s for _, s, _ in reference]
    want = R.expected_counters(streams, inflate_decoder)
    old = eng.set_decoder_options(count_paths=1)
    try:
        eng.path_counters()  # (reset)
        ok, out, prod = _decode_blobs(eng, hint, streams, SEG)
        pc = eng.path_counters()
    finally:
        eng.set_decoder_options(**old)
    _check(reference, ok, out, prod, SEG)
    got = {k: pc[k] for k in want}
    print("routes:", got, "of", len(streams), "streams; predicted", want)
    assert got == want
    assert want["inflate_wave"] == len(streams) if not inflate_decoder \
        else want["inflate_wave_reject"] < want["inflate_wave"] < len(streams)


def test_batch_path_runs_where_it_must_and_only_where_it_can(eng, reference, hint):
    """the wave inflater alone: every stream of the must_batch subset runs at least one batch,
    none of the cannot_batch subset does"""
    bits = R.LIT_FAST[hint]
    must = [e for e in reference if R.must_batch(e[1], bits)]
    cannot = [e for e in reference if R.cannot_batch(e[1])]
    assert must and cannot
    old = eng.set_decoder_options(inflate_lanes=0, count_paths=1)
    try:
        for subset, want in ((must, len(must)), (cannot, 0)):
            eng.path_counters()
            ok, out, prod = _decode_blobs(eng, hint, [s for _, s, _ in subset], SEG)
            pc = eng.path_counters()
            _check(subset, ok, out, prod, SEG)
            print("batch segments:", pc["inflate_batch_segs"], "of", len(subset), "want", want)
            assert pc["inflate_wave"] == len(subset)
            assert pc["inflate_batch_segs"] == want, pc
    finally:
        eng.set_decoder_options(**old)


def test_a_64_byte_match_is_one_batch_and_65_bytes_are_none(eng, reference, hint):
    """mlen <= 64 is what a batch copies itself; one byte more goes to long_match, which
    counts no batch.  Each stream holds that one match and nothing else a batch could take."""
    old = eng.set_decoder_options(inflate_lanes=0, count_paths=1)
    try:
        for name, want in (("batch/match64-only", 1), ("batch/match65-only", 0)):
            one = [e for e in reference if e[0] == name]
            eng.path_counters()
            ok, out, prod = _decode_blobs(eng, hint, [one[0][1]], SEG)
            pc = eng.path_counters()
            assert _check(one, ok, out, prod, SEG) == 1
            assert (pc["inflate_batch_segs"], pc["inflate_batches"]) == (want, want), (name, pc)
    finally:
        eng.set_decoder_options(**old)


def test_exact_capacity_and_one_byte_short(eng, reference, inflate_decoder, hint):
    """the accepted streams of one plain length decoded side by side at seg = that length (an
    overrun of one slot lands in the next slot's bytes), then at seg - 1: all rejected, as by
    the oracle"""
    for L in DS.CAPACITY_LENGTHS:
        group = [(n, s, ref) for n, s, ref in reference if ref is not None and len(ref) == L]
        assert len(group) >= 2, L
        for n, s, ref in group:
            assert O.inflate(s, L) == (0, ref), n
            assert O.inflate(s, L - 1)[0] != 0, n
        ok, out, prod = _decode_blobs(eng, hint, [s for _, s, _ in group], L)
        assert ok
        assert _check(group, ok, out, prod, L) == len(group)
        ok, out, prod = _decode_blobs(eng, hint, [s for _, s, _ in group], L - 1)
        assert not ok
        assert all(p == ERR for p in prod), (L, [int(p) for p in prod])


def _decode_filled(eng, codec, blobs, seg, fill):
    """_decode_blobs with `fill` instead of zeros behind every stream in its slab slot"""
    import bitar_amd
    nseg = len(blobs)
    stride = max(256, max(len(b) for b in blobs) + 64)
    slab = np.full(nseg * stride, fill, np.uint8)
    for i, b in enumerate(blobs):
        slab[i * stride:i * stride + len(b)] = np.frombuffer(b, np.uint8)
    d_slab = up(slab)
    d_sizes = torch.tensor([len(b) for b in blobs], dtype=torch.int32).cuda()
    out = eng.empty(nseg * seg)
    prod = eng.empty(nseg, dtype=torch.int32)
    eng.decompress_slab_into(codec, d_slab, stride, d_sizes, nseg, seg, out, prod)
    torch.cuda.synchronize()
    try:
        eng.sync()
        ok = True
    except bitar_amd.BitarError as ex:
        assert ex.code == -5
        ok = False
    return ok, down(out), down(prod).astype(np.uint32)


def test_garbage_behind_each_stream_changes_nothing(eng, reference, inflate_decoder, hint):
    """the readers mask by csize (peek4, the batch's nine-dword read, the lane inflater's
    refill): 0xFF behind every stream in its slot gives the verdicts and bytes of zeros"""
    ok, out, prod = _decode_filled(eng, hint, [s for _, s, _ in reference], SEG, 0xFF)
    n_ok = _check(reference, ok, out, prod, SEG)
    assert 0 < n_ok < len(reference)
