"""The hand-built RFC 8878 corpus (tests/zstd_frames.py) through the HIP Zstandard decoders,
under the three decoder configurations of tests/test_gpu_zstd.py: every frame gets the
oracle's verdict and bytes -- accepted and rejected frames interleaved in one call, at exact
capacity, one byte short of it, and in a context that runs the literal and sequence kernels
in series -- and the path counters equal what a Python restatement of the kernels' routing
(tests/zstd_routing.py: lane decoder's scope, last-block hand-off, multi-block hand-off)
predicts for the corpus.

The CPU-side guard that each route is fed by accepted and by rejected frames is
tests/test_zstd_frames.py::test_every_route_has_frames."""
import numpy as np
import pytest

import oracle_lib as O
import zstd_frames as ZF
from zstd_routing import expected_counters, interleaved

pytestmark = pytest.mark.gpu

SEG = ZF.SEG

torch = pytest.importorskip("torch")
from test_gpu_lz4 import _decode_blobs, down, eng, up  # noqa: E402,F401  (fixture reuse)


@pytest.fixture(params=[(16, 1), (64, 0), (0, 1)], ids=["lanes16-seq", "lanes64-handoff", "wave-seq"])
def zstd_decoder(request, eng):
    """(a local copy of tests/test_gpu_zstd.py's fixture; every GPU test here asks for it) the
    lane-per-segment decoder in front, 16 or 64 segments per wave, or the wave decoder alone;
    handed sequence sections through the two-phase record path or the lane executor"""
    lanes, seq = request.param
    old = eng.set_decoder_options(zstd_lanes=lanes, zstd_seq=seq)
    yield request.param
    eng.set_decoder_options(**old)


@pytest.fixture(scope="module")
def reference():
    """[(name, frame, oracle's bytes or None)] in the interleaved order; computed once"""
    out = []
    for name, f, _ in interleaved():
        r, ref = O.zstd_decompress(f, SEG)
        out.append((name, f, ref if r == 0 else None))
    return out


def _check(reference, ok, out, prod, seg):
    n_ok = 0
    for k, (name, f, ref) in enumerate(reference):
        if ref is None:
            assert prod[k] == 0xFFFFFFFF, (name, int(prod[k]))
        else:
            n_ok += 1
            assert prod[k] == len(ref), (name, int(prod[k]), len(ref))
            assert out[k * seg:k * seg + len(ref)].tobytes() == ref, name
    assert ok == (n_ok == len(reference))
    return n_ok


def test_whole_corpus_like_the_oracle(eng, reference, zstd_decoder):
    ok, out, prod = _decode_blobs(eng, O.CODEC_ZSTD, [f for _, f, _ in reference], SEG)
    n_ok = _check(reference, ok, out, prod, SEG)
    assert 0 < n_ok < len(reference)


# the handed frames with malformed Huffman literal streams (the last one in a later block of a
# multi-block hand-off)
LIT_FAULT_FRAMES = ("huf_stream_short", "huf_stream_short_4", "huf_stream_regen_plus1",
                    "huf_stream_regen_minus1", "huf_stream_zero_last", "huf_jump_shift",
                    "mb_later_bad_literals")


def test_path_counters_equal_the_routing_predicate(eng, reference, zstd_decoder):
    lanes, seq = zstd_decoder
    frames = [f for _, f, _ in reference]
    want, R = expected_counters(frames, lanes, seq)
    old = eng.set_decoder_options(count_paths=1)
    try:
        eng.path_counters()  # (reset)
        ok, out, prod = _decode_blobs(eng, O.CODEC_ZSTD, frames, SEG)
        pc = eng.path_counters()
    finally:
        eng.set_decoder_options(**old)
    _check(reference, ok, out, prod, SEG)
    lo = want.pop("zstd_seqdec_serial")
    got = {k: pc[k] for k in want}
    print("routes:", got, "of", len(frames), "frames; predicted", want, "seqdec >=", lo)
    assert (got["zstd_wave"], got["zstd_handed"]) == (want["zstd_wave"], want["zstd_handed"])
    # zstd_seqdec is exact but for the handed frames whose Huffman streams are malformed
    # (route() lit_fault: zstd_hlit_kernel may fail them before zstd_seqdec_kernel looks);
    # these frames and no others, so the bound is as wide as their count
    faults = sorted(name for (name, _, _), r in zip(reference, R) if r["seqdec"] and r["lit_fault"])
    assert faults == sorted(LIT_FAULT_FRAMES if seq else []), faults
    assert want["zstd_seqdec"] - lo == len(faults)
    assert lo <= got["zstd_seqdec"] <= want["zstd_seqdec"]
    taken = [r for r in R if not (lanes and r["lanes"])]
    for key in ("handed", "seqdec", "multi") if seq else ("handed",):
        assert any(r[key] and r["accepted"] for r in taken), key
        assert any(r[key] and not r["accepted"] for r in taken), key
    if lanes:
        assert want["zstd_wave"] < len(frames)


CAPACITY_LENGTHS = (102, 256, 693, 4100, 65536)


def test_exact_capacity_and_one_byte_short(eng, reference, zstd_decoder):
    """the accepted frames of one plain length decoded side by side at seg = that length (an
    overrun of one slot lands in the next slot's bytes), then at seg - 1: all rejected, as by
    the oracle"""
    for L in CAPACITY_LENGTHS:
        group = [(n, f, ref) for n, f, ref in reference if ref is not None and len(ref) == L]
        assert len(group) >= 2, L
        ok, out, prod = _decode_blobs(eng, O.CODEC_ZSTD, [f for _, f, _ in group], L)
        assert ok
        assert _check(group, ok, out, prod, L) == len(group)
        for n, f, _ in group:
            assert O.zstd_decompress(f, L - 1)[0] != 0, n
        ok, out, prod = _decode_blobs(eng, O.CODEC_ZSTD, [f for _, f, _ in group], L - 1)
        assert not ok
        assert all(p == 0xFFFFFFFF for p in prod), (L, [int(p) for p in prod])


def test_serial_context_gives_the_same_verdicts_and_bytes(eng, reference, zstd_decoder):
    import bitar_amd
    lanes, seq = zstd_decoder
    frames = [f for _, f, _ in reference]
    ok_a, out_a, prod_a = _decode_blobs(eng, O.CODEC_ZSTD, frames, SEG)
    serial = bitar_amd.Engine(0, num_streams=1,
                              flags=bitar_amd.FLAG_ZSTD_SERIAL | bitar_amd.FLAG_COUNT_PATHS)
    try:
        serial.set_decoder_options(zstd_lanes=lanes, zstd_seq=seq)
        ok_b, out_b, prod_b = _decode_blobs(serial, O.CODEC_ZSTD, frames, SEG)
        pc = serial.path_counters()
    finally:
        serial.close()
    # in series the literal kernel runs first: the counters are exact
    want, _ = expected_counters(frames, lanes, seq)
    print("serial routes:", {k: pc[k] for k in ("zstd_wave", "zstd_handed", "zstd_seqdec")}, want)
    assert (pc["zstd_wave"], pc["zstd_handed"], pc["zstd_seqdec"]) == \
        (want["zstd_wave"], want["zstd_handed"], want["zstd_seqdec_serial"])
    _check(reference, ok_b, out_b, prod_b, SEG)
    assert ok_a == ok_b and np.array_equal(prod_a, prod_b)
    for k in range(len(frames)):
        if prod_a[k] != 0xFFFFFFFF:
            n = int(prod_a[k])
            assert out_a[k * SEG:k * SEG + n].tobytes() == out_b[k * SEG:k * SEG + n].tobytes(), k
