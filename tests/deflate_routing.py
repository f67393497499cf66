"""Which HIP inflater decodes a raw DEFLATE stream, and whether the wave inflater's batch path
runs on it, restated in Python (no GPU, no torch) from runtime.hip, inflate_lanes.hip and
inflate.hip.  tests/test_gpu_deflate_streams.py holds the path counters against it;
tests/test_deflate_streams.py guards on the CPU that every route is fed.  Test infrastructure
only.

  * inflate_lanes_kernel (decoder option inflate_lanes != 0) goes first over every segment and
    keeps the streams it can finish: those the oracle accepts whose block headers are all
    stored or fixed.  Everything else -- a dynamic or reserved block type, any failed check --
    it defers, and inflate_kernel / inflate_fixed_kernel (the DYNAMIC / the FIXED hint of the
    call, whatever the stream holds) decides.
  * huff_batch (inflate.hip) runs where kBatchStreamBytes = 48 bytes of stream lie past the
    position and the segment has room; it counts a batch when it produced output, which it
    does at the latest when the first symbol of a body is a literal of the fast table."""
import functools
import math

import deflate_streams as DS
import oracle_lib as O

SEG = DS.SEG
LIT_FAST = {O.CODEC_DEFLATE_DYN: 10, O.CODEC_DEFLATE: 9}  # inflate.hip / inflate_fixed.hip


@functools.lru_cache(maxsize=None)
def accepted(stream, cap=SEG):
    return O.inflate(stream, cap)[0] == 0


def lanes_takes(stream, cap=SEG):
    return accepted(stream, cap) and all(b["type"] in (0, 1)
                                         for b in DS.walk(stream, cap)["blocks"])


def must_batch(stream, lit_fast_bits, cap=SEG):
    """some Huffman body reached starts >= 48 stream bytes before the end, has room, and opens
    with a literal whose code the fast table holds"""
    return any("body_bit" in b and (b["body_bit"] >> 3) + DS.BATCH_BYTES <= len(stream)
               and b["op_at_body"] < cap and b["first"] is not None and b["first"][0] < 256
               and b["first"][1] <= lit_fast_bits for b in DS.walk(stream, cap)["blocks"])


def cannot_batch(stream, cap=SEG):
    """only stored blocks, or fewer than 48 stream bytes"""
    return len(stream) < DS.BATCH_BYTES or all(b["type"] == 0
                                               for b in DS.walk(stream, cap)["blocks"])


def expected_counters(streams, lanes, cap=SEG):
    wave = [s for s in streams if not (lanes and lanes_takes(s, cap))]
    return dict(inflate_wave=len(wave),
                inflate_wave_reject=sum(not accepted(s, cap) for s in streams))


def interleaved():
    """the corpus ordered so that neighbours differ: accepted and rejected streams alternate as
    long as both last, and the streams of one class (consecutive in corpus()) are dealt out over
    the whole batch"""
    C = DS.corpus()

    def deal(v):  # (a stride coprime to the count spreads a class's streams apart)
        st = next(k for k in (7, 11, 13, 17, 19) if math.gcd(k, len(v)) == 1)
        return [v[(i * st) % len(v)] for i in range(len(v))]
    acc = deal([c for c in C if c[3] is not None])
    rej = deal([c for c in C if c[3] is None])
    out = []
    step = len(acc) / len(rej)
    k = 0.0
    for r in rej:
        n = int(k + step) - int(k)
        k += step
        out += acc[:n] + [r]
        acc = acc[n:]
    return out + acc
