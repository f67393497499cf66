#!/usr/bin/env python3
"""What INTPACK costs and buys against the filter path it is an alternative to.  The input
stays in HBM, every timing is a pair of HIP events around one call (compress, or decompress),
and the legs that are compared run alternately in this one process: each repetition runs every
leg once, so drift and other people's work hit all of them alike.

For kind 5 (int64 in [0, 1000), element width 8) and kind 2 (the Arrow record-batch body,
element width 4, its dictionary-index column's width):
  intpack              bitar_hip_compress / _decompress_slab with the INTPACK id of the width
  shuffle + lz4        filter_into + LZ4 compress; LZ4 decompress + unfilter_into
  bitshuffle + lz4     the same with BITSHUFFLE
  lz4                  LZ4 alone, for scale
Each leg's last output is checked against the input after the timed window.

usage: python scripts/measure_intpack.py [--bytes N] [--reps 7] [--warmup 2]
Prints one JSON line per (kind, leg)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEG = 65536


def alternate(torch, legs, reps, warmup):
    """{name: [ms, ...]}: every repetition runs each leg once, in order"""
    s = torch.cuda.current_stream()
    ms = {k: [] for k in legs}
    for r in range(warmup + reps):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize()
            if r >= warmup:
                ms[name].append(a.elapsed_time(b))
    return ms


class Leg:
    """one way to store the column: its slots, and the calls that fill and read them"""

    def __init__(self, eng, torch, B, name, codec, dcodec, filt, width, data, n):
        self.name, self.codec, self.dcodec, self.filt, self.width = name, codec, dcodec, filt, width
        self.eng, self.data, self.n = eng, data, n
        self.nseg = (n + SEG - 1) // SEG
        self.stride = B.slot_size(codec, SEG)
        self.slab = eng.empty(self.nseg * self.stride)
        self.sizes = eng.empty(self.nseg, dtype=torch.int32)
        self.prod = eng.empty(self.nseg, dtype=torch.int32)
        self.back = eng.empty(n)
        self.mid = eng.empty(n) if filt else None  # the filtered bytes, either direction

    def compress(self):
        src = self.data
        if self.filt:
            self.eng.filter_into(self.filt, self.width, self.data, SEG, self.mid)
            src = self.mid
        self.eng.compress_into(self.codec, src, SEG, self.slab, self.stride, self.sizes, n=self.n)

    def decompress(self):
        dst = self.mid if self.filt else self.back
        self.eng.decompress_slab_into(self.dcodec, self.slab, self.stride, self.sizes, self.nseg,
                                      SEG, dst, self.prod, capacity=self.nseg * SEG)
        if self.filt:
            self.eng.unfilter_into(self.filt, self.width, self.mid, SEG, self.back, n=self.n,
                                   lens=self.prod, nseg=self.nseg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    import bitar_amd as B
    if not torch.cuda.is_available():
        sys.exit("measure_intpack.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    n = a.bytes // SEG * SEG
    gib = n / float(1 << 30)
    data = eng.empty(n)
    for kind, w in ((5, 8), (2, 4)):
        eng.fill(kind, a.seed, data)
        legs = [Leg(eng, torch, B, *spec, w, data, n) for spec in (
            ("intpack", B.codec_intpack(w), B.codec_intpack(w), 0),
            ("shuffle+lz4", B.CODEC_LZ4, B.CODEC_LZ4, B.FILTER_SHUFFLE),
            ("bitshuffle+lz4", B.CODEC_LZ4, B.CODEC_LZ4, B.FILTER_BITSHUFFLE),
            ("lz4", B.CODEC_LZ4, B.CODEC_LZ4, 0))]
        calls = {}
        for leg in legs:  # (a leg's compress runs before its decompress in every repetition)
            calls[leg.name + " compress"] = leg.compress
            calls[leg.name + " decompress"] = leg.decompress
        ms = alternate(torch, calls, a.reps, a.warmup)
        eng.sync()
        for leg in legs:
            c, d = ms[leg.name + " compress"], ms[leg.name + " decompress"]
            total = int(leg.sizes.to(torch.int64).sum().item())
            print(json.dumps({
                "kind": kind, "width": w, "leg": leg.name, "bytes": n, "seg": SEG,
                "ratio": round(n / total, 4),
                "compress_ms_per_GiB": round(statistics.median(c) / gib, 4),
                "compress_spread_ms": round(max(c) - min(c), 4),
                "decompress_ms_per_GiB": round(statistics.median(d) / gib, 4),
                "decompress_spread_ms": round(max(d) - min(d), 4),
                "compress_ms": [round(x, 3) for x in c],
                "decompress_ms": [round(x, 3) for x in d],
                "round_trip_ok": bool(torch.equal(leg.back, data))}), flush=True)
        del legs, calls
    eng.close()


if __name__ == "__main__":
    main()
