#!/usr/bin/env python3
"""What FLTPACK costs and buys against the ways a float column could be stored before it.  The
input stays in HBM, every timing is a pair of HIP events around one call (compress, or
decompress), and the legs that are compared run alternately in this one process: each
repetition runs every leg once, so drift and other people's work hit all of them alike.

Columns (a 64 MiB tile made on the host, where the division is numpy's, repeated to --bytes):
  prices       float64, integers in [0, 100000) over 100
  sensor       float32, integers in [-500, 500) over 10
  normal       float64, N(0,1): no exponent holds it, the stored path
Legs per column:
  fltpack              bitar_hip_compress / _decompress_slab with the FLTPACK id of the width
  bitshuffle + lz4     filter_into + LZ4 compress; LZ4 decompress + unfilter_into
  zstd                 Zstd alone
  intpack (integers)   INTPACK of the same width on the column's integers themselves (random
                       integers for `normal`): the same memory work and the same bit widths
                       without the multiply, the rint and the division
Each leg's last output is checked against its input after the timed window.

usage: python scripts/measure_fltpack.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per (column, leg) and writes them to FILE
(profiles/fltpack/measure_fltpack.jsonl)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
SEG = 65536
TILE = 64 << 20

from measure_intpack import alternate  # noqa: E402


class Leg:
    """one way to store a column: its slots, and the calls that fill and read them"""

    def __init__(self, eng, torch, B, name, codec, filt, width, data):
        self.name, self.codec, self.filt, self.width = name, codec, filt, width
        self.eng, self.data, self.n = eng, data, data.numel()
        self.nseg = (self.n + SEG - 1) // SEG
        self.stride = B.slot_size(codec, SEG)
        self.slab = eng.empty(self.nseg * self.stride)
        self.sizes = eng.empty(self.nseg, dtype=torch.int32)
        self.prod = eng.empty(self.nseg, dtype=torch.int32)
        self.back = eng.empty(self.n)
        self.mid = eng.empty(self.n) if filt else None  # the filtered bytes, either direction

    def compress(self):
        src = self.data
        if self.filt:
            self.eng.filter_into(self.filt, self.width, self.data, SEG, self.mid)
            src = self.mid
        self.eng.compress_into(self.codec, src, SEG, self.slab, self.stride, self.sizes, n=self.n)

    def decompress(self):
        dst = self.mid if self.filt else self.back
        self.eng.decompress_slab_into(self.codec, self.slab, self.stride, self.sizes, self.nseg,
                                      SEG, dst, self.prod, capacity=self.nseg * SEG)
        if self.filt:
            self.eng.unfilter_into(self.filt, self.width, self.mid, SEG, self.back, n=self.n,
                                   lens=self.prod, nseg=self.nseg)


def columns(np, seed):
    """-> [(name, width, float tile, integer tile)], each tile TILE bytes"""
    rng = np.random.default_rng(seed)
    n8, n4 = TILE // 8, TILE // 4
    cents = rng.integers(0, 100000, n8)
    tenths = rng.integers(-500, 500, n4)
    return [("prices", 8, (cents / 100.0).astype("<f8"), cents.astype("<i8")),
            ("sensor", 4, (tenths / 10.0).astype("<f4"), tenths.astype("<i4")),
            ("normal", 8, rng.normal(0, 1, n8).astype("<f8"),
             rng.integers(-2 ** 63, 2 ** 63 - 1, n8).astype("<i8"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fltpack",
                                                  "measure_fltpack.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bitar_amd as B
    if not torch.cuda.is_available():
        sys.exit("measure_fltpack.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    tiles = max(a.bytes // TILE, 1)
    n = tiles * TILE
    gib = n / float(1 << 30)
    lines = []
    for name, w, floats, ints in columns(np, a.seed):
        up = lambda t: torch.from_numpy(t.view(np.uint8)).to("cuda:0").repeat(tiles)  # noqa: E731
        fdata, idata = up(floats), up(ints)
        legs = [Leg(eng, torch, B, *spec) for spec in (
            ("fltpack", B.codec_fltpack(w), 0, w, fdata),
            ("bitshuffle+lz4", B.CODEC_LZ4, B.FILTER_BITSHUFFLE, w, fdata),
            ("zstd", B.CODEC_ZSTD, 0, w, fdata),
            ("intpack (integers)", B.codec_intpack(w), 0, w, idata))]
        calls = {}
        for leg in legs:  # (a leg's compress runs before its decompress in every repetition)
            calls[leg.name + " compress"] = leg.compress
            calls[leg.name + " decompress"] = leg.decompress
        ms = alternate(torch, calls, a.reps, a.warmup)
        eng.sync()
        for leg in legs:
            c, d = ms[leg.name + " compress"], ms[leg.name + " decompress"]
            total = int(leg.sizes.to(torch.int64).sum().item())
            lines.append(json.dumps({
                "column": name, "width": w, "leg": leg.name, "bytes": n, "seg": SEG,
                "ratio": round(n / total, 4),
                "compress_ms_per_GiB": round(statistics.median(c) / gib, 4),
                "compress_spread_ms": round(max(c) - min(c), 4),
                "decompress_ms_per_GiB": round(statistics.median(d) / gib, 4),
                "decompress_spread_ms": round(max(d) - min(d), 4),
                "compress_ms": [round(x, 3) for x in c],
                "decompress_ms": [round(x, 3) for x in d],
                "round_trip_ok": bool(torch.equal(leg.back, leg.data))}))
            print(lines[-1], flush=True)
        del legs, calls, fdata, idata
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
