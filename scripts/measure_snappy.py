#!/usr/bin/env python3
"""What the Snappy codec costs against the LZ4 codec, whose parse it shares.  The input stays in
HBM, every timing is a pair of HIP events around one call (compress, or decompress), and the legs
that are compared run alternately in this one process: each repetition runs every leg once, so
drift and other people's work hit all of them alike.

Per input kind (0, 1, 2, 5, 6; --bytes of it, 64 KiB segments):
  snappy        CODEC_SNAPPY compress and decode of its own streams
  lz4           CODEC_LZ4 on the same input: the same parse, the LZ4 emitter and decoder
  stock-snappy  GPU decode of pyarrow's Snappy streams (offsets up to 65535: the far path)
  stock-lz4     GPU decode of liblz4's blocks of the same bytes (bench.py's stock_decode input)
The stock streams are made on the host for one 64 MiB tile of the input and repeated in HBM.
A line holds the medians, the spreads (max - min), the ratio, and for the snappy legs the margin
against the lz4 leg with the project's bar: three times the larger of the two spreads.

usage: python scripts/measure_snappy.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per (kind, leg) and writes them to FILE
(profiles/snappy/measure_snappy.jsonl)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from measure_fltpack import SEG, TILE, Leg  # noqa: E402
from measure_intpack import alternate  # noqa: E402

KINDS = (0, 1, 2, 5, 6)


class StockLeg:
    """decode of a host-made slab of one tile, repeated `tiles` times in HBM"""

    def __init__(self, eng, torch, name, codec, slab, stride, sizes, tiles):
        self.name, self.eng, self.codec, self.stride = name, eng, codec, stride
        self.slab = torch.from_numpy(slab).to("cuda:0").repeat(tiles)
        self.sizes = torch.from_numpy(sizes.astype("int32")).to("cuda:0").repeat(tiles)
        self.nseg = self.sizes.numel()
        self.prod = eng.empty(self.nseg, dtype=torch.int32)
        self.back = eng.empty(self.nseg * SEG)

    def decompress(self):
        self.eng.decompress_slab_into(self.codec, self.slab, self.stride, self.sizes, self.nseg,
                                      SEG, self.back, self.prod, capacity=self.nseg * SEG)


def snappy_slab(np, pa, host):
    """pyarrow's raw Snappy stream of every segment of host -> (slab, stride, sizes)"""
    codec = pa.Codec("snappy")
    streams = [codec.compress(host[o:o + SEG].tobytes()).to_pybytes()
               for o in range(0, host.size, SEG)]
    stride = (max(len(s) for s in streams) + 255) & ~255
    slab = np.zeros(len(streams) * stride, np.uint8)
    for i, s in enumerate(streams):
        slab[i * stride:i * stride + len(s)] = np.frombuffer(s, np.uint8)
    return slab, stride, np.array([len(s) for s in streams], np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snappy",
                                                  "measure_snappy.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    import torch
    import bitar_amd as B
    import stock_lib as S
    if not torch.cuda.is_available():
        sys.exit("measure_snappy.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    tiles = max(a.bytes // TILE, 1)
    n = tiles * TILE
    gib = n / float(1 << 30)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    med = statistics.median
    lines = []

    def verdict(line, key, mine, theirs):
        margin = med(theirs) - med(mine)
        bar = 3 * max(spread(mine), spread(theirs))
        line[f"{key}_margin_ms"] = round(margin, 4)
        line[f"{key}_bar_ms"] = round(bar, 4)
        line[f"faster_{key}"] = bool(margin > bar)
        line[f"slower_{key}"] = bool(-margin > bar)

    for kind in KINDS:
        data = eng.empty(n)
        for t in range(tiles):  # (every tile the same bytes: the stock slabs repeat with them)
            eng.fill(kind, a.seed, data[t * TILE:(t + 1) * TILE])
        eng.sync()
        host = data[:TILE].cpu().numpy()
        legs = [Leg(eng, torch, B, "snappy", B.CODEC_SNAPPY, 0, 1, data),
                Leg(eng, torch, B, "lz4", B.CODEC_LZ4, 0, 1, data)]
        s_slab, s_stride, s_sizes = snappy_slab(np, pa, host)
        l_slab, l_stride, l_sizes = S.compress(S.LZ4, host, SEG, level=1, threads=16)
        stock = [StockLeg(eng, torch, "stock-snappy", B.CODEC_SNAPPY, s_slab, s_stride, s_sizes,
                          tiles),
                 StockLeg(eng, torch, "stock-lz4", B.CODEC_LZ4, l_slab, l_stride, l_sizes, tiles)]
        calls = {}
        for leg in legs:  # (a leg's compress runs before its decompress in every repetition)
            calls[leg.name + " compress"] = leg.compress
            calls[leg.name + " decompress"] = leg.decompress
        for leg in stock:
            calls[leg.name + " decompress"] = leg.decompress
        ms = alternate(torch, calls, a.reps, a.warmup)
        eng.sync()
        for leg in legs + stock:
            d = ms[leg.name + " decompress"]
            total = int(leg.sizes.to(torch.int64).sum().item())
            line = {"kind": kind, "leg": leg.name, "bytes": n, "seg": SEG,
                    "ratio": round(n / total, 4),
                    "decompress_ms_per_GiB": round(med(d) / gib, 4),
                    "decompress_spread_ms": round(spread(d), 4),
                    "decompress_ms": [round(x, 3) for x in d],
                    "round_trip_ok": bool(torch.equal(leg.back[:n], data))}
            if leg in legs:
                c = ms[leg.name + " compress"]
                line.update({"compress_ms_per_GiB": round(med(c) / gib, 4),
                             "compress_spread_ms": round(spread(c), 4),
                             "compress_ms": [round(x, 3) for x in c]})
            if leg.name == "snappy":
                verdict(line, "compress_than_lz4", ms["snappy compress"], ms["lz4 compress"])
                verdict(line, "decompress_than_lz4", d, ms["lz4 decompress"])
                line["decompress_over_lz4"] = round(med(d) / med(ms["lz4 decompress"]), 4)
            if leg.name == "stock-snappy":
                verdict(line, "decompress_than_stock_lz4", d, ms["stock-lz4 decompress"])
                line["decompress_over_stock_lz4"] = round(
                    med(d) / med(ms["stock-lz4 decompress"]), 4)
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        del legs, stock, calls, data
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
