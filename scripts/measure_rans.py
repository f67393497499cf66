#!/usr/bin/env python3
"""What RANS costs and buys against LZ4 and Zstd on inputs whose gain is their histogram.  The
input stays in HBM, every timing is a pair of HIP events around one call (compress, or
decompress; with a filter the filter's kernel is inside the pair), and the legs that are compared
run alternately in this one process: each repetition runs every leg once, so drift and other
people's work hit all of them alike.

Inputs (1 GiB, 64 KiB segments):
  kind1        the engine's generator of log-like text (fill kind 1), no filter
  normal_f32   N(0,1) float32 behind the shuffle filter at width 4 (a 64 MiB tile, repeated)
  walk_f32     a smooth float32 walk behind the shuffle filter at width 4 (likewise)
  random       random bytes, no filter
Legs per input: rans, lz4, zstd, each behind the input's filter.
Each leg's last output is checked against its input after the timed window.  A rans line says for
each other leg whether RANS took less time by more than three times the larger of the two spreads
(`*_beats_<leg>`), or more time by that margin (`*_slower_than_<leg>`); neither: level.

usage: python scripts/measure_rans.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per (input, leg) and writes them to FILE
(profiles/rans/measure_rans.jsonl)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from measure_fltpack import SEG, TILE, Leg  # noqa: E402
from measure_intpack import alternate  # noqa: E402


def inputs(np, torch, eng, B, n, seed):
    """-> (name, filter, width, the n bytes in HBM), one at a time"""
    tiles = n // TILE
    data = eng.empty(n)
    eng.fill(1, 7, data)
    eng.sync()
    yield "kind1", 0, 1, data
    rng = np.random.default_rng(seed)
    tile = rng.normal(0, 1, TILE // 4).astype("<f4").view(np.uint8)
    yield "normal_f32", B.FILTER_SHUFFLE, 4, torch.from_numpy(tile.copy()).to("cuda:0").repeat(tiles)
    tile = np.cumsum(rng.normal(0, 0.01, TILE // 4)).astype("<f4").view(np.uint8)
    yield "walk_f32", B.FILTER_SHUFFLE, 4, torch.from_numpy(tile.copy()).to("cuda:0").repeat(tiles)
    tile = rng.integers(0, 256, TILE, dtype=np.uint8)
    yield "random", 0, 1, torch.from_numpy(tile).to("cuda:0").repeat(tiles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rans", "measure_rans.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bitar_amd as B
    if not torch.cuda.is_available():
        sys.exit("measure_rans.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    n = max(a.bytes // TILE, 1) * TILE
    gib = n / float(1 << 30)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    lines = []

    for name, filt, w, cdata in inputs(np, torch, eng, B, n, a.seed):
        specs = [("rans", B.CODEC_RANS), ("lz4", B.CODEC_LZ4), ("zstd", B.CODEC_ZSTD)]
        legs = [Leg(eng, torch, B, leg, codec, filt, w, cdata) for leg, codec in specs]
        calls = {}
        for leg in legs:  # (a leg's compress runs before its decompress in every repetition)
            calls[leg.name + " compress"] = leg.compress
            calls[leg.name + " decompress"] = leg.decompress
        ms = alternate(torch, calls, a.reps, a.warmup)
        eng.sync()
        for leg in legs:
            c, d = ms[leg.name + " compress"], ms[leg.name + " decompress"]
            total = int(leg.sizes.to(torch.int64).sum().item())
            line = {
                "input": name, "filter": filt, "width": w, "leg": leg.name, "bytes": n, "seg": SEG,
                "ratio": round(n / total, 4),
                "compress_ms_per_GiB": round(statistics.median(c) / gib, 4),
                "compress_spread_ms": round(spread(c), 4),
                "decompress_ms_per_GiB": round(statistics.median(d) / gib, 4),
                "decompress_spread_ms": round(spread(d), 4),
                "compress_ms": [round(x, 3) for x in c],
                "decompress_ms": [round(x, 3) for x in d],
                "round_trip_ok": bool(torch.equal(leg.back, leg.data))}
            if leg.name == "rans":
                for other in legs[1:]:
                    for way in ("compress", "decompress"):
                        mine, theirs = ms["rans " + way], ms[other.name + " " + way]
                        margin = statistics.median(theirs) - statistics.median(mine)
                        bar = 3 * max(spread(mine), spread(theirs))
                        line[f"{way}_beats_{other.name}"] = bool(margin > bar)
                        line[f"{way}_slower_than_{other.name}"] = bool(-margin > bar)
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        del legs, calls, cdata
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
