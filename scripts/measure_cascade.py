#!/usr/bin/env python3
"""What CASCADE costs and buys against RUNPACK, INTPACK and Zstd on the columns it is for.  The
input stays in HBM, every timing is a pair of HIP events around one call (compress, or
decompress), and the legs that are compared run alternately in this one process: each repetition
runs every leg once, so drift and other people's work hit all of them alike.

Columns (tests/cascade_cases.py; a 64 MiB tile drawn on the host, repeated to --bytes):
  sorted_keys  int32, sorted, runs of geometric length, mean 20, neighbouring keys 1..8 apart
  ticks        int64 millisecond timestamps one second apart, about 50 rows per tick
  status       int32 codes 0..15 drawn at random, runs of mean 30
  random_keys  int64 random keys in runs of mean 20: runs whose values nothing packs
Legs per column, all at the column's width: cascade, runpack, intpack, zstd.
Each leg's last output is checked against its input after the timed window.  A cascade line says
for each other leg whether CASCADE took less time by more than three times the larger of the two
spreads (`*_beats_<leg>`), or more time by that margin (`*_slower_than_<leg>`); neither: level.

usage: python scripts/measure_cascade.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per (column, leg) and writes them to FILE
(profiles/cascade/measure_cascade.jsonl)."""
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


def columns(np, seed):
    """-> [(name, width, column tile)], each tile TILE bytes"""
    import cascade_cases as C
    rng = np.random.default_rng(seed)
    return [("sorted_keys", 4, C.sorted_keys(rng, TILE, 4, 20, 8)),
            ("ticks", 8, C.ticks(rng, TILE, 50)),
            ("status", 4, C.status(rng, TILE, 4, 30, 16)),
            ("random_keys", 8, C.random_keys(rng, TILE, 8, 20))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascade",
                                                  "measure_cascade.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bitar_amd as B
    if not torch.cuda.is_available():
        sys.exit("measure_cascade.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    tiles = max(a.bytes // TILE, 1)
    n = tiles * TILE
    gib = n / float(1 << 30)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    lines = []

    for name, w, col in columns(np, a.seed):
        assert col.size == TILE
        cdata = torch.from_numpy(col.copy()).to("cuda:0").repeat(tiles)
        specs = [("cascade", B.codec_cascade(w), 0), ("runpack", B.codec_runpack(w), 0),
                 ("intpack", B.codec_intpack(w), 0), ("zstd", B.CODEC_ZSTD, 0)]
        legs = [Leg(eng, torch, B, leg, codec, filt, w, cdata) for leg, codec, filt in specs]
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
                "column": name, "width": w, "leg": leg.name, "bytes": n, "seg": SEG,
                "ratio": round(n / total, 4),
                "compress_ms_per_GiB": round(statistics.median(c) / gib, 4),
                "compress_spread_ms": round(spread(c), 4),
                "decompress_ms_per_GiB": round(statistics.median(d) / gib, 4),
                "decompress_spread_ms": round(spread(d), 4),
                "compress_ms": [round(x, 3) for x in c],
                "decompress_ms": [round(x, 3) for x in d],
                "round_trip_ok": bool(torch.equal(leg.back, leg.data))}
            if leg.name == "cascade":
                for other in legs[1:]:
                    for way in ("compress", "decompress"):
                        mine, theirs = ms["cascade " + way], ms[other.name + " " + way]
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
