#!/usr/bin/env python3
"""What PATCHPACK costs and buys against INTPACK and Zstd on the columns it is for.  The input
stays in HBM, every timing is a pair of HIP events around one call (compress, or decompress), and
the legs that are compared run alternately in this one process: each repetition runs every leg
once, so drift and other people's work hit all of them alike.

Columns (tests/patchpack_cases.py; a 64 MiB tile drawn on the host, repeated to --bytes):
  timestamps   sorted int64 milliseconds, steps 1..199, 1 % gaps of 10^6..10^9
  offsets      int32 string offsets, strings of 5..39 bytes, 0.5 % of 2000..60000
  missing_high int32 in [0, 1000) with 1 % INT_MAX
  missing_low  int64 ids 10^9 + [0, 1000) with 1 % zeros
  lognormal    int32 log-normal counts (mu 3, sigma 2): a heavy tail
  uniform      int32 uniform in [0, 1000): no outliers -- what the width rule and the bitmap cost
Legs per column, all at the column's width: patchpack, intpack, zstd.
Each leg's last output is checked against its input after the timed window.  A patchpack line says
for each other leg whether PATCHPACK took less time by more than three times the larger of the two
spreads (`*_beats_<leg>`), or more time by that margin (`*_slower_than_<leg>`); neither: level.

usage: python scripts/measure_patchpack.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per (column, leg) and writes them to FILE
(profiles/patchpack/measure_patchpack.jsonl)."""
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
    import patchpack_cases as C
    rng = np.random.default_rng(seed)
    return [("timestamps", 8, C.timestamps(rng, TILE)),
            ("offsets", 4, C.string_offsets(rng, TILE)),
            ("missing_high", 4, C.missing_high(rng, TILE)),
            ("missing_low", 8, C.missing_low(rng, TILE)),
            ("lognormal", 4, C.lognormal_counts(rng, TILE)),
            ("uniform", 4, C.uniform(rng, TILE))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patchpack",
                                                  "measure_patchpack.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bitar_amd as B
    if not torch.cuda.is_available():
        sys.exit("measure_patchpack.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    tiles = max(a.bytes // TILE, 1)
    n = tiles * TILE
    gib = n / float(1 << 30)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    lines = []

    for name, w, col in columns(np, a.seed):
        assert col.size == TILE
        cdata = torch.from_numpy(col.copy()).to("cuda:0").repeat(tiles)
        specs = [("patchpack", B.codec_patchpack(w), 0), ("intpack", B.codec_intpack(w), 0),
                 ("zstd", B.CODEC_ZSTD, 0)]
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
            if leg.name == "patchpack":
                for other in legs[1:]:
                    for way in ("compress", "decompress"):
                        mine, theirs = ms["patchpack " + way], ms[other.name + " " + way]
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
