#!/usr/bin/env python3
"""What DECPACK costs and buys on decimal128 columns against everything else the engine can do
with 16-byte elements.  The input stays in HBM, every timing is a pair of HIP events around one
call (compress, or decompress), and the legs that are compared run alternately in this one
process: each repetition runs every leg once, so drift and other people's work hit all of them
alike.

Columns (tests/decpack_cases.py; a 64 MiB tile drawn on the host, repeated to --bytes):
  prices   DECIMAL(12,2) prices, unscaled values uniform in [0, 10^7)
  amounts  signed amounts in +-10^6: high bytes 00 and FF side by side
  total    an ascending running total that passes 2^64 (delta mode)
  random   random 16-byte values (stored)
Legs per column: decpack, dictpack128, runpack128, autopack128, shuffle(16) + lz4,
bitshuffle(16) + lz4, zstd, and intpack64 over the low halves alone (half the bytes, the same
number of elements): the same bits packed with 64-bit arithmetic, which is what shows the cost of
the 128-bit path.  Its `*_ms_per_column_GiB` is its time over the column's size, to be read next
to decpack's ms/GiB; its ratio is over its own half.
Each leg's last output is checked against its input after the timed window.  A decpack line says
for each other leg whether DECPACK took less time by more than three times the larger of the two
spreads (`*_beats_<leg>`), or more time by that margin (`*_slower_than_<leg>`); neither: level.

usage: python scripts/measure_decpack.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per (column, leg) and writes them to FILE
(profiles/decpack/measure_decpack.jsonl)."""
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
    """-> [(name, column tile)], each tile TILE bytes"""
    import decpack_cases as C
    rng = np.random.default_rng(seed)
    return [("prices", C.prices(rng, TILE)), ("amounts", C.signed_amounts(rng, TILE)),
            ("total", C.running_total(rng, TILE)), ("random", C.random_values(rng, TILE))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decpack",
                                                  "measure_decpack.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bitar_amd as B
    import decpack_model as M
    if not torch.cuda.is_available():
        sys.exit("measure_decpack.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    tiles = max(a.bytes // TILE, 1)
    n = tiles * TILE
    gib = n / float(1 << 30)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    lines = []

    for name, col in columns(np, a.seed):
        assert col.size == TILE
        # the ratio the format's arithmetic gives: the model's sizes of the tile's first segments
        model = [len(s) for s in M.encode(col[:16 * SEG], SEG)]
        cdata = torch.from_numpy(col.copy()).to("cuda:0").repeat(tiles)
        low = torch.from_numpy(col.view("<u8")[0::2].copy().view(np.uint8)).to("cuda:0").repeat(tiles)
        specs = [("decpack", B.codec_decpack(16), 0, 16, cdata),
                 ("dictpack128", B.codec_dictpack(16), 0, 16, cdata),
                 ("runpack128", B.codec_runpack(16), 0, 16, cdata),
                 ("autopack128", B.codec_autopack(16), 0, 16, cdata),
                 ("shuffle16+lz4", B.CODEC_LZ4, B.FILTER_SHUFFLE, 16, cdata),
                 ("bitshuffle16+lz4", B.CODEC_LZ4, B.FILTER_BITSHUFFLE, 16, cdata),
                 ("zstd", B.CODEC_ZSTD, 0, 16, cdata),
                 ("intpack64_low_halves", B.codec_intpack(8), 0, 8, low)]
        legs = [Leg(eng, torch, B, leg, codec, filt, w, data) for leg, codec, filt, w, data in specs]
        calls = {}
        for leg in legs:  # (a leg's compress runs before its decompress in every repetition)
            calls[leg.name + " compress"] = leg.compress
            calls[leg.name + " decompress"] = leg.decompress
        ms = alternate(torch, calls, a.reps, a.warmup)
        eng.sync()
        for leg in legs:
            c, d = ms[leg.name + " compress"], ms[leg.name + " decompress"]
            sizes = leg.sizes.to(torch.int64)
            total = int(sizes.sum().item())
            own = leg.n / float(1 << 30)
            line = {
                "column": name, "leg": leg.name, "bytes": leg.n, "seg": SEG,
                "ratio": round(leg.n / total, 4),
                "compress_ms_per_GiB": round(statistics.median(c) / own, 4),
                "compress_spread_ms": round(spread(c), 4),
                "decompress_ms_per_GiB": round(statistics.median(d) / own, 4),
                "decompress_spread_ms": round(spread(d), 4),
                "compress_ms": [round(x, 3) for x in c],
                "decompress_ms": [round(x, 3) for x in d],
                "round_trip_ok": bool(torch.equal(leg.back, leg.data))}
            if leg.n != n:
                line["compress_ms_per_column_GiB"] = round(statistics.median(c) / gib, 4)
                line["decompress_ms_per_column_GiB"] = round(statistics.median(d) / gib, 4)
            if leg.name == "decpack":
                line["model_ratio_first_16_segments"] = round(16 * SEG / sum(model), 4)
                line["sizes_equal_model"] = sizes[:16].tolist() == model
                for other in legs[1:]:
                    for way in ("compress", "decompress"):
                        mine, theirs = ms["decpack " + way], ms[other.name + " " + way]
                        margin = statistics.median(theirs) - statistics.median(mine)
                        bar = 3 * max(spread(mine), spread(theirs))
                        line[f"{way}_beats_{other.name}"] = bool(margin > bar)
                        line[f"{way}_slower_than_{other.name}"] = bool(-margin > bar)
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        del legs, calls, cdata, low
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
