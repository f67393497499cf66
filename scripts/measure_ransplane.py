#!/usr/bin/env python3
"""What RANSPLANE costs and buys against RANS, LZ4 and Zstd behind the shuffle filter on float
and weight tensors.  The input stays in HBM, every timing is a pair of HIP events around one call
(compress, or decompress; with a filter the filter's kernel is inside the pair), and the legs that
are compared run alternately in this one process: each repetition runs every leg once, so drift
and other people's work hit all of them alike.

Inputs (1 GiB, 64 KiB segments, a 64 MiB tile repeated):
  bf16_weights  N(0, 0.02) float32 truncated to its high 16 bits, width 2
  normal_f32    N(0,1) float32, width 4
  walk_f32      a smooth float32 walk, width 4
  normal_f64    N(0,1) float64, width 8
  random        random bytes, width 4
Legs per input: ransplane at the width (no filter), then rans, lz4 and zstd, each behind the
shuffle filter at the width.
Each leg's last output is checked against its input after the timed window.  A ransplane line
says for each other leg whether RANSPLANE took less time by more than three times the larger of
the two spreads (`*_beats_<leg>`), or more time by that margin (`*_slower_than_<leg>`); neither:
level.

usage: python scripts/measure_ransplane.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per (input, leg) and writes them to FILE
(profiles/ransplane/measure_ransplane.jsonl)."""
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


def inputs(np, torch, n, seed):
    """-> (name, element width, the n bytes in HBM), one at a time"""
    tiles = n // TILE
    rng = np.random.default_rng(seed)
    up = lambda t: torch.from_numpy(t.view(np.uint8).copy()).to("cuda:0").repeat(tiles)  # noqa: E731
    x = rng.normal(0, 0.02, TILE // 2).astype("<f4")
    yield "bf16_weights", 2, up((x.view("<u4") >> 16).astype("<u2"))
    yield "normal_f32", 4, up(rng.normal(0, 1, TILE // 4).astype("<f4"))
    yield "walk_f32", 4, up(np.cumsum(rng.normal(0, 0.01, TILE // 4)).astype("<f4"))
    yield "normal_f64", 8, up(rng.normal(0, 1, TILE // 8).astype("<f8"))
    yield "random", 4, up(rng.integers(0, 256, TILE, dtype=np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransplane",
                                                  "measure_ransplane.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bitar_amd as B
    if not torch.cuda.is_available():
        sys.exit("measure_ransplane.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    n = max(a.bytes // TILE, 1) * TILE
    gib = n / float(1 << 30)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    lines = []

    for name, w, cdata in inputs(np, torch, n, a.seed):
        specs = [("ransplane", B.codec_ransplane(w), 0), ("rans", B.CODEC_RANS, B.FILTER_SHUFFLE),
                 ("lz4", B.CODEC_LZ4, B.FILTER_SHUFFLE), ("zstd", B.CODEC_ZSTD, B.FILTER_SHUFFLE)]
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
                "input": name, "filter": leg.filt, "width": w, "leg": leg.name, "bytes": n,
                "seg": SEG, "ratio": round(n / total, 4),
                "compress_ms_per_GiB": round(statistics.median(c) / gib, 4),
                "compress_spread_ms": round(spread(c), 4),
                "decompress_ms_per_GiB": round(statistics.median(d) / gib, 4),
                "decompress_spread_ms": round(spread(d), 4),
                "compress_ms": [round(x, 3) for x in c],
                "decompress_ms": [round(x, 3) for x in d],
                "round_trip_ok": bool(torch.equal(leg.back, leg.data))}
            if leg.name == "ransplane":
                for other in legs[1:]:
                    for way in ("compress", "decompress"):
                        mine, theirs = ms["ransplane " + way], ms[other.name + " " + way]
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
