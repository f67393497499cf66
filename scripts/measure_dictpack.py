#!/usr/bin/env python3
"""What DICTPACK costs and buys against the ways a low-cardinality column of wide values could
be stored before it.  The input stays in HBM, every timing is a pair of HIP events around one
call (compress, or decompress), and the legs that are compared run alternately in this one
process: each repetition runs every leg once, so drift and other people's work hit all of them
alike.

Columns (a 64 MiB tile drawn on the host, repeated to --bytes):
  ids          int64, 40 distinct values of 63 random bits
  reals        float64, 200 distinct N(0,1) values
  uuids        16-byte values, 500 distinct, all bytes random
  random       random bytes as 8-byte elements: more than 1024 values, the stored path
Legs per column:
  dictpack             bitar_hip_compress / _decompress_slab with the DICTPACK id of the width
  bitshuffle + lz4     filter_into + LZ4 compress; LZ4 decompress + unfilter_into
  zstd                 Zstd alone
  intpack64 (indices)  INTPACK64 on the draws themselves, as int64 (as many bytes as the column):
                       the same memory work and bit widths without the hash table and the
                       lookup, so it bounds what those cost
Each leg's last output is checked against its input after the timed window.  The dictpack line
also says whether it beat Zstd by more than three times the larger of the two spreads.

usage: python scripts/measure_dictpack.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per (column, leg) and writes them to FILE
(profiles/dictpack/measure_dictpack.jsonl)."""
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


def columns(np, seed):
    """-> [(name, width, column tile, int64 index tile)], each tile TILE bytes"""
    rng = np.random.default_rng(seed)
    out = []
    for name, w, values in (
            ("ids", 8, rng.integers(0, 1 << 63, 40).astype("<u8").view(np.uint8).reshape(40, 8)),
            ("reals", 8, rng.normal(0, 1, 200).astype("<f8").view(np.uint8).reshape(200, 8)),
            ("uuids", 16, rng.integers(0, 256, (500, 16), dtype=np.uint8))):
        assert np.unique(values, axis=0).shape[0] == values.shape[0]
        draws = rng.integers(0, values.shape[0], TILE // 8)
        out.append((name, w, values[draws[:TILE // w]].reshape(-1), draws.astype("<i8")))
    out.append(("random", 8, rng.integers(0, 256, TILE, dtype=np.uint8),
                rng.integers(-2 ** 63, 2 ** 63 - 1, TILE // 8).astype("<i8")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dictpack",
                                                  "measure_dictpack.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bitar_amd as B
    if not torch.cuda.is_available():
        sys.exit("measure_dictpack.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    tiles = max(a.bytes // TILE, 1)
    n = tiles * TILE
    gib = n / float(1 << 30)
    lines = []
    for name, w, col, idx in columns(np, a.seed):
        up = lambda t: torch.from_numpy(t.view(np.uint8)).to("cuda:0").repeat(tiles)  # noqa: E731
        cdata, idata = up(col), up(idx)
        legs = [Leg(eng, torch, B, *spec) for spec in (
            ("dictpack", B.codec_dictpack(w), 0, w, cdata),
            ("bitshuffle+lz4", B.CODEC_LZ4, B.FILTER_BITSHUFFLE, w, cdata),
            ("zstd", B.CODEC_ZSTD, 0, w, cdata),
            ("intpack64 (indices)", B.CODEC_INTPACK64, 0, 8, idata))]
        calls = {}
        for leg in legs:  # (a leg's compress runs before its decompress in every repetition)
            calls[leg.name + " compress"] = leg.compress
            calls[leg.name + " decompress"] = leg.decompress
        ms = alternate(torch, calls, a.reps, a.warmup)
        eng.sync()
        spread = lambda v: max(v) - min(v)  # noqa: E731
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
            if leg.name == "dictpack":
                for way in ("compress", "decompress"):
                    mine, zstd = ms["dictpack " + way], ms["zstd " + way]
                    margin = statistics.median(zstd) - statistics.median(mine)
                    line[way + "_beats_zstd"] = bool(margin > 3 * max(spread(mine), spread(zstd)))
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        del legs, calls, cdata, idata
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
