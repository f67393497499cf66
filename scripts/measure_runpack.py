#!/usr/bin/env python3
"""What RUNPACK costs and buys against the ways a sorted or clustered column could be stored
before it.  The input stays in HBM, every timing is a pair of HIP events around one call
(compress, or decompress), and the legs that are compared run alternately in this one process:
each repetition runs every leg once, so drift and other people's work hit all of them alike.

Columns (a 64 MiB tile drawn on the host, repeated to --bytes):
  timestamps   int64, 50 distinct values, sorted within the tile
  ids16        16-byte values in runs of geometric length, mean 500
  flags        bytes 0x00 / 0xFF in alternating runs of geometric length, mean 200
  keys         int32 drawn from 1000 values, runs of geometric length, mean 20
  random       random bytes as 1-byte elements and, for w = 1 against w = 8, as 8-byte ones:
               the stored path
Legs per column:
  runpack              bitar_hip_compress / _decompress_slab with the RUNPACK id of the width
  intpack              INTPACK of the width (it takes delta where that is smaller); widths 1..8
  dictpack             DICTPACK of the width; widths 4..16
  zstd                 Zstd alone
  bitshuffle + lz4     filter_into + LZ4 compress; LZ4 decompress + unfilter_into (LZ4 alone for
                       1-byte elements, which the filters do not take)
and once per run `memset`, hipMemsetAsync of --bytes: the store-only floor of a decoder.
Each leg's last output is checked against its input after the timed window.  A runpack line
says for each other leg whether RUNPACK took less time by more than three times the larger of
the two spreads (`*_beats_<leg>`), or more time by that margin (`*_slower_than_<leg>`).

usage: python scripts/measure_runpack.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per (column, leg) and writes them to FILE
(profiles/runpack/measure_runpack.jsonl)."""
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


def geometric_runs(np, rng, m, mean, values):
    """m elements in runs of geometric length, run k's value a row of `values`"""
    lengths = rng.geometric(1.0 / mean, m // mean + 1024)
    while lengths.sum() < m:
        lengths = np.append(lengths, rng.geometric(1.0 / mean, 4096))
    if values.shape[0] == 2:
        rows = values[np.arange(lengths.size) & 1]
    else:
        rows = values[rng.integers(0, values.shape[0], lengths.size)]
    return np.repeat(rows, lengths, axis=0)[:m].reshape(-1)


def columns(np, seed):
    """-> [(name, width, column tile)], each tile TILE bytes"""
    rng = np.random.default_rng(seed)
    u8 = lambda a: np.ascontiguousarray(a).view(np.uint8)  # noqa: E731
    stamps = 1_700_000_000_000 + 60_000 * np.sort(rng.integers(0, 50, TILE // 8))
    ids = rng.integers(0, 256, (4000, 16), dtype=np.uint8)
    flags = np.array([[0x00], [0xFF]], np.uint8)
    keys = u8(rng.integers(0, 1 << 31, 1000).astype("<u4")).reshape(1000, 4)
    noise = rng.integers(0, 256, TILE, dtype=np.uint8)
    return [("timestamps", 8, u8(stamps.astype("<i8"))),
            ("ids16", 16, geometric_runs(np, rng, TILE // 16, 500, ids)),
            ("flags", 1, geometric_runs(np, rng, TILE, 200, flags)),
            ("keys", 4, geometric_runs(np, rng, TILE // 4, 20, keys)),
            ("random", 1, noise),
            ("random", 8, noise)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "runpack",
                                                  "measure_runpack.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bitar_amd as B
    if not torch.cuda.is_available():
        sys.exit("measure_runpack.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    tiles = max(a.bytes // TILE, 1)
    n = tiles * TILE
    gib = n / float(1 << 30)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    lines = []

    # the store-only floor
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    floor = eng.empty(n)

    def memset():
        if hip.hipMemsetAsync(floor.data_ptr(), 0x5A, n, torch.cuda.current_stream().cuda_stream):
            sys.exit("hipMemsetAsync failed")

    ms = alternate(torch, {"memset": memset}, a.reps, a.warmup)["memset"]
    assert bool((floor == 0x5A).all())
    del floor
    lines.append(json.dumps({"column": "-", "leg": "memset", "bytes": n,
                             "ms_per_GiB": round(statistics.median(ms) / gib, 4),
                             "spread_ms": round(spread(ms), 4), "ms": [round(x, 3) for x in ms]}))
    print(lines[-1], flush=True)

    for name, w, col in columns(np, a.seed):
        cdata = torch.from_numpy(col).to("cuda:0").repeat(tiles)
        specs = [("runpack", B.codec_runpack(w), 0)]
        if w <= 8:
            specs.append(("intpack", B.codec_intpack(w), 0))
        if w >= 4:
            specs.append(("dictpack", B.codec_dictpack(w), 0))
        specs.append(("zstd", B.CODEC_ZSTD, 0))
        if w >= 2:
            specs.append(("bitshuffle+lz4", B.CODEC_LZ4, B.FILTER_BITSHUFFLE))
        else:  # (the filters start at 2-byte elements)
            specs.append(("lz4", B.CODEC_LZ4, 0))
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
            if leg.name == "runpack":
                for other in legs[1:]:
                    for way in ("compress", "decompress"):
                        mine, theirs = ms["runpack " + way], ms[other.name + " " + way]
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
