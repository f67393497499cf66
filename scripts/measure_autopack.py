#!/usr/bin/env python3
"""What AUTOPACK costs and buys against picking one of the four column codecs by hand.  The
input stays in HBM, every timing is a pair of HIP events around one call (compress, or
decompress), and the legs that are compared run alternately in this one process: each repetition
runs every leg once, so drift and other people's work hit all of them alike.

Columns (a 64 MiB tile, repeated to --bytes), all of 8-byte elements:
  timestamps   int64, 50 distinct values, sorted within the tile        (RUNPACK's headline)
  prices       float64 with two decimals                                 (FLTPACK's)
  ids40        int64 ids drawn from 40 values                            (DICTPACK's)
  kind5        the engine's synthetic int64 column, kind 5               (INTPACK's)
  mixed        the four shapes above and random values, four segments of each in turn
  random       random bytes: the stored path
Legs per column:
  autopack             AUTOPACK64; decode sorts the segments into per-format lists on the device
  autopack-peek        the same slots decoded with BITAR_HIP_AUTOPACK_LISTS=0: every format's
                       decoder looks at every segment's tag (its compress leg is the same call)
  autopack-stores      compress with BITAR_HIP_AUTOPACK_STORELESS=0: the later candidates run the
                       codecs' own kernels, which write their stored forms into the scratch too
  runpack, intpack, dictpack, fltpack     each candidate alone
  zstd                 Zstd alone
Each leg's last output is checked against its input after the timed window.  An autopack line
holds: the census of its slab; per single codec whether its decode / compress took less or more
time than AUTOPACK's by more than three times the larger of the two spreads; `compress_sum_ms` =
the sum of the four candidates' own compress medians in this run, with the same verdict against
it; the lists form against the tag-peek form; and the store-less candidates against the storing
ones.

usage: python scripts/measure_autopack.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per (column, leg) and writes them to FILE
(profiles/autopack/measure_autopack.jsonl)."""
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

KNOB = "BITAR_HIP_AUTOPACK_LISTS"
STORE_KNOB = "BITAR_HIP_AUTOPACK_STORELESS"


class PeekLeg(Leg):
    """AUTOPACK with the tag-peek decode (the knob is read at every call)"""

    def decompress(self):
        os.environ[KNOB] = "0"
        try:
            super().decompress()
        finally:
            del os.environ[KNOB]


class StoresLeg(Leg):
    """AUTOPACK whose later candidates write their stored forms too"""

    def compress(self):
        os.environ[STORE_KNOB] = "0"
        try:
            super().compress()
        finally:
            del os.environ[STORE_KNOB]


def columns(np, eng, torch, seed):
    """-> [(name, column tile as a device tensor)], each tile TILE bytes of 8-byte elements"""
    rng = np.random.default_rng(seed)
    u8 = lambda a: np.ascontiguousarray(a).view(np.uint8)  # noqa: E731
    m = TILE // 8
    stamps = u8((1_700_000_000_000 + 60_000 * np.sort(rng.integers(0, 50, m))).astype("<i8"))
    prices = u8((rng.integers(0, 100000, m) / 100.0).astype("<f8"))
    ids = u8(rng.integers(0, 1 << 63, 40).astype("<u8")[rng.integers(0, 40, m)])
    kind5 = eng.empty(TILE)
    eng.fill(5, seed + 7, kind5)
    eng.sync()
    k5 = kind5.cpu().numpy()
    noise = rng.integers(0, 256, TILE, dtype=np.uint8)
    # mixed: four segments of each shape in turn (a sorted stretch keeps its few long runs)
    shapes = [stamps, prices, ids, k5, noise]
    mixed = np.empty(TILE, np.uint8)
    step = 4 * SEG
    for k, o in enumerate(range(0, TILE, step)):
        mixed[o:o + step] = shapes[k % 5][o:o + step]
    cols = [("timestamps", stamps), ("prices", prices), ("ids40", ids), ("kind5", k5),
            ("mixed", mixed), ("random", noise)]
    return [(name, torch.from_numpy(np.ascontiguousarray(t))) for name, t in cols]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autopack",
                                                  "measure_autopack.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bitar_amd as B
    if not torch.cuda.is_available():
        sys.exit("measure_autopack.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    tiles = max(a.bytes // TILE, 1)
    n = tiles * TILE
    gib = n / float(1 << 30)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    med = statistics.median
    lines = []
    w = 8
    singles = ("runpack", "intpack", "dictpack", "fltpack")

    def verdict(line, key, mine, theirs):
        margin = med(theirs) - med(mine)
        bar = 3 * max(spread(mine), spread(theirs))
        line[f"{key}_margin_ms"] = round(margin, 4)
        line[f"{key}_bar_ms"] = round(bar, 4)
        line[f"faster_{key}"] = bool(margin > bar)
        line[f"slower_{key}"] = bool(-margin > bar)

    for name, tile in columns(np, eng, torch, a.seed):
        cdata = tile.to("cuda:0").repeat(tiles)
        specs = [("autopack", B.codec_autopack(w), Leg), ("autopack-peek", B.codec_autopack(w), PeekLeg),
                 ("autopack-stores", B.codec_autopack(w), StoresLeg),
                 ("runpack", B.codec_runpack(w), Leg), ("intpack", B.codec_intpack(w), Leg),
                 ("dictpack", B.codec_dictpack(w), Leg), ("fltpack", B.codec_fltpack(w), Leg),
                 ("zstd", B.CODEC_ZSTD, Leg)]
        legs = [cls(eng, torch, B, leg, codec, 0, w, cdata) for leg, codec, cls in specs]
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
                "compress_ms_per_GiB": round(med(c) / gib, 4),
                "compress_spread_ms": round(spread(c), 4),
                "decompress_ms_per_GiB": round(med(d) / gib, 4),
                "decompress_spread_ms": round(spread(d), 4),
                "compress_ms": [round(x, 3) for x in c],
                "decompress_ms": [round(x, 3) for x in d],
                "round_trip_ok": bool(torch.equal(leg.back, leg.data))}
            if leg.name == "autopack":
                line["census"] = eng.autopack_census(leg.slab, leg.stride, leg.sizes, leg.nseg)
                for other in singles + ("zstd",):
                    verdict(line, f"decompress_than_{other}", d, ms[other + " decompress"])
                    verdict(line, f"compress_than_{other}", c, ms[other + " compress"])
                # (the sum of four medians; its spread is taken as the largest of the four)
                parts = [ms[s + " compress"] for s in singles]
                line["compress_sum_ms"] = round(sum(med(p) for p in parts), 4)
                margin = line["compress_sum_ms"] - med(c)
                bar = 3 * max([spread(c)] + [spread(p) for p in parts])
                line["compress_than_sum_margin_ms"] = round(margin, 4)
                line["compress_than_sum_bar_ms"] = round(bar, 4)
                line["faster_compress_than_sum"] = bool(margin > bar)
                line["slower_compress_than_sum"] = bool(-margin > bar)
                verdict(line, "decompress_than_peek", d, ms["autopack-peek decompress"])
                verdict(line, "compress_than_stores", c, ms["autopack-stores compress"])
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        del legs, calls, cdata
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
