#!/usr/bin/env python3
"""What SYMTAB costs and buys against LZ4, RANS and Zstd on string data.  The input stays in HBM,
every timing is a pair of HIP events around one call (compress, or decompress), and the legs that
are compared run alternately in this one process: each repetition runs every leg once, so drift
and other people's work hit all of them alike.

Inputs (1 GiB, 64 KiB segments):
  kind6    the engine's generator of log text (fill kind 6)
  names    person names of syllable words (tests/symtab_cases.py), a 4 MiB tile repeated
  random   random bytes (a 64 MiB tile, repeated)
Legs per input: symtab, lz4, rans, zstd.
Each leg's last output is checked against its input after the timed window.  A symtab line says
for each other leg whether SYMTAB took less time by more than three times the larger of the two
spreads (`*_beats_<leg>`), or more time by that margin (`*_slower_than_<leg>`); neither: level.

usage: python scripts/measure_symtab.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per (input, leg) and writes them to FILE
(profiles/symtab/measure_symtab.jsonl)."""
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

NAMES_TILE = 4 << 20


def inputs(np, torch, eng, n, seed):
    """-> (name, the n bytes in HBM), one at a time"""
    import symtab_cases as C
    data = eng.empty(n)
    eng.fill(6, 1, data)
    eng.sync()
    yield "kind6", data
    tile = C.names(NAMES_TILE)
    yield "names", torch.from_numpy(tile).to("cuda:0").repeat(n // NAMES_TILE)
    tile = np.random.default_rng(seed).integers(0, 256, TILE, dtype=np.uint8)
    yield "random", torch.from_numpy(tile).to("cuda:0").repeat(n // TILE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "symtab", "measure_symtab.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bitar_amd as B
    if not torch.cuda.is_available():
        sys.exit("measure_symtab.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    n = max(a.bytes // TILE, 1) * TILE
    gib = n / float(1 << 30)
    spread = lambda v: max(v) - min(v)  # noqa: E731
    lines = []

    for name, cdata in inputs(np, torch, eng, n, a.seed):
        specs = [("symtab", B.CODEC_SYMTAB), ("lz4", B.CODEC_LZ4), ("rans", B.CODEC_RANS),
                 ("zstd", B.CODEC_ZSTD)]
        legs = [Leg(eng, torch, B, leg, codec, 0, 1, cdata) for leg, codec in specs]
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
                "input": name, "leg": leg.name, "bytes": n, "seg": SEG,
                "ratio": round(n / total, 4),
                "compress_ms_per_GiB": round(statistics.median(c) / gib, 4),
                "compress_spread_ms": round(spread(c), 4),
                "decompress_ms_per_GiB": round(statistics.median(d) / gib, 4),
                "decompress_spread_ms": round(spread(d), 4),
                "compress_ms": [round(x, 3) for x in c],
                "decompress_ms": [round(x, 3) for x in d],
                "round_trip_ok": bool(torch.equal(leg.back, leg.data))}
            if leg.name == "symtab":
                for other in legs[1:]:
                    for way in ("compress", "decompress"):
                        mine, theirs = ms["symtab " + way], ms[other.name + " " + way]
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
