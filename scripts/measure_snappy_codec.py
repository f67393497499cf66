#!/usr/bin/env python3
"""What a whole-buffer raw Snappy stream costs on the GPU: the join that writes
one, the boundary scan that finds its fragments, and the one-launch decode of them, against the
slab decode of the same segments and against pyarrow's Snappy decompress of the same stream on
this host's CPU.  The input stays in HBM, every GPU timing is a pair of HIP events around one
call, and the legs run alternately in this one process: each repetition runs every leg once.

Per input kind (0, 1, 2, 5, 6; --bytes of it, a 64 MiB tile repeated):
  join            bitar_hip_snappy_join of the slots of one compress
  split           bitar_hip_snappy_split of that stream, with its rounds and tile walks per tile
  joined decode   bitar_hip_snappy_decompress_joined between the starts the split found
  split + decode  the two calls in one pair of events: what the Arrow adapter's Decompress runs
  slab decode     bitar_hip_decompress_slab of the same segments (the same kernel, with preambles)
  stock split / stock decode   the same two calls on pyarrow's stream of the same bytes (made on
                  the host for one tile; the blocks are independent, so the tiles' bodies repeat)
  pyarrow         pyarrow.Codec("snappy").decompress of the engine's stream, host memory, wall clock
A line holds the medians and spreads (max - min).  The project's bar is three times the larger
spread: `first_bar` says split + decode is faster than pyarrow by more than that, `second_bar`
that joined decode and slab decode are level inside it.

usage: python scripts/measure_snappy_codec.py [--bytes N] [--reps 7] [--warmup 2] [--out FILE]
Prints one JSON line per kind and writes them to FILE
(profiles/snappy_codec/measure_snappy_codec.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from measure_fltpack import SEG, TILE, Leg  # noqa: E402
from measure_intpack import alternate  # noqa: E402

KINDS = (0, 1, 2, 5, 6)


def varint(n):
    out = bytearray()
    while n >= 128:
        out.append(n & 127 | 128)
        n >>= 7
    out.append(n)
    return bytes(out)


class Stream:
    """a raw stream in HBM with what a split and a joined decode of it need"""

    def __init__(self, eng, torch, stream, length, n):
        self.eng, self.stream, self.length, self.n = eng, stream, length, n
        nfrag = (n + SEG - 1) // SEG
        self.starts = eng.empty(nfrag + 1, dtype=torch.int64)
        self.status = eng.empty(1, dtype=torch.int32)
        self.stats = eng.empty(4, dtype=torch.int32)
        self.prod = eng.empty(nfrag, dtype=torch.int32)
        self.back = eng.empty(n)

    def split(self, max_rounds=0):
        self.eng.snappy_split(self.stream, self.length, self.n, self.starts, self.status,
                              max_rounds, self.stats)

    def decode(self):
        self.eng.decompress_joined_into(self.stream, self.length, self.n, self.starts, self.back,
                                        self.prod, capacity=self.n)

    def both(self):
        self.split()
        self.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snappy_codec",
                                                  "measure_snappy_codec.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    import torch
    import bitar_amd as B
    if not torch.cuda.is_available():
        sys.exit("measure_snappy_codec.py needs a GPU: nothing is measured without one")
    eng = B.Engine(0)
    tiles = max(a.bytes // TILE, 1)
    n = tiles * TILE
    gib = n / float(1 << 30)
    nseg = n // SEG
    spread = lambda v: max(v) - min(v)  # noqa: E731
    med = statistics.median
    codec = pa.Codec("snappy")
    lines = []
    for kind in KINDS:
        data = eng.empty(n)
        for t in range(tiles):  # (every tile the same bytes: the stock stream repeats with them)
            eng.fill(kind, a.seed, data[t * TILE:(t + 1) * TILE])
        leg = Leg(eng, torch, B, "snappy", B.CODEC_SNAPPY, 0, 1, data)
        leg.compress()
        offsets = eng.empty(nseg + 1, dtype=torch.int64)
        length = eng.empty(1, dtype=torch.int64)
        joined = eng.empty(n + 4 * nseg + 5)

        def join():
            eng.snappy_join(leg.slab, leg.stride, leg.sizes, n, offsets, joined,
                            joined_len=length)

        join()
        eng.sync()
        total = int(length.item())
        own = Stream(eng, torch, joined, total, n)
        # pyarrow's stream of the same bytes: varint(n) + the tile's body, `tiles` times
        host = data[:TILE].cpu().numpy()
        tile_stream = codec.compress(host.tobytes()).to_pybytes()
        skip = len(varint(TILE))
        body = torch.from_numpy(np.frombuffer(tile_stream, np.uint8)[skip:].copy()).to("cuda:0")
        head = torch.from_numpy(np.frombuffer(varint(n), np.uint8).copy()).to("cuda:0")
        stock_stream = torch.cat([head, body.repeat(tiles)])
        stock = Stream(eng, torch, stock_stream, stock_stream.numel(), n)
        # the rounds each stream needs when none is cut off (untimed)
        need = {}
        for name, s in (("own", own), ("stock", stock)):
            s.split(256 | B.SNAPPY_NO_SERIAL_FINISH)
            eng.sync()
            need[name] = [int(s.status.item())] + s.stats.cpu().tolist()
        own.split()
        stock.split()
        eng.sync()
        calls = {"join": join, "split": own.split, "joined decode": own.decode,
                 "split + decode": own.both, "slab decode": leg.decompress,
                 "stock split": stock.split, "stock decode": stock.decode}
        ms = alternate(torch, calls, a.reps, a.warmup)
        eng.sync()
        # pyarrow on the host, the engine's stream
        blob = joined[:total].cpu().numpy().tobytes()
        cpu = []
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            out = codec.decompress(blob, decompressed_size=n)
            t1 = time.perf_counter()
            if r >= a.warmup:
                cpu.append((t1 - t0) * 1e3)
        cpu_ok = bool(np.array_equal(np.frombuffer(out, np.uint8)[:TILE], host))
        del out, blob
        line = {"kind": kind, "bytes": n, "seg": SEG, "stream_bytes": total,
                "ratio": round(n / total, 4), "stock_stream_bytes": stock_stream.numel(),
                "status": int(own.status.item()), "stock_status": int(stock.status.item()),
                # rounds, tile walks, tiles, serial finish: of the default call, and of a call
                # that may take 256 rounds (its status first: 3 = not converged in 256)
                "split_stats": own.stats.cpu().tolist(),
                "stock_split_stats": stock.stats.cpu().tolist(),
                "rounds_needed": need["own"], "stock_rounds_needed": need["stock"],
                "walks_per_tile": round(int(own.stats[1]) / int(own.stats[2]), 3),
                "stock_walks_per_tile": round(int(stock.stats[1]) / int(stock.stats[2]), 3),
                "round_trip_ok": bool(torch.equal(own.back, data)) and bool(
                    torch.equal(stock.back, data)) and bool(torch.equal(leg.back[:n], data)),
                "pyarrow_ok": cpu_ok}
        for name, v in list(ms.items()) + [("pyarrow", cpu)]:
            key = name.replace(" + ", "_").replace(" ", "_")
            line[key + "_ms_per_GiB"] = round(med(v) / gib, 4)
            line[key + "_spread_ms"] = round(spread(v), 4)
            line[key + "_ms"] = [round(x, 3) for x in v]
        both, slab, dec = ms["split + decode"], ms["slab decode"], ms["joined decode"]
        bar1 = 3 * max(spread(both), spread(cpu))
        line["first_margin_ms"] = round(med(cpu) - med(both), 4)
        line["first_bar_ms"] = round(bar1, 4)
        line["first_bar"] = bool(med(cpu) - med(both) > bar1)
        bar2 = 3 * max(spread(dec), spread(slab))
        line["second_margin_ms"] = round(med(slab) - med(dec), 4)
        line["second_bar_ms"] = round(bar2, 4)
        line["second_bar"] = bool(abs(med(slab) - med(dec)) <= bar2)
        line["split_share"] = round(med(ms["split"]) / med(both), 4)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
        del leg, own, stock, calls, data, joined, stock_stream, body
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
