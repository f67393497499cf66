#!/usr/bin/env python3
"""What the segment filters (bitar_hip_filter_apply / _invert) cost and buy.  The input stays
in HBM, every timing is a pair of HIP events, and the legs that are compared run alternately
in this one process: each repetition runs every leg once, so drift hits all of them alike.

  1. yardsticks: SHUFFLE moves the bytes a device-to-device bitar_hip_memcpy moves, so apply
     and invert (w = 4 and 8) are held to 2x that copy's median; BITSHUFFLE does ALU work per
     bit plane and is held to the LZ4 decode of the same kind-5 input, the fastest stage a
     filter ever accompanies (w = 8).
  2. for kinds 5 and 2 and LZ4 / Zstd / dynamic DEFLATE: ratio and ms/GiB of compress and
     decompress without a filter and with each (width 8), the filter's time included.

usage: python scripts/filter_bench.py [--bytes N] [--reps 5] [--warmup 2] [--skip-codecs]
Prints one JSON line per measurement."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEG = 65536


def alternate(torch, legs, reps, warmup):
    """{name: [ms, ...]}: every repetition runs each leg once, in order"""
    s = torch.cuda.current_stream()
    ms = {k: [] for k in legs}
    for r in range(warmup + reps):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize()
            if r >= warmup:
                ms[name].append(a.elapsed_time(b))
    return ms


def stats(ms):
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4),
            "spread_ms": round(max(ms) - min(ms), 4)}


def yardsticks(a, torch, B, eng):
    n = a.bytes
    nseg = (n + SEG - 1) // SEG
    data, out, back = eng.empty(n), eng.empty(n), eng.empty(n)
    eng.fill(5, a.seed, data)
    slab, stride, sizes = eng.compress(B.CODEC_LZ4, data, SEG)
    prod = eng.empty(nseg, dtype=torch.int32)
    lib = B.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    vp = ctypes.c_void_p
    legs = {"copy_d2d": lambda: B.check(lib.bitar_hip_memcpy(
        eng.ctx, vp(out.data_ptr()), vp(data.data_ptr()), n, stream))}
    for name, filt, widths in (("shuffle", B.FILTER_SHUFFLE, (4, 8)),
                               ("bitshuffle", B.FILTER_BITSHUFFLE, (8,))):
        for w in widths:
            legs[f"{name}_apply_w{w}"] = \
                lambda filt=filt, w=w: eng.filter_into(filt, w, data, SEG, out)
            legs[f"{name}_invert_w{w}"] = \
                lambda filt=filt, w=w: eng.unfilter_into(filt, w, out, SEG, back)
    legs["lz4_decode_kind5"] = lambda: eng.decompress_slab_into(
        B.CODEC_LZ4, slab, stride, sizes, nseg, SEG, out, prod, capacity=nseg * SEG)
    ms = alternate(torch, legs, a.reps, a.warmup)
    eng.sync()
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        rec = {"what": k, "bytes": n, "seg": SEG, **stats(v)}
        rec["GBs_read_plus_written"] = round(2 * n / (med[k] / 1e3) / 1e9, 1)
        if k.startswith("shuffle"):
            rec["x_copy"] = round(med[k] / med["copy_d2d"], 3)
            rec["within_2x_copy"] = bool(med[k] <= 2 * med["copy_d2d"])
        if k.startswith("bitshuffle"):
            rec["x_lz4_decode"] = round(med[k] / med["lz4_decode_kind5"], 3)
            rec["within_lz4_decode"] = bool(med[k] <= med["lz4_decode_kind5"])
        print(json.dumps(rec), flush=True)
    # the legs' last outputs: invert(apply(data)) of the last filter timed, and the decode
    ok = bool(torch.equal(out, data))
    eng.filter_into(B.FILTER_BITSHUFFLE, 8, data, SEG, out)
    eng.unfilter_into(B.FILTER_BITSHUFFLE, 8, out, SEG, back)
    eng.sync()
    print(json.dumps({"what": "yardstick_check", "lz4_round_trip_ok": ok,
                      "filter_round_trip_ok": bool(torch.equal(back, data))}), flush=True)


def codecs(a, torch, B, eng):
    n = a.bytes
    nseg = (n + SEG - 1) // SEG
    gib = n / float(1 << 30)
    data, filtered, out, back = eng.empty(n), eng.empty(n), eng.empty(n), eng.empty(n)
    prod = eng.empty(nseg, dtype=torch.int32)
    sizes = eng.empty(nseg, dtype=torch.int32)
    w = a.width
    for kind in (5, 2):
        eng.fill(kind, a.seed, data)
        for cname, codec, dcodec in (("lz4", B.CODEC_LZ4, B.CODEC_LZ4),
                                     ("zstd", B.CODEC_ZSTD, B.CODEC_ZSTD),
                                     ("deflate_dyn", B.CODEC_DEFLATE_DYNAMIC, B.CODEC_DEFLATE)):
            stride = B.slot_size(codec, SEG)
            slab = eng.empty(nseg * stride)
            for fname, filt in (("none", 0), ("shuffle", B.FILTER_SHUFFLE),
                                ("bitshuffle", B.FILTER_BITSHUFFLE)):
                def comp():
                    src = data
                    if filt:
                        eng.filter_into(filt, w, data, SEG, filtered)
                        src = filtered
                    eng.compress_into(codec, src, SEG, slab, stride, sizes, n=n)

                def decomp():
                    dst = out if filt else back
                    eng.decompress_slab_into(dcodec, slab, stride, sizes, nseg, SEG, dst, prod,
                                             capacity=nseg * SEG)
                    if filt:
                        eng.unfilter_into(filt, w, out, SEG, back, n=n, lens=prod, nseg=nseg)
                # compress first (decomp reads its slots), then the two alternately
                comp()
                ms = alternate(torch, {"compress": comp, "decompress": decomp}, a.reps, a.warmup)
                eng.sync()
                total = int(sizes.to(torch.int64).sum().item())
                print(json.dumps({
                    "what": "codec", "kind": kind, "codec": cname, "filter": fname,
                    "width": w if filt else None, "bytes": n, "ratio": round(n / total, 4),
                    "compress_ms_per_GiB": round(statistics.median(ms["compress"]) / gib, 4),
                    "compress_ms": [round(x, 3) for x in ms["compress"]],
                    "decompress_ms_per_GiB": round(statistics.median(ms["decompress"]) / gib, 4),
                    "decompress_ms": [round(x, 3) for x in ms["decompress"]],
                    "round_trip_ok": bool(torch.equal(back, data))}), flush=True)
            del slab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=8, help="element width of the codec runs")
    ap.add_argument("--skip-codecs", action="store_true")
    a = ap.parse_args()
    import torch
    import bitar_amd as B
    eng = B.Engine(0)
    yardsticks(a, torch, B, eng)
    if not a.skip_codecs:
        codecs(a, torch, B, eng)
    eng.close()


if __name__ == "__main__":
    main()
