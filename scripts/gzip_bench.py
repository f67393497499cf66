#!/usr/bin/env python3
"""What the GZIP codec adds on top of the DEFLATE segment codec (HBM-resident, HIP-event timed).

  1. bitar_hip_compress for both DEFLATE codecs, this build against another build of the
     library (--other-lib, e.g. the parent commit's), in fresh child processes run alternately,
     so the difference can be read against the spread of each build against itself.
  2. deflate_join + crc32_combine as a share of the compress they follow, and deflate_split as
     a share of the decode it precedes.
  3. the gzip stream's ratio next to zlib level 1 (on a prefix of the input: zlib is slow).

usage: python scripts/gzip_bench.py [--bytes N] [--kind 1] [--reps 5] [--other-lib PATH]
Prints one JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEG = 65536


def timed(torch, fn, reps, warmup):
    s = torch.cuda.current_stream()
    ms = []
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append(a.elapsed_time(b))
    return ms


def setup(a):
    import torch
    import bitar_amd
    eng = bitar_amd.Engine(0)
    n = a.bytes
    data = eng.empty(n)
    eng.fill(a.kind, a.seed, data)
    return torch, bitar_amd, eng, n, data


def child_compress(a):
    """bitar_hip_compress of the library named by BITAR_HIP_LIB (default: this build), bound
    with ctypes directly: another build's library need not export what this one adds"""
    import ctypes
    import torch
    path = os.environ.get("BITAR_HIP_LIB") or os.path.join(ROOT, "bitar_amd", "lib",
                                                           "libbitar_hip.so")
    L = ctypes.CDLL(path)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.bitar_hip_open.argtypes = [ctypes.c_int, vp, ctypes.POINTER(vp)]
    L.bitar_hip_fill.argtypes = [vp, vp, ctypes.c_int, u64, vp, u64]
    L.bitar_hip_slot_size.restype = u64
    L.bitar_hip_slot_size.argtypes = [u32, u32]
    L.bitar_hip_compress.argtypes = [vp, vp, u32, vp, u64, u32, vp, u64, vp]
    L.bitar_hip_sync.argtypes = [vp, vp]
    L.bitar_hip_close.argtypes = [vp]

    def ok(rc):
        if rc:
            raise RuntimeError(f"libbitar_hip call failed: {rc}")
    cfg = (u32 * 2)(1, 0)
    ctx = vp()
    ok(L.bitar_hip_open(0, ctypes.byref(cfg), ctypes.byref(ctx)))
    n = a.bytes
    nseg = (n + SEG - 1) // SEG
    stream = vp(torch.cuda.current_stream(0).cuda_stream)
    data = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ok(L.bitar_hip_fill(ctx, stream, a.kind, a.seed, vp(data.data_ptr()), n))
    for name, codec in (("deflate", 2), ("deflate_dyn", 4)):
        stride = int(L.bitar_hip_slot_size(codec, SEG))
        slab = torch.empty(nseg * stride, dtype=torch.uint8, device="cuda:0")
        sizes = torch.empty(nseg, dtype=torch.int32, device="cuda:0")
        ms = timed(torch, lambda: ok(L.bitar_hip_compress(
            ctx, stream, codec, vp(data.data_ptr()), n, SEG, vp(slab.data_ptr()), stride,
            vp(sizes.data_ptr()))), a.reps, a.warmup)
        ok(L.bitar_hip_sync(ctx, stream))
        print(json.dumps({"what": "compress", "lib": os.path.relpath(path, ROOT), "codec": name,
                          "ms": [round(x, 3) for x in ms], "min_ms": round(min(ms), 3),
                          "csum": int(sizes.to(torch.int64).sum().item())}), flush=True)
        del slab
    L.bitar_hip_close(ctx)


def passes(a):
    torch, B, eng, n, data = setup(a)
    nseg = (n + SEG - 1) // SEG
    codec = B.CODEC_DEFLATE_DYNAMIC
    stride = B.slot_size(codec, SEG)
    slab, slab2 = eng.empty(nseg * stride), eng.empty(nseg * stride)
    sizes, sizes2 = eng.empty(nseg, dtype=torch.int32), eng.empty(nseg, dtype=torch.int32)
    bits = eng.empty(nseg, dtype=torch.int32)
    starts = eng.empty(nseg + 1, dtype=torch.int64)
    cap = (nseg * (stride + 1) + 3) & ~3
    joined = eng.empty(cap)
    sums = eng.empty(nseg, dtype=torch.int64)
    crc = eng.empty(1, dtype=torch.int32)
    out = eng.empty(nseg * SEG)
    prod = eng.empty(nseg, dtype=torch.int32)
    t = {}
    t["compress_bits"] = timed(torch, lambda: eng.compress_bits_into(
        codec, data, SEG, slab, stride, sizes, bits, n=n), a.reps, a.warmup)
    t["deflate_join"] = timed(torch, lambda: eng.deflate_join(
        slab, stride, sizes, bits, nseg, starts, joined, capacity=cap), a.reps, a.warmup)
    eng.sync()
    end_bits = int(starts[nseg].item())
    body = (end_bits + 7) // 8
    # the same join into a buffer of the stream's own size: how much of the pass is the memset
    t["deflate_join_tight"] = timed(torch, lambda: eng.deflate_join(
        slab, stride, sizes, bits, nseg, starts, joined, capacity=(body + 3) & ~3),
        a.reps, a.warmup)
    t["checksum_crc32"] = timed(torch, lambda: eng.checksum(B.CHECKSUM_CRC32, data, SEG, sums,
                                                            n=n), a.reps, a.warmup)
    t["crc32_combine"] = timed(torch, lambda: eng.crc32_combine(sums, n, SEG, crc),
                               a.reps, a.warmup)
    eng.sync()
    host_bits = bits.cpu().numpy().astype("uint32")
    host_slab0 = slab.view(-1, stride)[:, 0].cpu().numpy()
    entries = torch.from_numpy((host_bits | (((host_slab0 & 6) == 0).astype("uint32") << 23))
                               .astype("int32")).cuda()
    t["deflate_split"] = timed(torch, lambda: eng.deflate_split(
        joined, body, starts, entries, nseg, slab2, stride, sizes2), a.reps, a.warmup)
    t["decompress_slab"] = timed(torch, lambda: eng.decompress_slab_into(
        codec, slab2, stride, sizes2, nseg, SEG, out, prod, capacity=nseg * SEG),
        a.reps, a.warmup)
    eng.sync()
    ok = bool(torch.equal(out[:n], data)) and bool(torch.equal(sizes, sizes2))
    crc_ok = (int(crc.item()) & 0xFFFFFFFF) == zlib.crc32(data[:n].cpu().numpy().tobytes())
    for k, ms in t.items():
        print(json.dumps({"what": k, "ms": [round(x, 3) for x in ms],
                          "min_ms": round(min(ms), 3)}), flush=True)
    m = {k: min(v) for k, v in t.items()}
    gz_len = 24 + 3 * nseg + body + 8
    sample = data[:min(n, a.zlib_bytes)].cpu().numpy().tobytes()
    z = zlib.compressobj(1, zlib.DEFLATED, 31)
    zl = len(z.compress(sample)) + len(z.flush())
    print(json.dumps({
        "what": "summary", "bytes": n, "kind": a.kind, "round_trip_ok": ok, "crc_ok": crc_ok,
        "joined_bytes": body, "join_traffic_GBs": round(2 * body / (m["deflate_join_tight"] / 1e3) / 1e9, 1),
        "join_plus_combine_share_of_compress": round(
            (m["deflate_join"] + m["crc32_combine"]) / m["compress_bits"], 4),
        "split_share_of_decode": round(m["deflate_split"] / m["decompress_slab"], 4),
        "gzip_ratio": round(n / gz_len, 4),
        "zlib1_ratio_on_prefix": round(len(sample) / zl, 4), "zlib_prefix_bytes": len(sample)}),
        flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--kind", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the two libraries")
    ap.add_argument("--zlib-bytes", type=int, default=64 << 20)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "compress":
        return child_compress(a)
    if a.other_lib:
        base = [sys.executable, os.path.abspath(__file__), "--child", "compress", "--bytes",
                str(a.bytes), "--kind", str(a.kind), "--seed", str(a.seed), "--reps", str(a.reps),
                "--warmup", str(a.warmup)]
        for _ in range(a.rounds):
            for lib in (a.other_lib, None):
                env = dict(os.environ)
                env.pop("BITAR_HIP_LIB", None)
                if lib:
                    env["BITAR_HIP_LIB"] = os.path.abspath(lib)
                subprocess.run(base, env=env, check=True, timeout=600)
    passes(a)


if __name__ == "__main__":
    main()
