#!/usr/bin/env python3
"""How the headline's two LZ4 launches end: a per-workgroup timeline from a probe build.

The probe build (scripts/build_variant.sh NAME "-DBITAR_LAUNCH_TIMELINE=1 ...", selected with
BITAR_HIP_LIB) makes lz4_compress_kernel and lz4_decompress_kernel<false> record per workgroup
its dispatch index, its segment and the device's 100 MHz wall clock at entry and before exit
(order.hip.h).  This script runs the headline's compress and decompress once each after a
warm-up and prints, per kernel: resident workgroups over time, when the last dense workgroup
was dispatched, the duration of dense and cheap segments by dispatch decile, and the tail
(from the last moment at which at least half the slots were taken to the end).  Never quote
the probe build's run time as the kernels': the stamps cost a little.

usage: BITAR_HIP_LIB=.../libbitar_hip_NAME.so python scripts/launch_timeline.py
           [--bytes N --seg N --kind K --out FILE.json --raw FILE.npz]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TICK_US = 0.01  # wall_clock64(): 100 MHz


def analyse(name, rec, cheap_of_seg, slots):
    import numpy as np
    rec = rec.reshape(-1, 3)
    live = rec[:, 2] != 0
    b = (rec[:, 0] >> np.uint64(32))[live].astype(np.int64)
    seg = (rec[:, 0] & np.uint64(0xFFFFFFFF))[live].astype(np.int64)
    t0 = rec[live, 1].astype(np.float64)
    t1 = rec[live, 2].astype(np.float64)
    origin = t0.min()
    t0 = (t0 - origin) * TICK_US
    t1 = (t1 - origin) * TICK_US
    end = float(t1.max())
    cheap = cheap_of_seg[seg]
    dense = ~cheap
    # resident workgroups over time: +1 at entry, -1 at exit
    ev_t = np.concatenate([t0, t1])
    ev_d = np.concatenate([np.ones_like(t0), -np.ones_like(t1)])
    o = np.lexsort((ev_d, ev_t))  # (at equal times the exits first)
    ev_t, res = ev_t[o], np.cumsum(ev_d[o])
    grid = np.linspace(0, end, 41)
    at = np.searchsorted(ev_t, grid, side="right") - 1
    resident = [int(res[max(k, 0)]) for k in at]
    slots = slots or int(res.max())
    half = slots / 2
    above = np.nonzero(res >= half)[0]
    tail_from = float(ev_t[above[-1] + 1]) if above.size and above[-1] + 1 < ev_t.size else 0.0

    def deciles(mask):
        idx = np.nonzero(mask)[0]
        if idx.size == 0:
            return []
        idx = idx[np.argsort(b[idx])]
        out = []
        for part in np.array_split(idx, 10):
            if part.size:
                d = t1[part] - t0[part]
                out.append({"first_b": int(b[part[0]]), "n": int(part.size),
                            "median_us": round(float(np.median(d)), 1),
                            "max_us": round(float(d.max()), 1)})
        return out

    r = {
        "kernel": name, "workgroups": int(live.sum()), "dense": int(dense.sum()),
        "cheap": int(cheap.sum()), "slots": slots, "peak_resident": int(res.max()),
        "makespan_us": round(end, 1),
        "last_dense_dispatch_us": round(float(t0[dense].max()), 1) if dense.any() else None,
        "last_dense_end_us": round(float(t1[dense].max()), 1) if dense.any() else None,
        "last_cheap_dispatch_us": round(float(t0[cheap].max()), 1) if cheap.any() else None,
        "tail_from_us": round(tail_from, 1), "tail_us": round(end - tail_from, 1),
        "resident_grid_us": [round(float(g), 1) for g in grid], "resident": resident,
        "dense_by_dispatch_decile": deciles(dense), "cheap_by_dispatch_decile": deciles(cheap),
    }
    return r, {"b": b, "seg": seg, "t0": t0, "t1": t1, "cheap": cheap}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seg", type=int, default=65536)
    ap.add_argument("--kind", type=int, default=1)
    ap.add_argument("--slots-compress", type=int, default=0, help="0: what the runtime found")
    ap.add_argument("--slots-decompress", type=int, default=0)
    ap.add_argument("--out", default=None, help="write the summary as JSON")
    ap.add_argument("--raw", default=None, help="write the raw records (.npz, launch_sim.py)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import bitar_amd
    L = bitar_amd.lib()
    try:
        setters = [getattr(L, "bitar_hip_timeline_compress"),
                   getattr(L, "bitar_hip_timeline_decompress")]
    except AttributeError:
        sys.exit("this library is not a probe build (-DBITAR_LAUNCH_TIMELINE=1)")
    for f in setters:
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p]
    eng = bitar_amd.Engine(0)
    codec, seg, n = bitar_amd.CODEC_LZ4, a.seg, a.bytes
    nseg = (n + seg - 1) // seg
    stride = bitar_amd.slot_size(codec, seg)
    data = eng.empty(n)
    slab = eng.empty(nseg * stride)
    sizes = eng.empty(nseg, dtype=torch.int32)
    out = eng.empty(nseg * seg)
    prod = eng.empty(nseg, dtype=torch.int32)
    eng.fill(a.kind, 0, data)

    def step():
        eng.compress_into(codec, data, seg, slab, stride, sizes, n=n)
        eng.decompress_slab_into(codec, slab, stride, sizes, nseg, seg, out, prod,
                                 capacity=nseg * seg)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    bufs = [torch.zeros(3 * nseg, dtype=torch.int64, device="cuda:0") for _ in setters]
    torch.cuda.synchronize()
    for f, t in zip(setters, bufs):
        assert f(t.data_ptr()) == 0
    step()
    torch.cuda.synchronize()
    for f in setters:
        assert f(None) == 0
    eng.sync()
    assert torch.equal(out[:n], data)
    cheap = (sizes.cpu().numpy().astype(np.int64) >= seg)
    # the slot counts the runtime found (hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs)
    L.bitar_hip_timeline_slots.restype = ctypes.c_uint32
    L.bitar_hip_timeline_slots.argtypes = [ctypes.c_void_p]
    # (the compressor's; the decoder has no lanes and its plateau is read off the timeline)
    asked = [int(L.bitar_hip_timeline_slots(eng.ctx)), 0]
    print(json.dumps({"slots_by_occupancy_query": {"compress": asked[0]}}), flush=True)
    res, raw = {"slots_by_occupancy_query": asked}, {}
    for name, t, slots, q in zip(("compress", "decompress"), bufs,
                                 (a.slots_compress, a.slots_decompress), asked):
        r, w = analyse(name, t.cpu().numpy().view(np.uint64), cheap, slots or q)
        res[name] = r
        raw.update({name + "_" + k: v for k, v in w.items()})
        print(json.dumps(r), flush=True)
    res["tail_us_both"] = round(res["compress"]["tail_us"] + res["decompress"]["tail_us"], 1)
    print(json.dumps({"tail_us_both": res["tail_us_both"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if a.raw:
        os.makedirs(os.path.dirname(os.path.abspath(a.raw)), exist_ok=True)
        np.savez_compressed(a.raw, **raw)
    eng.close()


if __name__ == "__main__":
    main()
