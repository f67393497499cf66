#!/usr/bin/env python3
"""List-scheduling replay of a recorded launch timeline (scripts/launch_timeline.py --raw):
what a priority-lane rule (order.hip.h lane_prio) can be expected to save before it is run.

Model: S slots; workgroups start in dispatch order, each in the slot that frees first; a
workgroup runs for its recorded duration, divided by `ratio` in the fast lane.  With
--conserve the other workgroups of a launch with fast lanes run slower by the factor that
keeps the issue rate of a full machine what it was (a share p of fast slots at speed r leaves
(1 - p r) / (1 - p) for the rest): priority moves issue slots, it does not make any.  That
share model breaks down where the fast lane is most of the machine (the decoder's f / S =
0.78): entries whose slow-down factor would exceed 2 are printed as null.
Recorded durations are those of a full machine for the rounds and of a nearly empty one for
the tail, so the replay of the recorded order reproduces the recorded makespan closely and the
lanes' replay is an estimate: a workgroup that moves out of the tail would run longer there.

usage: python scripts/launch_sim.py RAW.npz [--ratios 1.05,1.1,1.2,1.3] [--conserve]"""
import argparse
import heapq
import json


def lane(b, H, S):
    if S == 0 or b >= H:
        return False
    q, f = divmod(H, S)
    return q >= 1 and f > 0 and b % S < f


def replay(dur, S, fast, ratio, slow):
    """makespan of durations `dur` (dispatch order) over S slots"""
    free = [0.0] * min(S, len(dur))
    heapq.heapify(free)
    end = 0.0
    for d, f in zip(dur, fast):
        t = heapq.heappop(free)
        t += d / ratio if f else d * slow
        end = max(end, t)
        heapq.heappush(free, t)
    return end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("raw")
    ap.add_argument("--ratios", default="1.05,1.1,1.2,1.3,1.5")
    ap.add_argument("--slots-compress", type=int, default=5120)
    ap.add_argument("--slots-decompress", type=int, default=6144,
                    help="the decoder's measured plateau (DESIGN.md 4.29), not the 7168 of the "
                         "occupancy query")
    ap.add_argument("--conserve", action="store_true")
    a = ap.parse_args()
    import numpy as np
    z = np.load(a.raw)
    for name, S in (("compress", a.slots_compress), ("decompress", a.slots_decompress)):
        b, t0, t1, cheap = (z[f"{name}_{k}"] for k in ("b", "t0", "t1", "cheap"))
        o = np.argsort(b)
        dur = (t1 - t0)[o]
        H = int((~cheap).sum())
        fast = [lane(int(i), H, S) for i in range(len(dur))]
        q, f = divmod(H, S)
        base = replay(dur, S, fast, 1.0, 1.0)
        work = float(dur.sum())
        r = {"kernel": name, "H": H, "S": S, "q": q, "f": f, "recorded_us": round(float(t1.max()), 1),
             "replay_us": round(base, 1), "even_us": round(work / S, 1), "lanes": {}}
        for ratio in [float(x) for x in a.ratios.split(",")]:
            p = f / S
            # (slow: the others' durations grow by the issue share the fast lane takes; where
            # the lane would take most of the machine, p r -> 1, the share model has nothing
            # left to say: no figure beyond a factor of 2)
            slow = 1.0
            if a.conserve:
                slow = (1 - p) / (1 - p * ratio) if p * ratio < 1 else float("inf")
            r["lanes"][str(ratio)] = (round(replay(dur, S, fast, ratio, slow), 1)
                                      if slow <= 2.0 else None)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
