"""The mapper -> tracker hand-off, host route against device route, on one handle (GPU box).

  route A   get_pointcloud() (elements down, host sort, host transform) + the stochastic selection on the host + track_set_reference
            (2000 points up): what a tracking node pays once per mapping tick today
  route B   map_cloud_build() + the same selection as indices + track_set_reference_from_cloud (8 KB of indices up)

Both routes end in the same small synchronous tracker call (one residual), so each timing covers the work on the tracker's stream;
the two alternate inside every repetition, after a warm-up, and are checked once to hand the tracker the same bits.

usage: python tools/map_cloud_bench.py [--reps N (>= 9, default 15)] [--maps upenn1000,dsec10000,dsec_throughput] [--out FILE.jsonl]
                                       [--route-b-only]   (for a rocprofv3 --kernel-trace --stats run of its own: no route A, no timing)
Maps: the upenn map at 1000 events per tick, the DSEC map at 10 000 events per tick, and the DSEC throughput map bench.py's
workload leaves (every event of each 10 ms slice), all generated through benchlib.workload.  One JSON line per map."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib import workload  # noqa: E402
from esvo_amd import lib  # noqa: E402

MAPS = {  # name: (workload, events per tick -- 0: all of them --, ticks that build the map)
    "upenn1000": ("upenn346x260", 1000, 12),
    "dsec10000": ("dsec640x480", 10000, 12),
    "dsec_throughput": ("dsec640x480", 0, 8),
}
N_REF = 2000   # MAX_REGISTRATION_POINTS of the shipped tracking configs


def build_map(name):
    wl, cap, n_ticks = MAPS[name]
    rig, stream, p, ticks = workload.make_workload(wl, 12, events_cap=cap)
    dev = lib.Esvo(p, rig)
    dev.ts_push_events(0, stream.ev_left)
    dev.ts_push_events(1, stream.ev_right)
    workload.run_single(dev, stream, ticks, 0, n_ticks, sync_each=True)
    dev.track_set_current(None, 5)
    return dev, ticks[n_ticks - 1][3]


def route_a(dev, T, draws):
    xyz = dev.get_pointcloud()
    order = lib.stochastic_order_c(len(xyz), N_REF, draws)
    dev.track_set_reference(xyz[order], T)
    return dev.track_residuals(np.eye(4), 0, 1), len(xyz)


def route_b(dev, T, draws):
    n = dev.map_cloud_build()
    order = lib.stochastic_order_c(n, N_REF, draws)
    dev.track_set_reference_from_cloud(order, T)
    return dev.track_residuals(np.eye(4), 0, 1), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maps", default="upenn1000,dsec10000,dsec_throughput")
    ap.add_argument("--out", default="")
    ap.add_argument("--route-b-only", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 9
    draws = np.random.default_rng(7).integers(0, 2**31, size=N_REF, dtype=np.uint32)
    for name in a.maps.split(","):
        dev, T = build_map(name)
        if a.route_b_only:
            for _ in range(a.warmup + a.reps):
                route_b(dev, T, draws)
            print(f"{name}: {a.warmup + a.reps} device-route hand-offs, {dev.map_cloud_device()[1]} elements")
            dev.close()
            continue
        # same bits on both routes (all of the reference, not only the residual the timings end in)
        route_a(dev, T, draws)
        ra = dev.track_residuals(np.eye(4), 0, N_REF)
        route_b(dev, T, draws)
        rb = dev.track_residuals(np.eye(4), 0, N_REF)
        assert ra.tobytes() == rb.tobytes() and dev.map_cloud().tobytes() == dev.get_pointcloud().tobytes(), "the routes disagree"
        ms = {"A": [], "B": []}
        n_el = 0
        for rep in range(a.warmup + a.reps):
            for route, fn in (("A", route_a), ("B", route_b)) if rep % 2 == 0 else (("B", route_b), ("A", route_a)):
                t0 = time.perf_counter()
                _, n_el = fn(dev, T, draws)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    ms[route].append(dt)
        line = {"bench": "map_cloud", "map": name, "workload": MAPS[name][0], "events_per_tick": MAPS[name][1] or "all",
                "elements": int(n_el), "reference_points": int(min(N_REF, n_el)), "reps": a.reps, "warmup": a.warmup}
        for route in "AB":
            v = np.asarray(ms[route])
            line[f"route_{route}_ms"] = {"median": round(float(np.median(v)), 4), "best": round(float(v.min()), 4),
                                        "worst": round(float(v.max()), 4)}
        line["B_worst_beats_A_best"] = bool(line["route_B_ms"]["worst"] < line["route_A_ms"]["best"])
        print(json.dumps(line))
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        dev.close()


if __name__ == "__main__":
    main()
