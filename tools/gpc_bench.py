"""The mapper's global point cloud (publishPointCloud's branch, esvo_Mapping.cpp:955-977), host route against device route, on
one handle (GPU box).

  route A   get_pointcloud_near() (elements down, host sort, host predicate and transform) + lib.voxel_filter (host code) + the
            append on the host: what a node must do today, once per visualizeGPC_interval
  route B   gpc_update(): near cloud, voxel filter and append on the device; counts and a flag come back

Both routes refresh on every call (interval 0, stamps 1 us apart) with the shipped range and NumGPC_added_per_refresh of the
map's yaml; the two alternate inside every repetition, after a warm-up, and are checked once to leave the same cloud.

usage: python tools/gpc_bench.py [--reps N (>= 9, default 15)] [--maps upenn1000,dsec10000,dsec_throughput] [--out FILE.jsonl]
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
from esvo_amd import lib, params  # noqa: E402

MAPS = {  # name: (workload, events per tick -- 0: all of them --, ticks that build the map, GPC preset)
    "upenn1000": ("upenn346x260", 1000, 12, "mapping_upenn"),
    "dsec10000": ("dsec640x480", 10000, 12, "mapping_dsec"),
    "dsec_throughput": ("dsec640x480", 0, 8, "mapping_dsec"),
}


def build_map(name):
    wl, cap, n_ticks, _ = MAPS[name]
    rig, stream, p, ticks = workload.make_workload(wl, 12, events_cap=cap)
    dev = lib.Esvo(p, rig)
    dev.ts_push_events(0, stream.ev_left)
    dev.ts_push_events(1, stream.ev_right)
    workload.run_single(dev, stream, ticks, 0, n_ticks, sync_each=True)
    return dev


class HostCloud:
    """pc_global_ on the host: reserved once, appended to in place"""

    def __init__(self, cap):
        self.xyz, self.n = np.empty((cap, 3), np.float32), 0

    def append(self, pts):
        self.xyz[self.n:self.n + len(pts)] = pts
        self.n += len(pts)


def route_a(dev, cfg, host):
    near = dev.get_pointcloud_near(cfg["visualize_range"])
    filtered = lib.voxel_filter(near, params.GPC_LEAF)
    k = min(len(filtered), cfg["NumGPC_added_per_refresh"]) - 1 if len(filtered) else 0
    host.append(filtered[len(filtered) - k:] if k else filtered[:0])
    return len(near), len(filtered)


def route_b(dev, t_ns):
    assert dev.gpc_update(t_ns)
    st = dev.gpc_stats()
    return st.last_near, st.last_voxels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maps", default="upenn1000,dsec10000,dsec_throughput")
    ap.add_argument("--out", default="")
    ap.add_argument("--route-b-only", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 9
    for name in a.maps.split(","):
        dev = build_map(name)
        cfg = params.GPC_PRESETS[MAPS[name][3]]
        calls = a.warmup + a.reps + 1
        cap = calls * cfg["NumGPC_added_per_refresh"]
        dev.gpc_configure(visualize_range=cfg["visualize_range"], interval_s=0.0, num_added_per_refresh=cfg["NumGPC_added_per_refresh"],
                          capacity_points=cap, leaf=params.GPC_LEAF)
        t = 1_000_000_000
        if a.route_b_only:
            for _ in range(a.warmup + a.reps):
                t += 1000
                route_b(dev, t)
            st = dev.gpc_stats()
            print(f"{name}: {st.refreshes} device-route refreshes, {st.last_near} near points, {st.last_voxels} voxels, {st.total_points} global points")
            dev.close()
            continue
        host = HostCloud(cap)
        # same cloud on both routes
        t += 1000
        counts_a, counts_b = route_a(dev, cfg, host), route_b(dev, t)
        assert counts_a == counts_b and dev.gpc_cloud().tobytes() == host.xyz[:host.n].tobytes(), "the routes disagree"
        ms = {"A": [], "B": [], "B_device": []}
        for rep in range(a.warmup + a.reps):
            for route in ("AB" if rep % 2 == 0 else "BA"):
                t += 1000
                t0 = time.perf_counter()
                if route == "A":
                    route_a(dev, cfg, host)
                else:
                    route_b(dev, t)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    ms[route].append(dt)
                    if route == "B":
                        ms["B_device"].append(dev.gpc_stats().ms_last)
        assert dev.gpc_cloud().tobytes() == host.xyz[:host.n].tobytes(), "the routes disagree after the repetitions"
        line = {"bench": "gpc", "map": name, "workload": MAPS[name][0], "events_per_tick": MAPS[name][1] or "all",
                "visualize_range": cfg["visualize_range"], "num_added_per_refresh": cfg["NumGPC_added_per_refresh"],
                "elements": int(len(dev.get_pointcloud())), "near": int(counts_b[0]), "voxels": int(counts_b[1]),
                "reps": a.reps, "warmup": a.warmup}
        for route in ("A", "B", "B_device"):
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
