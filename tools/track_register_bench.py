#!/usr/bin/env python3
"""Times one registration of the tracker (esvo_track_solve) on one GPU, host loop against the one-launch device loop.

Two cases on the closed loop's scene (esvo_amd/closed_loop.py: the synthetic upenn stream, SGM bootstrap, a few tracker -> mapper
ticks; the reference cloud is 2000 points of the map those ticks fused, the current frame the next tick's Time Surface):
  closed_loop   all points in every iteration, Huber 50, 12 iterations: what closed_loop.register asks for
  yaml          BATCH_SIZE 300 of the 2000, 10 iterations: the shipped cfg/tracking/*.yaml schedule
For each case both paths -- on_device = 0 (esvo_hip::gauss_newton_register on the host, one launch per evaluation: the
arithmetic and launch pattern of esvo_track_register) and on_device = 1 (the whole loop in one launch) -- are timed in the same
process on the same handle, alternating, wall time around the call.  One JSON record per case is printed and appended to --out
(default profiles/track_register_bench.jsonl) with median / p90 per path, the iteration and trial counts of the trace, the host
path's launch count and whether the two paths returned the same bytes.
Usage: python tools/track_register_bench.py [--reps N] [--warmup W] [--ticks K] [--out FILE] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from esvo_amd import closed_loop as cl, lib  # noqa: E402


def scene(ticks):
    """a handle whose tracker holds the problem of tick `ticks` + 1 of the closed loop"""
    rig, st, p, t0 = cl._scene(20250419, 1.0)
    dev = lib.Esvo(p, rig)
    dev.ts_push_events(0, st.ev_left)
    dev.ts_push_events(1, st.ev_right)
    dev.ts_render(0, t0, download=False)
    dev.ts_render(1, t0, download=False)
    T0 = st.pose(t0)
    dev.set_observation(t0, None, None, T0)
    dev.init_sgm(None, None, min_points=100)
    out = cl._loop(rig, st, p, cl._OneGpu(dev), t0, T0, None, ticks, 10**9)
    t = t0 + (ticks + 1) * cl.TICK_NS
    dev.ts_render(0, t, download=False)
    dev.ts_render(1, t, download=False)
    xyz = dev.get_pointcloud()
    sel = np.random.default_rng(0).permutation(len(xyz))[:2000]
    dev.track_set_current(None, 5)
    dev.track_set_reference(xyz[sel], out["poses"][-1])
    return dev, len(sel)


def stats(v):
    v = np.asarray(v) * 1e3
    return dict(median_ms=float(np.median(v)), p90_ms=float(np.percentile(v, 90)), min_ms=float(v.min()))


def case(dev, name, n, batch, iters, reps, warmup):
    R0, t0 = np.eye(3), np.zeros(3)
    kw = dict(batch_size=batch, huber=True, huber_threshold=50.0, max_iterations=iters, damping=1e-3)
    wall = {False: [], True: []}
    res = {}
    for k in range(warmup + reps):
        for on_device in (False, True):
            c0 = time.perf_counter()
            r = dev.track_solve(n, R0, t0, on_device=on_device, **kw)
            dt = time.perf_counter() - c0
            if k >= warmup:
                wall[on_device].append(dt)
            res[on_device] = r
    (Rh, th, ih, trh), (Rd, td, idv, trd) = res[False], res[True]
    rec = dict(case=name, n_points=n, batch_size=batch, max_iterations=iters, reps=reps,
               host=stats(wall[False]), device=stats(wall[True]),
               iterations=int(ih.iterations), stop=int(ih.stop), trials=int(trh["trials"].sum()), picks=[int(x) for x in trh["pick"]],
               host_launches=int(ih.launches), device_launches=int(idv.launches),
               same_bytes=bool(Rh.tobytes() == Rd.tobytes() and th.tobytes() == td.tobytes() and trh.tobytes() == trd.tobytes()
                               and ih.iterations == idv.iterations and ih.rms == idv.rms))
    rec["device_over_host"] = rec["device"]["median_ms"] / rec["host"]["median_ms"]
    if batch == 0:  # the parent call itself: esvo_track_register, the same loop without the recorder
        w = []
        for k in range(warmup + reps):
            c0 = time.perf_counter()
            dev.track_register(n, R0, t0, huber=True, huber_threshold=50.0, max_iterations=iters, damping=1e-3)
            if k >= warmup:
                w.append(time.perf_counter() - c0)
        rec["track_register"] = stats(w)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--ticks", type=int, default=4, help="tracker -> mapper ticks behind the bootstrap before the measured frame")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_register_bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="5 repetitions, 2 warm-up (profiler runs)")
    a = ap.parse_args()
    if a.quick:
        a.reps, a.warmup = 5, 2
    dev, n = scene(a.ticks)
    recs = [case(dev, "closed_loop", n, 0, 12, a.reps, a.warmup), case(dev, "yaml", n, 300, 10, a.reps, a.warmup)]
    dev.close()
    with open(a.out, "a") as f:
        for r in recs:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
