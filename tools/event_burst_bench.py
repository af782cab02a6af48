"""The burst stage's cost per packet (esvo_ts_burst_configure), PCIe-inclusive, on one handle (GPU box).  Two measurements:

  --part off    No regression with the stage off.  The left camera of bench.py's DSEC workload cut into its 10 ms ticks (~196 k events
                per packet, as tools/event_filter_bench.py cuts it) is pushed as device columns with the filter on and the stage never
                configured -- by this tree's library and by another build (--parent LIB, the parent commit's), each in a process of
                its own, alternating: this, parent, parent again, per round.  The two parent series give the spread the machine has
                between two runs of the same code; the stage-off path passes if this tree's median differs from the parent's by no
                more than that.
  --part cost   The stage on a bursty packet: tests/event_burst_restated.py's generator scaled to the packet size (640 x 480, 56 000
                bursts of 1..6 events over 12 ms, the pixels from the low / high 146 columns and rows: the same events per pixel as
                the tests' stream).  Routes alternate inside every repetition: the filter alone, and filter + stage in each mode; a
                route pushes the packet --pushes times, the stamps moved on by the packet's span each time, the state carried.
                Reported per mode: ms per push with the filter alone, with filter + stage, and the share of the packet the stage drops.

Median, best and worst over the repetitions; a route's time is the time inside its calls (they are synchronous).  No pass threshold
for a new capability: a measurement.

usage: python tools/event_burst_bench.py --part off --parent LIB.so [--rounds 3] [--reps 5] [--out FILE.txt]
       python tools/event_burst_bench.py --part cost [--reps 7] [--pushes 6] [--out FILE.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MODES = {"trail": 1, "stc_cut": 2, "stc_keep": 3}
FILTER = dict(refractory_ns=250_000, support_ns=1_500_000)
BURST_NS = 300_000


def stats(v):
    v = np.asarray(v)
    return {"median": round(float(np.median(v)), 4), "best": round(float(v.min()), 4), "worst": round(float(v.max()), 4)}


def worker_off(a):
    """one process, one library (ESVO_HIP_LIB or this tree's): the DSEC packets through the filter, the stage never configured"""
    import torch
    import evt3_ingest_bench as E3
    from benchlib import workload
    from esvo_amd import abi, lib
    rig, stream, p, ticks = workload.make_workload("dsec640x480", a.ticks)
    _, packets = E3.packets_of(stream, ticks, "tick")
    ev = stream.ev_left
    us = (abi.event_ns(ev) // np.uint64(1000)).astype(np.int64)
    t_first = ticks[0][0] - int(workload.TICK_S * 1e9)
    edges = [int(np.searchsorted(us, t // 1000, side="left")) for t in [t_first] + [tk[0] for tk in ticks]]
    order = np.concatenate([np.lexsort((ev["x"][lo:hi], ev["polarity"][lo:hi] != 0, ev["y"][lo:hi], us[lo:hi])) + lo for lo, hi in zip(edges, edges[1:]) if hi > lo])
    cols = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (ev["x"][order].view(np.int16), ev["y"][order].view(np.int16), us[order],
                                                                         (ev["polarity"][order] != 0).astype(np.uint8))]
    torch.cuda.synchronize()
    mask = (np.random.default_rng(7).random((rig.height, rig.width)) < 0.001).astype(np.uint8)
    dev = lib.Esvo(p, rig)
    out = []
    for rep in range(1 + a.reps):
        dev.reset()
        dev.ts_filter_configure(0, 1_000_000, 5_000_000, mask)
        t_call, at = 0.0, 0
        for _, n_ev in packets:
            src = [c[at:at + n_ev] for c in cols]
            t0 = time.perf_counter()
            dev.ts_push_columns(0, *src, unit="us")
            t_call += time.perf_counter() - t0
            at += n_ev
        if rep:
            out.append(t_call * 1e3 / len(packets))
    dev.close()
    print(json.dumps({"ms": out, "events_per_packet": at // len(packets)}), flush=True)


def part_off(a):
    assert a.parent and os.path.exists(a.parent), "--part off needs --parent LIB.so (a build of the parent commit)"
    series = {"this": [], "parent_a": [], "parent_b": []}
    n_ev = 0
    for rnd in range(a.rounds):
        names = list(series)
        for name in names[rnd % 3:] + names[:rnd % 3]:
            env = dict(os.environ)
            env.pop("ESVO_HIP_LIB", None)
            if name != "this":
                env["ESVO_HIP_LIB"] = os.path.abspath(a.parent)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "worker_off", "--reps", str(a.reps), "--ticks", str(a.ticks)],
                               env=env, capture_output=True, text=True, timeout=600, check=True)
            got = json.loads(r.stdout.strip().splitlines()[-1])
            series[name] += got["ms"]
            n_ev = got["events_per_packet"]
    line = {"bench": "event_burst", "part": "stage_off_vs_parent", "events_per_packet": n_ev, "rounds": a.rounds, "reps": a.reps,
            "ms_per_push": {k: stats(v) for k, v in series.items()}}
    m = {k: line["ms_per_push"][k]["median"] for k in series}
    line["parent_vs_parent_ms"] = round(abs(m["parent_a"] - m["parent_b"]), 4)
    line["this_vs_parent_ms"] = round(m["this"] - (m["parent_a"] + m["parent_b"]) / 2, 4)
    line["within_spread"] = abs(line["this_vs_parent_ms"]) <= line["parent_vs_parent_ms"]
    return line, ["# stage off: filter on, stage never configured; ms per push of ~%d events (device columns), median (best - worst), %d rounds x %d repetitions" % (n_ev, a.rounds, a.reps)] + [
        "%-9s %.4f (%.4f - %.4f)" % (k, q["median"], q["best"], q["worst"]) for k, q in line["ms_per_push"].items()] + [
        "this - parent %+.4f ms; parent - parent %.4f ms; within the spread: %s" % (line["this_vs_parent_ms"], line["parent_vs_parent_ms"], line["within_spread"])]


def part_cost(a):
    import torch
    import event_burst_restated as B
    from benchlib import workload
    from esvo_amd import lib
    rig, _, p, _ = workload.make_workload("dsec640x480", 1)
    span_ns = 12_000_000
    ev, _ = B.bursty_stream(31, bursts=a.bursts, span_ns=span_ns, width=rig.width, height=rig.height, margin=146)
    x, y = np.array([e[0] for e in ev], np.uint16), np.array([e[1] for e in ev], np.uint16)
    t, pol = np.array([(e[2] - B.T_BASE) // 1000 for e in ev], np.int64), np.array([e[3] for e in ev], np.uint8)
    step_us = int(t.max()) + 1000
    dx, dy, dp = (torch.from_numpy(v).cuda() for v in (x.view(np.int16), y.view(np.int16), pol))
    dts = [torch.from_numpy(t + B.T_BASE // 1000 + k * step_us).cuda() for k in range(a.pushes)]
    torch.cuda.synchronize()
    mask = (np.random.default_rng(7).random((rig.height, rig.width)) < 0.001).astype(np.uint8)
    dev = lib.Esvo(p, rig)
    routes = ["filter"] + list(MODES)
    res, dropped = {r: [] for r in routes}, {}

    def run(route):
        dev.reset()
        dev.ts_filter_configure(0, mask=mask, **FILTER)
        dev.ts_burst_configure(0, MODES.get(route, 0), BURST_NS if route in MODES else 0)
        t_call = 0.0
        for dt in dts:
            t0 = time.perf_counter()
            dev.ts_push_columns(0, dx, dy, dt, dp, unit="us")
            t_call += time.perf_counter() - t0
        if route in MODES:
            dropped[route] = dev.ts_burst_stats(0)["dropped"] / (len(ev) * len(dts))
        assert dev.ts_filter_stats(0)["events_in"] + dev.ts_burst_stats(0)["dropped"] == len(ev) * len(dts)
        return t_call * 1e3 / len(dts)

    for rep in range(1 + a.reps):
        k = rep % len(routes)
        for r in routes[k:] + routes[:k]:
            ms = run(r)
            if rep:
                res[r].append(ms)
    dev.close()
    line = {"bench": "event_burst", "part": "stage_cost", "events_per_packet": len(ev), "pushes": a.pushes, "reps": a.reps, "burst_ns": BURST_NS, "filter": FILTER,
            "ms_per_push": {r: stats(v) for r, v in res.items()}, "dropped_share": {r: round(s, 4) for r, s in dropped.items()}}
    base = line["ms_per_push"]["filter"]["median"]
    text = ["# stage cost: bursty packet of %d events (640x480, device columns), ms per push, median (best - worst) over %d alternating repetitions" % (len(ev), a.reps),
            "%-9s %.4f (%.4f - %.4f)" % (("filter",) + tuple(line["ms_per_push"]["filter"].values()))]
    for r in MODES:
        q = line["ms_per_push"][r]
        text.append("%-9s %.4f (%.4f - %.4f)   %+.4f ms against the filter alone, %.1f %% of the packet dropped by the stage" % (
            r, q["median"], q["best"], q["worst"], q["median"] - base, 100 * dropped[r]))
    return line, text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("off", "cost", "worker_off"), required=True)
    ap.add_argument("--parent", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--pushes", type=int, default=6)
    ap.add_argument("--bursts", type=int, default=56000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.part == "worker_off":
        return worker_off(a)
    line, text = part_off(a) if a.part == "off" else part_cost(a)
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(text) + "\n" + json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
