#!/usr/bin/env python3
"""What the scale-loop guard of the LM refinement (esvo_params_t::lm_scale_pass_limit, esvo_map_lm_stats) costs and what it buys,
on the bench workloads (benchlib.workload.make_workload).  Each line of output is one JSON record.

  cost      the DSEC throughput workload with the limit 0, count-only and 64, alternating in one process, --reps repetitions
            each: ms per tick, the lm_refine launch time, abandoned matches per tick.
  crawler   the 346x260 stream in its 23-, 26-, 40- and 60-tick realisations (the noise events are drawn over the stream's whole
            duration: streams of different lengths are different realisations; the 26-tick one holds the match whose scale loop
            takes ~900 passes per evaluation, profiles/r06_extras_note.txt) with the limit 0 and --limit: ms per tick, abandoned
            matches per tick, map elements that differ from the limit-0 run after the timed ticks.
  dsec10k   DSEC at 10 000 events per tick (the tick the ROS node runs): abandoned matches per tick, map difference.

    python tools/lm_guard_bench.py cost --reps 9 >> profiles/lm_guard_bench.jsonl
    python tools/lm_guard_bench.py crawler dsec10k >> profiles/lm_guard_bench.jsonl"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import workload as WL  # noqa: E402
from esvo_amd import lib  # noqa: E402
from esvo_amd.abi import LM_SCALE_COUNT_ONLY  # noqa: E402

WARMUP = 3


def limit_name(limit):
    return "count_only" if limit == LM_SCALE_COUNT_ONLY else str(limit)


def run(rig, stream, p, ticks, limit, device, want_map=False):
    """WARMUP + len(ticks) - WARMUP ticks of one handle with two in flight; the figures of the timed part"""
    q = copy.copy(p)
    q.lm_scale_pass_limit = limit
    dev = lib.Esvo(q, rig, device=device)
    try:
        dev.ts_push_events(0, stream.ev_left)
        dev.ts_push_events(1, stream.ev_right)
        WL.run_single(dev, stream, ticks, 0, WARMUP)
        dev.synchronize()
        b, lb = dev.stats(), dev.lm_stats()
        t0 = time.perf_counter()
        WL.run_single(dev, stream, ticks, WARMUP, len(ticks))
        dev.synchronize()
        dt = time.perf_counter() - t0
        s, ls = dev.stats(), dev.lm_stats()
        n = len(ticks) - WARMUP
        ka = np.array(s.kernel_ms_mean(b))
        out = {"limit": limit_name(limit), "ticks": n, "ms_per_tick": round(dt / n * 1e3, 4), "lm_refine_ms": round(float(ka[3]), 4),
               "matches_per_tick": int(s.total_matches - b.total_matches) // n, "points_per_tick": int(s.total_points - b.total_points) // n,
               "abandoned_per_tick": round(int(ls.total_abandoned - lb.total_abandoned) / n, 2),
               "passes_per_eval": round(int(ls.total_passes - lb.total_passes) / max(1, int(ls.total_evals - lb.total_evals)), 3),
               "last_max_passes_eval": int(ls.last_max_passes_eval)}
        return out, (dev.get_map() if want_map else None)
    finally:
        dev.close()


def map_difference(a, b):
    """cells that hold an element in one map and not the other, or elements that differ in any field but the creation id"""
    key = lambda m: {(int(r), int(c)): m[i] for i, (r, c) in enumerate(zip(m["row"], m["col"]))}
    fields = [f for f in a.dtype.names if f != "seq"]
    ka, kb = key(a), key(b)
    only = len(set(ka) ^ set(kb))
    differ = sum(1 for k in set(ka) & set(kb) if any(ka[k][f].tobytes() != kb[k][f].tobytes() for f in fields))
    return {"map_elements": len(a), "map_elements_limit0": len(b), "in_one_map_only": only, "differ": differ}


def cost(args):
    rig, stream, p, ticks = WL.make_workload("dsec640x480", args.steps + WARMUP)
    limits = (0, LM_SCALE_COUNT_ONLY, args.limit)
    run(rig, stream, p, ticks, 0, args.device)   # (the process's first handle pays for the runtime's start)
    for rep in range(args.reps):
        for limit in limits:
            out, _ = run(rig, stream, p, ticks, limit, args.device)
            print(json.dumps(dict(out, mode="cost", workload="dsec640x480", rep=rep)), flush=True)


def crawler(args):
    for n_ticks in (23, 26, 40, 60):   # ascending: make_workload keeps the longest stream it has generated for a workload
        WL._STREAMS.pop(("upenn346x260", False), None)
        rig, stream, p, ticks = WL.make_workload("upenn346x260", n_ticks)
        ticks = ticks[:26]   # (the 23- and 26-tick realisations whole: the crawling match may sit in any tick)
        base_map = None
        for limit in (0, args.limit, 0, args.limit):   # twice, alternating: the second pair is the one to read
            out, mp = run(rig, stream, p, ticks, limit, args.device, want_map=True)
            if limit == 0:
                base_map = mp
            else:
                out.update(map_difference(mp, base_map))
            print(json.dumps(dict(out, mode="crawler", workload="upenn346x260", realisation_ticks=n_ticks)), flush=True)


def dsec10k(args):
    rig, stream, p, ticks = WL.make_workload("dsec640x480", 40, events_cap=10000)
    ticks = ticks[: args.steps + WARMUP]
    base_map = None
    for limit in (0, LM_SCALE_COUNT_ONLY, args.limit):
        out, mp = run(rig, stream, p, ticks, limit, args.device, want_map=True)
        if limit == 0:
            base_map = mp
        else:
            out.update(map_difference(mp, base_map))
        print(json.dumps(dict(out, mode="dsec10k", workload="dsec640x480", events_cap=10000)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("modes", nargs="+", choices=["cost", "crawler", "dsec10k"])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20, help="timed ticks per run")
    ap.add_argument("--reps", type=int, default=9, help="cost: repetitions per limit")
    ap.add_argument("--limit", type=int, default=64)
    args = ap.parse_args()
    for m in args.modes:
        {"cost": cost, "crawler": crawler, "dsec10k": dsec10k}[m](args)


if __name__ == "__main__":
    main()
