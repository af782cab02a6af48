"""Event ingest from DSEC-typed columns against the two record routes, PCIe-inclusive, on one handle (GPU box).

The source is what a DSEC file holds for the left camera of bench.py's DSEC workload: x u16, y u16, t u32 microseconds (+ t_offset),
p u8, cut into the workload's 10 ms ticks.  Every route stages the same 40 ticks into a freshly reset handle:

  a         abi.make_events (interleave + split stamps on the host) + ts_push_events          16 B/event up
  b         abi.serialize_event_array (the ROS wire format) + ts_push_event_array               13 B/event up
  c         ts_push_columns on the host columns as they are, pageable                           13 B/event up
  c_pinned  ... the same columns in pinned host memory (esvo_host_alloc)
  d         ts_push_columns on the columns in device memory (torch tensors, uploaded before)     8 B/event down

The routes alternate inside every repetition; the rate of a route is events / the time spent inside its ingest CALLS over the 40
ticks, the host's packing time (routes a and b) is reported beside it and is not part of the rate.  Median and worst over the
repetitions.  All routes are checked once to leave the same event ring.  No pass threshold: a measurement.

usage: python tools/ingest_columns_bench.py [--reps N (>= 9, default 11)] [--ticks 40] [--out FILE.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib import workload  # noqa: E402
from esvo_amd import abi, lib  # noqa: E402

ROUTES = ("a", "b", "c", "c_pinned", "d")


def dsec_columns(stream, ticks):
    """the left camera's events as DSEC-typed columns, and the [lo, hi) index range of every tick's 10 ms (the history before the
    first tick is not staged: every slice is one tick's worth)"""
    ev = stream.ev_left
    us = abi.event_ns(ev) // np.uint64(1000)
    t_offset = int(us[0]) - 1000
    cols = dict(x=ev["x"].copy(), y=ev["y"].copy(), t=(us - np.uint64(t_offset)).astype(np.uint32), p=ev["polarity"].copy())
    t_first = ticks[0][0] - int(workload.TICK_S * 1e9)
    edges = [int(np.searchsorted(us, (t // 1000), side="left")) for t in [t_first] + [tk[0] for tk in ticks]]
    return cols, t_offset, [(edges[k], edges[k + 1]) for k in range(len(ticks)) if edges[k + 1] > edges[k]]


def pinned_copy(cols):
    """the columns in one pinned block -> (views, pointer to free)"""
    so, ptr = lib.load(), C.c_void_p()
    sizes = {k: (v.nbytes + 63) // 64 * 64 for k, v in cols.items()}
    if so.esvo_host_alloc(sum(sizes.values()), C.byref(ptr)):
        raise lib.EsvoError("esvo_host_alloc failed")
    out, off = {}, 0
    for k, v in cols.items():
        buf = (C.c_char * v.nbytes).from_address(ptr.value + off)
        out[k] = np.frombuffer(buf, v.dtype, len(v))
        out[k][:] = v
        off += sizes[k]
    return out, ptr


def run_route(dev, route, src, t_offset, slices, W, H):
    """-> (seconds inside the ingest calls, seconds of host packing, events)"""
    dev.reset()
    t_call = t_pack = 0.0
    n = 0
    for lo, hi in slices:
        x, y, t, p = (src[k][lo:hi] for k in "xytp")
        if route in ("a", "b"):
            t0 = time.perf_counter()
            ev = abi.make_events(x, y, (t.astype(np.uint64) + np.uint64(t_offset)) * np.uint64(1000), p)
            msg = abi.serialize_event_array(ev, W, H) if route == "b" else None
            t1 = time.perf_counter()
            if route == "a":
                dev.ts_push_events(0, ev)
            else:
                dev.ts_push_event_array(0, msg)
            t2 = time.perf_counter()
            t_pack += t1 - t0
            t_call += t2 - t1
        else:
            t1 = time.perf_counter()
            dev.ts_push_columns(0, x, y, t, p, unit="us", t_offset=t_offset)
            t_call += time.perf_counter() - t1
        n += hi - lo
    return t_call, t_pack, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.reps >= 9
    import torch
    rig, stream, p, ticks = workload.make_workload("dsec640x480", a.ticks)
    cols, t_offset, slices = dsec_columns(stream, ticks)
    pinned, pin_ptr = pinned_copy(cols)
    on_device = {k: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for k, v in cols.items()}
    torch.cuda.synchronize()
    src = {"a": cols, "b": cols, "c": cols, "c_pinned": pinned, "d": on_device}
    dev = lib.Esvo(p, rig)
    # every route leaves the same ring
    tails = {}
    for r in ROUTES:
        _, _, n = run_route(dev, r, src[r], t_offset, slices, rig.width, rig.height)
        ev, st, b0, b1 = dev.debug_ts_ring(0, n - 4096, 4096)
        tails[r] = (ev.tobytes(), st.tobytes(), b0, b1)
    assert all(tails[r] == tails["a"] for r in ROUTES), "the routes leave different event rings"
    res = {r: dict(call=[], pack=[]) for r in ROUTES}
    for rep in range(a.warmup + a.reps):
        order = ROUTES[rep % len(ROUTES):] + ROUTES[:rep % len(ROUTES)]
        for r in order:
            t_call, t_pack, n = run_route(dev, r, src[r], t_offset, slices, rig.width, rig.height)
            if rep >= a.warmup:
                res[r]["call"].append(n / t_call)
                res[r]["pack"].append(t_pack * 1e3 / len(slices))
    line = {"bench": "ingest_columns", "workload": "dsec640x480", "camera": "left", "ticks": len(slices), "events": int(n),
            "events_per_tick": int(n // len(slices)), "reps": a.reps, "warmup": a.warmup, "routes": {}}
    for r in ROUTES:
        v = np.asarray(res[r]["call"])
        line["routes"][r] = {"events_per_s_median": round(float(np.median(v))), "events_per_s_worst": round(float(v.min())),
                             "host_pack_ms_per_tick_median": round(float(np.median(res[r]["pack"])), 4)}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    dev.close()
    del pinned
    lib.load().esvo_host_free(pin_ptr)


if __name__ == "__main__":
    main()
