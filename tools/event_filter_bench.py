"""The event filter's cost per packet (esvo_ts_filter_configure), PCIe-inclusive, on one handle (GPU box).

The source is the left camera of bench.py's DSEC workload, quantised to microseconds and cut into the workload's 10 ms ticks
(~196 k events per packet), as tools/evt3_ingest_bench.py cuts it.  Every route stages the same packets into a freshly reset handle:

  cols_off   ts_push_columns on device columns (x, y u16, t int64 us, p u8), no filter configured
  cols_on    the same with the filter on
  evt3_off   ts_push_evt3 on the EVT 3.0 words in device memory, no filter configured
  evt3_on    the same with the filter on

The filter: a random hot-pixel mask (--mask-share of the pixels), --refractory-us, --support-us.  The routes alternate inside every
repetition; a route's time is the time inside its calls (they are synchronous).  Median, best and worst over the repetitions; the
filter's cost is reported as a share of the unfiltered push and of the sustained tick it runs beside (--tick-ms).  With --no-filter
only the two unfiltered routes run: that is how a build without the filter (ESVO_HIP_LIB) is measured with the same tool and stream.
No pass threshold: a measurement.

usage: python tools/event_filter_bench.py [--reps N (>= 3, default 7)] [--ticks 40] [--no-filter] [--label TEXT] [--out FILE.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evt3_ingest_bench as E3  # noqa: E402
from benchlib import workload  # noqa: E402
from esvo_amd import abi, lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--mask-share", type=float, default=0.001)
    ap.add_argument("--refractory-us", type=int, default=1000)
    ap.add_argument("--support-us", type=int, default=5000)
    ap.add_argument("--tick-ms", type=float, default=1.24)
    ap.add_argument("--no-filter", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.reps >= 3
    import torch
    rig, stream, p, ticks = workload.make_workload("dsec640x480", a.ticks)
    base, packets = E3.packets_of(stream, ticks, "tick")
    # the same packets as device columns, in the order the words carry them
    ev = stream.ev_left
    us = (abi.event_ns(ev) // np.uint64(1000)).astype(np.int64)
    t_first = ticks[0][0] - int(workload.TICK_S * 1e9)
    edges = [int(np.searchsorted(us, t // 1000, side="left")) for t in [t_first] + [tk[0] for tk in ticks]]
    order = np.concatenate([np.lexsort((ev["x"][lo:hi], ev["polarity"][lo:hi] != 0, ev["y"][lo:hi], us[lo:hi])) + lo for lo, hi in zip(edges, edges[1:]) if hi > lo])
    cols = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (ev["x"][order].view(np.int16), ev["y"][order].view(np.int16), us[order],
                                                                         (ev["polarity"][order] != 0).astype(np.uint8))]
    dwords = torch.from_numpy(np.concatenate([w for w, _ in packets]).view(np.int16)).cuda()
    torch.cuda.synchronize()
    mask = (np.random.default_rng(7).random((rig.height, rig.width)) < a.mask_share).astype(np.uint8)
    dev = lib.Esvo(p, rig)
    dev.debug_evt3_device_min(0)
    routes = ("cols_off", "evt3_off") if a.no_filter else ("cols_off", "cols_on", "evt3_off", "evt3_on")

    def run(route):
        dev.reset()
        if not a.no_filter:
            if route.endswith("_on"):
                dev.ts_filter_configure(0, a.refractory_us * 1000, a.support_us * 1000, mask)
            else:
                dev.ts_filter_configure(0, off=True)
        t_call, at_ev, at_w = 0.0, 0, 0
        for words, n_ev in packets:
            if route.startswith("cols"):
                src = [c[at_ev:at_ev + n_ev] for c in cols]
                t0 = time.perf_counter()
                dev.ts_push_columns(0, *src, unit="us")
                t_call += time.perf_counter() - t0
            else:
                src = dwords[at_w:at_w + words.size]
                t0 = time.perf_counter()
                got = dev.ts_push_evt3(0, src, base)
                t_call += time.perf_counter() - t0
                assert got == n_ev
            at_ev += n_ev
            at_w += words.size
        kept = dev.ts_filter_stats(0)["kept"] if route.endswith("_on") else at_ev
        assert int(dev.stats().events_staged[0]) == kept
        return t_call * 1e3 / len(packets), at_ev, kept

    res = {r: [] for r in routes}
    info = {}
    for rep in range(a.warmup + a.reps):
        k = rep % len(routes)
        for r in routes[k:] + routes[:k]:
            ms, n, kept = run(r)
            info[r] = (n, kept)
            if rep >= a.warmup:
                res[r].append(ms)
    n_total = info[routes[0]][0]
    line = {"bench": "event_filter", "label": a.label, "workload": "dsec640x480", "camera": "left", "packets": len(packets),
            "events_per_packet": n_total // len(packets), "reps": a.reps, "lib": os.environ.get("ESVO_HIP_LIB", "libesvo_hip.so"), "routes": {}}
    if not a.no_filter:
        line["filter"] = {"mask_share": a.mask_share, "refractory_us": a.refractory_us, "support_us": a.support_us,
                          "kept_share": round(info["cols_on"][1] / n_total, 4)}
    for r in routes:
        v = np.asarray(res[r])
        line["routes"][r] = {"ms_per_packet_median": round(float(np.median(v)), 4), "ms_per_packet_best": round(float(v.min()), 4),
                             "ms_per_packet_worst": round(float(v.max()), 4)}
    if not a.no_filter:
        for src in ("cols", "evt3"):
            off, on = line["routes"][src + "_off"]["ms_per_packet_median"], line["routes"][src + "_on"]["ms_per_packet_median"]
            line["routes"][src + "_on"].update(filter_ms=round(on - off, 4), share_of_unfiltered_push=round((on - off) / off, 3),
                                               share_of_tick=round((on - off) / a.tick_ms, 3))
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("# tools/event_filter_bench.py %s: ms per packet of ~%d events, median (best - worst) over %d alternating repetitions\n" % (
                a.label, line["events_per_packet"], a.reps))
            for r in routes:
                q = line["routes"][r]
                extra = ""
                if "filter_ms" in q:
                    extra = "   filter %+.4f ms = %.0f %% of the unfiltered push, %.0f %% of a %.2f ms tick" % (
                        q["filter_ms"], 100 * q["share_of_unfiltered_push"], 100 * q["share_of_tick"], a.tick_ms)
                f.write("%-9s %.4f (%.4f - %.4f)%s\n" % (r, q["ms_per_packet_median"], q["ms_per_packet_best"], q["ms_per_packet_worst"], extra))
            f.write(json.dumps(line) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
