"""The event survey's cost per packet (esvo_ts_survey_begin) and the time of esvo_ts_survey_mask, PCIe-inclusive (GPU box).

Packets of --events events at 640x480 (the DSEC rig), consecutive in time, staged into a freshly reset handle with the event filter
on (a random hot-pixel mask of --mask-share of the pixels, --refractory-us, --support-us).  Two packet kinds:

  uniform     every event on a pixel drawn uniformly
  contended   every second event on ONE pixel, the rest uniform: the case the counting kernel combines on chip for

Two routes, each with the survey closed and open (flags 0), so eight variants:

  cols_*      ts_push_columns on device columns (x, y u16, t int64 us, p u8)
  evt3_*      ts_push_evt3 on EVT 3.0 words in device memory

The variants alternate inside every repetition on ONE handle; a variant's time is the time inside its push calls (they are
synchronous, and the counting kernel is launched in front of the wait the push makes anyway).  Median, best and worst over the
repetitions; the survey's cost is the open median minus the closed one.  With --no-survey only the closed variants run: that is how
a build without the survey (ESVO_HIP_LIB) is measured with the same tool and packets.  Then esvo_ts_survey_mask at 640x480 and
1280x720 on counts the tool plants (Poisson background, a few hot pixels), with and without the mask's way down.  No pass threshold:
a measurement.

usage: python tools/event_survey_bench.py [--reps N (>= 9, default 9)] [--packets 8] [--events 200000] [--no-survey] [--label TEXT]
                                          [--out profiles/event_survey_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evt3_ingest_bench as E3  # noqa: E402
from esvo_amd import calib, lib, params  # noqa: E402

T_BASE_US = 1_700_000_000_000_000


def make_packets(kind, n_packets, n, W, H, seed):
    """-> [(x, y, t_us relative, p)] sorted by (t, y, p, x), 10 ms per packet"""
    r = np.random.default_rng(seed)
    out = []
    for k in range(n_packets):
        x, y = r.integers(0, W, n), r.integers(0, H, n)
        if kind == "contended":
            x[::2], y[::2] = W // 3, H // 3
        t = np.sort(r.integers(0, 10_000, n)) + 10_000 * k + 1000
        p = r.integers(0, 2, n)
        order = np.lexsort((x, p, y, t))
        out.append((x[order], y[order], t[order], p[order]))
    return out


def stats_of(v):
    v = np.asarray(v)
    return {"median": round(float(np.median(v)), 4), "best": round(float(v.min()), 4), "worst": round(float(v.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--packets", type=int, default=8)
    ap.add_argument("--events", type=int, default=200_000)
    ap.add_argument("--mask-share", type=float, default=0.001)
    ap.add_argument("--refractory-us", type=int, default=1000)
    ap.add_argument("--support-us", type=int, default=5000)
    ap.add_argument("--no-survey", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.reps >= 9
    import torch
    rig = calib.dataset_rig("dsec")
    W, H = rig.width, rig.height
    p = params.make_params(params.PRESETS["mapping_dsec"], rig, event_ring_capacity=1 << 22, regularization=0)[0]
    dev = lib.Esvo(p, rig)
    dev.debug_evt3_device_min(0)
    mask = (np.random.default_rng(7).random((H, W)) < a.mask_share).astype(np.uint8)
    dev.ts_filter_configure(0, a.refractory_us * 1000, a.support_us * 1000, mask)
    data = {}
    for kind in ("uniform", "contended"):
        pk = make_packets(kind, a.packets, a.events, W, H, 11)
        cols = [[torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (x.astype(np.uint16).view(np.int16), y.astype(np.uint16).view(np.int16),
                                                                            t.astype(np.int64) + T_BASE_US, q.astype(np.uint8))] for x, y, t, q in pk]
        words = [torch.from_numpy(E3.encode(x, y, t, q).view(np.int16)).cuda() for x, y, t, q in pk]
        data[kind] = (cols, words)
    torch.cuda.synchronize()
    variants = [(route, kind, state) for route in ("cols", "evt3") for kind in ("uniform", "contended") for state in (("closed",) if a.no_survey else ("closed", "open"))]
    is_open = False

    def run(route, kind, state):
        nonlocal is_open
        if (state == "open") != is_open:
            dev.ts_survey_begin(0) if state == "open" else dev.ts_survey_end(0)
            is_open = state == "open"
        dev.reset()
        cols, words = data[kind]
        t_call = 0.0
        for k in range(a.packets):
            if route == "cols":
                t0 = time.perf_counter()
                dev.ts_push_columns(0, *cols[k], unit="us")
                t_call += time.perf_counter() - t0
            else:
                t0 = time.perf_counter()
                got = dev.ts_push_evt3(0, words[k], T_BASE_US)
                t_call += time.perf_counter() - t0
                assert got == a.events
        assert dev.ts_filter_stats(0)["events_in"] == a.packets * a.events
        if is_open:
            st = dev.ts_survey_stats(0)
            assert st["events_in"] == a.packets * a.events and st["packets"] == a.packets
        return t_call * 1e3 / a.packets

    res = {v: [] for v in variants}
    for rep in range(a.warmup + a.reps):
        k = rep % len(variants)
        for v in variants[k:] + variants[:k]:
            ms = run(*v)
            if rep >= a.warmup:
                res[v].append(ms)
    line = {"bench": "event_survey", "label": a.label, "sensor": [W, H], "packets": a.packets, "events_per_packet": a.events, "reps": a.reps,
            "lib": os.environ.get("ESVO_HIP_LIB", "libesvo_hip.so"),
            "filter": {"mask_share": a.mask_share, "refractory_us": a.refractory_us, "support_us": a.support_us}, "ms_per_packet": {}}
    for v in variants:
        line["ms_per_packet"]["_".join(v)] = stats_of(res[v])
    if not a.no_survey:
        line["survey_ms"] = {f"{r}_{k}": round(line["ms_per_packet"][f"{r}_{k}_open"]["median"] - line["ms_per_packet"][f"{r}_{k}_closed"]["median"], 4)
                             for r in ("cols", "evt3") for k in ("uniform", "contended")}
        if is_open:
            dev.ts_survey_end(0)
    dev.close()
    if not a.no_survey:   # esvo_ts_survey_mask on planted counts: factor 10 and a 1 kHz rate test
        line["mask_ms"] = {}
        for name, preset in (("dsec", "mapping_dsec"), ("hd", "mapping_hd")):
            rg = calib.dataset_rig(name)
            d = lib.Esvo(params.make_params(params.PRESETS[preset], rg, regularization=0)[0], rg)
            d.ts_filter_configure(0, 0, 0)
            d.ts_survey_begin(0, count_only=True)
            r = np.random.default_rng(3)
            planes = r.poisson(2.0, (2, rg.height, rg.width)).astype(np.uint32)
            planes[:, ::97, ::89] += 5000
            d.ts_survey_state(0, set=planes, stats=dict(events_in=int(planes.sum()), outside=0, packets=1, t_first=0, t_last=10 ** 9))
            rule = dict(min_count=10, factor=10, rank_permille=500, max_rate_hz=1000)
            got = {}
            for what, kw in (("report_only", dict(want_mask=False)), ("with_mask", dict()), ("with_mask_install", dict(install=1))):
                ts = []
                for rep in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    _, rep_ = d.ts_survey_mask(0, **kw, **rule)
                    if rep >= a.warmup:
                        ts.append((time.perf_counter() - t0) * 1e3)
                got[what] = stats_of(ts)
                got["n_hot"] = rep_["n_hot"]
            line["mask_ms"][f"{rg.width}x{rg.height}"] = got
            d.close()
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
