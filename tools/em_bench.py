#!/usr/bin/env python3
"""Times event-to-event matching (esvo_MVStereo modes 0 / 2, esvo_map_tick_em / esvo_map_match_em) on one GPU.

Two configurations:
  reference-faithful  upenn and rpg rigs, the mvstereo presets (EM_NUM_EVENT_MATCHING 3000): esvo_map_tick_em in mode 2
                      (EM_PLUS_ESTIMATION) per tick, wall time of the call and HIP-event time of the matching kernels
  throughput          DSEC rig and stream, the host-array seam esvo_map_match_em on >= 1e5 left events
Each line of output is one JSON record with the filter-stage counts of esvo_map_em_stats and, from them, estimates of the f64
operations and Time-Surface bytes the pair-cost kernel performs (per pair: three column-major passes over two bilinear
patches of patch_size_X x patch_size_Y, 7 flops per sample + 2-5 per pass element; 4 u8 reads per sample, mostly from L2).
Usage: python tools/em_bench.py [--ticks K] [--warmup W] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from esvo_amd import calib, lib, params, synth  # noqa: E402
import em_restated as R  # noqa: E402

NS = R.NS


def stamps(ev):
    return ev["sec"].astype(np.uint64) * np.uint64(NS) + ev["nsec"].astype(np.uint64)


def estimates(s, wx, wy):
    area = wx * wy
    flops = s.patch_ok * area * (3 * 2 * 7 + 2 + 4 + 6) + s.epipolar * 40
    bytes_ts = s.patch_ok * area * 3 * 2 * 4
    checks = s.time_polarity  # candidates that reached the epipolar test (the time-window scan reads ~2x as many)
    return dict(pairs_time_polarity=int(s.time_polarity), pairs_epipolar=int(s.epipolar), pairs_patch_ok=int(s.patch_ok),
                matches=int(s.matches), events=int(s.events), right_events=int(s.right_events), slices=int(s.slices),
                est_f64_flop=int(flops), est_ts_bytes=int(bytes_ts), candidate_checks=int(checks))


def faithful(name, ticks, warmup):
    rig = calib.dataset_rig(name)
    cfg = params.PRESETS[f"mvstereo_{name}"]
    st = synth.make_stream(rig, 6000, 0.3, 0.2, 1.0, seed=7)
    p, _ = params.make_params(cfg, rig, max_events_per_tick=4096)
    em = params.make_em_params(cfg)
    dev = lib.Esvo(p, rig, device=0)
    dev.ts_push_events(0, st.ev_left)
    dev.ts_push_events(1, st.ev_right)
    wall, kern, last = [], [], None
    for k in range(warmup + ticks):
        t = st.t0_ns + int(0.05e9) + k * 5_000_000
        for c in (0, 1):
            dev.ts_render(c, t, download=False)
        dev.set_observation(t, None, None, st.pose(t))
        t0 = time.perf_counter()
        dev.tick_em(em, 2, t - 10_000_000, t, st.pose)
        dt = (time.perf_counter() - t0) * 1e3
        s = dev.em_stats()
        if k >= warmup:
            wall.append(dt)
            kern.append(s.ms_match)
            last = s
    rec = dict(config="faithful", rig=name, mode=2, num_event_matching=em.num_event_matching, ticks=ticks,
               tick_ms_median=float(np.median(wall)), match_kernels_ms_median=float(np.median(kern)),
               map_size=len(dev.get_map()))
    rec.update(estimates(last, p.patch_size_x, p.patch_size_y))
    dev.close()
    return rec


def throughput(ticks, warmup, n_left):
    rig = calib.dataset_rig("dsec")
    st = synth.make_stream(rig, 20000, 0.12, 0.02, 0.25, seed=7, speed=2.0)
    p, _ = params.make_params(params.PRESETS["mapping_dsec"], rig, max_events_per_tick=4096, smooth_time_surface=0)
    em = params.make_em_params(params.PRESETS["mvstereo_upenn"], num_event_matching=n_left)  # the shipped EM_* values
    dev = lib.Esvo(p, rig, device=0)
    dev.ts_push_events(0, st.ev_left)
    dev.ts_push_events(1, st.ev_right)
    t = st.t0_ns + int(0.1e9)
    g = [dev.ts_render(c, t) for c in (0, 1)]
    dev.set_observation(t, g[0], g[1], st.pose(t))
    t_low = t - 90_000_000
    sl, nl = R.select(stamps(st.ev_left), t_low, t, n_left)
    sr, nr = R.select(stamps(st.ev_right), t_low, t, n_left)
    left, right = st.ev_left[sl:sl + nl], st.ev_right[sr:sr + nr]
    slices = R.slice_events(stamps(left), t_low, t, em.slice_thickness)
    b = np.array([s[0] for s in slices], np.uint32)
    c = np.array([s[1] for s in slices], np.uint32)
    T = np.stack([np.asarray(st.pose(s[2]), np.float64).reshape(4, 4) for s in slices])
    wall, kern = [], []
    for k in range(warmup + ticks):
        t0 = time.perf_counter()
        m = dev.match_em(em, left, b, c, T, right)
        dt = (time.perf_counter() - t0) * 1e3
        s = dev.em_stats()
        if k >= warmup:
            wall.append(dt)
            kern.append(s.ms_match)
    rec = dict(config="throughput", rig="dsec", seam="esvo_map_match_em", num_event_matching=n_left, calls=ticks,
               call_ms_median=float(np.median(wall)), match_kernels_ms_median=float(np.median(kern)), n_matches=len(m),
               left_events_per_s=float(s.events / (np.median(kern) * 1e-3)))
    rec.update(estimates(s, p.patch_size_x, p.patch_size_y))
    dev.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-left", type=int, default=150_000)
    ap.add_argument("--quick", action="store_true", help="3 ticks, 1 warm-up (profiler runs)")
    a = ap.parse_args()
    if a.quick:
        a.ticks, a.warmup = 3, 1
    for name in ("upenn", "rpg"):
        print(json.dumps(faithful(name, a.ticks, a.warmup)), flush=True)
    print(json.dumps(throughput(a.ticks, a.warmup, a.n_left)), flush=True)


if __name__ == "__main__":
    main()
