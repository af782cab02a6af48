#!/usr/bin/env python3
"""Times the per-tick semi-global matching mode (esvo_MVStereo mode 4, esvo_map_tick_sgm) on one GPU.

Two configurations:
  reference-faithful  upenn, rpg and DSEC rigs with their presets' PROCESS_EVENT_NUM: esvo_ts_render of both cameras,
                      esvo_map_set_observation and esvo_map_tick_sgm per tick on device-resident Time Surfaces; wall time of the
                      tick call and the HIP-event times of its stages (esvo_sgm_stats_t: StereoSGBM chain, point stage, naive
                      propagation of the window)
  throughput          DSEC rig, a dense stream, PROCESS_EVENT_NUM 100 000: every event of the selection window becomes a
                      candidate point
Each line of output is one JSON record: median, minimum and maximum over the ticks, the filter counts of the last tick.
Usage: python tools/sgm_tick_bench.py [--ticks K] [--warmup W] [--quick] [--case upenn,dsec] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from esvo_amd import calib, lib, params, synth  # noqa: E402

CASES = {  # rig, preset, make_stream arguments, parameter overrides
    "upenn": ("upenn", "mvstereo_upenn", (6000, 0.3, 0.16, 1.0), dict(seed=7), {}),
    "rpg": ("rpg", "mvstereo_rpg", (4000, 0.3, 0.2, 2.0), dict(seed=7), {}),
    "dsec": ("dsec", "mapping_dsec", (20000, 0.2, 0.02, 0.25), dict(seed=7, speed=2.0), {}),
    "dsec_throughput": ("dsec", "mapping_dsec", (60000, 0.2, 0.02, 0.25), dict(seed=7, speed=2.0), dict(throughput_events=100_000)),
}
COUNTS = ("events", "on_image", "matched_columns", "disp_ok", "points", "zero_disp")


def spread(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def run(case, ticks, warmup):
    rig_name, preset, args, kw, over = CASES[case]
    rig = calib.dataset_rig(rig_name)
    st = synth.make_stream(rig, *args, **kw)
    p, _ = params.make_params(params.PRESETS[preset], rig, **over)
    # the mode keeps maxNumFusionFrames frames of up to PROCESS_EVENT_NUM + 1 points whatever the fusion strategy; the presets size
    # the window ring for their own strategy (CONST_POINTS on upenn)
    p.max_window_points = max(p.max_window_points, p.max_fusion_frames * (p.process_event_num + 1))
    dev = lib.Esvo(p, rig, device=0)
    dev.ts_push_events(0, st.ev_left)
    dev.ts_push_events(1, st.ev_right)
    wall, stage, g = [], [], None
    for k in range(warmup + ticks):
        t = st.t0_ns + int(0.05e9) + k * 5_000_000
        for c in (0, 1):
            dev.ts_render(c, t, download=False)
        dev.set_observation(t, None, None, st.pose(t))
        t0 = time.perf_counter()
        dev.tick_sgm(want_disp=False)
        dt = (time.perf_counter() - t0) * 1e3
        g = dev.sgm_stats()
        if k >= warmup:
            wall.append(dt)
            stage.append((g.ms_sgbm, g.ms_points, g.ms_propagate))
    stage = np.asarray(stage)
    s = dev.stats()
    rec = dict(config="throughput" if "throughput" in case else "faithful", case=case, rig=rig_name, width=rig.width, height=rig.height,
               process_event_num=int(p.process_event_num), max_fusion_frames=int(p.max_fusion_frames), ticks=ticks,
               tick_ms=spread(wall), sgbm_ms=spread(stage[:, 0]), points_ms=spread(stage[:, 1]), propagate_ms=spread(stage[:, 2]),
               window_frames=int(s.last_window_frames), window_points=int(s.last_window_points), map_size=len(dev.get_map()))
    rec.update({c: int(getattr(g, c)) for c in COUNTS})
    dev.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="3 ticks, 1 warm-up (profiler runs)")
    ap.add_argument("--case", default=",".join(CASES), help="comma-separated subset of: " + ", ".join(CASES))
    ap.add_argument("--out", help="append the records to this file as well")
    a = ap.parse_args()
    if a.quick:
        a.ticks, a.warmup = 3, 1
    for case in a.case.split(","):
        line = json.dumps(run(case, a.ticks, a.warmup))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
