"""What the Time-Surface history adds to a rendered pair: one device-to-device copy per camera behind the render.

One handle per image size (240 x 180, 346 x 260, 640 x 480); the two settings -- history off, history on (100 pairs) --
alternate, each repetition renders `--pairs` consecutive pairs 1 ms apart on a stationary scene (the same event rate in every
repetition) in two ways:
  lone      render left, render right, wait: the latency a node sees that renders one pair and reads the result
  batch     all pairs enqueued, one wait at the end: the time the front queue is busy per pair
Prints per size the median and the worst of the per-pair times of either setting and their differences, and one JSON line.

    python tools/ts_history_bench.py [--reps 9] [--pairs 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SIZES = {"240x180": ("rpg", "mvstereo_rpg", 3000, (0.3, 1.8)), "346x260": ("upenn", "mapping_upenn", 5000, (0.16, 1.0)),
         "640x480": ("dsec", "mapping_dsec", 9000, (0.02, 0.25))}


def measure(name, reps, pairs):
    from esvo_amd import calib, lib, params, synth
    rig_name, preset, n_points, rho = SIZES[name]
    rig = calib.dataset_rig(rig_name)
    p, _ = params.make_params(params.PRESETS[preset], rig)
    blocks = 2 * 2 * reps + 2                       # (lone + batch) x (off + on) x reps, and a warm-up of each kind
    st = synth.make_stream(rig, n_points, (blocks * pairs + 20) * 1e-3, rho[0], rho[1], seed=20251019, stationary=True)
    dev = lib.Esvo(p, rig)
    dev.ts_push_events(0, st.ev_left)
    dev.ts_push_events(1, st.ev_right)
    t = [st.t0_ns + 10_000_000]

    def block(lone):
        c0 = time.perf_counter()
        for _ in range(pairs):
            t[0] += 1_000_000
            dev.ts_render(0, t[0], download=False)
            dev.ts_render(1, t[0], download=False)
            if lone:
                dev.synchronize()
        dev.synchronize()
        return (time.perf_counter() - c0) * 1e6 / pairs

    block(True), block(False)
    out = {"lone": {0: [], 1: []}, "batch": {0: [], 1: []}}
    for r in range(reps):
        for on in ((0, 1) if r % 2 == 0 else (1, 0)):
            dev.ts_history_configure(100 if on else 0)
            out["lone"][on].append(block(True))
            out["batch"][on].append(block(False))
    dev.close()
    res = {"size": name, "reps": reps, "pairs": pairs}
    for kind in ("lone", "batch"):
        off, on = np.array(out[kind][0]), np.array(out[kind][1])
        res[kind] = dict(off_median_us=float(np.median(off)), on_median_us=float(np.median(on)), off_worst_us=float(off.max()),
                         on_worst_us=float(on.max()), added_median_us=float(np.median(on) - np.median(off)),
                         added_worst_us=float((on - off).max()))
        print(f"{name} {kind:5s}: off {np.median(off):8.1f} us (worst {off.max():8.1f}), on {np.median(on):8.1f} us (worst {on.max():8.1f}), "
              f"added per pair: median {np.median(on) - np.median(off):6.1f} us, worst repetition {(on - off).max():6.1f} us")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--sizes", default=",".join(SIZES))
    a = ap.parse_args()
    assert a.reps >= 9, "at least 9 repetitions"
    res = [measure(s, a.reps, a.pairs) for s in a.sizes.split(",")]
    print(json.dumps({"ts_history_bench": res}))


if __name__ == "__main__":
    main()
