"""The tracker's reprojection map (Reproj_Map_Left): what the device route costs next to the download the host route cannot avoid
(GPU box).

  (a)  track_reprojection_map(..., download=True)    draw on the device, 3 W H bytes down
  (b)  track_reprojection_map(..., download=False)   draw on the device, the image stays there; the call returns n_inside, so it
                                                     ends with the wait on the tracker's stream
  (c)  esvo_track_get_images(neg only)               W H bytes down: the host route's share of the bus -- its ~2000 cv::circle
                                                     calls on a CPU come on top and are NOT measured here

Per case: one handle, a random left Time Surface through track_set_current(kernelSize 5), 2000 reference points spread over the
image at inverse depths across the preset's range, a small registered motion.  After a warm-up the three calls alternate inside
every repetition (their order rotates); a repetition times `inner` back-to-back calls of each and reports ms per call.  One JSON
line per case: median, best and worst over the repetitions.

usage: python tools/track_reproj_bench.py [--reps N (>= 9, default 15)] [--inner K] [--warmup W] [--cases rpg,upenn,dsec] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esvo_amd import calib, lib, params  # noqa: E402

CASES = {"rpg": ("rpg", "mapping_rpg"), "upenn": ("upenn", "mapping_upenn"), "dsec": ("dsec", "mapping_dsec")}
N_POINTS = 2000   # numVisualization's cap, and MAX_REGISTRATION_POINTS of the shipped tracking configs


def make_case(name):
    rig_name, preset = CASES[name]
    rig = calib.dataset_rig(rig_name)
    cfg = params.PRESETS[preset]
    p, _ = params.make_params(cfg, rig)
    dev = lib.Esvo(p, rig)
    rng = np.random.default_rng(17)
    W, H = rig.width, rig.height
    dev.track_set_current(rng.integers(0, 256, (H, W)).astype(np.uint8), 5)
    P = np.asarray(rig.left.P, np.float64).reshape(3, 4)
    lo, hi = float(cfg["invDepth_min_range"]), float(cfg["invDepth_max_range"])
    z = 1.0 / rng.uniform(lo, hi, N_POINTS)
    x, y = rng.uniform(0, W, N_POINTS), rng.uniform(0, H, N_POINTS)
    xyz = np.stack([(x - P[0, 2]) * z / P[0, 0], (y - P[1, 2]) * z / P[1, 1], z], axis=1).astype(np.float32)
    dev.track_set_reference(xyz, np.eye(4))
    c, s = np.cos(0.004), np.sin(0.004)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([0.002, -0.001, 0.003])
    return dev, rig, R, t, lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="rpg,upenn,dsec")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.reps >= 9 and a.inner >= 1
    for name in a.cases.split(","):
        dev, rig, R, t, lo, hi = make_case(name)
        neg = np.empty((rig.height, rig.width), np.uint8)

        def call_a():
            return dev.track_reprojection_map(R, t, N_POINTS, lo, hi, download=True)[1]

        def call_b():
            return dev.track_reprojection_map(R, t, N_POINTS, lo, hi, download=False)[1]

        def call_c():
            dev._ck(dev.lib.esvo_track_get_images(dev.h, neg.ctypes.data, None, None))
            return 0

        calls = [("a", call_a), ("b", call_b), ("c", call_c)]
        img, n_inside = dev.track_reprojection_map(R, t, N_POINTS, lo, hi)
        painted = int((img != np.repeat(dev.track_images()[0][:, :, None], 3, axis=2)).any(axis=2).sum())
        assert call_b() == n_inside and painted > N_POINTS, "the benchmark's image is not the one it means to draw"
        ms = {k: [] for k, _ in calls}
        for rep in range(a.warmup + a.reps):
            for k, fn in calls[rep % 3:] + calls[:rep % 3]:
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    fn()
                dt = (time.perf_counter() - t0) * 1e3 / a.inner
                if rep >= a.warmup:
                    ms[k].append(dt)
        line = {"bench": "track_reproj", "case": name, "width": rig.width, "height": rig.height, "points": N_POINTS,
                "n_inside": int(n_inside), "painted_pixels": painted, "reps": a.reps, "inner": a.inner, "warmup": a.warmup,
                "bytes_down": {"a": 3 * rig.width * rig.height, "b": 0, "c": rig.width * rig.height}}
        for k, label in (("a", "a_map_download_ms"), ("b", "b_map_on_device_ms"), ("c", "c_neg_download_ms")):
            v = np.asarray(ms[k])
            line[label] = {"median": round(float(np.median(v)), 4), "best": round(float(v.min()), 4), "worst": round(float(v.max()), 4)}
        line["a_minus_c_median_ms"] = round(line["a_map_download_ms"]["median"] - line["c_neg_download_ms"]["median"], 4)
        print(json.dumps(line))
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        dev.close()


if __name__ == "__main__":
    main()
