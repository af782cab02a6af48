"""EventBM::match_an_event restated for one event in plain Python (kernels_bm.hip's operation; the oracle: oracle/esvo_oracle.cpp,
BM::match_an_event).  Moments are exact Python integers, the cost is float64 in the expression order of the oracle's zncc_cost_int,
the argmin scans upwards with `<=` (the largest disparity among equal minima wins), the coarse / fine rule, the up-down variant and
the pose lower bound follow the reference line by line.  match() returns a trace that says which gate stopped the event and what
the search saw on the way; tests/bm_cases.py turns it into tags.

cost_definition() is a second, independent restatement: both patches normalised as tools::normalizePatch does, the products summed,
everything in np.longdouble."""
import math

import numpy as np

ZNCC_MAX = 1.0


def time_to_sec(sec, nsec):
    return float(sec) + 1e-9 * float(nsec)


def ns_to_sec(ns):
    ns = int(ns)
    return time_to_sec(ns // 1_000_000_000, ns % 1_000_000_000)


def moments(l, r):
    """(Sl, Sll, Sr, Srr, Slr) of two equal-size u8 patches as Python ints"""
    l = [int(v) for v in np.asarray(l).reshape(-1)]
    r = [int(v) for v in np.asarray(r).reshape(-1)]
    return (sum(l), sum(v * v for v in l), sum(r), sum(v * v for v in r), sum(a * b for a, b in zip(l, r)))


def cost_int(Sl, Sll, Sr, Srr, Slr, N):
    """zncc_cost_int: float64, the oracle's expression order"""
    n = float(N)
    varl = float(N * Sll - Sl * Sl) / (n * n)
    varr = float(N * Srr - Sr * Sr) / (n * n)
    sigl, sigr = math.sqrt(varl) + 1e-6, math.sqrt(varr) + 1e-6
    cov = float(N * Slr - Sl * Sr) / n
    return 0.5 * (1 - cov / (sigl * sigr) / n)


def cost_definition(l, r):
    """0.5 (1 - sum(l^ r^) / N) with x^ = (x - mean) / (sqrt(mean((x - mean)^2)) + 1e-6), in np.longdouble"""
    LD = np.longdouble
    out = []
    for p in (l, r):
        p = np.asarray(p).astype(LD).reshape(-1)
        mean = p.sum() / LD(p.size)
        s = p - mean
        sigma = np.sqrt((s * s).sum() / LD(p.size)) + LD(1e-6)
        out.append(s / sigma)
    return LD(0.5) * (LD(1) - (out[0] * out[1]).sum() / LD(out[0].size))


class Setup:
    """what one search reads: the rig's look-up table and mask, both images, the parameters"""

    def __init__(self, rig, left, right, p, baseline=None):
        self.W, self.H = rig.width, rig.height
        self.lut = np.asarray(rig.left.rect_lut, np.float32).reshape(self.H, self.W, 2)
        self.mask = None if rig.left.rect_mask is None else np.asarray(rig.left.rect_mask, np.uint8).reshape(self.H, self.W)
        self.left, self.right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
        self.wx, self.wy = int(p.patch_size_x), int(p.patch_size_y)
        self.hx, self.hy = (self.wx - 1) // 2, (self.wy - 1) // 2
        self.dmin, self.dmax, self.step = int(p.bm_min_disparity), int(p.bm_max_disparity), int(p.bm_step)
        self.updown, self.thr = bool(p.bm_updown), float(p.bm_zncc_threshold)
        self.bf = float(rig.baseline if baseline is None else baseline) * float(rig.left.P[0])   # baseline * P_left(0, 0)

    def valid_patch(self, x, y):
        return not (x - self.hx < 1 or y - self.hy < 1 or x + self.hx >= self.W - 1 or y + self.hy >= self.H - 1)

    def block(self, img, x, y):
        return img[y - self.hy:y - self.hy + self.wy, x - self.hx:x - self.hx + self.wx]

    def candidate(self, x1, y1, d):
        return (x1, y1 - d) if self.updown else (x1 - d, y1)

    def inside(self, x, y):
        """the block lies inside the image (an invalid candidate's may: the patch rule keeps one pixel more)"""
        return x - self.hx >= 0 and y - self.hy >= 0 and x - self.hx + self.wx <= self.W and y - self.hy + self.wy <= self.H


def _scan(costs, ds, best, bestd):
    """epipolarSearching's loop over the candidates ds (increasing): `cost <= min_cost` updates"""
    for d in ds:
        c = costs.get(d)
        if c is not None and c <= best:
            best, bestd = c, d
    return best, bestd


def match(s, ev, stamps):
    """one event -> trace: gate (None: matched) in 'raw', 'lut', 'mask', 'border', 'noise', 'coarse', 'fine', 'pose'; reason (the
    reference's failure counter: 1 info-noise, 2 coarse, 3 fine, 0 none); record (the match, when gate is None)"""
    t = dict(gate=None, reason=0, record=None, cnt=None, valid=[], row={}, ghost={}, ties=[], coarse=None, pose_idx=None, x1=None, y1=None,
             xr=None, yr=None, best=None, bestd=None, Sl=None, Sll=None)
    ex, ey = int(ev["x"]), int(ev["y"])
    if ex >= s.W or ey >= s.H:
        t["gate"] = "raw"
        return t
    xr, yr = float(s.lut[ey, ex, 0]), float(s.lut[ey, ex, 1])
    t["xr"], t["yr"] = xr, yr
    if xr < 0 or xr > float(s.W - 1) or yr < 0 or yr > float(s.H - 1):
        t["gate"] = "lut"
        return t
    if s.mask is not None and not s.mask[int(yr), int(xr)] > 125:      # index truncation
        t["gate"] = "mask"
        return t
    x1, y1 = int(math.floor(xr)), int(math.floor(yr))
    t["x1"], t["y1"] = x1, y1
    if not s.valid_patch(x1, y1):
        t["gate"] = "border"
        return t
    L = s.block(s.left, x1, y1)
    N = s.wx * s.wy
    t["cnt"] = int((L < 1).sum())
    if float(t["cnt"]) > 0.95 * float(N):
        t["gate"], t["reason"] = "noise", 1
        return t
    # the dense cost row: every candidate of [dmin, dmax] (a superset of what a coarse pass evaluates)
    for d in range(s.dmin, s.dmax + 1):
        x2, y2 = s.candidate(x1, y1, d)
        ok = s.valid_patch(x2, y2)
        if ok or s.inside(x2, y2):
            m = moments(L, s.block(s.right, x2, y2))
            c = cost_int(*m, N)
            t["Sl"], t["Sll"] = m[0], m[1]
            if ok:
                t["valid"].append(d)
                t["row"][d] = c
            else:
                t["ghost"][d] = c      # what the candidate would cost if the patch rule did not refuse it
    step = s.step
    coarse_ds = list(range(s.dmin, s.dmax + 1, step))
    best, bestd = _scan(t["row"], coarse_ds, ZNCC_MAX, None)
    found = False
    if step > 1:
        co = dict(cd=bestd, cbest=best, why=None)
        t["coarse"] = co
        if bestd is None:
            co["why"] = "none_valid"
        elif bestd - step < s.dmin or bestd - step not in coarse_ds:    # (size_t arithmetic: best - step must not wrap)
            co["why"] = "no_lower"
        elif bestd + step not in coarse_ds:
            co["why"] = "no_upper"
        elif not (t["row"].get(bestd - step, ZNCC_MAX) < ZNCC_MAX and t["row"].get(bestd + step, ZNCC_MAX) < ZNCC_MAX):
            co["why"] = "neighbour_invalid"
        elif not best < s.thr:
            co["why"] = "threshold"
        else:
            found = True
    else:
        found = bestd is not None and best < s.thr
    t["best"], t["bestd"] = best, bestd
    if not found:
        t["gate"], t["reason"] = "coarse", 2
        return t
    # fine pass over [best - (step - 1), best + (step - 1)] with the carried minimum
    fine_ds = list(range(bestd - (step - 1), bestd + (step - 1) + 1))
    if step > 1:
        t["coarse"]["fine_ds"] = fine_ds
    best, bestd = _scan(t["row"], fine_ds, best, bestd)
    t["best"], t["bestd"] = best, bestd
    t["ties"] = [d for d in (coarse_ds if step == 1 else fine_ds) if t["row"].get(d) == best]
    if not best < s.thr:
        t["gate"], t["reason"] = "fine", 3
        return t
    te = time_to_sec(int(ev["sec"]), int(ev["nsec"]))
    lo, hi = 0, len(stamps)
    while lo < hi:
        mid = (lo + hi) // 2
        if ns_to_sec(stamps[mid]) < te:
            lo = mid + 1
        else:
            hi = mid
    t["pose_idx"] = lo
    if lo == len(stamps):
        t["gate"] = "pose"
        return t
    disparity = float(bestd)
    with np.errstate(divide="ignore"):
        depth = np.float64(s.bf) / np.float64(disparity)
        inv = float(np.float64(1.0) / depth)
    t["record"] = dict(x_left=(xr, yr), inv_depth=inv, cost=best, disp=disparity, pose_idx=lo)
    return t


def match_all(s, events, stamps, num_threads):
    """(traces per event, records in the reference's thread-stride order as (event_idx, record), failure counts [1, 2, 3])"""
    traces = [match(s, e, stamps) for e in events]
    order = [i for th in range(num_threads) for i in range(th, len(events), num_threads)]
    recs = [(i, traces[i]["record"]) for i in order if traces[i]["gate"] is None]
    fails = [sum(t["reason"] == r for t in traces) for r in (1, 2, 3)]
    return traces, recs, fails
