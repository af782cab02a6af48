"""Crafted stamps, maps and event queues for the Time-Surface raster (kernels_ts.hip: ts_scatter, tsq_bin / tsq_merge / tsq_view,
ts_render_fused with ts_decay_u8, the FORWARD pair ts_decay_f64 + ts_forward_gather, ts_median_remap, gaussian5), run through the
public entries in tests/test_gpu_ts_cases.py; the cases themselves are tested on the CPU in tests/test_ts_cases.py.

A stream almost never brings the raster to a close decision.  Here every input is put where one is taken:
  decay     one event per pixel of a 128 x 96 image whose stamp lies within +-3 ns of a crossing of the quantised value (without
            polarity 255 e = q + 1/2 for q = 0 ... 254; with polarity 127.5 e = j for j = 1 ... 127 and both signs), for decay_ms
            1, 30 and 10000; the same crossings stepped away until the f64 value lies 5e-4 ... 1e-3 from the half-integer, just
            outside the float shortcut's guard band; stamps 0, T - 1, T, T + 1, dt beyond 2^24 and 2^32 ns, dt where a float
            exponential underflows, and crossings under stamps at 1.6e18 ns with nsec(T) < nsec(te);
  median    a lone lit pixel, exactly n / 2 and n / 2 + 1 lit values of the n = (2k + 1)^2 replicated window, and equal values
            on both sides of the rank, each at the four corners, on the four borders and inside, for k = 1, 2, 3;
  remap     exact ties of map * 32 towards even in both directions, zero-weight taps on the last column and row, coordinates
            in (-1, 0) and (W - 1, W), the -1e6 marker, a tile without any tap in the image, partly outside tiles, a mirrored and
            a transposed map;
  staging   tiles whose source box has exactly the staging capacity, the smallest box above it, a one-pixel box (a constant
            map), a box wider than 256, a magnifying map whose boxes never fit -- each for k = 0, 1, 2 (and 3);
  geometry  33 x 17 and 70 x 40: tiles of one column, of one row, of six columns, and a last tile row with rows 0 ... 7 only;
  queues    L = 1, 3, 20, 32 on 20 x 12 (tiles hang over both edges): more than L events on a pixel in one batch and across
            batches, more than L events newer than T hiding an older one, render times going backwards, a zero stamp, events
            outside the sensor, an event at T alone and above an older one, equal stamps; 1088 events of one tile in one batch with a second tile's events
            in the overflow list at the same time;
  FORWARD   look-up positions on integers, outside the image, nine sources on one destination whose running sum passes 1
            before the last addition (with polarity: the clamp after every addition decides), a negative sum, a source without
            an event between two contributing ones;
  gaussian  impulses of 255 at the corners, on the borders and two pixels in, an all-255 image.

Sizes: nothing above 128 x 96 and nothing below 8, with one exception: a source box wider than 256 cannot exist in an image
narrower than 251 pixels, so that one rig is 264 x 8 (2112 pixels, a sixth of 128 x 96).

observe() (through tests/ts_restated.py) turns what a case really reaches into tags; each case states the tags it was written for,
REQUIRED what the list as a whole has to reach.

Float-only disagreements with f64 per crossing sweep (pixels where rounding the numpy float32 evaluation of the short form gives
another value than f64; all of them lie inside the guard band, so the device re-evaluates them in f64), and the pixels of the
stepped-away sweeps that lie 5e-4 ... 1e-3 from a half-integer in f64 -- as counted by tests/test_ts_cases.py:
  decay_ms  ignore_polarity  float-only rounding differs  inside the band  float error  5e-4 ... 1e-3 from a half-integer
         1                1               13 of 1785             1568      3.3e-5        510 of 510
         1                0               63 of 1778             1778      2.4e-5        508 of 508
        30                1              447 of 1785             1785      3.3e-5        510 of 510
        30                0              629 of 1778             1778      2.7e-5        508 of 508
     10000                1              878 of 1785             1785      3.1e-5        510 of 510
     10000                0              879 of 1778             1778      1.5e-5        508 of 508
(required: at least 200 disagreements at decay_ms 30 and 10000, 10 at 1; at least 200 pixels just outside the band).
"""
import copy
import functools
import hashlib
import math

import numpy as np

import ts_restated as TR
from esvo_amd import abi, calib, params

NS = TR.NS
FOCAL, BASELINE = 100.0, 0.1
T_DEC = 100 * NS                               # render time of the decay cases (dt reaches 62.4 s at decay_ms = 10000)
T_EPOCH = 1_600_000_001 * NS + 100             # nsec(T) = 100: every stamp less than a second older has a larger nsec
T_TEX = 5 * NS                                 # render time of the textured cases
OFFS = (-3, -2, -1, 0, 1, 2, 3)
JUST_OVER = {0: 2574, 1: 2562, 2: 2562}        # the smallest rw * rh above 2560 that fits 70 x 40 (+ the ring): 66 x 39, 61 x 42, 61 x 42


# ---- rigs -------------------------------------------------------------------------------------------------------------------------
def _identity(W, H):
    y, x = np.mgrid[:H, :W]
    return x.astype(np.float64), y.astype(np.float64)


def _tile(W, H, tx, ty):
    return range(tx * 32, min(tx * 32 + 32, W)), range(ty * 16, min(ty * 16 + 16, H))


def fit_tile(mx, my, tx, ty, x0, y0, mw, mh):
    """the pixels of output tile (tx, ty) spread over the mw x mh source box at (x0, y0), its corners hit exactly"""
    H, W = mx.shape
    xs, ys = _tile(W, H, tx, ty)
    for y in ys:
        for x in xs:
            mx[y, x] = x0 + ((x - xs[0]) * (mw - 1)) / max(len(xs) - 1, 1)
            my[y, x] = y0 + ((y - ys[0]) * (mh - 1)) / max(len(ys) - 1, 1)


def _map_capacity():
    """70 x 40, per tile a source box at the staging capacity for one median size and beside it for the others"""
    W, H = 70, 40
    mx, my = _identity(W, H)
    fit_tile(mx, my, 0, 0, 0, 0, 64, 40)     # k = 0: 64 x 40 = 2560
    fit_tile(mx, my, 1, 0, 4, 1, 62, 38)     # k = 1: 64 x 40
    fit_tile(mx, my, 0, 1, 5, 2, 60, 36)     # k = 2: 64 x 40
    fit_tile(mx, my, 1, 1, 3, 0, 59, 40)     # k = 1: 61 x 42 = 2562
    fit_tile(mx, my, 0, 2, 2, 0, 66, 39)     # k = 0: 66 x 39 = 2574 (a tile of 8 rows)
    fit_tile(mx, my, 1, 2, 6, 1, 57, 38)     # k = 2: 61 x 42
    xs, ys = _tile(W, H, 2, 1)
    mx[ys.start:ys.stop, xs.start:xs.stop], my[ys.start:ys.stop, xs.start:xs.stop] = 10.0, 10.0      # a constant map: a box of one pixel
    return mx, my


def _map_edges():
    """70 x 40, per tile one kind of edge of the remap"""
    W, H = 70, 40
    mx, my = _identity(W, H)
    for y in range(16):
        for x in range(32):                  # (0, 0): map * 32 = n + 1/2 exactly; towards even is down for 1/64 and up for 3/64
            mx[y, x] = x + (1 / 64 if x % 2 == 0 else 3 / 64)
            my[y, x] = y + (3 / 64 if y % 2 == 0 else 1 / 64)
        for x in range(32, 64):              # (1, 0): coordinates in (-1, 0), and in (W - 1, W)
            mx[y, x] = -0.5 - (x - 32) / 64 if y < 8 else W - 1 + 0.25 + (x - 32) / 64
        for x in range(64, 70):              # (2, 0): fx = 0 at ix + 1 == W; fy = 0 at iy + 1 == H
            if x < 66:
                mx[y, x] = W - 1
            else:
                my[y, x] = H - 1
    for y in range(16, 32):
        for x in range(32):                  # (0, 1): no tap in the image -- the marker, and coordinates behind the last column
            mx[y, x], my[y, x] = (-1e6, -1e6) if x < 16 else (W + 5, y)
        for x in range(32, 64):              # (1, 1): partly outside
            mx[y, x], my[y, x] = x + 10.3, y - 20.6
        for x in range(64, 67):              # (2, 1): the marker on three of six columns
            mx[y, x], my[y, x] = -1e6, -1e6
    for y in range(32, 40):
        for x in range(32):                  # (0, 2): a constant map on an integer position
            mx[y, x], my[y, x] = 7.0, 33.0
        for x in range(32, 64):              # (1, 2): a constant map between four pixels
            mx[y, x], my[y, x] = 7.5, 33.5
    return mx, my


def _map_mirror(W, H):
    x, y = _identity(W, H)
    return W - 1 - x, H - 1 - y


def _map_transposed(W, H):
    x, y = _identity(W, H)
    return y, x                              # (source rows beyond H - 1: outside)


def _map_magnify():
    x, y = _identity(128, 96)
    return 3 * x + 0.25, 3 * y + 0.25


def _map_constant():
    x, y = _identity(128, 96)
    return np.full_like(x, 64.0), np.full_like(y, 48.0)


def _map_wide(rows):
    """264 x 8: the first tile's 32 columns spread over all 264 source columns and `rows` source rows"""
    mx, my = _identity(264, 8)
    fit_tile(mx, my, 0, 0, 0, 0, 264, rows)
    return mx, my


def _lut_forward(W, H):
    """33 x 17, FORWARD look-up table of the left camera: integer positions (the identity), positions outside the image, ten
    sources on the destination (20, 8), four on the pixels around (25.5, 10.5), fractional positions on the last rows"""
    lut = np.zeros((H, W, 2), np.float32)
    x, y = _identity(W, H)
    lut[..., 0], lut[..., 1] = x, y
    lut[0, 0], lut[0, 1], lut[0, 2], lut[0, 3], lut[0, 4] = (-0.5, 3.0), (W - 0.5, 3.0), (-1e6, -1e6), (5.0, H - 1.0), (W - 1.0, 5.0)
    lut[0, 5], lut[0, 6] = (5.0, -0.25), (W - 2.0, H - 2.0)          # (the last position that splats: u_i + 1 = W - 1)
    for sx in FWD_MANY:
        lut[5, sx] = (20.0, 8.0)
    for sx in FWD_NEG:
        lut[9, sx] = (25.5, 10.5)
    lut[13:, :, 0] += 0.37
    lut[13:, :, 1] -= 0.61
    return lut


FWD_MANY, FWD_NEG = tuple(range(3, 13)), tuple(range(3, 7))
FWD_GAP = 6                                    # the source of FWD_MANY without an event
# (polarity, expVal) of the sources of (20, 8) in raster order; the running sum with the clamp after every addition:
# .6, 1.2 -> 1, .5, [no event], .8, 1.2 -> 1, .1, .3, .2, .25; without the clamp it ends at .65
FWD_SEQ = ((1, .6), (1, .6), (0, .5), None, (1, .3), (1, .4), (0, .9), (1, .2), (0, .1), (1, .05))


@functools.lru_cache(maxsize=None)
def rig(key):
    """a StereoRig with crafted map_x / map_y (and rect_lut) arrays; cases that share a key share a device handle"""
    W, H, left, right, lut = {
        "id128": (128, 96, _identity, _identity, None),
        "mag128": (128, 96, lambda W, H: _map_magnify(), lambda W, H: _map_constant(), None),
        "s70": (70, 40, lambda W, H: _map_capacity(), lambda W, H: _map_edges(), None),
        "g33": (33, 17, _map_mirror, _map_transposed, _lut_forward),
        "m40": (40, 24, _identity, _identity, None),
        "wide": (264, 8, lambda W, H: _map_wide(3), lambda W, H: _map_wide(8), None),
        "q20": (20, 12, _identity, _identity, None),
    }[key]
    r = copy.deepcopy(calib.ideal_rig(W, H, FOCAL, BASELINE))
    for cam, f in ((r.left, left), (r.right, right)):
        mx, my = f(W, H)
        cam.map_x[...], cam.map_y[...] = mx, my
        assert np.isfinite(cam.map_x).all() and np.isfinite(cam.map_y).all()
    if lut is not None:
        r.left.rect_lut[...] = lut(W, H)
        x, y = _identity(W, H)
        r.right.rect_lut[..., 0], r.right.rect_lut[..., 1] = x + 0.5, y + 0.5
    for cam in (r.left, r.right):
        for a in (cam.map_x, cam.map_y, cam.rect_lut):
            a.setflags(write=False)
    return r


def cams(c):
    return c["rig"].left, c["rig"].right


# ---- events -----------------------------------------------------------------------------------------------------------------------
def events(rows):
    """rows of (x, y, stamp, polarity) -> esvo_event_t records in stamp order (stable: equal stamps keep the order of the rows)"""
    rows = sorted(rows, key=lambda r: r[2])
    ev = abi.make_events([r[0] for r in rows], [r[1] for r in rows], np.array([r[2] for r in rows], np.uint64), [r[3] for r in rows])
    ev.setflags(write=False)
    return ev


def texture_events(W, H, T, seed, span_ns=120_000_000, empty=0.1, skip=()):
    """one event per pixel (but a tenth of them, and `skip`) at a seeded stamp in [T - span, T), either polarity"""
    rng = np.random.default_rng(seed)
    pix = rng.permutation(W * H)[:int(W * H * (1 - empty))]
    t = np.sort(rng.integers(T - span_ns, T, len(pix)))
    pol = rng.integers(0, 2, len(pix))
    return [(int(p % W), int(p // W), int(s), int(q)) for p, s, q in zip(pix, t, pol) if (int(p % W), int(p // W)) not in skip]


def dt_of(e, decay_ms):
    """the age in ns at which exp(-dt / decay) = e"""
    return int(round(-decay_ms * 1e6 * math.log(e)))


def crossing_dts(decay_ms, ignore_polarity):
    """(dt, polarity) of every crossing of the quantised value: 255 e = q + 1/2, or 127.5 e = j under both signs"""
    if ignore_polarity:
        return [(dt_of((q + 0.5) / 255.0, decay_ms), 1) for q in range(255)]
    return [(dt_of(j / 127.5, decay_ms), p) for j in range(1, 128) for p in (1, 0)]


def in_raster(W, stamps_pol, T):
    """one event per pixel in raster order, oldest first"""
    rows = sorted(((T - dt, p) for dt, p in stamps_pol), key=lambda r: r[0])
    return [(i % W, i // W, t, p) for i, (t, p) in enumerate(rows)]


def _case(key, script, decay_ms=30.0, ignore_polarity=1, median_k=0, L=0, tags=(), group="", pinned=False, oracle=True, doc=""):
    r = rig(key)
    return dict(key=key, rig=r, W=r.width, H=r.height, script=script, decay_ms=float(decay_ms), ignore_polarity=int(ignore_polarity),
                median_k=int(median_k), L=int(L), tags=tuple(tags), group=group, pinned=pinned, oracle=oracle, doc=doc)


def both(T):
    return [("render", 0, T), ("render", 1, T)]


# ---- decay ------------------------------------------------------------------------------------------------------------------------
def _sweep(decay_ms, ip, T=T_DEC, every=1):
    """Left camera: stamps within +-3 ns of every crossing.  Right camera: every crossing stepped away by the age difference
    that moves the f64 value 7.5e-4 from the half-integer, to both sides."""
    W = 128
    cr = crossing_dts(decay_ms, ip)[::every]
    near = [(dt + o, p) for dt, p in cr for o in OFFS if dt + o > 0]
    amp = 255.0 if ip else 127.5
    away = []
    for dt, p in cr:
        slope = amp * math.exp(-dt / (decay_ms * 1e6)) / (decay_ms * 1e6)       # |dg / d dt| per ns
        n = max(int(round(7.5e-4 / slope)), 1)
        away += [(dt + s * n, p) for s in (-1, 1) if dt + s * n > 0]
    tags = ["dec:cross", "dec:away"] + (["dec:borrow"] if T == T_EPOCH else [])
    return _case("id128", [("push", 0, events(in_raster(W, near, T))), ("push", 1, events(in_raster(W, away, T)))] + both(T), decay_ms, ip,
                 tags=tags, group="decay", pinned=True, doc=_sweep.__doc__)


def _decay_edges(decay_ms, ip):
    """An empty pixel, a stamp of 0, events at T - 1, T and T + 1 ns, ages of 2^24 + 1, 2^24 + 3 and 2^25 + 1 ns (no float holds
    them), of 2^32 and 2^32 + 1 ns, of 2.7 and 60 s (at 30 ms the float exponential underflows to 0: with polarity 127.5 -> 128
    under both signs), and the ages around the 0 / 1 boundary of the quantised value (dt = ln 510 decay = 6.23 decay)."""
    T = T_DEC
    ages = [1, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 1, 2 ** 32, 2 ** 32 + 1, 2_700_000_000, 60 * NS]
    b = dt_of(0.5 / 255.0, decay_ms) if ip else dt_of(1 / 127.5, decay_ms)
    ages += [b + o for o in OFFS]
    rows = [(3 + 2 * i + 40 * p, 5 + (i % 3), T - a, (i + p) & 1) for p in (0, 1) for i, a in enumerate(ages)]      # (every age under both signs)
    rows += [(0, 0, 0, 1), (1, 0, 0, 0), (60, 50, T, 1), (61, 50, T + 1, 0), (62, 50, T + 1, 1)]
    tags = ["dec:empty", "dec:stamp0", "dec:T-1", "dec:T", "dec:T+1", "dec:dt>=2^24", "dec:dt>=2^32", "dec:boundary01"]
    tags += ["dec:e32_zero"] if decay_ms == 30 else []
    ev = events(rows)
    return _case("id128", [("push", 0, ev), ("push", 1, ev[::2])] + both(T), decay_ms, ip, tags=tags, group="decay", pinned=True, doc=_decay_edges.__doc__)


# ---- median -----------------------------------------------------------------------------------------------------------------------
MED_LOCS = {"c00": (0, 0), "c10": (39, 0), "c01": (0, 23), "c11": (39, 23), "bN": (20, 0), "bS": (20, 23), "bW": (0, 12), "bE": (39, 12), "in": (20, 12)}
MED_KINDS = ("lone", "below", "above", "equal")


def window_weights(W, H, x, y, k):
    """how often each pixel appears in the replicated (2k + 1)^2 window of (x, y)"""
    w = {}
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            p = (min(max(x + dx, 0), W - 1), min(max(y + dy, 0), H - 1))
            w[p] = w.get(p, 0) + 1
    return w


def pick(weights, target, taken=()):
    """pixels whose weights add up to the target: the heaviest first (the window holds enough pixels of weight 1)"""
    got, total = [], 0
    for p, w in sorted(weights.items(), key=lambda kv: (-kv[1], kv[0])):
        if p not in taken and total + w <= target:
            got.append(p)
            total += w
    assert total == target, (total, target)
    return got


def median_rows(W, H, k, kind, T):
    n = (2 * k + 1) ** 2
    lit, mid = 1, dt_of(200.2 / 255.0, 30.0)
    rows = []
    for c in MED_LOCS.values():
        w = window_weights(W, H, c[0], c[1], k)
        if kind == "lone":
            rows += [(c[0], c[1], T - lit, 1)]
        elif kind in ("below", "above"):
            rows += [(x, y, T - lit, 1) for x, y in pick(w, n // 2 + (kind == "above"))]
        else:      # n / 2 + 1 values of 200 with zeros below them and one or two pixels of 255 above: the rank lies among the equal ones
            eq = pick(w, n // 2 + 1)
            rest = sorted((v, p) for p, v in w.items() if p not in eq)
            top = [p for i, (v, p) in enumerate(rest[:2]) if sum(u for u, _ in rest[:i + 1]) <= n // 2 - 1]
            assert top
            rows += [(x, y, T - mid, 1) for x, y in eq] + [(x, y, T - lit, 1) for x, y in top]
    return rows


def _median(k, kinds):
    """Left and right camera carry one kind of pattern each, around nine centres: the corners, the middle of each border, the
    inside.  lone: the centre alone is lit; below / above: exactly n / 2 and n / 2 + 1 values of the replicated window are 255;
    equal: n / 2 + 1 values of 200 between zeros and two values of 255."""
    W, H, T = 40, 24, T_TEX
    script = [("push", cam, events(median_rows(W, H, max(k, 1), kind, T))) for cam, kind in enumerate(kinds)] + both(T)
    tags = [f"med:k{k}:{kind}:{loc}" for kind in kinds for loc in MED_LOCS] if k else ["med:k0"]
    c = _case("m40", script, 30.0, 1, k, tags=tags, group="median", doc=_median.__doc__)
    c["kinds"] = kinds
    return c


# ---- remap, staging, geometry -------------------------------------------------------------------------------------------------------
def _textured(key, k, ip, tags, group):
    """Both cameras under their own map and their own seeded texture: one event per pixel but a tenth, ages up to four decays."""
    r = rig(key)
    W, H = r.width, r.height
    script = [("push", cam, events(texture_events(W, H, T_TEX, 1000 * cam + W + k))) for cam in (0, 1)] + both(T_TEX)
    return _case(key, script, 30.0, ip, k, tags=tags, group=group, doc=_textured.__doc__)


S70_TAGS = {0: ("stage:k0:at_cap", "stage:k0:just_over"), 1: ("stage:k1:at_cap", "stage:k1:just_over"), 2: ("stage:k2:at_cap", "stage:k2:just_over"), 3: ()}
REMAP_TAGS = ("remap:tie_down", "remap:tie_up", "remap:fx0_last_col", "remap:fy0_last_row", "remap:x_in(-1,0)", "remap:x_in(W-1,W)", "remap:marker",
              "tile:empty", "tile:partial", "tile:rows8", "tile:cols6")


# ---- queues -----------------------------------------------------------------------------------------------------------------------
Q_T0 = 1 * NS
Q_T1, Q_T2, Q_TE = Q_T0 + 100_000, Q_T0 + 200_000, Q_T0 + 40_000


def queue_rows(L, mirror=False, shift=0, twin=True):
    """(rows of the first batch, rows of the second)"""
    A, D, E = (3, 2), (10, 5), (17, 9)
    b1 = [(2, 1, 0, 1)]                                                                    # a zero stamp
    b1 += [(A[0], A[1], Q_T0 + 1000 * i, i & 1) for i in range(L + 2)]                     # more than L on a pixel in one batch
    b1 += [(D[0], D[1], Q_T0 + 20_000 + 1000 * i, 1) for i in range(L)]                    # L now, two more in the second batch
    b1 += [(E[0], E[1], Q_T0 + 100, 1)] + [(E[0], E[1], Q_T0 + 50_000 + 1000 * i, 0) for i in range(L + 1)]   # an old one hidden by L + 1 newer
    b1 += [(19, 11, Q_T0 + 500, 1), (0, 0, Q_T0 + 600, 0), (19, 0, Q_T0 + 700, 1), (0, 11, Q_T0 + 800, 0)]    # the corners: tiles over both edges
    b1 += [(20, 5, Q_T0 + 900, 1), (5, 12, Q_T0 + 901, 1), (20, 12, Q_T0 + 902, 1)]        # outside the sensor
    b1 += [(7, 7, Q_T0 + 30_000, 1)] + ([(7, 7, Q_T0 + 30_000, 0)] if twin else [])        # equal stamps on one pixel (with polarity: eqpol_*)
    b1 += [(12, 3, Q_T1 - 1, 1), (13, 3, Q_T1, 1), (14, 3, Q_T1 + 1, 1)]                   # around the first render time
    b1 += [(13, 3, Q_T0 + 5000, 0)]                                                        # ... the event at T above an older one, which shows
    b2 = [(D[0], D[1], Q_T0 + 110_000, 0), (D[0], D[1], Q_T0 + 111_000, 1)][:min(2, L)] + [(4, 10, Q_T0 + 120_000, 1)]
    if mirror:
        f = lambda r: (19 - r[0] if r[0] < 20 else r[0], r[1], r[2] + shift if r[2] else 0, r[3])
        b1, b2 = [f(r) for r in b1], [f(r) for r in b2]
    return b1, b2


def _queue(L, k=0, ip=1):
    """Per-pixel queues of L events on 20 x 12: the batches of queue_rows, rendered at T1 (behind the first batch), at T2 (behind
    the second), back at TE (the old event of the hidden pixel has left its queue: the reference renders the pixel empty), at T1
    again and at T1 + 1 (the event at T1 appears).  The right camera: the same, mirrored and 7 ns later."""
    script = []
    for cam in (0, 1):
        b1, b2 = queue_rows(L, mirror=cam == 1, shift=7, twin=bool(ip))
        script += [("push", cam, events(b1)), ("render", cam, Q_T1 + (7 if cam else 0)), ("push", cam, events(b2))]
        script += [("render", cam, t + (7 if cam else 0)) for t in (Q_T2, Q_TE, Q_T1, Q_T1 + 1)]
    tags = [f"q:L{L}", "q:more_than_L_one_batch", "q:more_than_L_across_batches", "q:hidden_older", "q:backwards", "q:stamp0", "q:off_sensor",
            "q:tiles_over_edges", "q:event_at_T"] + (["q:equal_stamps"] if ip else []) + (["q:event_at_T_over_older"] if L > 1 else [])
    return _case("q20", script, 30.0, ip, k, L=L, tags=tags, group="queue", pinned=ip == 1 and k == 0, doc=_queue.__doc__)


def overflow_rows():
    """1030 events on the 4 x 4 in-image pixels of the tile at (16, 8), then 1088 on the same 16 pixel positions of the tile at
    (0, 0): both lists overflow in one batch, and every entry of the overflow list carries a pixel position that exists in
    every tile"""
    S = [(x, y) for y in range(4) for x in range(4)]
    rows = [(16 + S[i % 16][0], 8 + S[i % 16][1], Q_T0 + i, i & 1) for i in range(1030)]
    rows += [(S[i % 16][0], S[i % 16][1], Q_T0 + 2000 + i, i & 1) for i in range(1088)]
    return rows


def _overflow(L):
    """overflow_rows in one batch on the left camera, rendered behind it and back between the two tiles' events; the right
    camera receives the second tile's events only (its list overflows alone)."""
    rows = overflow_rows()
    script = [("push", 0, events(rows)), ("render", 0, Q_T0 + 10_000), ("render", 0, Q_T0 + 1500),
              ("push", 1, events(rows[1030:])), ("render", 1, Q_T0 + 10_000)]
    return _case("q20", script, 30.0, 1, 0, L=L, tags=["q:overflow", "q:overflow_two_tiles", "q:backwards"], group="queue", pinned=True, doc=_overflow.__doc__)


def _equal_stamps_polarity(L):
    """Two events of one pixel with the same stamp and opposite polarity under ignore_polarity = 0, in both arrival orders.  The
    reference keeps the later arrival; the device documents key order (kernels_ts.hip: the key is stamp << 1 | polarity, so the
    positive event wins in either order).  Held to that rule, not to the oracle: `expect` is the script without the negative
    twins."""
    rows = [(3, 3, Q_T0 + 1000, 1), (3, 3, Q_T0 + 1000, 0), (9, 6, Q_T0 + 2000, 0), (9, 6, Q_T0 + 2000, 1), (15, 9, Q_T0 + 2500, 0)]
    kept = [r for r in rows if not (r[3] == 0 and r[:2] in ((3, 3), (9, 6)))]
    c = _case("q20", [("push", 0, events(rows))] + both(Q_T0 + 5000), 30.0, 0, 0, L=L, tags=["q:equal_stamps_polarity"], group="queue", oracle=False,
              doc=_equal_stamps_polarity.__doc__)
    c["expect"] = [("push", 0, events(kept))] + both(Q_T0 + 5000)
    return c


# ---- FORWARD ----------------------------------------------------------------------------------------------------------------------
def _forward(ip, k):
    """The look-up table of _lut_forward under a texture: the sources of (20, 8) carry FWD_SEQ, the sources of the negative sum
    polarity 0; the destinations of both receive nothing else."""
    W, H, T = 33, 17, T_TEX
    ctrl = {(sx, 5) for sx in FWD_MANY} | {(sx, 9) for sx in FWD_NEG}
    quiet = {(20, 8), (25, 10), (26, 10), (25, 11), (26, 11)}
    rows = texture_events(W, H, T, 77, skip=ctrl | quiet)
    rows += [(sx, 5, T - dt_of(s[1], 30.0), s[0]) for sx, s in zip(FWD_MANY, FWD_SEQ) if s is not None]
    rows += [(sx, 9, T - dt_of(0.15 + 0.1 * i, 30.0), 0) for i, sx in enumerate(FWD_NEG)]
    script = [("push", 0, events(rows)), ("push", 1, events(texture_events(W, H, T, 78))), ("forward", 0, T), ("forward", 1, T)]
    tags = ["fwd:integer", "fwd:outside", "fwd:many_sources", "fwd:passes_1_early", "fwd:nan_between", f"fwd:k{k}"]
    tags += ["fwd:negative_sum", "fwd:clamp_order_decides"] if not ip else []
    return _case("g33", script, 30.0, ip, k, tags=tags, group="forward", pinned=k == 0, doc=_forward.__doc__)


# ---- gaussian ---------------------------------------------------------------------------------------------------------------------
def gauss_images(W, H):
    a, b, c = (np.zeros((H, W), np.uint8) for _ in range(3))
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2)):
        a[y, x] = 255
    for x, y in ((2, 2), (W - 3, 2), (2, H - 3), (W - 3, H - 3), (W // 2, 2), (W // 2, H - 3), (2, H // 2), (W - 3, H // 2)):
        b[y, x] = 255
    c[...] = 255
    return a, b, c


def _gauss(key):
    """track_set_current(image, 5) and track_images(): neg = 255 - GaussianBlur(5 x 5, BORDER_REFLECT_101) of impulses of 255 at
    the corners and on the borders, of impulses two pixels in from them, and of an all-255 image."""
    r = rig(key)
    return _case(key, [("gauss", img) for img in gauss_images(r.width, r.height)], tags=["gauss:corners", "gauss:two_in", "gauss:all255"], group="gauss",
                 doc=_gauss.__doc__)


# ---- the list ---------------------------------------------------------------------------------------------------------------------
DECAYS = (1, 30, 10000)


def _builders():
    b = {}
    for d in DECAYS:
        for ip in (1, 0):
            b[f"sweep_d{d}_ip{ip}"] = functools.partial(_sweep, d, ip)
    for d in (30, 10000):
        for ip in (1, 0):
            b[f"edges_d{d}_ip{ip}"] = functools.partial(_decay_edges, d, ip)
    for ip in (1, 0):
        b[f"epoch_ip{ip}"] = functools.partial(_sweep, 30, ip, T_EPOCH, 4)
    b["median_k0"] = functools.partial(_median, 0, ("above", "equal"))
    for k in (1, 2, 3):
        b[f"median_k{k}_a"] = functools.partial(_median, k, ("lone", "below"))
        b[f"median_k{k}_b"] = functools.partial(_median, k, ("above", "equal"))
    for k in (0, 1, 2, 3):
        b[f"s70_k{k}"] = functools.partial(_textured, "s70", k, 1, S70_TAGS[k] + REMAP_TAGS + ("stage:one_pixel",), "staging")
        b[f"g33_k{k}"] = functools.partial(_textured, "g33", k, 1, ("remap:mirrored", "remap:transposed", "tile:cols1", "tile:rows1"), "geometry")
    b["s70_k1_pol"] = functools.partial(_textured, "s70", 1, 0, S70_TAGS[1] + REMAP_TAGS, "staging")
    b["g33_k1_pol"] = functools.partial(_textured, "g33", 1, 0, ("remap:mirrored", "remap:transposed"), "geometry")
    for k in (0, 1, 2):
        b[f"mag128_k{k}"] = functools.partial(_textured, "mag128", k, 1, ("stage:direct_all_inside", "stage:one_pixel"), "staging")
    for k in (0, 1, 2, 3):
        b[f"wide_k{k}"] = functools.partial(_textured, "wide", k, 1, ("stage:wide", "tile:rows8"), "staging")
    b["id128_k1"] = functools.partial(_textured, "id128", 1, 1, ("remap:identity",), "geometry")
    for L in (1, 3, 20, 32):
        b[f"queue_L{L}"] = functools.partial(_queue, L)
    b["queue_L3_k1"] = functools.partial(_queue, 3, 1)
    b["queue_L3_pol"] = functools.partial(_queue, 3, 0, 0)
    b["queue_over_L3"] = functools.partial(_overflow, 3)
    b["queue_over_L20"] = functools.partial(_overflow, 20)
    b["eqpol_L0"] = functools.partial(_equal_stamps_polarity, 0)
    b["eqpol_L3"] = functools.partial(_equal_stamps_polarity, 3)
    for ip in (1, 0):
        for k in (0, 1):
            b[f"forward_ip{ip}_k{k}"] = functools.partial(_forward, ip, k)
    b["gauss_33x17"] = functools.partial(_gauss, "g33")
    b["gauss_70x40"] = functools.partial(_gauss, "s70")
    return b


_BUILDERS = _builders()
NAMES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = dict(_BUILDERS[name]())
    c["name"] = name
    return c


GROUPS = {g: [n for n in NAMES if case(n)["group"] == g] for g in ("decay", "median", "staging", "geometry", "queue", "forward", "gauss")}
PINNED = [n for n in NAMES if case(n)["pinned"]]
DIRECT_TWICE = GROUPS["staging"] + GROUPS["geometry"]      # run once more with every tile on the direct path


def case_params(c):
    """ParamsStruct of a case: mvstereo_upenn, a small event ring, the case's Time-Surface parameters"""
    p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], c["rig"], event_ring_capacity=1 << 14, decay_ms=c["decay_ms"],
                              ignore_polarity=c["ignore_polarity"], median_blur_kernel_size=c["median_k"], max_event_queue_len=c["L"])
    return p


def handle_key(c):
    return (c["key"], c["L"])


def input_digest(c):
    """sha256 over what a case feeds the raster: maps, look-up tables, the script, the parameters"""
    h = hashlib.sha256()
    for cam in cams(c):
        for a in (cam.map_x, cam.map_y, cam.rect_lut):
            h.update(np.ascontiguousarray(a).tobytes())
    for op in c["script"]:
        h.update(op[0].encode())
        for a in op[1:]:
            h.update(np.ascontiguousarray(a).tobytes() if isinstance(a, np.ndarray) else str(int(a)).encode())
    h.update(np.array([c["decay_ms"], c["ignore_polarity"], c["median_k"], c["L"], c["W"], c["H"]], np.float64).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# ---- running a script -------------------------------------------------------------------------------------------------------------
def run_script(c, script, push, render, forward, gauss):
    """the outputs of a script's render / forward / gauss steps, in order, as dicts(op, cam, T, img, ...)"""
    out = []
    for op in script:
        if op[0] == "push":
            push(op[1], op[2])
        elif op[0] == "render":
            out.append(dict(render(op[1], op[2]), op="render", cam=op[1], T=op[2]))
        elif op[0] == "forward":
            out.append(dict(forward(op[1], op[2]), op="forward", cam=op[1], T=op[2]))
        else:
            out.append(dict(gauss(op[1]), op="gauss", cam=0, T=0))
    return out


@functools.lru_cache(maxsize=None)
def restated(name, expect=False):
    """the case under tests/ts_restated.py: per output img (and pre: the image behind convertTo; f64: FORWARD's image before it)"""
    c = case(name)
    nodes = [TR.Node(c["W"], c["H"], c["L"] or 20) for _ in (0, 1)]
    d, ip, k = c["decay_ms"], c["ignore_polarity"], c["median_k"]

    def render(cam, T):
        img, pre = nodes[cam].render(T, d, ip, k, cams(c)[cam].map_x, cams(c)[cam].map_y)
        return dict(img=img, pre=pre)

    def forward(cam, T):
        img, f64 = nodes[cam].render_forward(T, d, ip, k, cams(c)[cam].rect_lut)
        return dict(img=img, f64=f64)

    return run_script(c, c["expect"] if expect else c["script"], lambda cam, ev: nodes[cam].push(ev), render, forward, lambda img: dict(img=TR.gaussian5_neg(img)))


@functools.lru_cache(maxsize=None)
def oracle(name, expect=False):
    """the case under oracle.OracleTS (queues of L, or of the reference's 20 where the device keeps one stamp per pixel)"""
    from oracle import oracle as O
    c = case(name)
    ots = [O.OracleTS(c["W"], c["H"], queue_len=c["L"] or 20) for _ in (0, 1)]
    d, ip, k = c["decay_ms"], c["ignore_polarity"], c["median_k"]

    def render(cam, T):
        img, pre = ots[cam].render(T, decay_ms=d, ignore_polarity=ip, median_k=k, map_x=cams(c)[cam].map_x, map_y=cams(c)[cam].map_y, want_prefilter=True)
        return dict(img=img, pre=pre)

    def forward(cam, T):
        img, f64 = ots[cam].render_forward(T, cams(c)[cam].rect_lut, decay_ms=d, ignore_polarity=bool(ip), median_k=k, want_f64=True)
        return dict(img=img, f64=f64)

    return run_script(c, c["expect"] if expect else c["script"], lambda cam, ev: ots[cam].push(ev), render, forward,
                      lambda img: dict(img=(255 - O.gaussian5(img).astype(np.int64)).astype(np.uint8)))


# ---- what a case reaches ----------------------------------------------------------------------------------------------------------
def pushed(c, cam, upto=None):
    """the events pushed to a camera by the first `upto` steps of the script"""
    evs = [op[2] for op in c["script"][:upto] if op[0] == "push" and op[1] == cam]
    return np.concatenate(evs) if evs else np.zeros(0, abi.EVENT_DTYPE)


def found_events(c, cam, T):
    """(te, polarity, y, x) of the event every raw pixel shows at T, by the restated queues"""
    node = TR.Node(c["W"], c["H"], c["L"] or 20)
    node.push(pushed(c, cam))
    rows = []
    for y in range(c["H"]):
        for x in range(c["W"]):
            hit = node.most_recent_before(x, y, T)
            if hit is not None and hit[0] > 0:
                rows.append((hit[0], hit[1], y, x))
    a = np.array(rows, np.int64).reshape(-1, 4)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3]


@functools.lru_cache(maxsize=None)
def decay_stats(name):
    """per camera the decay_tags of a decay case's pixels"""
    c = case(name)
    T = [op[2] for op in c["script"] if op[0] == "render"][0]
    out = []
    for cam in (0, 1):
        te, pol, y, x = found_events(c, cam, T)
        s = TR.decay_tags(te, pol, T, c["decay_ms"], c["ignore_polarity"])
        s.update(te=te, pol=pol, y=y, x=x, T=T)
        out.append(s)
    return out


def _remap_tags(c, cam_i):
    cam = cams(c)[cam_i]
    W, H = c["W"], c["H"]
    f32 = np.float32
    tags = set()
    for m, (lo_name, hi_name), top in ((cam.map_x, ("remap:x_in(-1,0)", "remap:x_in(W-1,W)"), W), (cam.map_y, ("remap:y_in(-1,0)", "remap:y_in(H-1,H)"), H)):
        v = m * f32(32)
        s = np.rint(v)
        tie = np.abs(v - np.floor(v) - f32(0.5)) == 0
        if (tie & (s < v)).any():
            tags.add("remap:tie_down")
        if (tie & (s > v)).any():
            tags.add("remap:tie_up")
        if ((m > -1) & (m < 0)).any():
            tags.add(lo_name)
        if ((m > top - 1) & (m < top)).any():
            tags.add(hi_name)
        if (m == f32(-1e6)).any():
            tags.add("remap:marker")
    sx, sy = np.rint(cam.map_x * f32(32)).astype(np.int64), np.rint(cam.map_y * f32(32)).astype(np.int64)
    if (((sx >> 5) + 1 == W) & ((sx & 31) == 0)).any():
        tags.add("remap:fx0_last_col")
    if (((sy >> 5) + 1 == H) & ((sy & 31) == 0)).any():
        tags.add("remap:fy0_last_row")
    x, y = _identity(W, H)
    for name, (mx, my) in (("identity", (x, y)), ("mirrored", _map_mirror(W, H)), ("transposed", _map_transposed(W, H))):
        if np.array_equal(cam.map_x, mx.astype(f32)) and np.array_equal(cam.map_y, my.astype(f32)):
            tags.add(f"remap:{name}")
    return tags


def _tile_tags(c, cam_i):
    cam = cams(c)[cam_i]
    k = c["median_k"]
    tags = set()
    for t in TR.tile_boxes(cam.map_x, cam.map_y, c["W"], c["H"], k).values():
        tags |= {f"tile:rows{t['rows']}", f"tile:cols{t['cols']}"}
        if t["empty"]:
            tags.add("tile:empty")
            continue
        if t["inside"] < t["pixels"]:
            tags.add("tile:partial")
        v = t["rw"] * t["rh"]
        if TR.STAGE_CAP - t["rw"] < v <= TR.STAGE_CAP:
            tags.add(f"stage:k{k}:at_cap")
        if v == JUST_OVER.get(k):
            tags.add(f"stage:k{k}:just_over")
        if t["rw"] == 1 + 2 * k and t["rh"] == 1 + 2 * k:
            tags.add("stage:one_pixel")
        if t["rw"] > 256 and t["staged"]:
            tags.add("stage:wide")
        if not t["staged"] and t["inside"] == t["pixels"]:
            tags.add("stage:direct_all_inside")
        tags.add("stage:staged" if t["staged"] else "stage:direct")
    return tags


def _median_tags(c, out):
    k = c["median_k"]
    if k == 0:
        return {"med:k0"}
    n = (2 * k + 1) ** 2
    tags = set()
    for o in out:
        kind = c["kinds"][o["cam"]]
        for loc, (x, y) in MED_LOCS.items():
            s = TR.window(o["pre"], x, y, k)
            lit = int((s == 255).sum())
            ok = dict(lone=lit == window_weights(c["W"], c["H"], x, y, k)[(x, y)] and int((s > 0).sum()) == lit and o["img"][y, x] == 0 and o["pre"][y, x] == 255,
                      below=lit == n // 2 and int((s > 0).sum()) == lit and o["img"][y, x] == 0,
                      above=lit == n // 2 + 1 and int((s > 0).sum()) == lit and o["img"][y, x] == 255,
                      equal=s[n // 2 - 1] == s[n // 2] == s[n // 2 + 1] == 200 and s[0] == 0 and s[-1] == 255 and o["img"][y, x] == 200)[kind]
            if ok:
                tags.add(f"med:k{k}:{kind}:{loc}")
    return tags


def _queue_tags(c, out):
    L, W, H = c["L"] or 20, c["W"], c["H"]      # (one stamp per pixel: held to the reference's queues of 20)
    tags = {f"q:L{c['L']}"}
    T_seen = {0: [], 1: []}
    batch = {0: [], 1: []}
    node = [TR.Node(W, H, L), TR.Node(W, H, L)]
    ever = [TR.Node(W, H, 1 << 30), TR.Node(W, H, 1 << 30)]     # queues that never lose an event
    for op in c["script"]:
        cam = op[1]
        if op[0] == "push":
            batch[cam].append(op[2])
            node[cam].push(op[2])
            ever[cam].push(op[2])
            ev = op[2]
            if len(ev) and TR.stamp(ev[0]) == 0:
                tags.add("q:stamp0")
            if ((ev["x"] >= W) | (ev["y"] >= H)).any():
                tags.add("q:off_sensor")
            if ((ev["x"] == W - 1) & (ev["y"] == H - 1)).any() and (W % TR.QTILE and H % TR.QTILE):
                tags.add("q:tiles_over_edges")
            continue
        T = op[2]
        if batch[cam]:       # a batch: what was pushed since the camera's last render
            ev = np.concatenate(batch[cam])
            batch[cam] = []
            per_px = {}
            for e in ev:
                if e["x"] < W and e["y"] < H:
                    per_px[(int(e["x"]), int(e["y"]))] = per_px.get((int(e["x"]), int(e["y"])), 0) + 1
            if max(per_px.values()) > L:
                tags.add("q:more_than_L_one_batch")
            over = [t for t, n in TR.queue_batches(ev, W, H).items() if n > TR.QTILE_CAP]
            if over:
                tags.add("q:overflow")
            if len(over) >= 2:
                tags.add("q:overflow_two_tiles")
        if T_seen[cam] and T < max(T_seen[cam]):
            tags.add("q:backwards")
        T_seen[cam].append(T)
        for i, qe in enumerate(ever[cam].q):
            if any(t == T for t, _ in qe):
                tags.add("q:event_at_T")
                if any(t == T for t, _ in node[cam].q[i]) and any(t < T for t, _ in node[cam].q[i]):
                    tags.add("q:event_at_T_over_older")
            if len(qe) > L:
                x, y = i % W, i // W
                lost, kept = ever[cam].most_recent_before(x, y, T), node[cam].most_recent_before(x, y, T)
                if lost is not None and kept is None:
                    tags.add("q:hidden_older")
            st = [t for t, _ in qe]
            if len(st) != len(set(st)):
                pols = {t: set() for t in st}
                for t, p in qe:
                    pols[t].add(p)
                tags.add("q:equal_stamps_polarity" if any(len(v) == 2 for v in pols.values()) and not c["ignore_polarity"] else "q:equal_stamps")
    # across batches: a pixel that received more than L events, no single batch bringing more than L of them
    for cam in (0, 1):
        pushes = [op[2] for op in c["script"] if op[0] == "push" and op[1] == cam]
        if len(pushes) >= 2:
            cnt = [{} for _ in pushes]
            for d, ev in zip(cnt, pushes):
                for e in ev:
                    d[(int(e["x"]), int(e["y"]))] = d.get((int(e["x"]), int(e["y"])), 0) + 1
            for px in cnt[0]:
                if px[0] < W and px[1] < H and all(d.get(px, 0) <= L for d in cnt) and sum(d.get(px, 0) for d in cnt) > L:
                    tags.add("q:more_than_L_across_batches")
    return tags


def _forward_tags(c, out):
    W, H = c["W"], c["H"]
    lut = cams(c)[0].rect_lut
    tags = {f"fwd:k{c['median_k']}"}
    u, v = lut[..., 0].astype(np.float64), lut[..., 1].astype(np.float64)
    inside = (u >= 0) & (v >= 0) & (np.floor(u) + 1 < W) & (np.floor(v) + 1 < H)
    if (inside & (u == np.floor(u)) & (v == np.floor(v))).any():
        tags.add("fwd:integer")
    if (~inside).any() and (u < 0).any() and (np.floor(u) + 1 >= W).any() and (np.floor(v) + 1 >= H).any() and (lut == np.float32(-1e6)).any():
        tags.add("fwd:outside")
    T = [op[2] for op in c["script"] if op[0] == "forward"][0]
    node = TR.Node(W, H, 20)
    node.push(pushed(c, 0))
    e, _ = node.exp_plane(T, c["decay_ms"], c["ignore_polarity"])
    for dst in {(int(np.floor(u[y, x])), int(np.floor(v[y, x]))) for y in range(H) for x in range(W) if inside[y, x]}:
        src = [(y, x) for y in range(H) for x in range(W) if inside[y, x] and (int(np.floor(u[y, x])), int(np.floor(v[y, x]))) == dst]
        if len(src) < 4:
            continue
        w00 = [(1 - (u[s] - np.floor(u[s]))) * (1 - (v[s] - np.floor(v[s]))) * e[s] for s in src]
        acc, clamped_at, plain = 0.0, None, 0.0
        for i, w in enumerate(w00):
            if w != w:
                if 0 < i < len(w00) - 1 and not np.isnan(w00[i - 1]) and not np.isnan(w00[i + 1]):
                    tags.add("fwd:nan_between")
                continue
            acc, plain = acc + w, plain + w
            if acc > 1:
                acc, clamped_at = 1.0, i if clamped_at is None else clamped_at
        if len(src) >= 8:
            tags.add("fwd:many_sources")
            if clamped_at is not None and clamped_at < len(w00) - 1:
                tags.add("fwd:passes_1_early")
            if min(plain, 1.0) != acc:
                tags.add("fwd:clamp_order_decides")
        if acc < 0:
            tags.add("fwd:negative_sum")
    return tags


@functools.lru_cache(maxsize=None)
def observe(name):
    """the tags a case reaches"""
    c = case(name)
    g = c["group"]
    tags = set()
    if g == "decay":
        st = decay_stats(name)
        near, away = st
        if len(near["g"]) and (near["dist"] <= 3.5 * 255.0 / (c["decay_ms"] * 1e6)).all():      # within 3 ns (+ the rounding of the crossing to a whole ns)
            tags.add("dec:cross")
        if int(((away["dist"] > 5e-4) & (away["dist"] < 1e-3)).sum()) >= 10:
            tags.add("dec:away")
        T = near["T"]
        ev = pushed(c, 0)
        stamps = np.array([TR.stamp(e) for e in ev])
        tags |= {t for t, on in (("dec:stamp0", (stamps == 0).any()), ("dec:T-1", (stamps == T - 1).any()), ("dec:T", (stamps == T).any()),
                                 ("dec:T+1", (stamps == T + 1).any()), ("dec:empty", len(near["g"]) < c["W"] * c["H"]),
                                 ("dec:dt>=2^24", ((near["dt_ns"] >= 2 ** 24) & (near["dt_ns"].astype(np.float32).astype(np.uint64) != near["dt_ns"])).any()),
                                 ("dec:dt>=2^32", (near["dt_ns"] >= 2 ** 32).any()), ("dec:e32_zero", near["e32_zero"].any()),
                                 ("dec:borrow", len(near["te"]) and T > 15 * 10 ** 17 and (near["te"] % NS > T % NS).all())) if on}
        lo, hi = (0.5, 0.5) if c["ignore_polarity"] else (127.5 - 1.0, 127.5 + 1.0)
        if any(abs(v - b) < 1e-3 for v in near["g"] for b in (lo, hi)):
            tags.add("dec:boundary01")
        return tags
    out = restated(name)
    if g == "median":
        return _median_tags(c, out)
    if g in ("staging", "geometry"):
        for cam in (0, 1):
            tags |= _remap_tags(c, cam) | _tile_tags(c, cam)
        return tags
    if g == "queue":
        return _queue_tags(c, out)
    if g == "forward":
        return _forward_tags(c, out)
    imgs = [op[1] for op in c["script"]]
    W, H = c["W"], c["H"]
    if any(im[0, 0] == 255 and im[H - 1, W - 1] == 255 and im[0, W // 2] == 255 and im.sum() == 8 * 255 for im in imgs):
        tags.add("gauss:corners")
    if any(im[2, 2] == 255 and im[H - 3, W - 3] == 255 and im.sum() == 8 * 255 for im in imgs):
        tags.add("gauss:two_in")
    if any((im == 255).all() for im in imgs):
        tags.add("gauss:all255")
    return tags


# The targets the case list has to reach (tests/test_ts_cases.py asserts that it does), as tags of observe().
REQUIRED = (
    "dec:cross", "dec:away", "dec:empty", "dec:stamp0", "dec:T-1", "dec:T", "dec:T+1", "dec:dt>=2^24", "dec:dt>=2^32", "dec:e32_zero", "dec:boundary01",
    "dec:borrow", "med:k0",
) + tuple(f"med:k{k}:{kind}:{loc}" for k in (1, 2, 3) for kind in MED_KINDS for loc in MED_LOCS) + (
    "remap:identity", "remap:tie_down", "remap:tie_up", "remap:fx0_last_col", "remap:fy0_last_row", "remap:x_in(-1,0)", "remap:x_in(W-1,W)",
    "remap:y_in(-1,0)", "remap:marker", "remap:mirrored", "remap:transposed", "tile:empty", "tile:partial",
    "tile:rows8", "tile:rows1", "tile:cols1", "tile:cols6", "tile:rows16", "tile:cols32",
    "stage:one_pixel", "stage:wide", "stage:direct_all_inside", "stage:staged", "stage:direct",
) + tuple(f"stage:k{k}:{w}" for k in (0, 1, 2) for w in ("at_cap", "just_over")) + tuple(f"q:L{L}" for L in (1, 3, 20, 32)) + (
    "q:more_than_L_one_batch", "q:more_than_L_across_batches", "q:hidden_older", "q:backwards", "q:stamp0", "q:off_sensor", "q:tiles_over_edges",
    "q:overflow", "q:overflow_two_tiles", "q:equal_stamps", "q:equal_stamps_polarity", "q:event_at_T", "q:event_at_T_over_older",
    "fwd:integer", "fwd:outside", "fwd:many_sources", "fwd:passes_1_early", "fwd:negative_sum", "fwd:nan_between", "fwd:clamp_order_decides", "fwd:k0", "fwd:k1",
    "gauss:corners", "gauss:two_in", "gauss:all255",
)
# ... and per rig: the one-pixel box, the wide box and the box that never fits under each of k = 0, 1, 2
REQUIRED_PER_K = ("stage:one_pixel", "stage:wide", "stage:direct_all_inside")
# Float-only disagreements a crossing sweep has to hold, and pixels just outside the band (the issue's thresholds, from a numpy
# float32 simulation of the short form: 447 / 629 at 30 ms, 878 / 879 at 10000 ms, 13 / 63 at 1 ms)
MIN_FLOAT_WRONG = {1: 10, 30: 200, 10000: 200}
MIN_JUST_OUTSIDE = 200
