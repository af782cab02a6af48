"""Crafted problems of the tracker's point evaluation (tests/test_track_cases.py on the CPU, tests/test_gpu_track_cases.py on the
device): small images, about 400 named reference points whose projections sit at the switch points of reprojection, interpolation,
mask, Jacobian and Huber weight, and a 2049-point problem for the wide sums.  Built once per (rig variant, image size), read-only.

Rig variants (copies of calib.ideal_rig(W, H, 120, 0.1), made as the existing tests copy rig.left):
  plain    the ideal rig as it is (an all-255 mask)
  masked   rig.left.rect_mask overwritten with blocks of 0, 124, 125, 126 and 255
  skewed   the left P overwritten ON THE COPY with non-zero P[0,1], P[1,0], P[0,3], P[1,3]: rig_from_intrinsics derives its maps
           from K / D / R and would accept such a P, but the tracker reads only P, W, H and the mask, so the overwrite is the
           route taken (intr_left["P"] is overwritten too: that is what the reference's calibration file is written from).
           Targets are placed by inverting this P in f64.

Exact hits.  Points travel as f32.  Under the identity motion and a P with zero skew a point (X, Y, Z) = ((x - cx) s, (y - cy) s,
f s) with s = 2^-6 projects to exactly (x, y) whenever x - cx and y - cy have few bits: every product is exact.  The bounds kinds
are built this way and tests/test_track_cases.py asserts the value per name; -0.0 comes from Z = -f s (hm[0] = +0, hm[2] < 0).
Under the moved pose and under the skewed P the same names are placed in f64 and rounded to f32: near their target, not on it.
Dropped by name:
  huge_1e300  |x| of 1e300 needs |z| near 1e-298 in the reference frame; the input is f32 (smallest subnormal 1.4e-45, largest
              finite 3.4e38), so the largest reachable |x| is about 1e85.  The huge_* points use that: far beyond any int.
A correction to the plan's wording: ux + 1 >= W fails at ux == W-1, i.e. at x == W-1 exactly (x > W-1 is rejected before), not for
every x above W-2; x just above W-2 is valid, interpolates and reads the last column.  The names keep both values."""
import copy
import hashlib

import numpy as np

import reproj_cases as RC
import reproj_restated as RR
import track_restated as TR
from esvo_amd import calib

FOCAL = 120.0
SIZES = ((96, 64), (95, 63))
VARIANTS = ("plain", "masked", "skewed")
MOTIONS = RC.MOTIONS
I4 = np.eye(4)
THRESHOLDS = (50.0, float(np.nextafter(50.0, 0.0)), 0.0, 1e300)
NORMS = (("l2", False, 50.0),) + tuple((f"huber{i}", True, thr) for i, thr in enumerate(THRESHOLDS))
COUNTS = (0, 1, 255, 256, 257, 511, 512, 513)
LONG_N = 2049
LONG_N_POINTS = (1023, 1024, 1025, 1279, 1280, 1281, 2047, 2048, 2049)
LONG_BATCHES = (0, 1024, 1025)
S = 2.0 ** -6
SKEW = dict(P01=0.75, P10=-0.5, P03=2.5, P13=-1.75)

# image regions (rows, cols), the same at both sizes
FLAT50 = (slice(4, 20), slice(4, 24))        # Time Surface 205: neg == 50
FLAT0 = (slice(4, 20), slice(28, 48))        # Time Surface 255: neg == 0
CHECKER = (slice(24, 40), slice(4, 24))      # 0 / 255 in 4 x 4 squares: Sobel reaches +-1020
RAMP = (slice(24, 40), slice(28, 60))        # neg = 8 + 3 (col - 28): 50 at col 42
MASK_ROWS = slice(44, 60)
MASK_BLOCKS = ((0, slice(4, 12)), (124, slice(12, 20)), (125, slice(20, 28)), (126, slice(28, 36)), (255, slice(36, 44)))

# what the reference (RegProblemLM compiled from source, oracle/ref_harness_track.cpp) cannot be asked, per point and motion
UNPINNED_KINDS = {
    "nonfinite": "a NaN projection passes isValidPatch's comparisons and indexes the mask matrix with (int)NaN: undefined; the "
                 "device and the oracle reject every non-finite projection first",
    "border_gradient": "a valid point at x == W-1 or y == H-1: patchInterpolation fails and df reads gx(0, 0) of a matrix it never "
                       "set: undefined (the device and the oracle define the gradient as 0)",
    "mask_byte": "the harness injects the mask through the stand-in remap, which hands the reference 1.0 for every non-zero byte and "
                 "thresholds that to 255: bytes other than 0 / 255 (124, 125, 126) cannot be expressed.  Dropped: every point that projects "
                 "onto such a byte or within PIN_MARGIN pixels of one (the pin also evaluates at PIN_X, which moves projections)",
}


def time_surface(W, H):
    ts = np.random.default_rng(1000 + W).integers(0, 256, (H, W)).astype(np.uint8)
    ts[FLAT50] = 205
    ts[FLAT0] = 255
    yy, xx = np.mgrid[24:40, 4:24]
    ts[CHECKER] = np.where(((yy - 24) // 4 + (xx - 4) // 4) % 2 == 0, 0, 255)
    ts[RAMP] = (255 - (8 + 3 * (np.arange(28, 60) - 28))).astype(np.uint8)[None, :]
    return ts


def crafted_mask(W, H):
    m = np.full((H, W), 255, np.uint8)
    for v, cols in MASK_BLOCKS:
        m[MASK_ROWS, cols] = v
    return m


def rig_variant(variant, W, H):
    base = calib.ideal_rig(W, H, FOCAL, 0.1)
    rig = copy.copy(base)
    rig.left = copy.copy(base.left)
    if variant == "masked":
        rig.left.rect_mask = crafted_mask(W, H)
    elif variant == "skewed":
        P = np.array(base.left.P, np.float64).reshape(3, 4).copy()
        P[0, 1], P[1, 0], P[0, 3], P[1, 3] = SKEW["P01"], SKEW["P10"], SKEW["P03"], SKEW["P13"]
        rig.left.P = np.ascontiguousarray(P.reshape(12))
        rig.intr_left = dict(base.intr_left, P=P.copy())
    else:
        assert variant == "plain"
    return rig


def _f32_next(v, up):
    v = np.float32(v)
    return float(np.nextafter(v, np.float32(np.inf if up else -np.inf)))


def _exact(x, y, W, H, nx=0, ny=0, behind=False, S=S):
    """the f32 point that the identity motion and the ideal P project to exactly (x, y); nx / ny = +-1: its X / Y moved to the
    neighbouring f32 value, so that x / y is the nearest coordinate above / below that the input can produce"""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    sgn = -1.0 if behind else 1.0
    X, Y, Z = sgn * (x - cx) * S, sgn * (y - cy) * S, sgn * FOCAL * S
    assert float(np.float32(X)) == X and float(np.float32(Y)) == Y
    if nx:
        X = _f32_next(X, (nx > 0) != behind)
    if ny:
        Y = _f32_next(Y, (ny > 0) != behind)
    return (X, Y, Z)


def _bounds_targets(W, H):
    """[(name, (x, y), exact-builder kwargs)]: the closed bounds of isValidPatch and the last column / row of the interpolation"""
    xm, ym = 66.5, 42.25                                        # an interior coordinate for the other axis (noise)
    out = []
    for ax, lim, n, mid in (("x", "W", W, ym), ("y", "H", H, xm)):
        for tag, v, kw in (("=-0", 0.0, dict(behind=True)), ("=+0", 0.0, {}), ("<0", 0.0, dict(step=-1)), (f"={lim}-2", n - 2.0, {}),
                           (f">{lim}-2", n - 2.0, dict(step=1)), (f"={lim}-1", n - 1.0, {}), (f">{lim}-1", n - 1.0, dict(step=1))):
            kw = dict(kw)
            step = kw.pop("step", 0)
            xy = (v, mid) if ax == "x" else (mid, v)
            if step:
                kw["nx" if ax == "x" else "ny"] = step
            out.append((ax + tag, xy, kw))
    for name, xy in (("corner00", (0.0, 0.0)), ("cornerW0", (W - 1.0, 0.0)), ("corner0H", (0.0, H - 1.0)), ("cornerWH", (W - 1.0, H - 1.0))):
        out.append((name, xy, {}))
    return out


def _interior_targets(rng):
    """[(kind, name, (x, y, z))]: ordinary interior points, integer and half-integer coordinates on every image region"""
    out = []
    regions = (("flat50", 5, 22, 5, 18), ("flat0", 29, 46, 5, 18), ("checker", 5, 22, 25, 38), ("ramp", 29, 58, 25, 38),
               ("noise", 50, 90, 3, 20), ("noise2", 62, 90, 24, 58))
    for reg, x0, x1, y0, y1 in regions:
        k = 0
        for fx, fy in ((0.0, 0.0), (0.5, 0.5), (0.0, 0.5), (0.5, 0.0), (0.25, 0.75)):
            for _ in range(3 if reg.startswith("noise") else 2):
                x = float(rng.integers(x0, x1)) + fx
                y = float(rng.integers(y0, y1)) + fy
                out.append(("interior", f"{reg}_{'int' if (fx, fy) == (0.0, 0.0) else 'frac'}{k}", (x, y, float(rng.uniform(0.8, 4.0)))))
                k += 1
    for k in range(54):
        out.append(("interior", f"any{k}", (float(rng.uniform(2, 90)), float(rng.uniform(2, 58)), float(rng.uniform(0.6, 6.0)))))
    return out


def _huber_targets():
    out = []
    for k, (x, y) in enumerate(((6.0, 7.0), (10.5, 9.5), (14.25, 12.0), (20.0, 17.75), (8.0, 15.5), (17.5, 6.0))):
        out.append(("huber_flat50", f"flat50_h{k}", (x, y, 1.5 + 0.25 * k)))
    for k, x in enumerate((41.0, 41.75, 42.0, 42.0 + 2.0 ** -10, 42.25, 43.0, 58.0)):         # neg = 8 + 3 (x - 28): 47 .. 53, 98
        out.append(("huber_ramp", f"ramp_h{k}", (x, 30.0 + k, 2.0)))
    for k, (x, y) in enumerate(((30.0, 6.0), (35.5, 10.5), (44.25, 16.0), (40.0, 12.75))):
        out.append(("huber_flat0", f"flat0_h{k}", (x, y, 1.25 + 0.5 * k)))
    return out


def _mask_targets():
    """interior on every block, the pair 19.99 | 20.0 across 124 | 125 (x = k + 0.99 indexes pixel k), the rows 43.99 | 44.0"""
    out = []
    for v, cols in MASK_BLOCKS:
        out.append(("mask", f"mask{v}_in", (cols.start + 3.5, 50.25, 2.0)))
        out.append(("mask", f"mask{v}_int", (cols.start + 2.0, 53.0, 3.0)))
    out += [("mask", "mask_x19.99", (19.99, 47.5, 2.0)), ("mask", "mask_x20.0", (20.0, 47.5, 2.0)),
            ("mask", "mask_x27.99", (27.99, 55.5, 2.0)), ("mask", "mask_x11.99", (11.99, 56.5, 2.0)), ("mask", "mask_x12.0", (12.0, 56.5, 2.0)),
            ("mask", "mask_y43.99", (8.5, 43.99, 2.0)), ("mask", "mask_y44.0", (8.5, 44.0, 2.0)),
            ("mask", "mask_y43.99b", (22.5, 43.99, 2.0)), ("mask", "mask_y44.0b", (22.5, 44.0, 2.0))]
    return out


def _unproject(P, x, y, z):
    """the left-frame point of depth z that P projects to (x, y): P[:, :3] pl = z (x, y, 1) - P[:, 3], in f64"""
    return np.linalg.solve(P[:, :3], z * np.array([x, y, 1.0]) - P[:, 3])


def points(variant, W, H):
    """-> (names, kinds, motions, xyz float32 (n, 3)), permuted so that every prefix mixes kinds"""
    rig = rig_variant(variant, W, H)
    P = np.asarray(rig.left.P, np.float64).reshape(3, 4)
    exact = variant != "skewed"
    rng = np.random.default_rng(77 + W)
    rows = []                                                   # (name, kind, motion, xyz)
    for mname, (R, t) in MOTIONS.items():
        def place(x, y, z):
            return R @ _unproject(P, x, y, z) + t
        for name, (x, y), kw in _bounds_targets(W, H):
            if exact and mname == "identity":
                p = _exact(x, y, W, H, **kw)
            else:
                z = -FOCAL * S if kw.get("behind") else FOCAL * S
                step = 2.0 ** -12
                p = place(x + step * kw.get("nx", 0), y + step * kw.get("ny", 0), z)
            rows.append((f"{name}@{mname}", "bounds", mname, p))
        for kind, name, (x, y, z) in _interior_targets(rng) + _huber_targets() + _mask_targets():
            # integer, half- and quarter-integer targets are exact as well (q2 == 0, q4 == 0; a mask block's first column / row),
            # at one of three depths
            dyadic = not name.startswith("any") and (1024 * x).is_integer() and (4 * y).is_integer()
            if dyadic and exact and mname == "identity":
                rows.append((f"{name}@{mname}", kind, mname, _exact(x, y, W, H, S=2.0 ** (-7 + len(rows) % 3))))
            else:
                rows.append((f"{name}@{mname}", kind, mname, place(x, y, z)))
        for k, (x, y, z) in enumerate(((W / 2.0, H / 2.0, -2.0), (W / 4.0, H / 3.0, -0.7), (3 * W / 4.0, H / 5.0, -6.0))):
            rows.append((f"behind{k}@{mname}", "behind", mname, place(x, y, z)))
    # p_ref.z == 0: under the identity pl.z == 0 (x = +-inf: rejected); under the moved pose z_left is about -t_z and the point
    # projects inside, mirrored, with D = P / 0: NaN rows
    tm = MOTIONS["moved"][1]
    for k, (dx, dy) in enumerate(((0.0, 0.0), (0.004, -0.003), (-0.005, 0.002))):
        rows.append((f"zref0_{k}", "zref0", "moved", (tm[0] + dx, tm[1] + dy, 0.0)))
    rows += [("plz0_a", "plz0", "identity", (0.3, 0.2, 0.0)), ("plz0_b", "plz0", "identity", (0.0, 0.0, 0.0))]
    rows += [("nan_z", "nonfinite", "both", (0.1, 0.1, np.nan)), ("nan_x", "nonfinite", "both", (np.nan, 0.0, 2.0)),
             ("inf_x", "nonfinite", "both", (np.inf, 0.0, 2.0)), ("ninf_y", "nonfinite", "both", (0.0, -np.inf, 2.0)),
             ("inf_z", "nonfinite", "both", (0.0, 0.0, np.inf))]
    rows += [("huge_x", "huge", "identity", (3e38, 0.5, 1e-44)), ("huge_negx", "huge", "identity", (-3e38, 0.5, 1e-44)),
             ("huge_y", "huge", "identity", (0.0, -1.0, 1e-40))]
    order = np.random.default_rng(78 + W).permutation(len(rows))
    rows = [rows[i] for i in order]
    with np.errstate(all="ignore"):
        xyz = np.ascontiguousarray(np.array([r[3] for r in rows], np.float64), np.float32)
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], xyz


def long_points(xyz, kinds, nan_free):
    """the 2049-point problem: the list tiled, copy k scaled by (1 + k / 64) about the reference origin (the identity projects a
    copy where it projected the original, at another depth: the rows differ); nan_free: without the points of reference depth 0
    (zref0, plz0), the only ones whose rows can be NaN (a rejected point has zero rows whatever its coordinates)"""
    keep = np.array([not (nan_free and k in ("zref0", "plz0")) for k in kinds])
    base = xyz[keep].astype(np.float64)
    reps = -(-LONG_N // len(base))
    with np.errstate(all="ignore"):
        tiled = np.concatenate([base * (1.0 + k / 64.0) for k in range(reps)])[:LONG_N]
    return np.ascontiguousarray(tiled, np.float32)


def all_invalid_points(n=300):
    """every point projects far outside the image under the identity and under small motions: H = 0, b = 0, cost = n 255^2"""
    rng = np.random.default_rng(5)
    return np.ascontiguousarray(np.stack([rng.uniform(50.0, 90.0, n), rng.uniform(-90.0, -50.0, n), rng.uniform(1.0, 2.0, n)], axis=1),
                                np.float32)


def batches(n):
    """(offset, count) around the point count n"""
    return ((0, n), (0, n + 10), (n - 1, 1), (n - 1, 2), (n, 1), (n + 1, 3), (7, n - 8), (7, n - 7), (7, n - 6), (3, 0), (130, 1), (64, 257))


_CACHE = {}


def problem(variant, W, H):
    """dict: rig, P, mask, ts, images0 = (neg, du, dv) at kernelSize 0, names / kinds / motions, xyz (f32), pts (f64 reference-frame
    points), long_xyz / long_pts, long_free_xyz / long_free_pts; arrays are read-only"""
    key = (variant, W, H)
    if key not in _CACHE:
        rig = rig_variant(variant, W, H)
        names, kinds, motions, xyz = points(variant, W, H)
        ts = time_surface(W, H)
        c = dict(variant=variant, W=W, H=H, rig=rig, P=np.asarray(rig.left.P, np.float64).reshape(3, 4).copy(),
                 mask=rig.left.rect_mask, ts=ts, images0=TR.track_images(ts), names=names, kinds=kinds, motions=motions, xyz=xyz,
                 pts=RR.reference_points(xyz, I4))
        for tag, free in (("long", False), ("long_free", True)):
            c[tag + "_xyz"] = long_points(xyz, kinds, free)
            c[tag + "_pts"] = RR.reference_points(c[tag + "_xyz"], I4)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        for a in c["images0"]:
            a.setflags(write=False)
        _CACHE[key] = c
    return _CACHE[key]


def infos(c, motion):
    """the restatement's intermediate values of every point under a motion (kernelSize 0 images), computed once"""
    key = ("info", c["variant"], c["W"], c["H"], motion)
    if key not in _CACHE:
        R, t = MOTIONS[motion]
        T = RR.pose_left_ref(R, t)
        _CACHE[key] = [TR.point_info(c["images0"][0], c["mask"], c["P"], p, T) for p in c["pts"]]
    return _CACHE[key]


PIN_MARGIN = 3.0   # pixels: the pin also evaluates at the increment PIN_X, which moves a projection by up to about 1.5 px


def pinned(c, motion):
    """bool per point: whether the reference is defined on it under this motion (UNPINNED_KINDS), and the reason where it is not"""
    keep, why = [], []
    box = None
    if c["mask"] is not None and ((c["mask"] != 0) & (c["mask"] != 255)).any():
        ys, xs = np.nonzero((c["mask"] != 0) & (c["mask"] != 255))
        box = (xs.min() - PIN_MARGIN, xs.max() + 1 + PIN_MARGIN, ys.min() - PIN_MARGIN, ys.max() + 1 + PIN_MARGIN)
    for info, p in zip(infos(c, motion), c["pts"]):
        reason = None
        if not (np.isfinite(p).all() and np.isfinite(info["x"]) and np.isfinite(info["y"])):
            reason = "nonfinite"
        elif info["valid"] and not info["interp_ok"]:
            reason = "border_gradient"
        elif box is not None and box[0] <= info["x"] <= box[1] and box[2] <= info["y"] <= box[3]:
            reason = "mask_byte"                                  # on such a byte, or near enough to reach one at PIN_X
        keep.append(reason is None)
        why.append(reason)
    return np.array(keep), why


def input_digest(c, motion):
    h = hashlib.sha256()
    for a in (c["ts"], c["xyz"], c["P"], pinned(c, motion)[0].astype(np.uint8), np.asarray(MOTIONS[motion][0], np.float64),
              np.asarray(MOTIONS[motion][1], np.float64)):
        h.update(np.ascontiguousarray(a).tobytes())
    if c["mask"] is not None:
        h.update(np.ascontiguousarray(c["mask"]).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


PIN_X = np.array([0.002, -0.001, 0.003, 0.004, -0.002, 0.001])   # the non-zero increment of the reference pin


def same_bits(got, want, label=""):
    """equality byte for byte where no NaN occurs; elsewhere the NaN positions are equal and the remaining bytes are equal (the
    host and the device may produce NaNs of different sign or payload)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (label, "NaN positions differ", np.argwhere(gn != wn)[:5].tolist())
    if got[~gn].tobytes() != want[~wn].tobytes():
        bad = np.argwhere((got != want) & ~gn)
        if len(bad) == 0:
            bad = np.argwhere((np.signbit(got) != np.signbit(want)) & ~gn)
        raise AssertionError(f"{label}: {len(bad)} values differ, first at {bad[:5].tolist()}: "
                             f"{[float(got[tuple(b)]) for b in bad[:3]]} != {[float(want[tuple(b)]) for b in bad[:3]]}")
