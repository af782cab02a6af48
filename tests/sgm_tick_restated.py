"""CPU restatement of esvo_MVStereo's PURE_SEMI_GLOBAL_MATCHING mode (MVStereoMode 4) behind the disparity image, written from
the reference's text: the DepthPoint rule of esvo_MVStereo.cpp:329-353 on createEdgeMask(..., true, 0) (:1127-1170), the window
(:357-359) and DepthFusion::naive_propagation (DepthFusion.cpp:234-327) of every frame, newest first (:360-361).

Independent of the library: numpy only.  Element-wise float64 operations in the device's order, with the closed forms the
device and the project's oracle use (em_restated.Cam's constants, rigid_inverse, mat4_mul) -- so the device can equal it bit
for bit -- and no np.dot / @, which use BLAS or FMA.  tests/test_sgm_tick_restated.py pins it to the reference's own compiled
mode-4 branch.

Two definitions where the reference leaves the behaviour open (both as everywhere else in the project):
  * scale2 / nu of a Gaussian DepthPoint are uninitialised memory upstream; 0 here.
  * a propagated coordinate that is not finite passes the reference's boundaryCheck (DepthFusion.cpp:195-205: every comparison
    is false) and the float-to-integer conversion behind it is undefined; here such a point touches no cell.
"""
import numpy as np

import em_restated as E
from esvo_amd.abi import DEPTH_POINT_DTYPE

NUM_DISPARITIES = 48
FIELDS = ("row", "col", "x", "inv_depth", "scale2", "nu", "variance", "residual", "age", "p_cam", "pose_idx", "seq")


def _cam2world(cam, x, y, inv_depth):
    """PerspectiveCamera::cam2World in the closed form (em_restated.Cam.cam2world), element-wise; inv_depth 0 gives 1 / 0 = inf"""
    K, Kt = cam.Kinv, cam.Kinv_t
    with np.errstate(divide="ignore", invalid="ignore"):
        z = 1.0 / inv_depth
        return np.stack([z * ((K[r * 3 + 0] * x + K[r * 3 + 1] * y) + K[r * 3 + 2]) - Kt[r] for r in range(3)], axis=-1)


def points(rig, params, disp16, ev):
    """The frame of one tick: (DEPTH_POINT_DTYPE array in the events' order, counts at each filter).
    disp16: (H, W) int16 disparity x 16; ev: vEventsPtr_left_SGM_ in the node's order."""
    W, H = rig.width, rig.height
    camL, camR = E.Cam(rig.left.P), E.Cam(rig.right.P)
    bf = E.baseline(camR) * camL.P[0]                                          # P_(0,0) * baseline_, :341
    lut = np.asarray(rig.left.rect_lut, np.float32).reshape(H, W, 2)
    disp16 = np.asarray(disp16, np.int16).reshape(H, W)
    ex, ey = np.asarray(ev["x"], np.int64), np.asarray(ev["y"], np.int64)
    on_sensor = (ex < W) & (ey < H)                                            # no rectified coordinate off the sensor
    c = lut[np.where(on_sensor, ey, 0), np.where(on_sensor, ex, 0)].astype(np.float64)
    x, y = np.floor(c[:, 0]).astype(np.int64), np.floor(c[:, 1]).astype(np.int64)   # :1152-1153
    on_image = on_sensor & (x >= 0) & (x < W) & (y >= 0) & (y < H)            # :1160
    col_ok = on_image & (x >= NUM_DISPARITIES)                                 # :333
    disp = disp16[np.where(col_ok, y, 0), np.where(col_ok, x, 0)] / 16.0       # :335
    keep = col_ok & ~(disp < 0)                                                # :336
    x, y, disp = x[keep], y[keep], disp[keep]
    out = np.zeros(len(x), DEPTH_POINT_DTYPE)
    out["row"], out["col"] = x, y                                              # DepthPoint dp(x, y): (row, col), :338
    out["x"][:, 0], out["x"][:, 1] = x * 1.0, y * 1.0                          # :339-340
    inv = disp / bf                                                            # :341
    out["inv_depth"] = inv
    out["p_cam"] = _cam2world(camL, out["x"][:, 0], out["x"][:, 1], inv)       # :344-346
    out["variance"] = 1e-6                                                     # update(invDepth, 0) + boundVariance, :347
    out["residual"] = 0.0                                                      # :348
    out["age"] = int(params.age_vis_threshold)                                 # :349
    out["seq"] = np.arange(len(x))
    stats = dict(events=len(ev), on_image=int(on_image.sum()), matched_columns=int(col_ok.sum()), disp_ok=int(keep.sum()),
                 points=len(x), zero_disp=int((disp == 0).sum()))
    return out, stats


def naive_propagation(rig, frames, T_world_obs):
    """DepthFusion::naive_propagation of `frames` = [(points, T_world of the frame)], given in the order they are propagated
    (the window newest first), into an empty DepthFrame at T_world_obs.  Every residual is equal, so an occupied cell is never
    replaced (`prop.residual < existing.residual` is false): a cell belongs to the first point that touches it, in (frame, point,
    dy, dx) order.  Returns the map in the list order of the DepthFrame (creation order)."""
    W, H = rig.width, rig.height
    cam = E.Cam(rig.left.P)
    P = cam.P
    T_frame_world = E.rigid_inverse(T_world_obs)
    rows, cols, invs, vars_, res, ages = [], [], [], [], [], []
    for pts, T_world in frames:
        if len(pts) == 0:
            continue
        T = E.mat4_mul(T_frame_world, T_world)                                 # T_frame_obs, DepthFusion.cpp:80
        p = [pts["p_cam"][:, k] for k in range(3)]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            pp = [((T[r * 4 + 0] * p[0] + T[r * 4 + 1] * p[1]) + T[r * 4 + 2] * p[2]) + T[r * 4 + 3] for r in range(3)]
            h = [((P[r * 4 + 0] * pp[0] + P[r * 4 + 1] * pp[1]) + P[r * 4 + 2] * pp[2]) + P[r * 4 + 3] for r in range(3)]
            u, v = h[0] / h[2], h[1] / h[2]                                    # world2Cam
            ok = ~((u < 0) | (u >= float(W)) | (v < 0) | (v >= float(H))) & (u == u) & (v == v)   # boundaryCheck + "finite"
            den = (T[8] * p[0] + T[9] * p[1]) + T[11]
            den = den / p[2]
            den = den + T[10]
            J = T[10] / (den * den)
            inv = 1.0 / pp[2]
            var = J * J * pts["variance"]
        var = np.where(var < 1e-6, 1e-6, var)                                  # boundVariance
        row = np.floor(np.where(ok, v, 0.0)).astype(np.int64)
        col = np.floor(np.where(ok, u, 0.0)).astype(np.int64)
        r4 = np.stack([row, row, row + 1, row + 1], axis=1)                    # the 2 x 2 block, dy outer, dx inner (:254-256)
        c4 = np.stack([col, col + 1, col, col + 1], axis=1)
        ok4 = ok[:, None] & (r4 < H) & (c4 < W)
        sel = ok4.reshape(-1)
        rep = lambda a: np.repeat(a, 4)[sel]
        rows.append(r4.reshape(-1)[sel]); cols.append(c4.reshape(-1)[sel])
        invs.append(rep(inv)); vars_.append(rep(var)); res.append(rep(pts["residual"])); ages.append(rep(pts["age"]))
    if not rows:
        return np.zeros(0, DEPTH_POINT_DTYPE)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    _, first = np.unique(rows * W + cols, return_index=True)                   # the first record of each cell ...
    first.sort()                                                               # ... in record order = creation order
    out = np.zeros(len(first), DEPTH_POINT_DTYPE)
    out["row"], out["col"] = rows[first], cols[first]
    out["x"][:, 0], out["x"][:, 1] = cols[first] + 0.5, rows[first] + 0.5      # DepthPoint(row, col): the cell's centre
    out["inv_depth"] = np.concatenate(invs)[first]
    v = np.concatenate(vars_)[first]
    out["variance"] = np.where(v < 1e-6, 1e-6, v)
    out["residual"] = np.concatenate(res)[first]
    out["age"] = np.concatenate(ages)[first]
    out["p_cam"] = _cam2world(cam, out["x"][:, 0], out["x"][:, 1], out["inv_depth"])
    out["seq"] = np.arange(len(first))
    return out


class Mapper:
    """the mode's state: the window of (frame, pose) and the map of the last tick"""

    def __init__(self, rig, params):
        self.rig, self.params = rig, params
        self.window = []
        self.map = np.zeros(0, DEPTH_POINT_DTYPE)
        self.stats = None

    def tick(self, disp16, ev, T_world_obs):
        """MappingAtTime behind sgbm_->compute; returns the new frame"""
        T = np.asarray(T_world_obs, np.float64).reshape(4, 4).copy()
        frame, self.stats = points(self.rig, self.params, disp16, ev)
        self.window.append((frame, T))                                         # pushed even when empty, :357
        while len(self.window) > int(self.params.max_fusion_frames):           # :358-359
            self.window.pop(0)
        self.map = naive_propagation(self.rig, self.window[::-1], T)           # rbegin .. rend, :360-361
        return frame

    def window_sizes(self):
        return [len(f) for f, _ in self.window]


def same_bits(a, b, fields=FIELDS):
    """None when the two DEPTH_POINT_DTYPE arrays hold the same bytes in every field, else the first field that differs.  Two NaNs
    count as equal whatever their sign and payload (0 * inf has no defined payload across processors)."""
    if len(a) != len(b):
        return "len"
    for f in fields:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.dtype.kind == "f":
            xb, yb = x.view(np.uint64), y.view(np.uint64)
            if not np.all((xb == yb) | (np.isnan(x) & np.isnan(y))):
                return f
        elif not np.array_equal(x, y):
            return f
    return None
