"""The tracker's reprojection map (Reproj_Map_Left) restated in plain numpy: the visualisation block of
RegProblemSolverLM::solve_analytical (RegProblemSolverLM.cpp:180-209) with Visualization::DrawPoint (Visualization.cpp:74-94),
as a sequential loop over the points -- the rules esvo_amd/csrc/kernels_track_viz.hip states in its header, literally:

    img = GRAY2BGR(TS_negative_left_)                                            // :185-188
    for i in 0 .. n-1:                                                            // :194-204, ResItems_ order
      p_3D = R^T p_i + (-R^T t);  (x, y) = world2Cam(p_3D)                        // no bounds test, no mask
      DrawPoint(1 / p_i.z, max_range, min_range, (x, y), img)                     // p_i.z: z in the REFERENCE frame
        index = clamp(floor((val - min_range) / (max_range - min_range) * 255), 0, 255)
        cv::circle(img, (int)x, (int)y, 1, jet[index], FILLED)                    // the 5-pixel plus, clipped to the image

Every f64 expression is formed element by element in the kernel's order (no @, no np.dot: their summation order is not the
kernel's).  Where the reference is undefined the point is skipped: x or y not finite or of magnitude >= 2^30, a NaN index.
cv::circle's raster is restated (centre + 4 neighbours), not pinned to OpenCV -- as for the mapper's debug images."""
import math

import numpy as np


def pose_left_ref(R, t):
    """T_left_ref = [R^T | -R^T t] as esvo_track_jacobian builds it on the host (api_track.hip): 3 x 4, f64"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    T = np.zeros((3, 4), np.float64)
    for r in range(3):
        for c in range(3):
            T[r, c] = R[c, r]
        T[r, 3] = (-R[0, r] * t[0] + -R[1, r] * t[1]) + -R[2, r] * t[2]
    return T


def reference_points(xyz_world, T_world_ref):
    """setProblem's point loop (RegProblemLM.cpp:44-56) in the expression order of track_reference_kernel:
    d = (f64)p - t_world_ref;  p_cam[c] = (R[0,c] d0 + R[1,c] d1) + R[2,c] d2"""
    xyz = np.asarray(xyz_world, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T_world_ref, np.float64).reshape(4, 4)
    d = [xyz[:, k] - T[k, 3] for k in range(3)]
    out = np.empty_like(xyz)
    with np.errstate(all="ignore"):                           # (a test's point may hold an infinity or a NaN)
        for c in range(3):
            out[:, c] = (T[0, c] * d[0] + T[1, c] * d[1]) + T[2, c] * d[2]
    return out


def _div(a, b):
    """IEEE f64 division (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def color_index(z_ref, inv_min, inv_max):
    """DrawPoint's table index for a point of reference-frame depth z_ref, or None where it is NaN"""
    val = _div(1.0, z_ref)
    with np.errstate(all="ignore"):
        v = float(np.floor(np.float64(val - inv_min) / np.float64(inv_max - inv_min) * np.float64(255.0)))
    if math.isnan(v):
        return None
    v = 255.0 if v > 255.0 else (0.0 if v < 0.0 else v)     # clamped in f64, then converted
    return int(v)


def project(p, T, P):
    """(x, y) of the reference point p under T_left_ref T (3 x 4) and the projection matrix P (3 x 4)"""
    p = [float(p[0]), float(p[1]), float(p[2])]
    with np.errstate(all="ignore"):
        pl = [np.float64(((T[r, 0] * p[0] + T[r, 1] * p[1]) + T[r, 2] * p[2]) + T[r, 3]) for r in range(3)]
        hm = [np.float64(((P[r, 0] * pl[0] + P[r, 1] * pl[1]) + P[r, 2] * pl[2]) + P[r, 3]) for r in range(3)]
    return _div(hm[0], hm[2]), _div(hm[1], hm[2])


def reprojection_map(neg, pts_ref, R, t, P, n, inv_min, inv_max, jet):
    """neg: (H, W) uint8; pts_ref: (m, 3) f64 points in the reference camera frame; (R, t): the registered motion;
    P: 3 x 4 left projection matrix; n: points to draw (clamped to m); jet: (256, 3) uint8 BGR.
    -> ((H, W, 3) uint8 BGR, n_inside)"""
    neg = np.asarray(neg, np.uint8)
    H, W = neg.shape
    img = np.repeat(neg[:, :, None], 3, axis=2).copy()
    pts = np.asarray(pts_ref, np.float64).reshape(-1, 3)
    P = np.asarray(P, np.float64).reshape(3, 4)
    jet = np.asarray(jet, np.uint8).reshape(256, 3)
    T = pose_left_ref(R, t)
    n_inside = 0
    for i in range(min(int(n), len(pts))):
        x, y = project(pts[i], T, P)
        if not (math.isfinite(x) and math.isfinite(y)) or abs(x) >= 2.0**30 or abs(y) >= 2.0**30:
            continue
        index = color_index(pts[i, 2], inv_min, inv_max)
        if index is None:
            continue
        cx, cy = int(x), int(y)                               # truncation toward zero, as cv::Point from doubles
        if 0 <= cx < W and 0 <= cy < H:
            n_inside += 1
        for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
            px, py = cx + dx, cy + dy
            if 0 <= px < W and 0 <= py < H:
                img[py, px] = jet[index]                      # a later point paints over an earlier one
    return img, n_inside
