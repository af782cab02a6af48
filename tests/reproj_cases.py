"""Crafted inputs of the reprojection-map tests (tests/test_gpu_track_reproj.py; their power is checked on the CPU in
tests/test_track_reproj_restated.py): about 400 reference points whose projections sit where the drawing rules differ, built once
per image size and only read afterwards."""
import os

import numpy as np

import reproj_restated as RR

JET = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jet256.npy")).reshape(256, 3)
INV_MIN, INV_MAX = 0.16, 1.0          # val = 1 / z inside the range for z in (1, 6.25)
FOCAL = 120.0


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


MOTIONS = {  # (R, t) of the registration: p_left = R^T (p_ref - t)
    "identity": (np.eye(3), np.zeros(3)),
    "moved": (_rot(0.011, -0.017, 0.023), np.array([0.031, -0.022, 0.047])),
}


def _targets(W, H, rng):
    """(x, y, z_left) triples: where a point shall project, and its depth in the left (warped) frame"""
    out = []
    # 64 points into a 4 x 4 pixel area, all depths distinct: the overlap order decides almost every pixel there
    x0, y0 = W // 3, H // 2
    for k in range(64):
        out.append((x0 + 4.0 * rng.random(), y0 + 4.0 * rng.random(), 1.05 + 0.08 * k))
    xm, ym = W / 2 + 0.4, H / 2 + 0.3
    for z in (0.5, 2.0, 10.0):                                  # val above, inside, below the range
        # centres on each edge, one pixel outside each edge, far outside
        out += [(0.5, ym, z), (W - 0.5, ym, z), (xm, 0.5, z), (xm, H - 0.5, z)]
        out += [(-1.5, ym + 3, z), (W + 0.5, ym + 3, z), (xm + 3, -1.5, z), (xm + 3, H + 0.5, z)]
        out += [(-2.5, ym, z), (W + 1.5, ym, z), (xm, -2.5, z), (xm, H + 1.5, z), (-50.0, ym, z), (W + 200.0, -300.0, z), (1e6, ym, z)]
        # fractional coordinates in (-1, 0): they truncate to 0
        out += [(-0.6, ym - 5, z), (xm - 5, -0.3, z), (-0.9, -0.2, z), (-0.1, H - 0.5, z), (W - 0.5, -0.7, z)]
        # the corners and just beyond them
        out += [(0.5, 0.5, z), (W - 0.5, H - 0.5, z), (-1.5, -1.5, z), (W + 0.5, H + 0.5, z), (-1.5, 0.5, z), (W - 0.5, H + 0.5, z)]
    for _ in range(70):                                          # anywhere in and around the image
        out.append((rng.uniform(-3, W + 3), rng.uniform(-3, H + 3), rng.uniform(0.4, 12.0)))
    return out


def crafted(W, H, P, seed=3):
    """(n, 3) float32 reference points (handed to track_set_reference with T_world_ref = I: they ARE the reference frame)"""
    rng = np.random.default_rng(seed)
    P = np.asarray(P, np.float64).reshape(3, 4)
    fx, fy, cx, cy = P[0, 0], P[1, 1], P[0, 2], P[1, 2]
    pts = []
    for R, t in MOTIONS.values():                               # each motion gets targets of its own: p_ref = R p_left + t
        for x, y, z in _targets(W, H, rng):
            pts.append(R @ np.array([(x - cx) * z / fx, (y - cy) * z / fy, z]) + t)
    for x, y, z in ((W / 2, H / 2, -2.0), (W / 4, H / 3, -0.7), (3 * W / 4, H / 5, -6.0)):   # behind the camera: still drawn, mirrored
        pts.append([(x - cx) * z / fx, (y - cy) * z / fy, z])
    pts += [[0.3, 0.2, 0.0], [0.0, 0.0, 0.0],                    # warped z == 0 under the identity: x = inf / NaN, skipped
            [0.1, 0.1, np.nan], [np.inf, 0.0, 2.0], [0.0, 0.0, np.inf],
            [1.0, 0.0, 1e-8], [0.0, -1.0, 1e-8],                # |x| or |y| >= 2^30: skipped
            [1.0, 0.5, 3e-7]]                                    # x about 4e8 < 2^30: drawn, far outside the image
    pts = np.array(pts, np.float64)
    order = np.random.default_rng(seed + 1).permutation(len(pts))   # the kinds interleave: every prefix holds several of them
    return np.ascontiguousarray(pts[order], np.float32)


def n_values(n_all):
    return (0, 1, 63, 64, 65, n_all, n_all + 10)


def check_power(neg, pts_ref, P):
    """what makes a byte-for-byte comparison on these inputs worth something; returns the identity-motion restatement"""
    R, t = MOTIONS["identity"]
    n = len(pts_ref)
    grey = np.repeat(neg[:, :, None], 3, axis=2)
    fwd, n_in = RR.reprojection_map(neg, pts_ref, R, t, P, n, INV_MIN, INV_MAX, JET)
    assert int((fwd != grey).any(axis=2).sum()) > 200, "too few painted pixels"
    rev, n_rev = RR.reprojection_map(neg, pts_ref[::-1], R, t, P, n, INV_MIN, INV_MAX, JET)
    assert n_rev == n_in and not np.array_equal(fwd, rev), "the image does not depend on the order of the points"
    assert 0 < n_in < n                                          # some centres inside, some outside or skipped
    return fwd, n_in
