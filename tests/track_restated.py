"""The tracker's point evaluation restated in plain numpy / Python: one value of RegProblemLM::operator() + thread()
(RegProblemLM.cpp:91-176), one row of df at x = 0 (:178-269), reprojection / isValidPatch / patchInterpolation (:366-483) for the
1 x 1 patch, and the normal equations in the summation order esvo_amd/csrc/kernels_track.hip documents -- a sequential loop over
the points in f64, every expression formed element by element in the written order (no @, no np.dot):

    pl = T_left_ref p;  hm = P pl;  (x, y) = hm[0:2] / hm[2]
    rejected: x or y not finite | x < 0 | x > W-1 | y < 0 | y > H-1 | mask[(int)y, (int)x] < 125        (closed bounds; -0.0 passes)
    interp:   ux = floor(x), uy = floor(y); fails where ux + 1 >= W or uy + 1 >= H  (x == W-1, y == H-1: valid, no interpolation)
              (q3 (q1 s00 + q2 s01)) + (q4 (q1 s10 + q2 s11)),  q1 = (ux+1) - x, q2 = x - ux, q3 = (uy+1) - y, q4 = y - uy
    r = interp(neg) or 255;  Huber: w = thr / r where r > thr, else 1;  f = sqrt(w) r
    Jacobian row: zeros for a rejected point; else g = interp(du) / 8, interp(dv) / 8 (0 where the interpolation fails) through
              D = dPi/dT, J_constPart, D again, dT/dG and the factor p.z, then -fjacBlock J_G(0)

Signed zeros, infinities and NaNs arise as IEEE 754 makes them: divisions go through numpy scalars, nothing is caught."""
import math

import numpy as np

import reproj_restated as RR

NE_THREADS = 256          # TRK_NE_THREADS: partial sums of the normal equations


def reproject(p, T, P, W, H, mask):
    """-> dict(x, y, valid, reason, mask_byte): reason is None or the first test that rejected the point, in the kernel's order"""
    x, y = RR.project(p, T, P)
    out = dict(x=x, y=y, valid=False, reason=None, mask_byte=None)
    if not (math.isfinite(x) and math.isfinite(y)):
        out["reason"] = "nonfinite"
    elif x < 0.0:
        out["reason"] = "left"
    elif x > float(W - 1):
        out["reason"] = "right"
    elif y < 0.0:
        out["reason"] = "top"
    elif y > float(H - 1):
        out["reason"] = "bottom"
    else:
        if mask is not None:
            out["mask_byte"] = int(mask[int(y), int(x)])            # truncation toward zero; x, y >= 0 here
        if mask is not None and out["mask_byte"] < 125:
            out["reason"] = "mask"
        else:
            out["valid"] = True
    return out


def interp(img, x, y):
    """-> (value or None, None | 'right' | 'bottom' | 'outside'): bilinear read of an integer-valued (H, W) image"""
    H, W = img.shape
    ux, uy = int(math.floor(x)), int(math.floor(y))
    if ux < 0 or uy < 0 or ux >= W or uy >= H:
        return None, "outside"
    q1, q2 = float(ux + 1) - x, x - float(ux)
    q3, q4 = float(uy + 1) - y, y - float(uy)
    if uy + 1 >= H:
        return None, "bottom"
    if ux + 1 >= W:
        return None, "right"
    s00, s01, s10, s11 = float(img[uy, ux]), float(img[uy, ux + 1]), float(img[uy + 1, ux]), float(img[uy + 1, ux + 1])
    r0 = q1 * s00 + q2 * s01
    r1 = q1 * s10 + q2 * s11
    return q3 * r0 + q4 * r1, None


def huber_weighted(r, huber, thr):
    if not huber:
        return r
    w = 1.0
    if r > thr:
        w = RR._div(thr, r)
    return math.sqrt(w) * r


def point_info(neg, mask, P, p, T):
    """the intermediate values of one point's residual: reproject's dict + interp_ok, interp_fail, r (before the norm)"""
    H, W = neg.shape
    info = reproject(p, T, P, W, H, mask)
    info.update(interp_ok=False, interp_fail=None, r=255.0)
    if info["valid"]:
        tau, why = interp(neg, info["x"], info["y"])
        info["interp_ok"], info["interp_fail"] = tau is not None, why
        if tau is not None:
            info["r"] = tau
    return info


def residuals(neg, mask, P, pts_ref, T_left_ref, offset, count, huber, thr):
    """fvec of the batch [offset, offset + count) cut at the point count (setStochasticSampling, :71-88)"""
    P = np.asarray(P, np.float64).reshape(3, 4)
    T = np.asarray(T_left_ref, np.float64).reshape(-1, 4)[:3]
    pts = np.asarray(pts_ref, np.float64).reshape(-1, 3)
    out = []
    for i in range(offset, min(offset + count, len(pts))):
        out.append(huber_weighted(point_info(neg, mask, P, pts[i], T)["r"], huber, thr))
    return np.array(out, np.float64)


def const_part(R, P):
    """J_constPart = R^T diag(1 / P11, 1 / P22; 0) (:189-194): 3 x 2"""
    iP11, iP22 = RR._div(1.0, P[0, 0]), RR._div(1.0, P[1, 1])
    return [[float(R[0, r]) * iP11, float(R[1, r]) * iP22] for r in range(3)]


def jacobian_row(du, dv, mask, P, p, T, Jc):
    H, W = du.shape
    p = [float(p[0]), float(p[1]), float(p[2])]
    info = reproject(p, T, P, W, H, mask)
    if not info["valid"]:
        e = [0.0] * 12
    else:
        gx, _ = interp(du, info["x"], info["y"])
        gy, _ = interp(dv, info["x"], info["y"])
        gx = 0.0 if gx is None else gx                            # border pixel: the reference reads an unset matrix; defined as 0
        gy = 0.0 if gy is None else gy
        g0, g1 = gx / 8, gy / 8
        z = p[2]
        z2 = z * z
        P11, P12, P14, P21, P22, P24 = (float(P[0, 0]), float(P[0, 1]), float(P[0, 3]), float(P[1, 0]), float(P[1, 1]),
                                        float(P[1, 3]))
        D = [[RR._div(P11, z), RR._div(P12, z), RR._div(-((P11 * p[0] + P12 * p[1]) + P14), z2)],
             [RR._div(P21, z), RR._div(P22, z), RR._div(-((P21 * p[0] + P22 * p[1]) + P24), z2)]]
        av = [g0 * D[0][j] + g1 * D[1][j] for j in range(3)]
        b = [(av[0] * Jc[0][j] + av[1] * Jc[1][j]) + av[2] * Jc[2][j] for j in range(2)]
        c = [b[0] * D[0][j] + b[1] * D[1][j] for j in range(3)]
        e = [0.0] * 12
        for j in range(3):
            e[j] = (c[j] * p[0]) * z
            e[3 + j] = (c[j] * p[1]) * z
            e[6 + j] = (c[j] * p[2]) * z
            e[9 + j] = c[j] * z
    return [-(2.0 * e[5] - 2.0 * e[7]), -(2.0 * e[6] - 2.0 * e[2]), -(2.0 * e[1] - 2.0 * e[3]), -e[9], -e[10], -e[11]]


def jacobian(neg_du_dv, mask, P, pts_ref, R, t, offset, count):
    """(n, 6) rows of df at x = 0 for the batch; neg_du_dv: the (neg, du, dv) images (neg is not read)"""
    _, du, dv = neg_du_dv
    P = np.asarray(P, np.float64).reshape(3, 4)
    R = np.asarray(R, np.float64).reshape(3, 3)
    T = RR.pose_left_ref(R, t)
    Jc = const_part(R, P)
    pts = np.asarray(pts_ref, np.float64).reshape(-1, 3)
    rows = [jacobian_row(du, dv, mask, P, pts[i], T, Jc) for i in range(offset, min(offset + count, len(pts)))]
    return np.array(rows, np.float64).reshape(-1, 6)


def sum_normal_equations(J, f):
    """(H 6 x 6, b 6, cost) from the rows J (n, 6) and values f (n) in the documented order: partial sum t of 256 takes the points
    t, t + 256, ... in turn, then the tree s[t] += s[t + 128], ..., s[0] += s[1].  Each addition is one elementwise numpy
    operation on the 28 terms of up to 256 partial sums: the order of the additions into any one sum is the written one."""
    n = len(f)
    with np.errstate(all="ignore"):
        terms = np.empty((n, 28), np.float64)
        k = 0
        for i in range(6):
            for j in range(i, 6):
                terms[:, k] = J[:, i] * J[:, j]
                k += 1
        for i in range(6):
            terms[:, 21 + i] = J[:, i] * f
        terms[:, 27] = f * f
        part = np.zeros((NE_THREADS, 28), np.float64)
        for base in range(0, n, NE_THREADS):
            m = min(NE_THREADS, n - base)
            part[:m] = part[:m] + terms[base:base + m]
        s = NE_THREADS // 2
        while s > 0:
            part[:s] = part[:s] + part[s:2 * s]
            s //= 2
    out = part[0]
    Hm = np.zeros((6, 6), np.float64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            Hm[i, j] = Hm[j, i] = out[k]
            k += 1
    return Hm, out[21:27].copy(), float(out[27])


def normal_equations(neg_du_dv, mask, P, pts_ref, R, t, offset, count, huber, thr):
    """(H, b, |f|^2, n) of one iteration at (R, t): f = operator()(0) with the Huber weights, J = df(0) (no weight)"""
    f = residuals(neg_du_dv[0], mask, P, pts_ref, RR.pose_left_ref(R, t), offset, count, huber, thr)
    J = jacobian(neg_du_dv, mask, P, pts_ref, R, t, offset, count)
    return sum_normal_equations(J, f) + (len(f),)


def track_images(blurred):
    """neg = 255 - blurred; du, dv = its 3 x 3 Sobel derivatives with BORDER_REFLECT_101 (TimeSurfaceObservation.h:118-147), integers"""
    neg = 255 - np.asarray(blurred, np.uint8).astype(np.int32)
    pad = np.pad(neg, 1, mode="reflect")
    H, W = neg.shape

    def at(dy, dx):
        return pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    du = (at(-1, 1) - at(-1, -1)) + 2 * (at(0, 1) - at(0, -1)) + (at(1, 1) - at(1, -1))
    dv = (at(1, -1) - at(-1, -1)) + 2 * (at(1, 0) - at(-1, 0)) + (at(1, 1) - at(-1, 1))
    return neg.astype(np.uint8), du.astype(np.int16), dv.astype(np.int16)
