"""DepthProblem::operator() (DepthProblem.cpp:34-262) and the one-unknown Levenberg-Marquardt loop around it
(DepthProblemSolver.cpp:138-214 over MINPACK's lmdif), restated in plain Python floats for tests/lm_cases.py.

The evaluator is the plan's classifier and a second opinion on the oracle: evaluate() returns, beside the residual vector, WHY an
evaluation took the failure fill (which of warping's and patchInterpolation's tests refused it) and how the Student-t scale loop
ran (non-zero residuals, the smallest of them, iterations, whether the running scale left [2^-100, 2^100], whether the loop ended
on a sum of exactly zero).  It sums a patch in index order with numpy's sequential accumulate -- the literal order of the
reference; the device and the canonical oracle sum per column and then by halving, so against those it agrees to a tolerance only
(tests/test_lm_cases.py measures it).

trace() drives ANY residual function through the solver and records every point it evaluates and every branch of the trust-region
update it takes.  Fed with oracle.eval_residual it reproduces the oracle's own solve -- tests/test_lm_cases.py asserts the same
iterations, evaluations, status and result bit for bit -- so what it records IS what the oracle's solver did."""
import math

import numpy as np

EPS = 2.220446049250313e-16
SQRT_EPS = 1.4901161193847656e-08
DWARF = 2.2250738585072014e-308
LO, HI = 2.0 ** -100, 2.0 ** 100   # the device's window for shared reciprocals (kernels_lm.hip: tight evaluation)


class Problem:
    """what an evaluation reads: the rig's two projection matrices, the image pair as doubles, patch size, nu, scale, norm"""

    def __init__(self, rig, left, right, wx=15, wy=7, nu=2.182, scale=17.277, l2=False):
        self.W, self.H = int(rig.width), int(rig.height)
        self.PL = [float(v) for v in np.asarray(rig.left.P, np.float64).reshape(-1)]
        self.PR = [float(v) for v in np.asarray(rig.right.P, np.float64).reshape(-1)]
        self.L = np.asarray(left, np.float64).reshape(self.H, self.W)
        self.R = np.asarray(right, np.float64).reshape(self.H, self.W)
        self.wx, self.wy, self.nu, self.scale, self.l2 = int(wx), int(wy), float(nu), float(scale), bool(l2)
        a, b, c, d, e, f, g, h, i = (self.PL[k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10))
        det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
        inv = 1.0 / det   # cam2World's inverse of P[:, :3] in cofactor form (the oracle's and the device's closed form)
        self.Kinv = [(e * i - f * h) * inv, (c * h - b * i) * inv, (b * f - c * e) * inv, (f * g - d * i) * inv, (a * i - c * g) * inv,
                     (c * d - a * f) * inv, (d * h - e * g) * inv, (b * g - a * h) * inv, (a * e - b * d) * inv]
        self.Kinv_t = [(self.Kinv[3 * r] * self.PL[3] + self.Kinv[3 * r + 1] * self.PL[7]) + self.Kinv[3 * r + 2] * self.PL[11] for r in range(3)]


def t_left_virtual(T_world_obs, T_world_virtual):
    """setProblem (:17-32): the rigid inverse of the observation's pose times the match's pose, first three rows, row-major"""
    a = np.asarray(T_world_obs, np.float64).reshape(4, 4)
    b = np.asarray(T_world_virtual, np.float64).reshape(4, 4)
    inv = np.eye(4)
    inv[:3, :3] = a[:3, :3].T
    for i in range(3):
        inv[i, 3] = -((inv[i, 0] * a[0, 3] + inv[i, 1] * a[1, 3]) + inv[i, 2] * a[2, 3])
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            out[i, j] = ((inv[i, 0] * b[0, j] + inv[i, 1] * b[1, j]) + inv[i, 2] * b[2, j]) + inv[i, 3] * b[3, j]
    return [float(v) for v in out[:3].reshape(-1)]


def _div(a, b):
    """IEEE division of Python floats (x / 0 and 0 / 0 included)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def warp_many(pr, cx, cy, T, rho):
    """warping (:162-191) without its bounds test, elementwise over arrays of coordinates and inverse depths (IEEE doubles, the
    operations of cam2World and world2Cam in their order) -> (x1u, x1v, x2u, x2v)"""
    cx, cy, rho = (np.asarray(v, np.float64) for v in (cx, cy, rho))
    with np.errstate(all="ignore"):
        z = np.float64(1.0) / rho
        p = [z * ((pr.Kinv[3 * r] * cx + pr.Kinv[3 * r + 1] * cy) + pr.Kinv[3 * r + 2]) - pr.Kinv_t[r] for r in range(3)]
        pl = [((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3] for r in range(3)]
        hl = [((pr.PL[4 * r] * pl[0] + pr.PL[4 * r + 1] * pl[1]) + pr.PL[4 * r + 2] * pl[2]) + pr.PL[4 * r + 3] for r in range(3)]
        hr = [((pr.PR[4 * r] * pl[0] + pr.PR[4 * r + 1] * pl[1]) + pr.PR[4 * r + 2] * pl[2]) + pr.PR[4 * r + 3] for r in range(3)]
        return hl[0] / hl[2], hl[1] / hl[2], hr[0] / hr[2], hr[1] / hr[2]


def warp(pr, coor, T, rho):
    """warp_many for one point, as Python floats"""
    return tuple(float(v) for v in warp_many(pr, coor[0], coor[1], T, rho))


def warp_refuses(pr, u, v):
    """warping's test on one camera's coordinate (:186-189)"""
    hx, hy = (pr.wx - 1) // 2, (pr.wy - 1) // 2
    return u < hx or u > pr.W - hx or v < hy or v > pr.H - hy


def interp_refuses(pr, u, v):
    """patchInterpolation's three tests (:207, :215, :239)"""
    hx, hy = (pr.wx - 1) // 2, (pr.wy - 1) // 2
    fu, fv = math.floor(u), math.floor(v)
    return fu - hx < 0 or fv - hy < 0 or fu + hx >= pr.W or fv + hy >= pr.H or fv - hy + pr.wy >= pr.H or fu - hx + pr.wx >= pr.W


def patch(pr, img, u, v):
    """patchInterpolation's bilinear patch (:224-260), wy x wx"""
    hx, hy = (pr.wx - 1) // 2, (pr.wy - 1) // 2
    l1, l0 = math.floor(u), math.floor(v)
    q1, q2, q3, q4 = (l1 + 1) - u, u - l1, (l0 + 1) - v, v - l0
    src = img[l0 - hy:l0 - hy + pr.wy + 1, l1 - hx:l1 - hx + pr.wx + 1]
    R = q1 * src[:, :pr.wx] + q2 * src[:, 1:]
    return q3 * R[:pr.wy] + q4 * R[1:]


def fill_value(pr):
    if pr.l2:
        return 255.0
    return math.sqrt((pr.nu + 1) / (pr.nu + (255.0 / pr.scale) ** 2)) * 255.0


def evaluate(pr, coor, T, rho, max_iters=1 << 20):
    """DepthProblem::operator() at inverse depth rho -> dict:
      f         residual vector (wy * wx, index y * wx + x)
      ok        1 unless the failure fill was taken;  fail: which test took it ('nonfinite', 'warp_left', 'warp_right',
                'interp_left', 'interp_right') or None;  x: the four warped coordinates
      knz, minabs, r2max   non-zero temporal residuals, the smallest magnitude among them, the largest square (Student-t only)
      iters     passes of the scale loop;  s2: the scale it ended with
      left_window   the running scale s1 left [2^-100, 2^100] at some pass;  on_zero: the loop ended on sum == 0
      shortcut  knz (nu + 1) / N <= 0.94 and minabs >= 1e-6: the device takes the collapse the literal loop must reach
      margin    the closest any pass's |s2 - s1| / s1 came to the 5 % it is compared with"""
    N = pr.wx * pr.wy
    x1u, x1v, x2u, x2v = warp(pr, coor, T, rho)
    out = dict(x=(x1u, x1v, x2u, x2v), knz=0, minabs=math.inf, iters=0, s2=None, left_window=False, on_zero=False, shortcut=False,
               margin=math.inf)
    fail = None
    if not all(math.isfinite(c) for c in out["x"]):
        fail = "nonfinite"   # undefined in the reference; the oracle and the device define: warping fails
    elif warp_refuses(pr, x1u, x1v):
        fail = "warp_left"
    elif warp_refuses(pr, x2u, x2v):
        fail = "warp_right"
    elif interp_refuses(pr, x1u, x1v):
        fail = "interp_left"
    elif interp_refuses(pr, x2u, x2v):
        fail = "interp_right"
    out["fail"], out["ok"] = fail, int(fail is None)
    if fail:
        out["f"] = np.full(N, fill_value(pr))
        return out
    r = (patch(pr, pr.L, x1u, x1v) - patch(pr, pr.R, x2u, x2v)).reshape(-1)
    if pr.l2:
        out["f"] = r
        return out
    r2 = r * r
    nz = r != 0
    out["knz"], out["r2max"] = int(nz.sum()), float(r2.max())
    out["minabs"] = float(np.abs(r[nz]).min()) if nz.any() else math.inf
    nu = pr.nu
    out["shortcut"] = out["knz"] * (nu + 1) / N <= 0.94 and out["minabs"] >= 1e-6
    s0 = pr.scale * pr.scale
    s1, s2, first, iters = s0, -1.0, True, 0
    with np.errstate(all="ignore"):
        while first or abs(s2 - s1) / s1 > 0.05:
            if not first:
                out["margin"] = min(out["margin"], abs(abs(s2 - s1) / s1 - 0.05))
                s1 = s2
            if not (LO <= s1 <= HI):
                out["left_window"] = True
            terms = np.where(nz, r2 * (nu + 1) / (nu + r2 / s1), 0.0)
            total = float(np.add.accumulate(terms)[-1])
            if total == 0:
                s2 = s0
                out["on_zero"] = True
                break
            s2 = total / N
            first = False
            iters += 1
            if iters >= max_iters:
                raise RuntimeError("scale loop did not end")
            if not out["on_zero"]:
                out["margin"] = min(out["margin"], abs(abs(s2 - s1) / s1 - 0.05))
        out["f"] = np.sqrt((nu + 1) / (nu + r2 / s2)) * r
    out["iters"], out["s2"] = iters, s2
    return out


def canonical_sum(v, wx, wy):
    """the device's and the canonical oracle's patch sum: per column over the rows in order, then halving over the columns
    padded to a power of two"""
    v = np.asarray(v, np.float64).reshape(wy, wx)
    P = 1
    while P < wx:
        P <<= 1
    col = [0.0] * P
    for x in range(wx):
        a = float(v[0, x])
        for y in range(1, wy):
            a = a + float(v[y, x])
        col[x] = a
    w = 1
    while w < P:
        col = [col[x] + col[x ^ w] for x in range(P)]
        w <<= 1
    return col[0]


def literal_sum(v, wx=None, wy=None):
    return float(np.add.accumulate(np.asarray(v, np.float64).reshape(-1))[-1]) if len(v) else 0.0


def trace(F, x0, max_iter=10, wx=15, wy=7, canonical=False, ftol=1e-6, xtol=1e-6, factor=100.0):
    """solve_single_problem_numerical (DepthProblemSolver.cpp:138-214) around Eigen's LevenbergMarquardt<NumericalDiff<>> for one
    unknown.  F(x) -> residual vector.  Returns dict:
      x, iterations, nfev, status, fnorm, r   as the solver leaves them;  solved: x > 0.001
      evals     [(kind, x)] in order: 'init', 'base' (NumericalDiff's F(x)), 'diff' (F(x + h)), 'trial' (F(x + p))
      steps     one dict per pass of the inner loop: ratio, actred, prered, par, delta, fnorm, fnorm1, accepted, branch
                ('shrink_dirder' ratio <= 1/4 with actred < 0, 'shrink_tenth' ... with 0.1 fnorm1 >= fnorm, 'shrink_half',
                 'grow' par == 0 or ratio >= 3/4, 'keep'), clip (iter == 1 cut delta to pnorm), status
      outer     the status each minimizeOneStep returned;  exit: 'iteration_cap' or 'two_step'
      h_eps, delta_factor   the forward difference fell back to sqrt(eps) / delta to factor (x == 0)"""
    summ = canonical_sum if canonical else literal_sum
    dot = lambda a, b: summ(np.asarray(a) * np.asarray(b), wx, wy)
    norm = lambda a: math.sqrt(dot(a, a))
    maxfev = 3 * max_iter
    T = dict(evals=[], steps=[], outer=[], h_eps=False, delta_factor=False)

    def ev(kind, x):
        T["evals"].append((kind, x))
        return np.asarray(F(x), np.float64)

    x = float(x0)
    fvec = ev("init", x)
    nfev, it, par = 1, 1, 0.0
    fnorm = norm(fvec)
    diag = delta = xnorm = r = qtf = 0.0
    iteration, opt_state = 0, 0
    while True:
        # ---- minimizeOneStep
        val1 = ev("base", x)
        h = SQRT_EPS * abs(x)
        if h == 0.0:
            h = SQRT_EPS
            T["h_eps"] = True
        val2 = ev("diff", x + h)
        with np.errstate(all="ignore"):
            fjac = (val2 - val1) / h
        nfev += 2
        wa2n = norm(fjac)
        jtf = dot(fjac, fvec)
        r = wa2n
        qtf = jtf / r if r != 0.0 else float(fvec[0])
        if it == 1:
            diag = 1.0 if wa2n == 0.0 else wa2n
            xnorm = abs(diag * x)
            delta = factor * xnorm
            if delta == 0.0:
                delta = factor
                T["delta_factor"] = True
        gnorm = 0.0
        if fnorm != 0.0 and wa2n != 0.0:
            gnorm = max(gnorm, abs(r * (qtf / fnorm) / wa2n))
        status = -1
        if gnorm <= 0.0:
            status = 4
        else:
            diag = max(diag, wa2n)
            while True:
                # lmpar2, n == 1
                p = _div(qtf, r)
                wa2 = diag * p
                dxnorm = abs(wa2)
                fp = dxnorm - delta
                if fp <= 0.1 * delta:
                    par = 0.0
                else:
                    wa1 = diag * wa2 / dxnorm
                    wa1 = wa1 / r
                    temp = abs(wa1)
                    parl = fp / delta / temp / temp
                    wa1 = r * qtf / diag
                    gn = abs(wa1)
                    paru = gn / delta
                    if paru == 0.0:
                        paru = DWARF / min(delta, 0.1)
                    par = min(max(par, parl), paru)
                    if par == 0.0:
                        par = gn / dxnorm
                    k = 0
                    while True:
                        k += 1
                        if par == 0.0:
                            par = max(DWARF, 0.001 * paru)
                        ds = math.sqrt(par) * diag
                        sdiag2 = r * r + ds * ds
                        sdiag = math.sqrt(sdiag2)
                        p = r * qtf / sdiag2
                        wa2 = diag * p
                        dxnorm = abs(wa2)
                        temp = fp
                        fp = dxnorm - delta
                        if abs(fp) <= 0.1 * delta or (parl == 0.0 and fp <= temp and temp < 0.0) or k == 10:
                            break
                        wa1 = diag * (wa2 / dxnorm)
                        wa1 = wa1 / sdiag
                        temp = abs(wa1)
                        parc = fp / delta / temp / temp
                        if fp > 0.0:
                            parl = max(parl, par)
                        if fp < 0.0:
                            paru = min(paru, par)
                        par = max(parl, par + parc)
                wa1 = -p
                xnew = x + wa1
                pnorm = abs(diag * wa1)
                clip = False
                if it == 1:
                    clip = pnorm < delta
                    delta = min(delta, pnorm)
                wa4 = ev("trial", xnew)
                nfev += 1
                fnorm1 = norm(wa4)
                actred = -1.0
                if 0.1 * fnorm1 < fnorm:
                    actred = 1.0 - (fnorm1 / fnorm) * (fnorm1 / fnorm)
                t1 = abs(r * wa1) / fnorm
                t2 = math.sqrt(par) * pnorm / fnorm
                temp1, temp2 = t1 * t1, t2 * t2
                prered = temp1 + temp2 / 0.5
                dirder = -(temp1 + temp2)
                ratio = actred / prered if prered != 0.0 else 0.0
                step = dict(ratio=ratio, actred=actred, prered=prered, fnorm=fnorm, fnorm1=fnorm1, clip=clip, x=x, xnew=xnew, iter=it)
                if ratio <= 0.25:
                    temp = 0.5
                    step["branch"] = "shrink_half"
                    if actred < 0.0:
                        temp = 0.5 * dirder / (dirder + 0.5 * actred)
                        step["branch"] = "shrink_dirder"
                    if 0.1 * fnorm1 >= fnorm or temp < 0.1:
                        temp = 0.1
                        if 0.1 * fnorm1 >= fnorm:
                            step["branch"] = "shrink_tenth"
                    delta = temp * min(delta, pnorm / 0.1)
                    par /= temp
                elif not (par != 0.0 and ratio < 0.75):
                    delta = pnorm / 0.5
                    par = 0.5 * par
                    step["branch"] = "grow"
                else:
                    step["branch"] = "keep"
                step["accepted"] = ratio >= 1e-4
                if ratio >= 1e-4:
                    x = xnew
                    fvec = wa4
                    xnorm = abs(diag * x)
                    fnorm = fnorm1
                    it += 1
                small = abs(actred) <= ftol and prered <= ftol and 0.5 * ratio <= 1.0
                tiny = abs(actred) <= EPS and prered <= EPS and 0.5 * ratio <= 1.0
                if small and delta <= xtol * xnorm:
                    status = 3
                elif small:
                    status = 1
                elif delta <= xtol * xnorm:
                    status = 2
                elif nfev >= maxfev:
                    status = 5
                elif tiny:
                    status = 6
                elif delta <= EPS * xnorm:
                    status = 7
                elif gnorm <= EPS:
                    status = 8
                step.update(par=par, delta=delta, status=status)
                T["steps"].append(step)
                if status != -1 or ratio >= 1e-4:
                    break
        T["outer"].append(status)
        iteration += 1
        if iteration >= max_iter:
            T["exit"] = "iteration_cap"
            break
        if status in (2, 3):
            if opt_state == 0:
                opt_state = 1
            else:
                T["exit"] = "two_step"
                break
    T.update(x=x, iterations=iteration, nfev=nfev, status=status, fnorm=fnorm, r=r, solved=x > 0.001)
    return T
