"""Crafted matches for the inverse-depth refinement (kernels_lm.hip: lm_eval and the lmdif state machine around it, in its wide,
pair and narrow layouts; kernels_lm_any.hip), pushed through esvo_map_refine (tests/test_gpu_lm_cases.py; the cases themselves are
tested on the CPU in tests/test_lm_cases.py).

A stream decides by accident which of the evaluator's rare paths its matches take.  Here every match is put where one of them is
taken: a warped coordinate exactly on a bound of warping or patchInterpolation and on the doubles beside it (place() searches
the neighbouring doubles of the pixel and of the inverse depth with the restated warp of tests/lm_restated.py until the
coordinate IS the target), image pairs whose residuals are all zero, of rounding size in a handful of elements, or non-zero in
exactly as many elements as the collapse shortcut allows and in one more, start points whose trial step leaves the image, and
solver runs picked for the status they end with and the trust-region branches they take.  observe() says what a match really
does: it drives the oracle's residual function through the restated solver (lm_restated.trace, which tests/test_lm_cases.py holds
to the oracle's own solve bit for bit) and classifies every evaluation point with the restated evaluator.  Each case states the
tags its matches were written for, so a case that drifts off its switch point fails as a test of the case.

Small ideal rig, identity observation pose, two poses in the table (the identity and a small translation, so that T_left_virtual
is not always the identity).  Images come from seeded generators and are stored nowhere; built once per process, read-only."""
import functools
import hashlib
import math

import numpy as np

import lm_restated as LR
from esvo_amd import calib, params
from esvo_amd.abi import LSNORM_L2, MATCH_DTYPE

W0, H0 = 240, 180      # the smallest size the suite creates a handle on
FOCAL, BASELINE = 100.0, 0.1   # disparity = 10 x inverse depth
SHIFT = 10             # the right image is the left one moved by this many pixels: aligned at inverse depth 1
T_OBS = np.eye(4)
POSES = np.stack([np.eye(4), np.eye(4)])
POSES[1][:3, 3] = (0.004, -0.002, 0.0)
POSES.setflags(write=False)
STAMPS = np.array([1_000_000_000, 1_000_000_001], np.uint64)
T_NS = 1_000_000_000
NU, SCALE = 2.182, 17.277   # mapping_dsec's
# matches that fail at F(x0) whatever the images hold (left warp: x, y; right warp: x): three of them close every case, so that a
# narrow launch can pair any match with three such neighbours
FAILING = ((3.0, 90.0, 1.0, 0), (120.0, 1.5, 1.0, 1), (12.0, 90.0, 1.0, 0))


@functools.lru_cache(maxsize=None)
def rig():
    return calib.ideal_rig(W0, H0, FOCAL, BASELINE)


def below(v):
    return float(np.nextafter(v, -np.inf))


def above(v):
    return float(np.nextafter(v, np.inf))


# ---- images -----------------------------------------------------------------------------------------------------------------------
def _shifted(wide):
    """(left, right) of a (H, W + 64) image: right[y, x] = left[y, x + SHIFT]"""
    return np.ascontiguousarray(wide[:, :W0]), np.ascontiguousarray(wide[:, SHIFT:SHIFT + W0])


def tex_pair(seed=1, k=9):
    """a smooth texture (uniform noise under a k x k box filter, stretched to 0..255) and itself moved by SHIFT pixels"""
    a = np.random.default_rng(seed).uniform(0, 255, (H0, W0 + 64))
    ker = np.ones(k) / k
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, ker, mode="same"), ax, a)
    a = (a - a.min()) / (a.max() - a.min()) * 255
    return _shifted(np.round(a).astype(np.uint8))


def noise_pair(seed):
    """white noise and itself moved by SHIFT pixels"""
    return _shifted(np.random.default_rng(seed).integers(0, 256, (H0, W0 + 64)).astype(np.uint8))


def indep_pair(seed):
    """two unrelated noise images: no inverse depth aligns them"""
    return noise_pair(seed)[0], noise_pair(seed + 1)[0]


def flat_pair(a, b):
    return np.full((H0, W0), a, np.uint8), np.full((H0, W0), b, np.uint8)


def blob_pair(base, nb, amp, seed, at=(88, 118)):
    """a constant image with an nb x nb block of other values, and itself moved by SHIFT pixels: aligned, the residuals of the few
    patch elements the block reaches are rounding errors of the bilinear weights, every other residual is exactly zero"""
    a = np.full((H0, W0 + 64), base, np.int64)
    a[at[0]:at[0] + nb, at[1]:at[1] + nb] += np.random.default_rng(seed).integers(1, amp + 1, (nb, nb))
    return _shifted(a.astype(np.uint8))


def shortcut_count(wx=15, wy=7, nu=NU):
    """the largest number of non-zero residuals for which the device takes the collapse for granted: floor(0.94 N / (nu + 1))"""
    return int(math.floor(0.94 * wx * wy / (nu + 1)))


def sparse_pair(knz, x2u, x2v, wx=15, wy=7):
    """a black left image and a right one with single pixels of 200 in the (wy + 1) x (wx + 1) source block of a patch at the
    fractional right coordinate (x2u, x2v), chosen so that exactly knz patch elements see one: a pixel inside the block reaches
    2 x 2 elements, one on its first row two, its corner one"""
    ulx, uly = math.floor(x2u) - (wx - 1) // 2, math.floor(x2v) - (wy - 1) // 2
    inner = [(sy, sx) for sy in range(2, wy, 2) for sx in range(2, wx, 2)]
    n4, rest = divmod(knz, 4)
    pix = inner[:n4] + ([(0, 2)] if rest & 2 else []) + ([(0, 0)] if rest & 1 else [])
    if n4 > len(inner):
        raise ValueError(f"{knz} non-zero residuals do not fit a {wx} x {wy} patch this way")
    right = np.zeros((H0, W0), np.uint8)
    for sy, sx in pix:
        right[uly + sy, ulx + sx] = 200
    return np.zeros((H0, W0), np.uint8), right


# ---- placing a warped coordinate --------------------------------------------------------------------------------------------------
def around(v, k):
    """v and the k doubles on either side of it"""
    out, up, dn = [v], v, v
    for _ in range(k):
        up, dn = above(up), below(dn)
        out += [up, dn]
    return np.array(out)


def place(pr, T, rho, axis, k, target, other, span=100, side=0):
    """(coordinate, inverse depth, value) next to (target's preimage, rho) for which coordinate k of the restated warp (0: x1u,
    1: x1v, 2: x2u) IS target: the pixel's `axis` and the inverse depth are searched over their neighbouring doubles, `other` is
    the pixel's other coordinate.  side -1 / +1: where no neighbour gives the target exactly (the warp's own rounding is coarser
    than the doubles beside a small bound), the value nearest to it below / above is taken; the value reached is returned."""
    c = float(target)
    for _ in range(3):
        c += target - LR.warp(pr, (c, other) if axis == 0 else (other, c), T, rho)[k]
    for reach in (span, 4 * span):   # (most targets lie within a few doubles; the wider search serves the few that do not)
        cs, rs = around(c, reach), around(rho, reach)
        C, R = np.meshgrid(cs, rs, indexing="ij")
        v = LR.warp_many(pr, C if axis == 0 else other, other if axis == 0 else C, T, R)[k]
        hit = np.argwhere(v == target)
        if len(hit):
            i, j = hit[np.argmin(hit.sum(axis=1))]
            return float(cs[i]), float(rs[j]), float(target)
    if side:
        d = np.where((v < target) if side < 0 else (v > target), np.abs(v - target), np.inf)
        i, j = np.unravel_index(np.argmin(d), d.shape)
        return float(cs[i]), float(rs[j]), float(v[i, j])
    raise ValueError(f"no pixel and inverse depth near ({c!r}, {rho!r}) warp to {target!r} exactly")


def bounds(wx, wy, W=W0, H=H0):
    """the bounds a single coordinate can decide alone, as (name, pixel axis, warp coordinate, bound, what refuses the coordinate
    [one pixel below, one ulp below, on, one ulp above, one pixel above] the bound; None: the evaluation succeeds).
    The right image lies left of the left one (x2u < x1u), so only the right warp can decide at the left edge and only the left
    one at the right edge; the two cameras share their row, and the left one is asked first.  patchInterpolation's
    `upper-left + size < image` rule refuses the last column and row that warping admits: its bound lies one pixel inside."""
    hx, hy = (wx - 1) // 2, (wy - 1) // 2
    wl, il, wr = "warp_left", "interp_left", "warp_right"
    return (("x2u_low", 0, 2, float(hx), (wr, wr, None, None, None)),
            ("x1u_interp_high", 0, 0, float(W - hx - 1), (None, None, il, il, il)),
            ("x1u_warp_high", 0, 0, float(W - hx), (il, il, il, wl, wl)),
            ("v_low", 1, 1, float(hy), (wl, wl, None, None, None)),
            ("v_interp_high", 1, 1, float(H - hy - 1), (None, None, il, il, il)),
            ("v_warp_high", 1, 1, float(H - hy), (il, il, il, wl, wl)))


OFFSETS = ("-1px", "-1ulp", "on", "+1ulp", "+1px")


def _offsets(b):
    return (b - 1.0, below(b), b, above(b), b + 1.0)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def _matches(lst):
    m = np.zeros(len(lst), MATCH_DTYPE)
    for i, (x, y, rho, pose) in enumerate(lst):
        m["x_left"][i] = (x, y)
        m["inv_depth"][i], m["pose_idx"][i], m["event_idx"][i] = rho, pose, i
        m["disp"][i] = math.floor(FOCAL * BASELINE * rho) if 0 <= rho < 100 else 0.0   # (read by the narrow launch's ordering only)
        m["cost"][i] = 0.05
    return m


def _case(pair, lst, tags=None, over=None, expect=None, ub=(), last_bit=(), doc=""):
    """tags: {tag: match indices that must show it (observe)};  expect: {match index: (warp coordinate, value it must have at
    F(x0), what refuses it, the tag observe() gives the match when both hold)};  ub: matches on which the reference itself is
    undefined;  last_bit: matches whose outcome hangs on the last bit of cam2World (knife_edge) for another reason than a bound;
    both are kept out of the pin to the reference"""
    left, right = pair
    lst = list(lst)
    n_own = len(lst)
    lst += FAILING
    m = _matches(lst)
    for a in (left, right, m):
        a.setflags(write=False)
    return dict(left=left, right=right, matches=m, n_own=n_own, tags=tags or {}, over=over or {}, expect=expect or {}, ub=frozenset(ub), last_bit=frozenset(last_bit),
                doc=doc)


def problem(c):
    """the restated evaluator's view of a case"""
    p = case_params(c)
    return LR.Problem(rig(), c["left"], c["right"], p.patch_size_x, p.patch_size_y, p.td_nu, p.td_scale, p.ls_norm == LSNORM_L2)


def t_left_virtual(pose):
    return LR.t_left_virtual(T_OBS, POSES[pose])


def _borders(wx=15, wy=7, poses=(0, 1), l2=False):
    """Failure fill at F(x0): for every bound one coordinate can decide alone (bounds()) a match whose deciding coordinate lies
    one pixel below the bound, on the double below it, on it, on the double above it and one pixel above; under the identity and
    under the translated pose.  The other coordinates stay well inside, at fractional positions.  (Where the warp's rounding
    is coarser than the doubles beside a small bound -- x2u = 2 and v = 2 of the 5 x 5 patch -- the nearest value it can give on
    that side stands in for the neighbouring double: tags `...:-near`, `...:+near`.)"""
    pair = tex_pair()
    over = dict(patch_size_x=wx, patch_size_y=wy, **({"ls_norm": LSNORM_L2} if l2 else {}))
    pr = LR.Problem(rig(), pair[0], pair[1], wx, wy, NU, SCALE, l2)
    lst, expect, tags = [], {}, {}
    for pose in poses:
        T = t_left_virtual(pose)
        for name, axis, k, b, refuses in bounds(wx, wy):
            for off, target, why in zip(OFFSETS, _offsets(b), refuses):
                other = 90.25 if axis == 0 else 120.25
                c, rho, reached = place(pr, T, 1.0, axis, k, target, other, side={"-1ulp": -1, "+1ulp": 1}.get(off, 0))
                expect[len(lst)] = (k, reached, why, f"{name}:{off}" if reached == target else f"{name}:{off[0]}near")
                tags.setdefault(f"init_{why}" if why else "init_ok", []).append(len(lst))
                tags.setdefault(expect[len(lst)][3], []).append(len(lst))
                lst.append(((c, other) if axis == 0 else (other, c)) + (rho, pose))
    return _case(pair, lst, tags, over, expect, doc=_borders.__doc__)


def _trial_fill():
    """The right warp leaves the image as the inverse depth grows.  Match 0: F(x0) succeeds with x2u on the double above the
    bound, F(x0 + h) takes the fill -- the Jacobian is (fill - f) / h, the trial is rejected and the inner loop repeats.  Matches
    1 and 2: F(x0) and F(x0 + h) succeed, a trial point takes the fill: 0.1 |F(trial)| >= |F|, the trust region shrinks to a
    tenth.  Found by a seeded search over start points beside the left edge; frozen here."""
    pair = tex_pair()
    pr = LR.Problem(rig(), pair[0], pair[1])
    c, rho, _ = place(pr, t_left_virtual(0), 1.0, 0, 2, above(7.0), 90.25)
    lst = [(c, 90.25, rho, 0), (16.591649672068705, 54.19690995847508, 0.9579636388172466, 0),
           (16.77045695419234, 53.96503178425916, 0.9769943314728358, 0)]
    tags = {"diff_fill_only": [0], "rejected_twice": [0, 2], "trial_fill_only": [1, 2], "shrink_tenth": [1, 2], "status5": [1], "maxfev_decides": [1]}
    return _case(pair, lst, tags, doc=_trial_fill.__doc__)


def _flat(a, b, lst, tags, doc):
    return _case(flat_pair(a, b), lst, tags, doc=doc)


def _solver(kind):
    """Solver runs picked from seeded pools for what they do (observe): statuses 1, 2, 3, 4 and 5; a first 2 or 3 that continues
    and a second that ends; one 2 or 3 and then the iteration cap; the evaluation budget deciding an inner loop; steps rejected
    twice in a row; and the trust-region branches -- shrink by the dirder formula, by a half, keep, grow, the first step's clip."""
    rng = np.random.default_rng(0 if kind == "tex" else 5)
    cand = lambda n, lo, hi: [(float(rng.uniform(30, 200)), float(rng.uniform(10, 160)), float(rng.uniform(lo, hi)), int(rng.integers(0, 2))) for _ in range(n)]
    if kind == "tex":
        pool = cand(40, 0.6, 1.5)
    else:   # (four pools drawn one after the other from one generator)
        pool = dict(zip(("noise", "indep", "unused", "far"), (cand(60, 0.3, 2.0), cand(60, 0.3, 2.0), cand(60, 0.3, 2.0), cand(60, 0.05, 4.0))))[kind]
    pair = dict(tex=tex_pair, noise=lambda: noise_pair(2), indep=lambda: indep_pair(3), far=lambda: tex_pair(8, 9))[kind]()
    pick, tags = {
        "tex": ([0, 1, 8, 16, 23, 27],
                {'status5': [0], 'saw5': [0], 'exit_iteration_cap': [0, 1, 3, 4, 5], 'grow': [0, 1, 2, 3, 4, 5], 'clip': [0, 1, 2, 3, 4, 5], 'status4': [1],
                 'one_23_then_cap': [1, 4], 'status2': [2, 5], 'two_step_second_ends': [2], 'shrink_dirder': [2], 'rejected': [2], 'status1': [3],
                 'saw1': [3, 4], 'status3': [4], 'shrink_half': [5]}),
        "noise": ([1, 2, 15, 23, 42, 48],
                  {'status4': [0], 'one_23_then_cap': [0, 3], 'exit_iteration_cap': [0, 1, 3, 4], 'status1': [1], 'saw1': [1, 3, 5], 'status2': [2],
                   'saw5': [2, 4], 'two_step_second_ends': [2, 5], 'shrink_dirder': [2], 'rejected_twice': [2], 'status3': [3, 5], 'status5': [4],
                   'shrink_half': [5]}),
        "indep": ([7, 8, 11, 28, 54],
                  {'status2': [0], 'saw1': [0, 2, 3, 4], 'two_step_second_ends': [0, 2], 'status5': [1], 'saw5': [1, 4], 'exit_iteration_cap': [1, 3, 4],
                   'status3': [2, 3], 'shrink_half': [2], 'one_23_then_cap': [3], 'status1': [4], 'maxfev_decides': [4], 'shrink_dirder': [4],
                   'rejected_twice': [4]}),
        "far": ([1, 4, 11, 14, 22],
                {'status2': [0], 'two_step_second_ends': [0], 'status5': [1], 'saw5': [1, 3], 'exit_iteration_cap': [1, 2, 3, 4], 'maxfev_decides': [1, 3],
                 'shrink_dirder': [1, 3, 4], 'rejected_twice': [1, 3], 'status4': [2], 'status1': [3], 'saw1': [3, 4], 'one_23_then_cap': [3, 4],
                 'status3': [4], 'shrink_half': [4]}),
    }[kind]
    return _case(pair, [pool[i] for i in pick], tags, doc=_solver.__doc__)


def _builders():
    b = {"borders": _borders, "trial_fill": _trial_fill}
    b["zero"] = lambda: _flat(100, 100, [(50.3, 60.7, 0.7, 0), (100.5, 90.5, 1.0, 1), (120.0, 90.0, 1.0, 0), (60.1, 50.9, 0.001, 0), (60.1, 50.9, above(0.001), 0)],
                              {"zero_residuals": [0, 1, 2, 3, 4], "status4": [0, 1, 2, 3, 4], "exit_iteration_cap": [0], "unsolved": [3], "solved": [4]},
                              "Two equal constant images: every residual is exactly zero at every evaluation (knz = 0, |F| = 0, r = 0, qtf from "
                              "fvec[0], variance 0; status 4 ten times, until the iteration cap).  Start points exactly 0.001 (x <= 0.001: "
                              "unsolved, n_solved unchanged) and on the double above (solved).")
    b["one_pass"] = lambda: _flat(100, 117, [(50.3, 60.7, 0.7, 0), (100.5, 90.5, 1.0, 1)], {"iters1": [0, 1], "status4": [0, 1]},
                                  "Constant images 100 and 117: |r| = 17 = about Tdist_scale everywhere, the scale loop ends after one pass; the "
                                  "gradient is exactly zero with |F| > 0.")
    b["flat_right"] = lambda: _case((tex_pair()[0], flat_pair(100, 100)[1]), [(120.0, 90.0, 1.0, 0), (50.3, 60.7, 0.7, 0), (100.5, 90.5, 1.0, 1)],
                                    {"status4": [0, 1], "exit_iteration_cap": [0, 1, 2], "iters6": [0, 1, 2], "unsolved": [1], "rejected_twice": [2], "saw5": [2]},
                                    last_bit=(0, 1, 2),
                                    doc="The texture against a constant right image.  Identity pose: the left patch does not move with the inverse "
                                        "depth, the gradient is exactly zero on non-zero residuals, status 4 repeats until the iteration cap (match 1 "
                                        "first steps to a negative inverse depth: unsolved).  Translated pose: the left patch moves; rejected steps, "
                                        "40 evaluations.  The whole Jacobian is the left coordinate's dependence on the inverse depth: exactly zero "
                                        "under the closed-form cam2World, a rounding residue under the reference's per-call 4 x 4 inverse (last_bit).")
    for name, (base, nb, amp) in dict(blob100=(100, 4, 60), blob1=(1, 3, 1), blob8=(8, 4, 4)).items():
        b[name] = functools.partial(_blob, base, nb, amp)
    b["sparse_at"] = functools.partial(_sparse, 0)
    b["sparse_above"] = functools.partial(_sparse, 1)
    for kind in ("tex", "noise", "indep", "far"):
        b[f"solver_{kind}"] = functools.partial(_solver, kind)
    b["extreme"] = _extreme
    for k, nu in enumerate((below(2.0 ** 100), 2.0 ** 100)):
        b[f"nu_high{k}"] = functools.partial(_nu, nu)
    # the Gaussian model (no scale loop, no weights): the narrow layout's L2 instance
    b["l2_borders"] = functools.partial(_borders, 15, 7, (0,), True)
    b["l2_zero"] = lambda: _l2(b["zero"](), {"zero_residuals": [0, 1, 2, 3, 4], "unsolved": [3], "solved": [4]})
    b["l2_tex"] = lambda: _l2(_solver("tex"), {})
    b["l2_flat_right"] = lambda: _l2(b["flat_right"](), {"status4": [0]})
    # other patch sizes: kernels_lm_any.hip
    for wx, wy in ((5, 5), (25, 25)):
        s = f"{wx}x{wy}"
        b[f"any{s}_borders"] = functools.partial(_borders, wx, wy, (0,))
        b[f"any{s}_tex"] = functools.partial(_any_tex, wx, wy)
        b[f"any{s}_zero"] = functools.partial(_any_of, "zero", wx, wy, {"zero_residuals": [0, 1, 2, 3, 4], "unsolved": [3], "solved": [4]})
        # (a one-pixel block for the 5 x 5 patch: the four elements it reaches are fewer than the seven the shortcut allows)
        b[f"any{s}_blob"] = functools.partial(_blob, 100, 1 if wx == 5 else 4, 60, wx, wy, (90, 120) if wx == 5 else (88, 118), int(wx == 5))
        b[f"any{s}_sparse_at"] = functools.partial(_sparse, 0, wx, wy)
        b[f"any{s}_sparse_above"] = functools.partial(_sparse, 1, wx, wy)
    b["any5x5_l2"] = lambda: _l2(_any_tex(5, 5), {})
    return b


def _blob(base, nb, amp, wx=15, wy=7, at=(88, 118), who=0):
    """A few rounding-size residuals (aligned pair, fractional pixel: |r| < 1e-6 in the elements the block reaches, exactly zero
    elsewhere): too small for the shortcut, so the literal loop runs, contracts for ever, leaves [2^-100, 2^100] -- the tight loop
    hands over to the general one -- and ends on sum == 0.  Match 0 starts aligned (residuals of rounding size only at x + h),
    match 1 three percent off."""
    tags = {"tiny_residuals": [who], "on_zero": [who], "handover": [who]}
    return _case(blob_pair(base, nb, amp, nb, at), [(120.3, 90.6, 1.0, 0), (120.3, 90.6, 0.97, 0)], tags, dict(patch_size_x=wx, patch_size_y=wy), doc=_blob.__doc__)


def _sparse(extra, wx=15, wy=7):
    """Exactly floor(0.94 N / (nu + 1)) non-zero residuals, none below 1e-6 (the device takes the collapse for granted; the
    oracle's literal loop runs thousands of passes to reach it), and one more (the loop converges)."""
    k = shortcut_count(wx, wy) + extra
    pair = sparse_pair(k, 110.3, 90.6, wx, wy)
    tags = {f"init_knz{k}": [0], ("init_no_shortcut" if extra else "init_shortcut"): [0]}
    if not extra:
        tags["collapse"] = [0]
    elif wx * wy == 105:
        tags["iters6"] = [0]
    return _case(pair, [(120.3, 90.6, 1.0, 0)], tags, dict(patch_size_x=wx, patch_size_y=wy), doc=_sparse.__doc__)


def _extreme():
    """Inverse depth 1e-31: the projection's common divisor 1e31 lies outside the shared-reciprocal window, four plain quotients.
    x0 = 0: h = sqrt(eps), delta = factor, a NaN coordinate (undefined in the reference; defined here: the fill).  x0 < 0."""
    lst = [(120.3, 90.6, 1e-31, 0), (120.3, 90.6, 0.0, 0), (120.3, 90.6, -0.5, 0), (120.3, 90.6, 1e-31, 1), (60.0, 50.0, -1e-3, 1)]
    tags = {"plain_division": [0, 3], "unsolved": [0, 1, 3], "init_nonfinite": [1], "h_eps": [1], "delta_factor": [1], "keep": [1], "negative_start": [2, 4],
            "status5": [0, 2, 3, 4], "maxfev_decides": [0, 3]}
    return _case(tex_pair(), lst, tags, ub=(1,), doc=_extreme.__doc__)


def _nu(nu):
    """Tdist_nu just inside and just outside the upper end of [2^-100, 2^100): outside, no evaluation is tight.  (The lower end
    cannot be reached: a handle refuses nu <= 2, where the reference's variance nu / (nu - 2) is negative or undefined.)"""
    lst = [(120.3, 90.6, 0.9, 0), (60.2, 40.1, 1.05, 1), (16.900001, 90.25, 0.99, 0)]
    return _case(tex_pair(), lst, {"nu_tight" if nu < 2.0 ** 100 else "nu_not_tight": [0, 1, 2]}, dict(td_nu=nu), doc=_nu.__doc__)


def _l2(c, tags):
    """a case under LSnorm l2"""
    return dict(c, over=dict(c["over"], ls_norm=LSNORM_L2), tags=tags)


def _any_tex(wx, wy):
    """ordinary solves on the texture at another patch size"""
    c = _solver("tex")
    return dict(c, over=dict(patch_size_x=wx, patch_size_y=wy), tags={})


def _any_of(name, wx, wy, tags):
    c = _BUILDERS[name]()
    return dict(c, over=dict(c["over"], patch_size_x=wx, patch_size_y=wy), tags=tags)


_BUILDERS = _builders()
NAMES = list(_BUILDERS)
TDIST_15x7 = [n for n in NAMES if not n.startswith(("l2_", "any"))]
L2 = [n for n in NAMES if n.startswith("l2_")]
ANY = [n for n in NAMES if n.startswith("any")]


@functools.lru_cache(maxsize=None)
def case(name):
    c = dict(_BUILDERS[name]())
    c["name"] = name
    return c


def case_params(c, **more):
    """ParamsStruct of a case: mapping_dsec without the Time-Surface blur, a small event ring, the case's overrides"""
    p, _ = params.make_params(params.PRESETS["mapping_dsec"], rig(), event_ring_capacity=4096, smooth_time_surface=0, **dict(c["over"], **more))
    return p


def observe_on(mapper, c):
    mapper.set_observation(T_NS, c["left"], c["right"], T_OBS)
    mapper.set_poses(STAMPS, POSES.reshape(2, 16))


def knife_edge(c):
    """the matches whose start point warps to within eight doubles of a bound of warping or patchInterpolation.  Which side of
    the bound such a coordinate falls on is decided by the last bit of cam2World, which the reference computes by inverting a 4 x 4
    matrix with Eigen on every call (CameraSystem.cpp:121-139) and the oracle and the device by the closed form
    z K^-1 [u v 1]^T - K^-1 t: equal to 1e-12, not to the bit.  These matches are what the device is held to the oracle on; the
    reference cannot say which side is right, so they are kept out of the pin to the reference."""
    pr = problem(c)
    hx, hy = (pr.wx - 1) // 2, (pr.wy - 1) // 2
    bx, by = (hx, pr.W - hx - 1, pr.W - hx), (hy, pr.H - hy - 1, pr.H - hy)
    out = set()
    for i, m in enumerate(c["matches"]):
        x = LR.warp(pr, (float(m["x_left"][0]), float(m["x_left"][1])), t_left_virtual(int(m["pose_idx"])), float(m["inv_depth"]))
        near = lambda v, b: abs(v - b) <= 8 * np.spacing(float(b))
        if any(near(x[k], b) for k in (0, 2) for b in bx) or any(near(x[k], b) for k in (1, 3) for b in by):
            out.add(i)
    return frozenset(out)


def pinned_matches(c):
    """the matches of a case that are held to the reference: all but those on which the reference is undefined (ub) and those
    whose side of a bound hangs on cam2World's last bit (knife_edge)"""
    out = c["ub"] | c["last_bit"] | knife_edge(c)
    keep = np.array([i not in out for i in range(len(c["matches"]))])
    return np.ascontiguousarray(c["matches"][keep])


def input_digest(c):
    """sha256 over what a case feeds the solver: both images, the matches, the poses, and the parameters the refinement reads"""
    p = case_params(c)
    h = hashlib.sha256()
    for a in (c["left"], c["right"], c["matches"], POSES, T_OBS, STAMPS):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.array([p.patch_size_x, p.patch_size_y, p.ls_norm, p.lm_max_iteration, p.num_threads, W0, H0], np.int64).tobytes())
    h.update(np.array([p.td_nu, p.td_scale, FOCAL, BASELINE], np.float64).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# ---- what a match does ------------------------------------------------------------------------------------------------------------
def trace_tags(t):
    """tags of one restated solver run (lm_restated.trace)"""
    s = {f"status{t['status']}", "exit_" + t["exit"], "solved" if t["solved"] else "unsolved"}
    s |= {f"saw{v}" for v in t["outer"] if v > 0}
    run = 0
    for st in t["steps"]:
        s.add(st["branch"])
        if st["clip"]:
            s.add("clip")
        run = 0 if st["accepted"] else run + 1
        if run:
            s.add("rejected")
        if run >= 2:
            s.add("rejected_twice")   # ratio < 1e-4 repeated the inner loop at least twice
        if st["status"] == 5 and not st["accepted"]:
            s.add("maxfev_decides")   # the inner loop would have gone on: nfev >= maxfev ended it
    n23 = sum(v in (2, 3) for v in t["outer"])
    if t["exit"] == "two_step":
        s.add("two_step_second_ends")
    elif n23 == 1:
        s.add("one_23_then_cap")
    s |= {k for k in ("h_eps", "delta_factor") if t[k]}
    return s


def eval_tags(pr, evals):
    """tags of the evaluation points of one solve: [(kind, restated evaluation)]"""
    s = set()
    N = pr.wx * pr.wy
    k0 = int(math.floor(0.94 * N / (pr.nu + 1)))
    init = evals[0][1]
    s.add(f"init_{init['fail']}" if init["fail"] else "init_ok")
    first_diff = next(e for k, e in evals if k == "diff")
    trials = [e for k, e in evals if k == "trial"]
    if init["ok"] and not first_diff["ok"]:
        s.add("diff_fill_only")
    if init["ok"] and first_diff["ok"] and any(not e["ok"] for e in trials):
        s.add("trial_fill_only")
    if pr.l2:
        if init["ok"] and not init["f"].any():
            s.add("zero_residuals")
        return s
    if init["ok"]:
        s.add(f"init_knz{init['knz']}")
        s.add("init_shortcut" if init["shortcut"] else "init_no_shortcut")
        if all(e["ok"] and e["knz"] == 0 for _, e in evals):
            s.add("zero_residuals")
    nu_mid = LR.LO <= pr.nu < LR.HI
    for _, e in evals:
        if not e["ok"]:
            continue
        if e["knz"] and e["minabs"] < 1e-6 and e["knz"] <= k0:
            s.add("tiny_residuals")      # few non-zero residuals, too small for the shortcut: the literal loop runs
        if e["on_zero"] and e["knz"] and not e["shortcut"]:
            s.add("on_zero")
        if e["shortcut"] and e["on_zero"] and e["iters"] > 1000:
            s.add("collapse")            # the literal loop is seen to reach what the device takes for granted
        if e["left_window"] and not e["shortcut"] and nu_mid and e["minabs"] ** 2 >= LR.LO and e["r2max"] < 2.0 ** 98:
            s.add("handover")            # a tight evaluation whose running scale leaves the window part-way
        if e["iters"] == 1:
            s.add("iters1")
        if e["iters"] >= 6 and not e["on_zero"]:
            s.add("iters6")
        s.add("nu_tight" if nu_mid else "nu_not_tight")
    return s


@functools.lru_cache(maxsize=None)
def observe(name):
    """per match of a case: dict(trace, evals [(kind, x, restated evaluation)], tags) -- the canonical oracle's residual function
    driven through the restated solver, every point it visits classified by the restated evaluator"""
    from oracle import oracle as O
    c = case(name)
    p = case_params(c)
    o = O.OracleMapper(p, rig())
    o.set_mode(True, True)
    observe_on(o, c)
    pr = problem(c)
    out = []
    for i, m in enumerate(c["matches"]):
        coor, pose, x0 = (float(m["x_left"][0]), float(m["x_left"][1])), int(m["pose_idx"]), float(m["inv_depth"])
        t = LR.trace(lambda v: o.eval_residual(coor, pose, v)[0], x0, p.lm_max_iteration, p.patch_size_x, p.patch_size_y, canonical=True)
        T = t_left_virtual(pose)
        cache = {}
        evals = []
        for kind, x in t["evals"]:
            if x not in cache:
                cache[x] = LR.evaluate(pr, coor, T, x)
            evals.append((kind, x, cache[x]))
        tags = trace_tags(t) | eval_tags(pr, [(k, e) for k, _, e in evals])
        with np.errstate(all="ignore"):
            if not (LR.LO <= abs(1.0 / np.float64(x0)) <= LR.HI):
                tags.add("plain_division")
        if x0 < 0:
            tags.add("negative_start")
        if i in c["expect"]:   # a placed coordinate: the restated warp gives exactly the intended double, and the intended test refuses it
            k, target, why, label = c["expect"][i]
            if evals[0][2]["x"][k] == target and evals[0][2]["fail"] == why:
                tags.add(label)
        out.append(dict(trace=t, evals=evals, tags=tags))
    return out


def longest(name):
    """the match of a case that works longest: most scale-loop passes over its evaluations, then most evaluations"""
    obs = observe(name)
    return max(range(len(obs)), key=lambda i: (sum(e["iters"] for _, _, e in obs[i]["evals"]), obs[i]["trace"]["nfev"]))


# The targets the case list has to reach (tests/test_lm_cases.py and tests/test_gpu_lm_cases.py assert that it does), as tags of
# observe() over the Student-t cases at 15 x 7.
REQUIRED = (
    "init_warp_left", "init_warp_right", "init_interp_left",             # failure fill at F(x0), by each test that can decide alone
    "diff_fill_only", "trial_fill_only", "rejected_twice",               # fill only at x + h / only at a trial point
    "zero_residuals",                                                    # knz = 0, |F| = 0
    f"init_knz{shortcut_count()}", "init_shortcut", "collapse", f"init_knz{shortcut_count() + 1}", "init_no_shortcut",   # both sides of 0.94
    "tiny_residuals", "on_zero", "handover",                             # minabs < 1e-6; ends on sum == 0; tight loop hands over
    "iters1", "iters6",                                                  # scale loop: one pass, six and more
    "nu_tight", "nu_not_tight",                                          # Tdist_nu below and at 2^100
    "plain_division", "h_eps", "delta_factor", "init_nonfinite", "negative_start",
    "status1", "status2", "status3", "status4", "status5", "saw1", "saw5",
    "two_step_second_ends", "one_23_then_cap", "exit_iteration_cap", "maxfev_decides",
    "shrink_dirder", "shrink_tenth", "shrink_half", "keep", "grow", "clip",
    "unsolved", "solved",
) + tuple(f"{b[0]}:{off}" for b in bounds(15, 7) for off in OFFSETS)
# What cannot be reached, and why (tests/test_lm_cases.py asserts that no case reaches them either):
UNREACHED = {
    "status6": "|actred| <= eps and prered <= eps imply both <= ftol: status 1 or 3 is returned first",
    "status7": "delta <= eps xnorm implies delta <= xtol xnorm: status 2 or 3 is returned first",
    "status8": "needs 0 < |J^T f| / (|J| |f|) <= 2.2e-16 -- a Jacobian orthogonal to the residuals to the last bit but not exactly; "
               "no pair of u8 images found gives it (an exactly orthogonal one gives gnorm = 0: status 4)",
    "interp_right": "patchInterpolation refuses the right patch only at the right edge or on rows, where the left patch (x1u > x2u, "
                    "same row, asked first) is refused before it",
    "nu_low": "Tdist_nu at 2^-100: a handle refuses nu <= 2 (the reference's variance nu / (nu - 2) is negative there)",
    "r2_outside": "r^2 outside [2^-100, 2^98] with u8 images needs |r| < 9e-16 (below the rounding of any bilinear sum that is not "
                  "exactly zero at the intensities tried) or |r| > 5e14",
}


# ---- the narrow launch: many copies of a case's matches, arranged by solver slot --------------------------------------------------
def stride_order(n, T):
    """slot -> item of the reference's thread-stride order (DepthProblemSolver.cpp:75-90)"""
    return np.concatenate([np.arange(t, n, T) for t in range(T)])


def slot_plan(k, n, lead=None, fails=None):
    """which of k distinct matches each of n solver slots holds: waves of four consecutive slots that run (b, b + 1, b + 2, b + 3)
    mod k in all four rotations for every b -- every match takes each of a wave's four positions and sits beside six different
    neighbours (three where k = 4) -- behind one wave that holds `lead` with the three matches `fails`; repeated up to n slots."""
    waves = []
    if lead is not None:
        waves.append([lead] + list(fails))
    for rot in range(4):
        for b in range(k):
            w = [(b + j) % k for j in range(4)]
            waves.append(w[rot:] + w[:rot])
    flat = np.array([m for w in waves for m in w], np.int64)
    return np.resize(flat, n)


def tiled(c, plan, T):
    """the match list whose solver slots hold plan[s] of the case's matches (slot s solves item stride_order[s])"""
    m = np.zeros(len(plan), MATCH_DTYPE)
    m[stride_order(len(plan), T)] = c["matches"][plan]
    m["event_idx"] = np.arange(len(plan))
    return m


def assemble(per_match, plan):
    """the frame a launch over plan must return, from the oracle's result per distinct match -- [(0- or 1-element point array,
    solved)] -- in the solver's output order (slot order, unsolved and culled slots closed up) -> (points, solved count)"""
    got = [per_match[i][0] for i in plan if len(per_match[i][0])]
    pts = np.concatenate(got) if got else np.zeros(0, per_match[0][0].dtype)
    pts["seq"] = np.arange(len(pts))
    return pts, int(sum(per_match[i][1] for i in plan))
