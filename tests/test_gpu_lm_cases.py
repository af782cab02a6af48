"""The refinement kernels of the device on the crafted cases of tests/lm_cases.py, through esvo_map_refine, at production
capacities.  Every layout of lm_refine_kernel and the general kernel are held to the canonical oracle bit for bit -- every field
of every returned point, the point count and stats().last_solved:
  wide     one match per wave: any handle, at most 40 000 matches                      test_wide_*
  pair     two waves per match: the wide tests again under ESVO_LM_PAIR=1              test_pair_layout_in_a_child_process
  narrow   four matches per wave, ordered launch: a handle for 45 000 events and a launch of 40 001 to 40 003 matches
           (lm_cases.slot_plan: every match in each position of a wave, beside changing neighbours, the case's longest-running
           match beside three that fail at F(x0), every tail length)                   test_narrow_*
  narrow, slot order: the narrow tests again under ESVO_LM_ORDER=0                      test_narrow_unordered_in_a_child_process
  l2       the Gaussian model's instance of the narrow layout                          test_l2_*
  any      kernels_lm_any.hip at 5 x 5 and 25 x 25                                      test_any_patch_size_*
The oracle is a pure function of the match, so a launch of 40 000 copies is expected to return the oracle's result per distinct
match, assembled in the solver's output order.  What the cases reach is asserted on the CPU (tests/test_lm_cases.py) and, for the
case list as a whole, here."""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import lm_cases as LC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("row", "col", "x", "inv_depth", "scale2", "nu", "variance", "residual", "age", "p_cam", "pose_idx", "seq")
NARROW_EVENTS = 45000   # a handle for more than 40 000 events owns the narrow launch's order buffers
NARROW_N = 40001        # the smallest launch that takes the narrow layout
OPEN = dict(stdvar_vis_threshold=1e150, residual_vis_threshold=1e150, invdepth_min=-1.0, invdepth_max=1e300)   # culling that keeps every valid point


def _oracle(c, **more):
    from oracle import oracle as O
    m = O.OracleMapper(LC.case_params(c, **more), LC.rig())
    m.set_mode(True, True)
    LC.observe_on(m, c)
    return m


@functools.lru_cache(maxsize=None)
def oracle_frame(name, cull):
    """(points, solved count) of the canonical oracle on a case's own match list; computed once, read-only"""
    c = LC.case(name)
    pts, info = _oracle(c).refine(c["matches"], cull=cull, want_info=True)
    pts.setflags(write=False)
    return pts, int(info[:, 3].sum())


@functools.lru_cache(maxsize=None)
def oracle_per_match(name, cull):
    """per distinct match of a case the oracle's point (a 0- or 1-element array) and whether it was solved"""
    c = LC.case(name)
    m = _oracle(c)
    out = []
    for i in range(len(c["matches"])):
        pts, info = m.refine(c["matches"][i:i + 1], cull=cull, want_info=True)
        pts.setflags(write=False)
        out.append((pts, bool(info[0, 3])))
    return out


def _device(c, **more):
    from esvo_amd import lib
    dev = lib.Esvo(LC.case_params(c, **more), LC.rig())
    LC.observe_on(dev, c)
    return dev


def _same(g, o, what):
    assert len(g) == len(o), (what, len(g), len(o))
    for f in FIELDS:
        assert np.array_equal(g[f], o[f]), (what, f, np.flatnonzero((g[f] != o[f]).reshape(len(g), -1).any(axis=1))[:8])


def _check_small(name):
    """a case's own matches in one launch, before and after culling"""
    c = LC.case(name)
    dev = _device(c)
    try:
        for cull in (False, True):
            pts, solved = oracle_frame(name, cull)
            g = dev.refine(c["matches"], cull=cull)
            _same(g, pts, (name, cull))
            assert dev.stats().last_solved == solved and dev.stats().last_points == len(pts), (name, cull)
    finally:
        dev.close()


def _exact_root(v, scale=1.0):
    """a double s with (s * s) * scale == v exactly, or None"""
    s = float(np.sqrt(v / scale))
    for q in LC.around(s, 8):
        if (float(q) * float(q)) * scale == v:
            return float(q)
    return None


def cull_variants(c, pts):
    """parameter sets whose culling thresholds sit exactly on a value of the unculled frame, and on the doubles beside it:
    [(what, overrides, index of the point it is aimed at, whether that point must survive)]"""
    N = LC.case_params(c).patch_size_x * LC.case_params(c).patch_size_y
    out = []
    for j in range(len(pts)):   # stdVar_vis_threshold^2 == variance
        s = _exact_root(float(pts["variance"][j])) if pts["variance"][j] > 0 else None
        if s is not None:
            lo = LC.below(s)
            while lo * lo >= pts["variance"][j]:
                lo = LC.below(lo)
            out += [("var_on", dict(OPEN, stdvar_vis_threshold=s), j, True), ("var_below", dict(OPEN, stdvar_vis_threshold=lo), j, False)]
            break
    for j in range(len(pts)):   # residual_vis_threshold^2 * N == residual
        s = _exact_root(float(pts["residual"][j]), float(N)) if pts["residual"][j] > 0 else None
        if s is not None:
            lo = LC.below(s)
            while (lo * lo) * N >= pts["residual"][j]:
                lo = LC.below(lo)
            out += [("cost_on", dict(OPEN, residual_vis_threshold=s), j, True), ("cost_below", dict(OPEN, residual_vis_threshold=lo), j, False)]
            break
    for j in range(len(pts)):
        x = float(pts["inv_depth"][j])
        if x > 0:
            out += [("min_on", dict(OPEN, invdepth_min=x), j, True), ("min_below", dict(OPEN, invdepth_min=LC.below(x)), j, True),
                    ("min_above", dict(OPEN, invdepth_min=LC.above(x)), j, False),
                    ("max_on", dict(OPEN, invdepth_max=x), j, True), ("max_below", dict(OPEN, invdepth_max=LC.below(x)), j, False),
                    ("max_above", dict(OPEN, invdepth_max=LC.above(x)), j, True)]
            break
    return out


# ---- wide (and, in the child process, pair) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.TDIST_15x7)
def test_wide_layout(name):
    _check_small(name)


@pytest.mark.parametrize("name", LC.TDIST_15x7)
def test_wide_layout_culling_on_a_produced_value(name):
    """pointCulling with a threshold exactly on a variance, a cost and an inverse depth that the unculled run produced, and on
    the doubles beside it: the device keeps and drops what the oracle keeps and drops, and the point aimed at flips"""
    c = LC.case(name)
    base, _ = oracle_frame(name, False)
    variants = cull_variants(c, base)
    if not len(base):
        return
    assert {"min_on", "max_on"} <= {v[0] for v in variants}
    dev = _device(c)
    try:
        for what, over, j, survives in variants:
            p = LC.case_params(c, **over)
            orc = _oracle(c, **over)
            o = orc.refine(c["matches"], cull=True)
            hit = (o["x"] == base["x"][j]).all(axis=1) & (o["inv_depth"] == base["inv_depth"][j]) & (o["pose_idx"] == base["pose_idx"][j])
            assert bool(hit.any()) == survives, (name, what, j)
            dev.set_params(copy.copy(p))
            _same(dev.refine(c["matches"], cull=True), o, (name, what))
    finally:
        dev.close()


def _child(env, select):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", select], cwd=ROOT,
                       env=dict(os.environ, ESVO_DEV_SWITCHES="1", **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]


def test_pair_layout_in_a_child_process():
    """the wide tests with every launch forced into the pair layout (ESVO_LM_PAIR is read at esvo_create)"""
    _child(dict(ESVO_LM_PAIR="1"), "test_wide_layout")


# ---- narrow -----------------------------------------------------------------------------------------------------------------------
def _narrow_setup(name):
    c = LC.case(name)
    n = NARROW_N + LC.NAMES.index(name) % 3   # tails of one, two and three matches in the last wave, over the cases
    k = len(c["matches"])
    plan = LC.slot_plan(k, n, lead=LC.longest(name), fails=range(k - 3, k))
    more = dict(process_event_num=NARROW_EVENTS, max_events_per_tick=NARROW_EVENTS, max_window_points=5 * NARROW_EVENTS)
    return c, plan, more


def _expected(name, plan, cull):
    return LC.assemble(oracle_per_match(name, cull), plan)


def _check_narrow(name, **over):
    c, plan, more = _narrow_setup(name)
    T = LC.case_params(c).num_threads
    matches = LC.tiled(c, plan, T)
    dev = _device(c, **dict(more, **over))
    try:
        for cull in (False, True):
            pts, solved = _expected(name, plan, cull)
            g = dev.refine(matches, cull=cull)
            _same(g, pts, (name, cull, len(plan)))
            assert dev.stats().last_solved == solved, (name, cull)
    finally:
        dev.close()


@pytest.mark.parametrize("name", LC.TDIST_15x7)
def test_narrow_layout(name):
    """the ordered launch in this process; in the child process of the test below, the same in slot order"""
    _check_narrow(name)


def test_narrow_unordered_in_a_child_process():
    """the narrow tests on handles created under ESVO_LM_ORDER=0: the launch takes its slots in grid order, so a wave holds exactly
    the four matches slot_plan put side by side"""
    _child(dict(ESVO_LM_ORDER="0"), "test_narrow_layout")


# ---- l2, other patch sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.L2)
def test_l2_narrow_layout(name):
    _check_small(name)


def test_l2_narrow_layout_full_waves():
    """the Gaussian instance with four different matches per wave and a tail: a few hundred slots are enough, it has one layout"""
    name = "l2_tex"
    c = LC.case(name)
    plan = LC.slot_plan(len(c["matches"]), 4 * 37 + 3, lead=LC.longest(name), fails=range(len(c["matches"]) - 3, len(c["matches"])))
    dev = _device(c)
    try:
        for cull in (False, True):
            pts, solved = _expected(name, plan, cull)
            _same(dev.refine(LC.tiled(c, plan, LC.case_params(c).num_threads), cull=cull), pts, (name, cull))
            assert dev.stats().last_solved == solved
    finally:
        dev.close()


@pytest.mark.parametrize("name", LC.ANY)
def test_any_patch_size(name):
    _check_small(name)


# ---- the case list ----------------------------------------------------------------------------------------------------------------
def test_case_list_covers_the_targets():
    """per the oracle (lm_cases.observe), the Student-t cases at 15 x 7 reach every required target; what is left out is listed
    with its reason in lm_cases.UNREACHED: statuses 6, 7 and 8, patchInterpolation refusing the right patch alone, Tdist_nu at the
    lower end of its window, r^2 outside [2^-100, 2^98]"""
    seen = set()
    for name in LC.TDIST_15x7:
        for o in LC.observe(name):
            seen |= o["tags"]
    assert [t for t in LC.REQUIRED if t not in seen] == []
    assert sorted(LC.UNREACHED) == ["interp_right", "nu_low", "r2_outside", "status6", "status7", "status8"]


def test_handle_refuses_nu_at_the_lower_end_of_the_window():
    """Tdist_nu = 2^-100 and the double below cannot be given to a handle at all (lm_cases.UNREACHED, nu_low)"""
    from esvo_amd import lib
    c = LC.case("solver_tex")
    for nu in (2.0 ** -100, LC.below(2.0 ** -100), 2.0):
        with pytest.raises(lib.EsvoError):
            lib.Esvo(LC.case_params(c, td_nu=nu), LC.rig()).close()
