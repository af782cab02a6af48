"""The scale-loop guard of the LM refinement (ParamsStruct.lm_scale_pass_limit, esvo_map_lm_stats) on the device, through
esvo_map_refine on the crafted cases of tests/lm_cases.py as tests/test_gpu_lm_cases.py runs them, and through whole ticks.

Every field of every returned point is held bit for bit to the canonical oracle's per-match results, assembled in the solver's
output order with the abandoned matches left out (lm_guard.reduced); which matches a limit abandons and what the counters must
read come from the restated evaluator (tests/lm_guard.py; asserted of the cases on the CPU in tests/test_lm_guard_cases.py).
  count only   ESVO_LM_SCALE_COUNT_ONLY: the oracle's frame, the helper's counters             test_count_only
  wide         one match per wave, (case, limit) pairs                                          test_wide_limits
  narrow       four matches per wave, ordered launch: 40 001 to 40 003 matches laid out by lm_cases.slot_plan -- every match in each
               wave position beside changing neighbours, an abandoned match among them          test_narrow_*
  narrow, slot order: the same in a child process under ESVO_LM_ORDER=0                          test_narrow_unordered_in_a_child_process
  general      kernels_lm_any.hip at 5 x 5 and 25 x 25                                           test_general_kernel_limits
  pair         a forced ESVO_LM_PAIR=1 loses to the guard                                        test_forced_pair_layout_loses_to_the_guard
  ticks        esvo_map_tick on a synthetic 346 x 260 stream                                     test_whole_ticks_*"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import lm_cases as LC
import lm_guard as G
from test_gpu_lm_cases import NARROW_EVENTS, NARROW_N, _device, _same, oracle_frame, oracle_per_match

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTALS = (("total_passes", "last_passes"), ("total_evals", "last_evals"), ("total_shortcut_evals", "last_shortcut_evals"),
          ("total_abandoned", "last_abandoned"))


def _read(st):
    return {k: int(getattr(st, k)) for k in G.FIELDS}


def _expected_frame(name, limit, plan, cull):
    return LC.assemble(G.reduced(oracle_per_match(name, cull), G.abandoned(name, limit)), plan)


def _check(name, limit, plan=None, matches=None, **more):
    """a launch over plan (None: the case's own matches) under a limit, before and after culling: frame, solved and point counts,
    every counter"""
    c = LC.case(name)
    if plan is None:   # the case's own list: slot s solves match stride_order[s], and the frame comes in slot order
        plan = LC.stride_order(len(c["matches"]), LC.case_params(c).num_threads)
    matches = c["matches"] if matches is None else matches
    want = G.counters(name, limit, plan)
    dev = _device(c, lm_scale_pass_limit=limit, **more)
    try:
        for cull in (False, True):
            pts, solved = _expected_frame(name, limit, plan, cull)
            g = dev.refine(matches, cull=cull)
            _same(g, pts, (name, limit, cull, len(plan)))
            s, ls = dev.stats(), dev.lm_stats()
            assert s.last_solved == solved and s.last_points == len(pts), (name, limit, cull, s.last_solved, solved)
            print(f"{name} limit {limit} cull {cull}: device {_read(ls)}  expected {want}")
            assert ls.enabled == 1 and _read(ls) == want, (name, limit, cull)
    finally:
        dev.close()


# ---- count only ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["solver_noise", "one_pass", "zero", "sparse_at", "sparse_above", "blob1", "any5x5_blob", "any25x25_blob"])
def test_count_only(name):
    c = LC.case(name)
    want = G.counters(name, G.COUNT_ONLY)
    assert want["last_abandoned"] == 0
    dev = _device(c, lm_scale_pass_limit=G.COUNT_ONLY)
    try:
        for k, cull in enumerate((False, True)):
            pts, solved = oracle_frame(name, cull)
            _same(dev.refine(c["matches"], cull=cull), pts, (name, cull))
            assert dev.stats().last_solved == solved
            ls = dev.lm_stats()
            print(f"{name} count only: device {_read(ls)}  expected {want}")
            assert ls.enabled == 1 and _read(ls) == want, (name, cull)
            for tot, last in TOTALS:   # two calls: the totals add up
                assert getattr(ls, tot) == (k + 1) * want[last], (name, tot)
        dev.reset()
        ls = dev.lm_stats()
        assert ls.enabled == 1 and all(getattr(ls, f) == 0 for f, _ in ls._fields_ if f != "enabled"), name
    finally:
        dev.close()


# ---- wide --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,limit,gone", G.WIDE_LIMITS)
def test_wide_limits(name, limit, gone):
    assert G.abandoned(name, limit) == gone
    _check(name, limit)


# ---- narrow ------------------------------------------------------------------------------------------------------------------------
def _narrow(name, limit):
    c = LC.case(name)
    n = NARROW_N + LC.NAMES.index(name) % 3
    k = len(c["matches"])
    plan = LC.slot_plan(k, n, lead=LC.longest(name), fails=range(k - 3, k))
    more = dict(process_event_num=NARROW_EVENTS, max_events_per_tick=NARROW_EVENTS, max_window_points=5 * NARROW_EVENTS)
    _check(name, limit, plan, LC.tiled(c, plan, LC.case_params(c).num_threads), **more)


def test_narrow_tail_lengths_differ():
    assert {(NARROW_N + LC.NAMES.index(n) % 3) % 4 for n in ("solver_noise", "blob1", "blob8")} == {1, 2, 3}


@pytest.mark.parametrize("name,limit", [("solver_noise", 7), ("blob1", 64), ("solver_noise", G.COUNT_ONLY), ("blob8", 64)])
def test_narrow_layout(name, limit):
    """the ordered launch in this process; in the child process of the test below, the same in slot order.  The neighbours of an
    abandoned group keep their bits: the frame is the oracle's without the abandoned matches, field for field."""
    _narrow(name, limit)


def _child(env, select):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", select], cwd=ROOT,
                       env=dict(os.environ, ESVO_DEV_SWITCHES="1", **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]


def test_narrow_unordered_in_a_child_process():
    """handles created under ESVO_LM_ORDER=0: a wave holds exactly the four matches slot_plan put side by side"""
    _child(dict(ESVO_LM_ORDER="0"), "test_narrow_layout")


# ---- the general kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,limit,gone", G.ANY_LIMITS)
def test_general_kernel_limits(name, limit, gone):
    assert G.abandoned(name, limit) == gone
    _check(name, limit)


# ---- off, and the pair layout ------------------------------------------------------------------------------------------------------
def test_limit_zero_counts_nothing():
    name = "solver_noise"
    c = LC.case(name)
    dev = _device(c)
    try:
        assert dev.params.lm_scale_pass_limit == 0
        for cull in (False, True):
            pts, solved = oracle_frame(name, cull)
            _same(dev.refine(c["matches"], cull=cull), pts, (name, cull))
            assert dev.stats().last_solved == solved
            ls = dev.lm_stats()
            assert all(getattr(ls, f) == 0 for f, _ in ls._fields_)
        # switched on between two launches, and off again
        p = LC.case_params(c, lm_scale_pass_limit=7)
        dev.set_params(copy.copy(p))
        pts, _ = _expected_frame(name, 7, LC.stride_order(len(c["matches"]), p.num_threads), True)
        _same(dev.refine(c["matches"], cull=True), pts, (name, "on"))
        assert dev.lm_stats().last_abandoned == 1
        dev.set_params(copy.copy(LC.case_params(c)))
        _same(dev.refine(c["matches"], cull=True), oracle_frame(name, True)[0], (name, "off again"))
        ls = dev.lm_stats()
        assert all(getattr(ls, f) == 0 for f, _ in ls._fields_)
    finally:
        dev.close()


def test_forced_pair_layout_loses_to_the_guard():
    """ESVO_LM_PAIR=1 (read at esvo_create) forces every small launch into the pair layout, whose second wave evaluates points the
    solver may never ask for: under the guard the launch is the wide one, with the wide test's expectation"""
    _child(dict(ESVO_LM_PAIR="1"), "test_wide_limits and blob1")


# ---- whole ticks -------------------------------------------------------------------------------------------------------------------
def _ticks(limit, n_ticks=3):
    from esvo_amd import calib, lib, params, rostime, synth
    rig = calib.dataset_rig("upenn")
    st = synth.make_stream(rig, 6000, 0.12, 0.16, 1.0, seed=20250419)
    p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], rig, process_event_num=1000, lm_scale_pass_limit=limit)
    dev = lib.Esvo(p, rig)
    try:
        dev.ts_push_events(0, st.ev_left)
        dev.ts_push_events(1, st.ev_right)
        for k in range(n_ticks):
            t = st.t0_ns + int(0.1e9) + k * 5_000_000
            stamps, poses = rostime.pose_table(st.pose, t, p.bm_half_slice_thickness)
            dev.tick_resident(t, st.pose(t), stamps, poses)
        frame, dmap, s, ls = dev.get_last_frame(), dev.get_map(), dev.stats(), dev.lm_stats()
        return dict(frame=frame, map=dmap, matches=int(s.last_matches), points=int(s.last_points), ls={f: int(getattr(ls, f)) for f, _ in ls._fields_})
    finally:
        dev.close()


@pytest.fixture(scope="module")
def ticks_off():
    return _ticks(0)


def test_whole_ticks_count_only(ticks_off):
    on = _ticks(G.COUNT_ONLY)
    assert len(ticks_off["frame"]) > 0 and len(ticks_off["map"]) > 0
    assert on["frame"].tobytes() == ticks_off["frame"].tobytes() and on["map"].tobytes() == ticks_off["map"].tobytes()
    assert all(v == 0 for v in ticks_off["ls"].values())
    ls = on["ls"]
    print("three ticks, count only:", ls)
    assert ls["enabled"] == 1 and ls["total_passes"] > 0 and ls["total_abandoned"] == 0 and ls["last_abandoned"] == 0
    assert ls["total_evals"] >= ls["last_evals"] > 0 and ls["last_max_passes_match"] >= ls["last_max_passes_eval"] > 0


def test_whole_ticks_limit_4(ticks_off):
    on = _ticks(4)
    off_f, on_f = ticks_off["frame"], on["frame"]
    ls = on["ls"]
    print("three ticks, limit 4:", ls, "frame", len(off_f), "->", len(on_f))
    assert on["matches"] == ticks_off["matches"]
    key = lambda f: [tuple(f[n][i].tobytes() for n in f.dtype.names if n != "seq") for i in range(len(f))]   # (seq: the position in the frame)
    it = iter(key(off_f))
    assert all(any(r == q for q in it) for r in key(on_f)), "the guarded frame is not a subsequence of the unguarded one"
    assert ls["last_abandoned"] > 0 and ls["last_max_passes_eval"] <= 4
    assert 0 <= len(off_f) - len(on_f) <= ls["last_abandoned"]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(fn):
    from esvo_amd import lib
    with pytest.raises(lib.EsvoError) as e:
        fn()
    return str(e.value)


def test_refused_on_sharded_and_tick_interleaved_handles():
    c = LC.case("solver_noise")
    dev = _device(c, lm_scale_pass_limit=64)
    try:
        for fn in (lambda: dev.set_band(0, LC.H0 // 2, 0, 2), lambda: dev.comm_init_callbacks(0, 1, lambda s, d, n, stream: 0)):
            assert "lm_scale_pass_limit" in _refused(fn)
        _same(dev.refine(c["matches"], cull=True), oracle_frame("solver_noise", True)[0], "still a plain handle")
    finally:
        dev.close()
    dev = _device(c)
    try:
        dev.set_band(0, LC.H0 // 2, 0, 2)
        assert "lm_scale_pass_limit" in _refused(lambda: dev.set_params(copy.copy(LC.case_params(c, lm_scale_pass_limit=64))))
        dev.set_params(copy.copy(LC.case_params(c)))   # the limit 0 is accepted as ever
    finally:
        dev.close()


def test_l2_has_no_scale_loop():
    name = "l2_tex"
    c = LC.case(name)
    dev = _device(c, lm_scale_pass_limit=64)
    try:
        pts, solved = oracle_frame(name, True)
        _same(dev.refine(c["matches"], cull=True), pts, name)
        assert dev.stats().last_solved == solved
        ls = dev.lm_stats()
        assert all(getattr(ls, f) == 0 for f, _ in ls._fields_)
    finally:
        dev.close()
