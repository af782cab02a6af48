"""The crafted refinement cases (tests/lm_cases.py) on the CPU: each case meets the plan it was written for, the case list reaches
every required target, the restated evaluator (tests/lm_restated.py) agrees with the oracle's at every point the solver visits,
the restated solver reproduces the oracle's solve, and the oracle -- in literal and in canonical mode -- agrees with what the
reference's own DepthProblem / DepthProblemSolver made of the cases (tests/golden/ref_lm_cases.npz, recorded by
tests/golden/make_ref_fixtures.py --lm-cases) within the bars of test_ref_pin.py.  Where oracle/_ref is present the reference is
run live against the fixture.  The device side: tests/test_gpu_lm_cases.py."""
import os

import numpy as np
import pytest

import lm_cases as LC
import lm_restated as LR
from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# The restated evaluator against oracle.eval_residual (canonical mode: the sums of the scale loop in another order), relative to
# max(1, |f|), over every evaluation point of every case.  Measured on the CPU: 1.22e-15 (any25x25_tex; the 15 x 7 cases stay
# below 1.1e-15).  Ten times that is allowed.
RESTATED_MEASURED = 1.22e-15
RESTATED_TOL = 10 * RESTATED_MEASURED
STOP_MARGIN = 1e-8


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ref_lm_cases.npz"))


def oracle_for(c, canonical):
    m = O.OracleMapper(LC.case_params(c), LC.rig())
    m.set_mode(canonical, canonical)
    LC.observe_on(m, c)
    return m


@pytest.mark.parametrize("name", LC.NAMES)
def test_case_meets_its_plan(name):
    """every tag a case claims for a match is what observe() sees the match do; a placed coordinate is exactly the intended double
    and is refused by exactly the intended test; every case brings the three failing matches a narrow wave needs"""
    c = LC.case(name)
    obs = LC.observe(name)
    for tag, idx in c["tags"].items():
        for i in idx:
            assert tag in obs[i]["tags"], (tag, i, sorted(obs[i]["tags"]))
    for i, (k, value, why, label) in c["expect"].items():
        e = obs[i]["evals"][0][2]
        assert e["x"][k] == value and e["fail"] == why and label in obs[i]["tags"], (i, label, e["x"], e["fail"])
    assert len(c["matches"]) >= 4 and c["n_own"] == len(c["matches"]) - len(LC.FAILING)
    for o in obs[c["n_own"]:]:
        assert not o["evals"][0][2]["ok"]
    # (the solver's info columns and the longest scale loop come from the oracle itself)
    m = oracle_for(c, True)
    _, info = m.refine(c["matches"], cull=False, want_info=True)
    for i, o in enumerate(obs):
        t = o["trace"]
        assert (t["iterations"], t["nfev"], t["status"], int(t["solved"])) == tuple(int(v) for v in info[i]), (i, info[i])
    if any("collapse" in o["tags"] for o in obs):   # the literal loop is seen to collapse where the device takes the shortcut
        assert m.counters()["max_scale_iters"] > 1000
        assert m.counters()["max_scale_iters"] == max(e["iters"] for o in obs for _, _, e in o["evals"])


def test_case_list_reaches_every_target():
    seen = set()
    for name in LC.TDIST_15x7:
        for o in LC.observe(name):
            seen |= o["tags"]
    assert [t for t in LC.REQUIRED if t not in seen] == []
    # what the plan declares out of reach is not reached by accident either (then it belongs to REQUIRED)
    assert not seen & {"status6", "status7", "status8", "saw6", "saw7", "saw8", "init_interp_right"}
    assert set(LC.UNREACHED) == {"status6", "status7", "status8", "interp_right", "nu_low", "r2_outside"}


@pytest.mark.parametrize("name", LC.NAMES)
def test_no_scale_loop_is_decided_on_its_threshold(name):
    """No pass of any scale loop of any case ends with |s2 - s1| / s1 within STOP_MARGIN of the 5 % it is compared with.  Two
    orders of summing 105 (625) terms differ by N eps = 2e-14 (1.4e-13) relative at the most, and so does the quotient; a case
    nearer than that to the threshold could take one pass more under one order than under the other -- the restatement would then
    differ from the oracle by a whole pass, not by rounding -- so such a case is refused here, with a margin of five orders."""
    for o in LC.observe(name):
        for kind, x, e in o["evals"]:
            assert e["margin"] > STOP_MARGIN, (kind, x, e["margin"])


@pytest.mark.parametrize("name", LC.NAMES)
def test_restated_evaluator_agrees_with_the_oracle(name):
    c = LC.case(name)
    m = oracle_for(c, True)
    worst = 0.0
    for mt, o in zip(c["matches"], LC.observe(name)):
        for kind, x, e in o["evals"]:
            f, ok = m.eval_residual(mt["x_left"], int(mt["pose_idx"]), x)
            assert ok == e["ok"], (kind, x, e["fail"])
            worst = max(worst, float((np.abs(f - e["f"]) / np.maximum(1.0, np.abs(f))).max()))
    print(f"{name}: restated evaluator against the oracle: {worst:.3g}")
    assert worst <= RESTATED_TOL, worst


@pytest.mark.parametrize("name", LC.NAMES)
def test_restated_solver_reproduces_the_oracle(name):
    """lm_restated.trace around the oracle's own residual function ends where the oracle's refine ends, in both reduction modes:
    the same inverse depth bit for bit"""
    c = LC.case(name)
    p = LC.case_params(c)
    for canonical in (False, True):
        m = oracle_for(c, canonical)
        for mt in c["matches"]:
            t = LR.trace(lambda v: m.eval_residual(mt["x_left"], int(mt["pose_idx"]), v)[0], float(mt["inv_depth"]), p.lm_max_iteration,
                         p.patch_size_x, p.patch_size_y, canonical=canonical)
            pts = m.refine(np.array([mt]), cull=False)
            assert len(pts) == int(t["solved"])
            if len(pts):
                assert pts["inv_depth"][0] == t["x"] and pts["residual"][0] == t["fnorm"] * t["fnorm"]


@pytest.mark.parametrize("name", LC.NAMES)
def test_fixture_was_recorded_on_these_inputs(name, golden):
    c = LC.case(name)
    assert np.array_equal(LC.input_digest(c), golden[f"{name}_sha"]), f"the generator of {name} drifted"
    assert golden[f"{name}_matches"].tobytes() == LC.pinned_matches(c).tobytes()


def check_against_fixture(name, pts, solved, golden):
    """points before culling and per-match solved flags against the recorded reference: the bars of
    test_ref_pin.py::test_oracle_stages_match_reference (check_points with its defaults)"""
    from test_ref_pin import check_points
    ref = golden[f"{name}_points"]
    assert np.array_equal(solved, golden[f"{name}_solved"]), (solved, golden[f"{name}_solved"])
    if LC.case_params(LC.case(name)).ls_norm == LC.LSNORM_L2:   # the Gaussian model never sets nu (Appendix A-8)
        pts, ref = pts.copy(), ref.copy()
        pts["nu"] = ref["nu"] = 0
    check_points(pts, ref)


@pytest.mark.parametrize("canonical", [False, True], ids=["literal", "canonical"])
@pytest.mark.parametrize("name", LC.NAMES)
def test_oracle_agrees_with_the_reference_on_the_crafted_cases(name, canonical, golden):
    c = LC.case(name)
    m = oracle_for(c, canonical)
    mt = LC.pinned_matches(c)
    pts, info = m.refine(mt, cull=False, want_info=True)
    check_against_fixture(name, pts, info[:, 3].astype(np.uint8), golden)


@pytest.mark.parametrize("name", LC.NAMES)
def test_live_reference_reproduces_the_crafted_fixture(name, golden):
    from oracle import ref as R
    if not os.path.isdir(os.path.join(R.REFERENCE, "esvo_core", "src")):
        pytest.skip("reference tree not present (GPU box): the fixture is the pin")
    import sys
    sys.path.insert(0, GOLDEN)
    import make_ref_fixtures as mk
    c = LC.case(name)
    pts, solved = mk.run_lm_case(c)
    assert np.array_equal(solved, golden[f"{name}_solved"])
    l2 = LC.case_params(c).ls_norm == LC.LSNORM_L2   # (the Gaussian model leaves nu and scale2 uninitialised, Appendix A-8)
    for f in pts.dtype.names:
        if not (l2 and f in ("nu", "scale2")):
            assert pts[f].tobytes() == golden[f"{name}_points"][f].tobytes(), f
    # DepthProblem::operator() itself at every start point, against the oracle's (the bar of test_oracle_units_match_reference)
    ref, orc = R.RefMapper(LC.case_params(c), LC.rig()), oracle_for(c, False)
    LC.observe_on(ref, c)
    for mt in LC.pinned_matches(c):
        a, ok_a = ref.eval_residual(mt["x_left"], int(mt["pose_idx"]), float(mt["inv_depth"]))
        b, ok_b = orc.eval_residual(mt["x_left"], int(mt["pose_idx"]), float(mt["inv_depth"]))
        assert bool(ok_a) == bool(ok_b) and np.abs(a - b).max() <= 1e-9


def test_slot_plan_of_the_narrow_launch():
    """every match in each of a wave's four positions, beside at least three different neighbours; the leading wave; the tail"""
    for k in (4, 5, 9, 63):
        for n in (40001, 40002, 40003):
            plan = LC.slot_plan(k, n, lead=1, fails=(k - 3, k - 2, k - 1))
            assert len(plan) == n and n % 4 == n - 40000 and list(plan[:4]) == [1, k - 3, k - 2, k - 1]
            waves = plan[:n - n % 4].reshape(-1, 4)
            for i in range(k):
                at = waves == i
                assert at.any(axis=0).all(), (k, i)
                assert len(set(waves[at.any(axis=1)].reshape(-1).tolist()) - {i}) >= 3
    order = LC.stride_order(11, 4)
    assert list(order) == [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7]
    c = LC.case("zero")
    plan = LC.slot_plan(len(c["matches"]), 23)
    m = LC.tiled(c, plan, 4)
    assert m[LC.stride_order(23, 4)]["x_left"].tobytes() == c["matches"][plan]["x_left"].tobytes()


@pytest.mark.parametrize("name", ["extreme", "zero", "trial_fill"])
def test_assembled_frame_is_what_the_oracle_returns_for_a_tiled_launch(name):
    """the expectation of the device's narrow launches -- the oracle's result per distinct match, assembled by slot -- equals the
    oracle's own refine on the tiled match list (small here: the oracle solves every copy)"""
    c = LC.case(name)
    m = oracle_for(c, True)
    k = len(c["matches"])
    plan = LC.slot_plan(k, 4 * (1 + 4 * k) + 3, lead=LC.longest(name), fails=range(k - 3, k))
    for cull in (False, True):
        per = []
        for i in range(k):
            pts, info = m.refine(c["matches"][i:i + 1], cull=cull, want_info=True)
            per.append((pts, bool(info[0, 3])))
        exp, solved = LC.assemble(per, plan)
        got, info = m.refine(LC.tiled(c, plan, LC.case_params(c).num_threads), cull=cull, want_info=True)
        assert got.tobytes() == exp.tobytes() and int(info[:, 3].sum()) == solved
