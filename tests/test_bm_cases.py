"""The crafted block-matching cases (tests/bm_cases.py) on the CPU: each case reaches what its tags claim, the case list reaches
every required target, the restated matcher (tests/bm_restated.py) equals the oracle's integer mode bit for bit -- match records,
the cost row of every event and the three failure counts -- the integer-mode cost stays within a measured bar of the cost's
definition in long double, and the fixture tests/golden/ref_bm_cases.npz (the reference's own EventBM on the cases, recorded by
tests/golden/make_ref_fixtures.py --bm-cases; held to the oracle in tests/test_ref_pin.py) was recorded on these inputs.  Where
oracle/_ref is present the reference is run live against the fixture.  The device side: tests/test_gpu_bm_cases.py."""
import os

import numpy as np
import pytest

import bm_cases as BC
import bm_restated as BR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# |integer-mode cost - the definition in long double| over every valid candidate of every distinct event of every case.
# Measured on the CPU: 2.1e-16, on a true match of cost 1.45e-8 (group16: 1 - x with x just below 1 keeps x's rounding, about two
# units in the last place of 0.5); four times that is allowed.
COST_MEASURED = 2.1e-16
COST_BAR = 4 * COST_MEASURED


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ref_bm_cases.npz"))


def distinct_events(c):
    seen, out = set(), []
    for i, e in enumerate(c["events"]):
        key = (int(e["x"]), int(e["y"]))
        if key not in seen:
            seen.add(key)
            out.append(i)
    return out


@pytest.mark.parametrize("name", BC.NAMES)
def test_case_meets_its_plan(name):
    """every tag a case claims for an event is what observe() sees the event do"""
    c = BC.case(name)
    obs, recs, fails = BC.observe(name)
    for tag, idx in c["tags"].items():
        for i in idx:
            assert tag in obs[i]["tags"], (tag, i, obs[i]["trace"]["gate"], sorted(obs[i]["tags"]))
    assert c["W"] <= 160 and c["H"] <= 120 and len(c["events"]) <= 1024
    if name not in BC.PLACEMENT:
        assert len(c["events"]) <= 24 and c["tags"]


def test_case_list_reaches_every_target():
    seen, events = {}, []
    for group, names in (("15x7", BC.REG_15x7), ("any", BC.ANY)):
        seen[group] = set()
        for name in names:
            for o in BC.observe(name)[0]:
                seen[group] |= o["tags"]
                events.append(o["tags"])
    assert BC.REQUIRED and [t for t in BC.REQUIRED_15x7 if t not in seen["15x7"]] == []
    assert [t for t in BC.REQUIRED_ANY if t not in seen["any"]] == []
    assert [combo for combo in BC.REQUIRED_TOGETHER if not any(set(combo) <= tags for tags in events)] == []
    # what the plan declares out of reach is not reached by accident either (then it belongs to REQUIRED)
    everything = seen["15x7"] | seen["any"]
    assert not everything & {"gate:fine", "clamp_hi", "cost:one"}
    assert set(BC.UNREACHED) == {"gate:fine", "clamp_hi", "cost:one"}
    assert not any(BC.clamp_hi_reachable(W, H) for W in range(17, 41) for H in (9, 11, 40))
    for name in BC.NAMES:   # no valid candidate of any case costs 1.0 or more; failure reason 3 never occurs
        obs, _, fails = BC.observe(name)
        assert fails[2] == 0 and all(v < 1.0 for o in obs for v in o["trace"]["row"].values()), name
    # image sizes: every residue of W mod 4 (the strip rows' byte phases), and images that end inside a dword
    sizes = {(BC.case(n)["W"], BC.case(n)["H"]) for n in BC.NAMES}
    assert {W % 4 for W, _ in sizes} == {0, 1, 2, 3} and any(W * H % 4 for W, H in sizes)


def test_group_widths_are_the_launcher_s():
    """the lane-group width per range, restated from launch_bm_match: the fewest candidate slots, a tie to the wider group.  (17, 33
    and 65 candidates take G = 8 -- 24, 40 and 72 slots, fewer than any wider group's; a group of 16, 32 or 64 lanes makes more
    than one trip only where the narrower ones waste as much: 41 ... 48, 89 ... 96, 121 ... 128.)"""
    assert [BC.group_width(nd) for nd in BC.GROUP_ND] == [8, 8, 16, 16, 8, 32, 8, 16, 16, 64, 8, 8, 32, 32, 64, 64]
    trips = {(BC.group_width(nd), -(-nd // BC.group_width(nd))) for nd in BC.GROUP_ND}
    assert {(8, 9), (16, 3), (32, 3), (64, 2)} <= trips and {(8, 1), (16, 1), (32, 1), (64, 1)} <= trips
    assert [BC.strip_dwords(nd)[1] for nd in range(9, 15)] == [False, True, True, True, True, False]
    assert all(BC.strip_dwords(nd)[1] for nd in BC.NOSLACK_ND) and not BC.strip_dwords(25)[1] and not BC.strip_dwords(30)[1]


@pytest.mark.parametrize("name", BC.NAMES)
def test_restated_matcher_equals_the_oracle(name):
    """records (every field, in the reference's thread-stride order), the three failure counts, and per distinct event the cost row
    (all candidates; under BM_step > 1 the oracle's row holds the coarse candidates only)"""
    c = BC.case(name)
    obs, recs, fails = BC.observe(name)
    m = BC.oracle_for(c)
    got, exp = m.match(c["events"]), BC.records_array(recs)
    assert len(got) == len(exp), (len(got), len(exp))
    for f in exp.dtype.names:
        assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(exp[f]).tobytes(), f
    assert list(m.bm_fail_counts()) == fails, (m.bm_fail_counts(), fails)
    s = BC.setup(c)
    for i in distinct_events(c):
        t = obs[i]["trace"]
        row = m.match_costs(c["events"][i], exact_int=True)
        if t["gate"] in ("raw", "lut", "mask", "border", "noise"):
            assert row is None, (i, t["gate"])
            continue
        for d in range(s.dmin, s.dmax + 1):
            v = row[d - s.dmin]
            if (d - s.dmin) % s.step:
                assert np.isnan(v)
            else:
                assert v == t["row"].get(d, 1.0), (i, d, v, t["row"].get(d))


def test_integer_cost_stays_within_the_bar_of_its_definition():
    """The cost from integer moments (what the device and the oracle's integer mode evaluate) against the definition -- both patches
    normalised as tools::normalizePatch does, the products summed -- in long double, over every valid candidate of every distinct
    event of every case.  Measured: 2.1e-16 at the most; the bar is four times that, 8.4e-16."""
    worst, where = 0.0, None
    for name in BC.NAMES:
        c = BC.case(name)
        s = BC.setup(c)
        obs = BC.observe(name)[0]
        for i in distinct_events(c):
            t = obs[i]["trace"]
            L = None if t["x1"] is None else s.block(s.left, t["x1"], t["y1"])
            for d, v in t["row"].items():
                x2, y2 = s.candidate(t["x1"], t["y1"], d)
                diff = float(abs(np.longdouble(v) - BR.cost_definition(L, s.block(s.right, x2, y2))))
                if diff > worst:
                    worst, where = diff, (name, i, d, v)
    print(f"integer-mode cost against the long-double definition: {worst:.4g} at {where}")
    assert np.finfo(np.longdouble).eps < 1e-18        # (a long double that is wider than a double)
    assert worst <= COST_BAR, (worst, where)


def test_slot_plan_puts_every_event_everywhere():
    """every matching kind in each position of a workgroup, beside copies of each failing kind; a last, partly filled workgroup;
    slot w of a launch holds the plan's kind w under both thread counts"""
    for epb in (2, 8):
        plan = BC.slot_plan(epb)
        full = plan[:len(plan) - len(plan) % epb].reshape(-1, epb)
        assert 0 < len(plan) % epb < epb and len(plan) <= 1024
        for g in range(BC.N_GOOD):
            for pos in range(epb):
                beside = {tuple(np.delete(wg, pos)) for wg in full if wg[pos] == g}
                assert {(f,) * (epb - 1) for f in BC.FAILING} <= beside, (g, pos)
    for name in BC.PLACEMENT:
        c = BC.case(name)
        T = BC.case_params(c).num_threads
        obs = BC.observe(name)[0]
        order = BC.stride_order(len(c["plan"]), T)
        assert 64 // BC.group_width(c["over"]["bm_max_disparity"]) in (2, 8)
        want = {0: "matched", 1: "matched", 2: "matched", 3: "gate:raw", 4: "gate:mask", 5: "gate:border", 6: "gate:noise", 7: "gate:coarse"}
        for w, kind in enumerate(c["plan"]):
            e = c["events"][order[w]]
            assert (int(e["x"]), int(e["y"])) == tuple(c["kinds"][kind]) and want[kind] in obs[order[w]]["tags"], (name, w, kind)
    assert list(BC.stride_order(11, 4)) == [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7]


@pytest.mark.parametrize("name", BC.NAMES)
def test_fixture_was_recorded_on_these_inputs(name, golden):
    c = BC.case(name)
    assert np.array_equal(BC.input_digest(c), golden[f"{name}_sha"]), f"the generator of {name} drifted"
    assert (f"{name}_matches" in golden.files) == (name not in BC.UNPINNED)


def test_unpinned_cases_are_the_threshold_cases():
    """only the cases whose threshold is an integer-mode cost or the double above it stay out of the pin; the periodic ties are in"""
    assert all("thr:eq" in BC.case(n)["tags"] or "thr:above" in BC.case(n)["tags"] for n in BC.UNPINNED)
    assert not [n for n in BC.NAMES if "tie" in n and n in BC.UNPINNED] and len(BC.UNPINNED) < len(BC.NAMES) // 5
    for n, (idx, _) in BC.UNPINNED_EVENTS.items():   # ... and of single events only the two under mask values 125 and 126
        tags = [BC.observe(n)[0][i]["tags"] for i in idx]
        assert len(idx) == 2 and "mask:126" in tags[0] and "mask:125" in tags[1]


@pytest.mark.parametrize("name", [n for n in BC.NAMES if n not in BC.UNPINNED])
def test_live_reference_reproduces_the_crafted_fixture(name, golden):
    from oracle import ref as R
    if not os.path.isdir(os.path.join(R.REFERENCE, "esvo_core", "src")):
        pytest.skip("reference tree not present (GPU box): the fixture is the pin")
    import sys
    sys.path.insert(0, GOLDEN)
    import make_ref_fixtures as mk
    got, ref = mk.run_bm_case(BC.case(name)), golden[f"{name}_matches"]
    assert got.tobytes() == ref.tobytes()
