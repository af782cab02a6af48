"""The crafted Time-Surface cases (tests/ts_cases.py) on the CPU: each case reaches what its tags claim, the case list reaches every
required target, the crossing sweeps hold the float-only disagreements and the just-outside-the-band pixels they were written for,
the restatement (tests/ts_restated.py, written from the reference's TimeSurface.cpp / TimeSurface.h) equals oracle.OracleTS bit for
bit on every case -- render with the plane behind convertTo, render_forward with its f64 plane, gaussian5 -- and the fixture
tests/golden/ref_ts_cases.npz (the reference's own TimeSurface class on the decay, queue and FORWARD cases, recorded by
tests/golden/make_ref_fixtures.py --ts-cases; held to the oracle in tests/test_ref_pin.py) was recorded on these inputs.  Where
oracle/_ref is present the reference is run live against the fixture.  The device side: tests/test_gpu_ts_cases.py."""
import os

import numpy as np
import pytest

import ts_cases as TC
import ts_restated as TR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# |float short form - f64| over every pixel of every decay case, as the numpy float32 evaluation gives it: the kernel's comment
# derives 4.8e-5 for the device's own float exponential; the guard band is 5e-4.
SHORT_FORM_BOUND = 4.8e-5


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ref_ts_cases.npz"))


@pytest.mark.parametrize("name", TC.NAMES)
def test_case_meets_its_plan(name):
    """every tag a case claims is what observe() sees it reach; the sizes stay small"""
    c = TC.case(name)
    obs = TC.observe(name)
    assert c["tags"] and [t for t in c["tags"] if t not in obs] == [], sorted(obs)
    assert min(c["W"], c["H"]) >= 8 and ((c["W"] <= 128 and c["H"] <= 96) or (c["key"] == "wide" and c["W"] * c["H"] < 128 * 96 // 4))
    for cam in TC.cams(c):
        assert np.isfinite(cam.map_x).all() and np.isfinite(cam.map_y).all()
    for op in c["script"]:      # pushes arrive in stamp order (the ingest's contract), nothing but the declared events lies off the sensor
        if op[0] == "push":
            st = op[2]["sec"].astype(np.int64) * TR.NS + op[2]["nsec"]
            assert (np.diff(st) >= 0).all() and len(op[2]) <= 128 * 96


def test_case_list_reaches_every_target():
    seen = {n: TC.observe(n) for n in TC.NAMES}
    everything = set().union(*seen.values())
    assert TC.REQUIRED and [t for t in TC.REQUIRED if t not in everything] == []
    for k in (0, 1, 2):      # the one-pixel box, the wide box and the box that never fits: under every median size
        at_k = set().union(*[seen[n] for n in TC.NAMES if TC.case(n)["median_k"] == k])
        assert [t for t in TC.REQUIRED_PER_K if t not in at_k] == [], k
    # the geometry the issue names: 33 x 17 and 70 x 40 with different maps and stamps per camera, 20 x 12 queues, 128 x 96 sweeps
    sizes = {(TC.case(n)["W"], TC.case(n)["H"]) for n in TC.NAMES}
    assert {(33, 17), (70, 40), (20, 12), (128, 96)} <= sizes
    for n in TC.GROUPS["staging"] + TC.GROUPS["geometry"]:
        c = TC.case(n)
        if n.startswith(("s70", "g33")):
            l, r = TC.cams(c)
            assert not np.array_equal(l.map_x, r.map_x) and not np.array_equal(TC.pushed(c, 0), TC.pushed(c, 1))
    assert TC.DIRECT_TWICE and all(TC.case(n)["L"] == 0 for n in TC.DIRECT_TWICE)
    # the capacity is the kernel's: 64 x 40 with the ring is exactly the buffer
    assert 64 * 40 == TR.STAGE_CAP and sorted(TC.JUST_OVER.values()) == [2562, 2562, 2574]
    # both overflowing tiles of the overflow case carry the same sixteen pixel positions
    rows = TC.overflow_rows()
    pos = lambda r: ((r[0] % 8, r[1] % 8), (r[0] // 8, r[1] // 8))
    tiles = {pos(r)[1] for r in rows}
    assert len(tiles) == 2 and all({pos(r)[0] for r in rows if pos(r)[1] == t} == {(x, y) for x in range(4) for y in range(4)} for t in tiles)
    assert sum(pos(r)[1] == (0, 0) for r in rows) == 1088


def sweep_counts():
    """per crossing sweep: (float-only disagreements, pixels, of them inside the guard band, largest float error) of the left
    camera and (pixels 5e-4 ... 1e-3 from a half-integer in f64, pixels) of the right"""
    rows = {}
    for d in TC.DECAYS:
        for ip in (1, 0):
            near, away = TC.decay_stats(f"sweep_d{d}_ip{ip}")
            rows[(d, ip)] = (int(near["float_wrong"].sum()), len(near["g"]), int(near["in_band"].sum()), float(near["err32"].max()),
                             int(((away["dist"] > 5e-4) & (away["dist"] < 1e-3)).sum()), len(away["g"]),
                             int((near["float_wrong"] & ~near["in_band"]).sum() + (away["float_wrong"] & ~away["in_band"]).sum()))
    return rows


def test_crossing_sweeps_hold_what_they_were_written_for():
    """Per sweep the pixels where float-only rounding disagrees with f64 (at least 200 at decay_ms 30 and 10000, at least 10 at
    1), the pixels just outside the band (at least 200), the stamp counts (1785 without polarity, 1778 with), and -- the premise of
    the shortcut -- no pixel outside the band whose float rounding is wrong, the float error below the kernel's bound."""
    for (d, ip), (wrong, n, band, err, outside, n_away, wrong_outside) in sweep_counts().items():
        print(f"decay_ms {d:5d} ignore_polarity {ip}: float-only rounding differs on {wrong:4d} of {n} pixels, {band} inside the band, "
              f"float error <= {err:.2g}; {outside} of {n_away} stepped-away pixels lie 5e-4 ... 1e-3 from a half-integer")
        assert n == (1785 if ip else 1778)
        assert wrong >= TC.MIN_FLOAT_WRONG[d], (d, ip, wrong)
        if d != 1:
            assert band == n and outside >= TC.MIN_JUST_OUTSIDE, (d, ip, band, outside)
        assert wrong_outside == 0 and err <= SHORT_FORM_BOUND, (d, ip, wrong_outside, err)
    for n in TC.GROUPS["decay"]:      # every other decay case: the float form is never wrong outside the band either
        for s in TC.decay_stats(n):
            assert not (s["float_wrong"] & ~s["in_band"]).any() and (not len(s["g"]) or s["err32"].max() <= SHORT_FORM_BOUND), n


def same_outputs(a, b, what):
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x["op"], x["cam"], x["T"]) == (y["op"], y["cam"], y["T"])
        for f in ("img", "pre", "f64"):
            assert (f in x) == (f in y)
            if f in x:
                assert x[f].dtype == y[f].dtype and x[f].tobytes() == y[f].tobytes(), (what, i, x["op"], x["cam"], f, int(np.count_nonzero(x[f] != y[f])))


@pytest.mark.parametrize("name", TC.NAMES)
def test_restatement_equals_the_oracle(name):
    """the mono8 image of every render, the plane behind convertTo (want_prefilter), FORWARD's f64 plane, the blurred negative"""
    same_outputs(TC.restated(name), TC.oracle(name), name)
    if not TC.case(name)["oracle"]:
        same_outputs(TC.restated(name, expect=True), TC.oracle(name, expect=True), name)


def test_equal_stamps_of_opposite_polarity_differ_from_the_key_order_rule_only_there():
    """eqpol_*: the reference keeps the later arrival, the device the larger key (the positive event).  Where the positive event
    arrives first the two rules differ -- on that one pixel of the left camera and nowhere else."""
    for n in ("eqpol_L0", "eqpol_L3"):
        ref, rule = TC.oracle(n), TC.oracle(n, expect=True)
        d = ref[0]["img"] != rule[0]["img"]
        assert d.sum() == 1 and d[3, 3] and ref[0]["img"][3, 3] < 128 < rule[0]["img"][3, 3] and np.array_equal(ref[1]["img"], rule[1]["img"])
        assert rule[0]["img"][6, 9] > 128 and rule[0]["img"][9, 15] < 128


FIXTURE_FIELDS = ("n", "lit", "u8", "f64sha")


@pytest.mark.parametrize("name", TC.PINNED)
def test_fixture_was_recorded_on_these_inputs(name, golden):
    c = TC.case(name)
    assert np.array_equal(TC.input_digest(c), golden[f"{name}_sha"]), f"the generator of {name} drifted"
    assert len(golden[f"{name}_n"]) == sum(op[0] in ("render", "forward") for op in c["script"])
    assert int(golden[f"{name}_n"].sum()) == len(golden[f"{name}_lit"]) == len(golden[f"{name}_u8"]) > 0


def test_pinned_cases_are_the_decay_queue_and_forward_cases():
    for g in ("decay", "queue", "forward"):
        assert [n for n in TC.GROUPS[g] if n in TC.PINNED], g
    assert all(TC.case(n)["group"] in ("decay", "queue", "forward") and TC.case(n)["oracle"] and TC.case(n)["median_k"] == 0 for n in TC.PINNED)
    assert {f"sweep_d{d}_ip{ip}" for d in TC.DECAYS for ip in (0, 1)} <= set(TC.PINNED)
    assert {f"queue_L{L}" for L in (1, 3, 20, 32)} | {"queue_over_L3", "queue_over_L20", "forward_ip0_k0", "forward_ip1_k0"} <= set(TC.PINNED)


@pytest.mark.parametrize("name", TC.PINNED)
def test_live_reference_reproduces_the_crafted_fixture(name, golden):
    from oracle import ref as R
    if not os.path.isdir(os.path.join(R.REFERENCE, "esvo_time_surface", "src")):
        pytest.skip("reference tree not present (GPU box): the fixture is the pin")
    import sys
    sys.path.insert(0, GOLDEN)
    import make_ref_fixtures as mk
    for f, a in mk.pack_case(mk.run_ts_case(TC.case(name)), TC.case(name)).items():
        assert np.array_equal(a, golden[f"{name}_{f}"]), f
