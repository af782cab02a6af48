"""The crafted tracker problems (tests/track_cases.py) on the CPU: the named points reach the branch they were built for, the oracle's
tracker (oracle/esvo_oracle.cpp, written beside the kernel) equals the plain restatement (tests/track_restated.py) byte for byte on
every case, the comparison is sensitive to summation order and to the skew terms of P, and the oracle agrees with what the
reference's own RegProblemLM made of the pinned points (tests/golden/ref_track_cases.npz, recorded by
tests/golden/make_ref_fixtures.py --track-cases).  The device side: tests/test_gpu_track_cases.py.

The reference pin compares values, as tests/test_ref_pin.py does for the tracker (np.array_equal): residuals turn out equal byte for
byte; in the Jacobian the reference's dense product -fjacBlock J_G(0) (a sum started at +0) leaves +0 in every entry that is zero -- a
rejected point's row, a gradient component of 0 on a flat or a ramp -- where the written expressions -(2 e5 - 2 e7), -e9 of the
oracle and the kernel leave -0 in some.  The test asserts that this is the only difference: both values are zero and the reference's
is +0.  (An entry of +-0 adds +-0 to sums that start at +0: no sum, and so no step of the registration, can tell the two apart.)"""
import os
import sys

import numpy as np
import pytest

import reproj_restated as RR
import track_cases as TC
import track_restated as TR
from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROBLEMS = [(v, W, H) for v in TC.VARIANTS for W, H in TC.SIZES]


def _pid(p):
    return f"{p[0]}-{p[1]}x{p[2]}"


def _T4(R, t):
    T = np.eye(4)
    T[:3] = RR.pose_left_ref(R, t)
    return T


def _oracle(c, xyz=None, ksize=0):
    trk = O.OracleTracker(c["rig"])
    trk.set_current(c["ts"], ksize)
    trk.set_reference(c["xyz"] if xyz is None else xyz, TC.I4)
    return trk


def _by_name(c, motion):
    return dict(zip(c["names"], TC.infos(c, motion)))


# ---- the image ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", TC.SIZES)
def test_image_holds_its_regions_and_the_oracle_derives_the_same_images(W, H):
    c = TC.problem("plain", W, H)
    neg, du, dv = c["images0"]
    assert (neg[TC.FLAT50] == 50).all() and (neg[TC.FLAT0] == 0).all()
    assert set(np.unique(neg[TC.CHECKER])) == {0, 255}
    assert du[TC.CHECKER].min() == -1020 and du[TC.CHECKER].max() == 1020 and dv[TC.CHECKER].min() == -1020 and dv[TC.CHECKER].max() == 1020
    assert np.array_equal(neg[TC.RAMP][0], 8 + 3 * np.arange(32)) and (du[25:39, 29:59] == 24).all()     # Sobel of a slope of 3: 8 x 3
    assert len(np.unique(neg[44:60, 62:90])) > 100                                                   # noise elsewhere
    for a, b in zip(_oracle(c).images(), c["images0"]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- reach -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "masked"])
@pytest.mark.parametrize("W,H", TC.SIZES)
def test_named_bounds_points_land_exactly(variant, W, H):
    """under the identity, per name: the coordinate the name states, and the branch it selects"""
    c = TC.problem(variant, W, H)
    info = _by_name(c, "identity")
    R, t = TC.MOTIONS["identity"]
    J = dict(zip(c["names"], TR.jacobian(c["images0"], c["mask"], c["P"], c["pts"], R, t, 0, len(c["pts"]))))
    tiny = 1e-5                                                   # the f32 neighbour of a coordinate moves the projection by about 4e-6
    for ax, k, n, low, high, side in (("x", "x", W, "left", "right", "right"), ("y", "y", H, "top", "bottom", "bottom")):
        i = info[f"{ax}=-0@identity"]
        assert i[k] == 0.0 and np.signbit(i[k]) and i["valid"] and i["interp_ok"] and i["r"] < 255.0
        i = info[f"{ax}=+0@identity"]
        assert i[k] == 0.0 and not np.signbit(i[k]) and i["valid"] and i["interp_ok"]
        i = info[f"{ax}<0@identity"]
        assert -tiny < i[k] < 0.0 and not i["valid"] and i["reason"] == low and i["r"] == 255.0
        lim = "W" if ax == "x" else "H"
        i = info[f"{ax}={lim}-2@identity"]
        assert i[k] == n - 2.0 and i["valid"] and i["interp_ok"]
        i = info[f"{ax}>{lim}-2@identity"]
        assert n - 2.0 < i[k] < n - 2.0 + tiny and i["valid"] and i["interp_ok"]     # valid: the last column / row is read
        i = info[f"{ax}={lim}-1@identity"]
        assert i[k] == n - 1.0 and i["valid"] and not i["interp_ok"] and i["interp_fail"] == side and i["r"] == 255.0
        row = J[f"{ax}={lim}-1@identity"]
        assert (row == 0.0).all() and np.signbit(row).any() and not np.signbit(row).all()              # signed zeros of both signs
        i = info[f"{ax}>{lim}-1@identity"]
        assert n - 1.0 < i[k] < n - 1.0 + tiny and not i["valid"] and i["reason"] == high
    for name, xy, ok in (("corner00", (0.0, 0.0), True), ("cornerW0", (W - 1.0, 0.0), False), ("corner0H", (0.0, H - 1.0), False),
                         ("cornerWH", (W - 1.0, H - 1.0), False)):
        i = info[f"{name}@identity"]
        assert (i["x"], i["y"]) == xy and i["valid"] and i["interp_ok"] == ok
    ints = [i for nm, i in info.items() if "_int" in nm and nm.endswith("@identity") and not nm.startswith("mask")]
    assert len(ints) >= 12 and all(i["x"] == int(i["x"]) and i["y"] == int(i["y"]) and i["interp_ok"] for i in ints)   # q2 == 0 and q4 == 0
    fracs = [i for nm, i in info.items() if "_frac" in nm and nm.endswith("@identity")]
    assert len(fracs) >= 40 and all((4 * i["x"]).is_integer() and (4 * i["y"]).is_integer() for i in fracs)
    assert len({c["pts"][c["names"].index(nm), 2] for nm in info if "_frac" in nm and nm.endswith("@identity")}) == 3    # three depths
    if variant == "masked":
        for name, byte, valid in (("mask_x19.99", 124, False), ("mask_x20.0", 125, True), ("mask_x27.99", 125, True), ("mask_x11.99", 0, False),
                                  ("mask_x12.0", 124, False), ("mask_y43.99", 255, True), ("mask_y44.0", 0, False), ("mask_y43.99b", 255, True),
                                  ("mask_y44.0b", 125, True), ("mask0_in", 0, False), ("mask124_in", 124, False), ("mask125_in", 125, True),
                                  ("mask126_in", 126, True), ("mask255_in", 255, True), ("mask124_int", 124, False), ("mask125_int", 125, True)):
            i = info[f"{name}@identity"]
            assert i["mask_byte"] == byte and i["valid"] == valid and (i["reason"] == "mask") == (not valid), (name, i)
        assert int(info["mask_x19.99@identity"]["x"]) == 19 and info["mask_x19.99@identity"]["x"] > 19.98     # k + 0.99 indexes pixel k


@pytest.mark.parametrize("prob", PROBLEMS, ids=_pid)
def test_point_list_reaches_every_kind(prob):
    c = TC.problem(*prob)
    n = len(c["xyz"])
    assert c["xyz"].dtype == np.float32 and 350 <= n <= 450 and len(set(c["names"])) == n
    assert len({tuple(p) for p in c["xyz"][np.isfinite(c["xyz"]).all(axis=1)].tolist()}) >= n - 10      # distinct points
    reasons, fails, negz, posz, nanrow, ordinary = set(), set(), 0, 0, 0, {}
    for motion, (R, t) in TC.MOTIONS.items():
        info = TC.infos(c, motion)
        J = TR.jacobian(c["images0"], c["mask"], c["P"], c["pts"], R, t, 0, n)
        valid = np.array([i["valid"] for i in info])
        reasons |= {i["reason"] for i in info}
        fails |= {i["interp_fail"] for i in info if i["valid"]}
        border = valid & ~np.array([i["interp_ok"] for i in info])
        negz += int((np.signbit(J[border]) & (J[border] == 0)).sum())
        posz += int((~np.signbit(J[border]) & (J[border] == 0)).sum())
        nanrow += int(np.isnan(J).all(axis=1).sum())
        assert not np.isnan(J[~valid]).any() and (J[~valid] == 0).all()                    # a rejected point: a row of zeros
        ordinary[motion] = float(np.mean([i["valid"] and i["interp_ok"] and np.isfinite(row).all() for i, row in zip(info, J)]))
        by = dict(zip(c["names"], info))
        if motion == "identity":                                  # kinds that reach their branch under the identity only
            assert by["plz0_a"]["reason"] == "nonfinite" and by["plz0_b"]["reason"] == "nonfinite"          # x = inf, x = NaN
            assert abs(by["huge_x"]["x"]) > 1e80 and by["huge_x"]["reason"] == "right" and by["huge_negx"]["reason"] == "left"
            assert by["huge_y"]["y"] < -1e40 and by["huge_y"]["reason"] == ("top" if prob[0] != "skewed" else "right")   # (P12 y / z)
            assert all(by[f"zref0_{k}"]["reason"] == "nonfinite" for k in range(3))
            for k in range(3):
                assert by[f"behind{k}@identity"]["valid"] and c["pts"][c["names"].index(f"behind{k}@identity"), 2] < 0
            r50 = [by[f"flat50_h{k}@identity"]["r"] for k in range(6)]
            assert all(r == 50.0 for r in r50), r50                # r == huber_threshold exactly: the weight stays 1
            assert all(by[f"flat0_h{k}@identity"]["r"] == 0.0 for k in range(4))
            if prob[0] != "skewed":
                ramp = [by[f"ramp_h{k}@identity"]["r"] for k in range(7)]
                assert ramp[0] < ramp[1] < 50.0 and 50.0 < ramp[4] < ramp[5], ramp                  # the ramp straddles the threshold
        else:
            z0 = [nm for nm, kind in zip(c["names"], c["kinds"]) if kind in ("zref0", "plz0") and by[nm]["valid"]]
            assert z0 and all(np.isnan(J[c["names"].index(nm)]).all() for nm in z0)        # p_ref.z == 0, a valid projection: NaN rows
            assert prob[0] == "skewed" or z0 == [nm for nm in c["names"] if nm.startswith("zref0")]    # (P14 / z moves them there)
        for nm in ("nan_z", "nan_x", "inf_x", "ninf_y", "inf_z"):
            assert by[nm]["reason"] == "nonfinite"
    assert {"nonfinite", "left", "right", "top", "bottom", None} <= reasons
    assert ("mask" in reasons) == (prob[0] == "masked")
    if prob[0] != "skewed":                                       # (exact hits need the ideal P: module docstring of track_cases)
        assert {"right", "bottom"} <= fails and negz > 0 and posz > 0
    assert nanrow >= 1
    assert min(ordinary.values()) >= 0.6, ordinary                # the edge kinds cannot crowd the sums
    # Huber at the threshold: r == thr keeps w = 1, r above it does not; thr == 0 with r == 0 and with r > 0; thr = 1e300 never weighs
    T = _T4(*TC.MOTIONS["identity"])
    raw = TR.residuals(c["images0"][0], c["mask"], c["P"], c["pts"], T, 0, n, False, 0.0)
    f = {name: TR.residuals(c["images0"][0], c["mask"], c["P"], c["pts"], T, 0, n, huber, thr) for name, huber, thr in TC.NORMS}
    at50 = raw == 50.0
    assert at50.sum() >= 6 and (f["huber0"][at50] == 50.0).all()                            # thr = 50: w = 1
    below = float(np.nextafter(50.0, 0.0))
    assert (raw[at50] > below).all() and (f["huber1"][at50] == np.sqrt(below / 50.0) * 50.0).all()          # thr one ulp below r
    above = raw > 50.0
    assert above.sum() > 100 and (f["huber0"][above] < raw[above]).all() and (f["huber0"][~above] == raw[~above]).all()
    assert (raw == 0.0).sum() >= 4 and (f["huber2"] == 0.0).all() and not np.signbit(f["huber2"]).any()        # thr = 0: w = 0 or r = 0
    assert f["huber3"].tobytes() == raw.tobytes() == f["l2"].tobytes()


# ---- oracle == restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob", PROBLEMS, ids=_pid)
def test_oracle_equals_the_restatement(prob):
    c = TC.problem(*prob)
    n = len(c["xyz"])
    for ksize in ((0, 5) if prob == ("plain", 96, 64) else (0,)):
        trk = _oracle(c, ksize=ksize)
        images = c["images0"] if ksize == 0 else trk.images()     # (the blur is tests/ts_cases.py's subject; its images are taken over)
        if ksize == 5:
            assert not np.array_equal(images[0], c["images0"][0])
        for motion, (R, t) in TC.MOTIONS.items():
            T = _T4(R, t)
            J_all = TR.jacobian(images, c["mask"], c["P"], c["pts"], R, t, 0, n)
            for name, huber, thr in TC.NORMS:
                f_all = TR.residuals(images[0], c["mask"], c["P"], c["pts"], T, 0, n, huber, thr)
                assert not np.isnan(f_all).any()
                for off, cnt in TC.batches(n):
                    m = max(0, min(cnt, n - off))
                    label = (ksize, motion, name, off, cnt)
                    got = trk.residuals(T, off, cnt, huber, thr)
                    assert len(got) == m and got.tobytes() == f_all[off:off + m].tobytes(), label
                    Jo = trk.jacobian(R, t, off, cnt)
                    TC.same_bits(Jo, J_all[off:off + m], label)
                    Ho, bo, co, no = trk.normal_equations(R, t, off, cnt, huber, thr)
                    Hr, br, cr = TR.sum_normal_equations(J_all[off:off + m], f_all[off:off + m])
                    assert no == m
                    TC.same_bits(Ho, Hr, label), TC.same_bits(bo, br, label), TC.same_bits([co], [cr], label)
            # the wrappers of the restatement give what their parts give
            assert TR.residuals(images[0], c["mask"], c["P"], c["pts"], T, 7, n - 8, True, 50.0).tobytes() == \
                TR.residuals(images[0], c["mask"], c["P"], c["pts"], T, 0, n, True, 50.0)[7:n - 1].tobytes()
            Hn, bn, cn, nn = TR.normal_equations(images, c["mask"], c["P"], c["pts"], R, t, 7, n - 8, True, 50.0)
            Ho, bo, co, no = trk.normal_equations(R, t, 7, n - 8, True, 50.0)
            assert nn == no == n - 8
            TC.same_bits(Hn, Ho), TC.same_bits(bn, bo), TC.same_bits([cn], [co])


def _long_parts(c, tag, motion, huber, thr):
    """(f, J) of every point of a long list under a motion, restated once"""
    R, t = TC.MOTIONS[motion]
    pts = c[tag + "_pts"]
    f = TR.residuals(c["images0"][0], c["mask"], c["P"], pts, _T4(R, t), 0, len(pts), huber, thr)
    J = TR.jacobian(c["images0"], c["mask"], c["P"], pts, R, t, 0, len(pts))
    return f, J


@pytest.mark.parametrize("prob", PROBLEMS, ids=_pid)
def test_oracle_equals_the_restatement_on_the_long_problem(prob):
    """2049 points: more than one staging round of the wide sums, an owner's fifth point, the tails around 1024, 1280 and 2048"""
    c = TC.problem(*prob)
    for tag in ("long", "long_free"):
        assert c[tag + "_xyz"].shape == (TC.LONG_N, 3)
        trk = _oracle(c, c[tag + "_xyz"])
        for motion, (R, t) in TC.MOTIONS.items():
            for name, huber, thr in (TC.NORMS[0], TC.NORMS[1]):
                f, J = _long_parts(c, tag, motion, huber, thr)
                assert trk.residuals(_T4(R, t), 0, TC.LONG_N, huber, thr).tobytes() == f.tobytes()
                TC.same_bits(trk.jacobian(R, t, 0, TC.LONG_N), J, (tag, motion))
                finite = []
                for off, cnt in [(0, k) for k in TC.LONG_N_POINTS] + [(3, k) for k in TC.COUNTS] + [(1024, 1024), (1024, 1025), (1025, 1025)]:
                    Ho, bo, co, no = trk.normal_equations(R, t, off, cnt, huber, thr)
                    m = max(0, min(cnt, TC.LONG_N - off))
                    Hr, br, cr = TR.sum_normal_equations(J[off:off + m], f[off:off + m])
                    assert no == m
                    TC.same_bits(Ho, Hr, (tag, motion, name, off, cnt)), TC.same_bits(bo, br), TC.same_bits([co], [cr])
                    finite.append(bool(np.isfinite(Ho).all() and np.isfinite(bo).all() and np.isfinite(co)))
                    if m > 300:
                        assert np.isfinite(co) and co > 0 and (not finite[-1] or np.linalg.eigvalsh(Ho).min() > 0)
                if tag == "long_free":
                    assert all(finite), (motion, name)            # a finite H, b and cost are compared
                elif motion == "moved":
                    assert not all(finite)                        # ... and sums that the NaN rows reach


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------
def test_normal_equations_depend_on_the_order_of_the_points():
    c = TC.problem("plain", 96, 64)
    f, J = _long_parts(c, "long_free", "moved", True, 50.0)
    fwd = TR.sum_normal_equations(J, f)
    rev = TR.sum_normal_equations(J[::-1], f[::-1])
    assert fwd[0].tobytes() != rev[0].tobytes() and fwd[1].tobytes() != rev[1].tobytes()
    assert np.allclose(fwd[0], rev[0], rtol=1e-9) and np.allclose(fwd[1], rev[1], rtol=1e-6, atol=1e-6 * np.abs(fwd[1]).max())
    trk = _oracle(c, np.ascontiguousarray(c["long_free_xyz"][::-1]))
    R, t = TC.MOTIONS["moved"]
    Ho, bo, co, _ = trk.normal_equations(R, t, 0, TC.LONG_N, True, 50.0)
    assert Ho.tobytes() == rev[0].tobytes() and bo.tobytes() == rev[1].tobytes() and Ho.tobytes() != fwd[0].tobytes()


@pytest.mark.parametrize("W,H", TC.SIZES)
def test_skew_terms_change_the_jacobian(W, H):
    """the same points under the skewed and under the ideal P: P12, P21, P14, P24 and P[r][3] are evaluated with non-zero operands"""
    c = TC.problem("skewed", W, H)
    P0 = TC.problem("plain", W, H)["P"]
    assert all(c["P"][i, j] != 0 and P0[i, j] == 0 for i, j in ((0, 1), (1, 0), (0, 3), (1, 3)))
    for motion, (R, t) in TC.MOTIONS.items():
        n = len(c["pts"])
        Js = TR.jacobian(c["images0"], c["mask"], c["P"], c["pts"], R, t, 0, n)
        Jp = TR.jacobian(c["images0"], c["mask"], P0, c["pts"], R, t, 0, n)
        valid = np.array([i["valid"] and i["interp_ok"] for i in TC.infos(c, motion)]) & np.isfinite(Js).all(axis=1) & np.isfinite(Jp).all(axis=1)
        changed = (Js != Jp).any(axis=1)
        assert valid.sum() > 200 and changed[valid].mean() >= 0.5, (motion, valid.sum(), changed[valid].mean())


# ---- the reference pin -------------------------------------------------------------------------------------------------------------
PINS = [(v, W, H, m) for v, W, H in PROBLEMS for m in TC.MOTIONS]


def _key(pin):
    return f"{pin[0]}_{pin[1]}x{pin[2]}_{pin[3]}"


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ref_track_cases.npz"))    # a missing fixture is a failure


@pytest.mark.parametrize("pin", PINS, ids=_key)
def test_fixture_was_recorded_on_these_inputs(pin, golden):
    c = TC.problem(*pin[:3])
    keep, why = TC.pinned(c, pin[3])
    assert np.array_equal(TC.input_digest(c, pin[3]), golden[_key(pin) + "_sha"]), f"the generator of {_key(pin)} drifted"
    assert keep.mean() >= 0.8 and len(golden[_key(pin) + "_order"]) == keep.sum()
    assert {w for w in why if w} <= set(TC.UNPINNED_KINDS)
    R, t = TC.MOTIONS[pin[3]]
    assert golden[_key(pin) + "_R"].tobytes() == np.asarray(R, np.float64).tobytes()      # setProblem derived the motion itself
    assert golden[_key(pin) + "_t"].tobytes() == np.asarray(t, np.float64).tobytes()


def check_against_fixture(c, motion, g, key):
    keep, _ = TC.pinned(c, motion)
    order = g[key + "_order"]
    xyz = c["xyz"][keep][order]                                  # the order the reference's shuffle produced
    trk = _oracle(c, xyz)
    for norm, huber in (("huber", True), ("l2", False)):
        for i in (0, 1):
            f = trk.residuals(g[f"{key}_{norm}_T{i}"], 0, len(xyz), huber, 50.0)
            assert f.tobytes() == g[f"{key}_{norm}_f{i}"].tobytes(), (key, norm, i)
        J, ref = trk.jacobian(g[key + "_R"], g[key + "_t"], 0, len(xyz)), g[f"{key}_{norm}_J"]
        assert J.shape == ref.shape and np.array_equal(np.isnan(J), np.isnan(ref)), (key, norm)
        ok = ~np.isnan(J)
        assert np.array_equal(J[ok], ref[ok]), (key, norm)
        sign = (np.signbit(J) != np.signbit(ref)) & ok
        assert sign.any() and (J[sign] == 0).all() and (ref[sign] == 0).all() and not np.signbit(ref[sign]).any(), (key, norm)
    return len(xyz)


@pytest.mark.parametrize("pin", PINS, ids=_key)
def test_oracle_agrees_with_the_reference_on_the_pinned_points(pin, golden):
    c = TC.problem(*pin[:3])
    if not np.array_equal(TC.input_digest(c, pin[3]), golden[_key(pin) + "_sha"]):
        pytest.skip("the fixture was recorded on other inputs (test_fixture_was_recorded_on_these_inputs fails)")
    n = check_against_fixture(c, pin[3], golden, _key(pin))
    assert n >= 0.8 * len(c["xyz"])
    f0, f1 = golden[_key(pin) + "_huber_f0"], golden[_key(pin) + "_huber_f1"]
    assert (f0 != f1).mean() > 0.5 and np.abs(golden[_key(pin) + "_l2_J"][np.isfinite(golden[_key(pin) + "_l2_J"])]).max() > 100


@pytest.mark.parametrize("pin", PINS, ids=_key)
def test_live_reference_reproduces_the_crafted_fixture(pin, golden):
    from oracle import ref as R
    if not os.path.isdir(os.path.join(R.REFERENCE, "esvo_core", "src")):
        pytest.skip("reference tree not present (GPU box): the fixture is the pin")
    sys.path.insert(0, GOLDEN)
    import make_ref_fixtures as mk
    c = TC.problem(*pin[:3])
    for f, a in mk.run_track_case(c, pin[3]).items():
        TC.same_bits(a, golden[f"{_key(pin)}_{f}"], f) if a.dtype == np.float64 else np.testing.assert_array_equal(a, golden[f"{_key(pin)}_{f}"])
