"""The tracker's point evaluation on the device (esvo_amd/csrc/kernels_track.hip: trk_reproject, trk_interp, trk_residual,
trk_jacobian_row, the reference kernel, track_normal_kernel and trk_normal_sums_wide inside track_solve_kernel) on the crafted
problems of tests/track_cases.py, held to the CPU oracle.  tests/test_track_cases.py shows on the CPU that the cases reach the
branches they name, that the oracle equals a plain restatement on these very inputs, and that it agrees with the reference's own
RegProblemLM on the pinned points.

Equality is byte for byte where no NaN occurs; elsewhere the NaN positions are equal and the remaining bytes are equal
(track_cases.same_bits).  The reference is set through track_set_reference only: a device-resident cloud comes out of mapper ticks
(map_cloud_build), no call uploads crafted points into it, so the second route stays with tests/test_gpu_track_from_cloud.py.
Handles are shared per rig variant and image size and closed at module end.

What the module notices (scratch builds of kernels_track.hip with one token changed, none of which can move an address or an index;
every row was built and run on an MI355X together with the older tracker tests -- test_gpu_track, test_track_normal, test_track_solve,
test_gpu_track_from_cloud; points: test_point_evaluation_equals_the_oracle, long: test_normal_equations_of_the_long_problem_equal_the_oracle,
solve: test_one_launch_solve_equals_the_host_loop_on_the_long_problem; `plain, masked` = those rig variants at both sizes):
  `x[0] > W-1` -> `>=`                    points, long: plain, masked (x == W-1 exactly; the residual is 255 either way, what differs  older: none
                                          is the sign of the zeros in the Jacobian row: -0 everywhere for a rejected point).  Not skewed:
                                          no exact hit there (track_cases).  solve: none -- signed zeros reach no sum
  `x[0] < 0.0` -> `<= 0.0`                points, long, solve: plain, masked (x == -0.0 and +0.0 rejected: residual 255, a row of zeros)    older: none
  `mask < 125` -> `<= 125`                points, long, solve: masked (the byte 125)                                                     older: none
  `r > huber_threshold` -> `>=`           points: all six, at huber_threshold == 0 with r == 0 only (w = 0 / 0).  At r == thr == 50 the    older: none
                                          mutant's w = thr / r is exactly 1: the same bits, unobservable by any input with thr > 0
  `gx / 8` -> `* 0.125`                   none, as expected: 8 is a power of two, both give the same bits for every finite gx             older: none
  `P12` -> 0 in `D[0][1]`                 points, long: skewed (1674 of 2250 Jacobian entries)                                            older: none
  `P14` dropped from `D[0][2]`            points, long: skewed (846 entries)                                                              older: none
  `e[6+j]` using `p[1]`                   points, long: all six                                                                           older: test_gpu_track (both),
                                                                                                                                          test_track_normal's gpu test
  trk_normal_sums_wide's owner loop       solve: all six (rms one ulp off at n_points 1023, the first case); points, long: none -- they      older: test_track_solve: the eight
    taken in descending q                 do not run that kernel                                                                          n >= 700 one-batch cases, the error
                                                                                                                                          paths test and the closed loop
The last row corrects the plan: tests/test_track_solve.py does reach an owner's second and third point (700 > 256), so it notices a
reversed order; what is new here is the second staging round, its tail and the fifth point (n_points 1025 .. 2049).
"""
import struct

import numpy as np
import pytest

import reproj_restated as RR
import track_cases as TC

pytestmark = pytest.mark.gpu
PROBLEMS = [(v, W, H) for v in TC.VARIANTS for W, H in TC.SIZES]
_HANDLES = {}


def _pid(p):
    return f"{p[0]}-{p[1]}x{p[2]}"


def _handle(c):
    from esvo_amd import lib, params
    key = (c["variant"], c["W"], c["H"])
    if key not in _HANDLES:
        p, _ = params.make_params(params.PRESETS["mapping_upenn"], c["rig"])
        _HANDLES[key] = lib.Esvo(p, c["rig"])
    return _HANDLES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for dev in _HANDLES.values():
        dev.close()
    _HANDLES.clear()


def _T4(R, t):
    T = np.eye(4)
    T[:3] = RR.pose_left_ref(R, t)
    return T


def _pair(c, xyz, ksize=0):
    """(device handle, oracle) with the problem's Time Surface and the given reference set on both"""
    from oracle import oracle as O
    dev = _handle(c)
    trk = O.OracleTracker(c["rig"])
    trk.set_current(c["ts"], ksize)
    dev.track_set_current(c["ts"], ksize)
    trk.set_reference(xyz, TC.I4)
    dev.track_set_reference(xyz, TC.I4)
    return dev, trk


def _same_sums(got, want, label):
    (Hg, bg, cg, ng), (Hw, bw, cw, nw) = got, want
    assert ng == nw, (label, ng, nw)
    TC.same_bits(Hg, Hw, label), TC.same_bits(bg, bw, label), TC.same_bits([cg], [cw], label)


def _four_poses():
    from esvo_amd import closed_loop
    rng = np.random.default_rng(5)
    Rs = [TC.MOTIONS["identity"][0], TC.MOTIONS["moved"][0]] + [closed_loop.orth(closed_loop.cayley2rot(rng.normal(0, 0.02, 3))) for _ in range(2)]
    ts = [TC.MOTIONS["identity"][1], TC.MOTIONS["moved"][1]] + [rng.normal(0, 0.03, 3) for _ in range(2)]
    return np.stack(Rs), np.stack(ts)


# ---- 1. per-point calls ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob", PROBLEMS, ids=_pid)
def test_point_evaluation_equals_the_oracle(prob):
    c = TC.problem(*prob)
    n = len(c["xyz"])
    Rs, ts = _four_poses()
    for ksize in ((0, 5) if prob == ("plain", 96, 64) else (0,)):
        dev, trk = _pair(c, c["xyz"], ksize)
        for a, b in zip(dev.track_images(), trk.images()):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        if ksize == 0:
            assert dev.track_images()[0].tobytes() == c["images0"][0].tobytes()
        for motion, (R, t) in TC.MOTIONS.items():
            T = _T4(R, t)
            for off, cnt in TC.batches(n):
                TC.same_bits(dev.track_jacobian(R, t, off, cnt), trk.jacobian(R, t, off, cnt), (ksize, motion, off, cnt))
                for name, huber, thr in TC.NORMS:
                    label = (ksize, motion, name, off, cnt)
                    g, o = dev.track_residuals(T, off, cnt, huber, thr), trk.residuals(T, off, cnt, huber, thr)
                    assert len(g) == len(o) == max(0, min(cnt, n - off)) and g.tobytes() == o.tobytes(), label
                    _same_sums(dev.track_normal_equations(R, t, off, cnt, huber, thr), trk.normal_equations(R, t, off, cnt, huber, thr), label)
        for name, huber, thr in TC.NORMS[:2]:                     # each pose of a 4-pose launch equals that pose alone
            for off, cnt in ((0, n), (7, n - 8)):
                Hb, bb, cb, nb = dev.track_normal_equations_batch(Rs, ts, off, cnt, huber, thr)
                for q in range(4):
                    _same_sums((Hb[q], bb[q], cb[q], nb), dev.track_normal_equations(Rs[q], ts[q], off, cnt, huber, thr), (ksize, name, off, cnt, q))
                    _same_sums((Hb[q], bb[q], cb[q], nb), trk.normal_equations(Rs[q], ts[q], off, cnt, huber, thr), (ksize, name, off, cnt, q))


# ---- 2. the long problem: counts above 700 in track_normal_kernel ---------------------------------------------------------------------
LONG_BATCHES = [(0, k) for k in TC.LONG_N_POINTS] + [(3, k) for k in TC.COUNTS] + [(1024, 1024), (1024, 1025), (1025, 1025), (2048, 5)]


@pytest.mark.parametrize("prob", PROBLEMS, ids=_pid)
def test_normal_equations_of_the_long_problem_equal_the_oracle(prob):
    c = TC.problem(*prob)
    Rs, ts = _four_poses()
    for tag in ("long", "long_free"):
        dev, trk = _pair(c, c[tag + "_xyz"])
        for motion, (R, t) in TC.MOTIONS.items():
            TC.same_bits(dev.track_jacobian(R, t, 0, TC.LONG_N), trk.jacobian(R, t, 0, TC.LONG_N), (tag, motion))
            for name, huber, thr in TC.NORMS[:2]:
                assert dev.track_residuals(_T4(R, t), 0, TC.LONG_N, huber, thr).tobytes() == trk.residuals(_T4(R, t), 0, TC.LONG_N, huber, thr).tobytes()
                for off, cnt in LONG_BATCHES:
                    _same_sums(dev.track_normal_equations(R, t, off, cnt, huber, thr), trk.normal_equations(R, t, off, cnt, huber, thr),
                               (tag, motion, name, off, cnt))
        Hb, bb, cb, nb = dev.track_normal_equations_batch(Rs, ts, 0, TC.LONG_N)
        for q in range(4):
            _same_sums((Hb[q], bb[q], cb[q], nb), trk.normal_equations(Rs[q], ts[q], 0, TC.LONG_N), (tag, q))


# ---- 3. the solver on the long problem: trk_normal_sums_wide beyond one staging round -------------------------------------------------
def _info_tuple(info):
    return (struct.pack("<d", info.rms), info.iterations, info.ok, info.stop)


def _same_solve(host, device, label):
    (Rh, th, ih, trh), (Rd, td, idv, trd) = host, device
    assert idv.launches == 1
    assert _info_tuple(idv) == _info_tuple(ih), (label, _info_tuple(idv), _info_tuple(ih))
    assert Rd.tobytes() == Rh.tobytes() and td.tobytes() == th.tobytes(), (label, Rd - Rh, td - th)
    assert len(trd) == len(trh) == ih.iterations
    for it in range(len(trh)):
        assert trd[it:it + 1].tobytes() == trh[it:it + 1].tobytes(), (label, it, trd[it], trh[it])


@pytest.mark.parametrize("prob", PROBLEMS, ids=_pid)
def test_one_launch_solve_equals_the_host_loop_on_the_long_problem(prob):
    """on the NaN-free list: pose, rms, iterations, ok, stop and every trace record, at every point count and batch size around the
    staging size of 1024 points and the owners' stride of 256; the host path's first cost is the oracle's for the same batch, which
    ties the wide sums to the oracle and not only to the other device path"""
    c = TC.problem(*prob)
    dev, trk = _pair(c, c["long_free_xyz"])
    picks, iterations = set(), []
    for start, (R0, t0) in TC.MOTIONS.items():
        for n_points in TC.LONG_N_POINTS:
            for batch in TC.LONG_BATCHES:
                label = (start, n_points, batch)
                host = dev.track_solve(n_points, R0, t0, batch_size=batch, on_device=False)
                _same_solve(host, dev.track_solve(n_points, R0, t0, batch_size=batch, on_device=True), label)
                tr = host[3]
                cnt = batch if batch and batch < n_points else n_points
                assert tr["n"][0] == cnt and tr["offset"][0] == 0
                cost = trk.normal_equations(R0, t0, 0, cnt)[2]
                assert np.isfinite(cost) and struct.pack("<d", tr["cost"][0]) == struct.pack("<d", cost), (label, tr["cost"][0], cost)
                picks |= set(int(p) for p in tr["pick"])
                iterations.append(host[2].iterations)
    print(_pid(prob), "picks", sorted(picks), "iterations", min(iterations), "..", max(iterations))
    assert max(iterations) >= 3 and any(p >= 0 for p in picks)    # the solves are no one-step affairs


# ---- 4. every point invalid ------------------------------------------------------------------------------------------------------------
def test_all_invalid_problem_ends_both_paths_alike():
    """H = 0 and b = 0: whatever the host loop makes of it (read from its trace, not assumed), the kernel makes the same.  (On an
    MI355X the host loop ends with ok = 1, stop = 2 after one iteration of six trials, none picked, with and without batches: the
    step of every damping is zero and pays nothing.)"""
    c = TC.problem("plain", 96, 64)
    xyz = TC.all_invalid_points()
    dev, trk = _pair(c, xyz)
    R0, t0 = np.eye(3), np.zeros(3)
    got, want = dev.track_normal_equations(R0, t0, 0, len(xyz)), trk.normal_equations(R0, t0, 0, len(xyz))
    _same_sums(got, want, "all invalid")
    assert not got[0].any() and not got[1].any() and abs(got[2] - len(xyz) * 50.0 * 255.0) < 1e-6    # f = sqrt(50 / 255) 255 on every point
    for batch in (0, 100):
        host = dev.track_solve(len(xyz), R0, t0, batch_size=batch, on_device=False)
        device = dev.track_solve(len(xyz), R0, t0, batch_size=batch, on_device=True)
        ih, trh = host[2], host[3]
        print("all invalid, batch", batch, "host: ok", ih.ok, "stop", ih.stop, "iterations", ih.iterations, "trials", list(trh["trials"]),
              "picks", list(trh["pick"]))
        _same_solve(host, device, ("all invalid", batch))
        assert (device[2].ok, device[2].stop, device[2].iterations) == (ih.ok, ih.stop, ih.iterations)
        assert list(device[3]["trials"]) == list(trh["trials"]) and list(device[3]["pick"]) == list(trh["pick"])
