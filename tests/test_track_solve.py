"""esvo_track_solve: the tracker's registration loop with the batch schedule and a trace, on the host (on_device = 0: today's
esvo_hip::gauss_newton_register over one launch per evaluation, plus a recorder) and in ONE kernel launch (on_device = 1).

  CPU   esvo_track_sizes against the ctypes bindings; gauss_newton_register with the trace sink attached returns the untraced
        driver's bytes (tests/cpp/gn_trace_oracle.cpp against gn_driver_oracle.cpp), and its trace is the one a trace-emitting
        copy of closed_loop.lm_gn_loop writes: the same trial in every iteration.
  GPU   on_device = 1 == on_device = 0 bit for bit -- pose, rms, iterations, ok, stop and every trace record -- on a case list
        whose HOST traces are shown to reach every branch of the loop; on_device = 0 with one batch == esvo_track_register;
        the error paths; the closed loop with the device registration reproduces the closed loop without it.

The problem is tests/golden/ref_track.npz as tests/test_track_normal.py::_problem sets it up (346 x 260 negated Time Surface,
700 reference points, kernelSize 5); the start poses are I, 0 and the *_R0 / *_t0 entries of tests/golden/ref_track_solve.npz.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from esvo_amd import abi, calib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _problem():
    from oracle import oracle as O
    g = np.load(os.path.join(GOLDEN, "ref_track.npz"))
    rig = calib.dataset_rig("upenn")
    n, order = int(g["n"]), g["order"]
    trk = O.OracleTracker(rig)
    trk.set_current(g["ts_left"], 5)
    xyz = g["xyz_world"][order][:n]
    trk.set_reference(xyz, g["T_world_ref"])
    return g, rig, trk, xyz


def _starts():
    s = np.load(os.path.join(GOLDEN, "ref_track_solve.npz"))
    d = {"I0": (np.eye(3), np.zeros(3))}
    for name in ("truth", "pert2mm", "pert20mm"):
        d[name] = (s[f"{name}_R0"], s[f"{name}_t0"])
    return d


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_track_sizes_match_bindings():
    from esvo_amd import lib
    assert lib.track_sizes() == [C.sizeof(abi.TrackSolveParamsStruct), C.sizeof(abi.TrackIterStruct),
                                 C.sizeof(abi.TrackSolveInfoStruct), 64]
    assert abi.TRACK_SOLVE_MAX_ITERATIONS == 64 and abi.TRACK_ITER_DTYPE.itemsize == C.sizeof(abi.TrackIterStruct)
    assert lib.abi_sizes()[7] == 8                                    # additive: the ABI number stays


def _build(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "oracle"), "-lesvo_oracle", f"-Wl,-rpath,{os.path.join(ROOT, 'oracle')}"])
    return exe


def _run(exe, tmp_path, rig, ts_left, xyz, T_world_ref, R0, t0, iters, batch):
    """-> the output file's bytes (gn_driver_oracle: 108; gn_trace_oracle: the same 108 + stop, ok, records)"""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2i", rig.width, rig.height))
        f.write(np.asarray(rig.left.P, "<f8").reshape(12).tobytes())
        f.write(np.ascontiguousarray(ts_left, np.uint8).tobytes())
        f.write(struct.pack("<Q", len(xyz)))
        f.write(np.ascontiguousarray(xyz, "<f4").tobytes())
        f.write(np.asarray(T_world_ref, "<f8").reshape(16).tobytes())
        f.write(np.asarray(R0, "<f8").reshape(9).tobytes())
        f.write(np.asarray(t0, "<f8").reshape(3).tobytes())
        f.write(struct.pack("<2i", iters, batch))
    rc = subprocess.call([exe, fin, fout])
    assert rc in (0, 1), rc            # gn_driver_oracle returns 1 for Registration::ok == false
    return open(fout, "rb").read()


def _traced_numpy_loop(evaluate, R_, t_, iters=12, damping=1e-3):
    """closed_loop.lm_gn_loop, emitting one (cost, lambda, pick) per iteration: the trial it took"""
    from esvo_amd.closed_loop import cayley2rot, orth
    H, b, cost, n = evaluate(R_, t_)
    lam, trace = damping, []
    for it in range(iters):
        accepted, pick = False, -1
        for k in range(6):
            dx = np.linalg.solve(H + lam * np.diag(np.diag(H)) + 1e-9 * np.eye(6), -b)
            dR = cayley2rot(dx[:3])
            Rn, tn = orth(dR @ R_), dx[3:] + dR @ t_
            Ht, bt, cost_t, nt = evaluate(Rn, tn)
            pred = -(2.0 * b @ dx + dx @ H @ dx)
            if pred > 0 and (cost - cost_t) >= 1e-4 * pred:
                accepted, pick = True, k
                break
            if k < 5:
                lam *= 10.0
        trace.append((cost, lam, pick))
        if not accepted:
            break
        R_, t_, H, b, cost, n = Rn, tn, Ht, bt, cost_t, nt
        lam = max(lam / 10.0, damping)
        if np.linalg.norm(dx) < 1e-6:
            break
    return trace


def test_traced_driver_returns_the_untraced_bytes_and_the_numpy_loops_trials(tmp_path):
    import copy
    from oracle import oracle as O
    g, rig, _, xyz = _problem()
    plain, traced = _build(tmp_path, "gn_driver_oracle"), _build(tmp_path, "gn_trace_oracle")
    rig2 = copy.copy(rig)                       # the drivers' oracle instance has no mask: the numpy loop on the same camera
    rig2.left = copy.copy(rig.left)
    rig2.left.rect_mask = None
    trk = O.OracleTracker(rig2)
    trk.set_current(g["ts_left"], 5)
    trk.set_reference(xyz, g["T_world_ref"])

    def evaluate(R, t):
        return trk.normal_equations(R, t, 0, len(xyz), huber=True, huber_threshold=50.0)

    picks = set()
    for name, (R0, t0) in _starts().items():
        for batch in (0, 300):
            a = _run(plain, tmp_path, rig, g["ts_left"], xyz, g["T_world_ref"], R0, t0, 12, batch)
            b = _run(traced, tmp_path, rig, g["ts_left"], xyz, g["T_world_ref"], R0, t0, 12, batch)
            assert len(a) == 108 and b[:108] == a, (name, batch)          # R, t, rms, iterations: byte for byte
            iters, stop, ok = struct.unpack_from("<3i", b, 104)
            rec = np.frombuffer(b, abi.TRACK_ITER_DTYPE, iters, 116)
            assert len(b) == 116 + 40 * iters and ok == 1 and stop in (0, 1, 2)
            assert (rec["n"] == (300 if batch else len(xyz))).all()
            assert list(rec["offset"]) == [(it % 2) * 300 if batch else 0 for it in range(iters)]     # 700 // 300 = 2 batches
            assert ((rec["trials"] == rec["pick"] + 1) | ((rec["pick"] == -1) & (rec["trials"] == 6))).all()
            if batch:
                continue
            ref = _traced_numpy_loop(evaluate, R0, t0, 12)
            assert len(ref) == iters, (name, len(ref), iters)
            for it, (cost, lam, pick) in enumerate(ref):
                assert rec["pick"][it] == pick and rec["lambda"][it] == lam, (name, it, rec[it], (cost, lam, pick))
                assert abs(rec["cost"][it] - cost) <= 1e-9 * cost, (name, it)
            picks |= set(int(p) for p in rec["pick"])
            assert (stop == 2) == (rec["pick"][-1] == -1)
    assert -1 in picks and 0 in picks and max(picks) >= 3     # the starts reach a rejected round and an exhausted iteration


# ---------------------------------------------------------------------------------------------------------------- GPU
# (start, n_points, batch_size, huber, max_iterations); 700 points in the cloud
CASES = ([(s, 700, b, True, 12) for s in ("I0", "truth", "pert2mm", "pert20mm") for b in (0, 300)]
         + [("I0", 700, 0, False, 12)]
         + [("I0", n, 0, True, 12) for n in (0, 1, 5, 64, 256, 257)]       # 257: the first count at which a thread owns two points
         + [("I0", 700, 0, True, 1), ("I0", 700, 0, True, 64), ("I0", 700, 300, True, 64)]
         + [("I0", 5000, 0, True, 12), ("I0", 5000, 300, True, 12)])        # more points than the cloud holds: clamped


def _id(c):
    return f"{c[0]}-n{c[1]}-b{c[2]}-{'huber' if c[3] else 'l2'}-it{c[4]}"


@pytest.fixture(scope="module")
def solver():
    """one small handle with the problem set, and the HOST path's result of every case, computed once"""
    from esvo_amd import lib, params
    g, rig, _, xyz = _problem()
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], rig)
    dev = lib.Esvo(p, rig, device=0)
    dev.track_set_current(g["ts_left"], 5)
    dev.track_set_reference(xyz, g["T_world_ref"])
    starts = _starts()

    def solve(case, on_device):
        s, n, b, huber, iters = case
        return dev.track_solve(n, starts[s][0], starts[s][1], batch_size=b, huber=huber, huber_threshold=50.0, max_iterations=iters,
                               damping=1e-3, on_device=on_device)
    host = {c: solve(c, False) for c in CASES}
    yield dev, solve, host, starts
    dev.close()


def _info_tuple(info):
    return (struct.pack("<d", info.rms), info.iterations, info.ok, info.stop)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gpu_one_launch_equals_the_host_loop_bit_for_bit(solver, case):
    dev, solve, host, _ = solver
    Rh, th, ih, trh = host[case]
    Rd, td, idv, trd = solve(case, True)
    print(_id(case), "host:", ih.iterations, ih.stop, ih.launches, list(trh["pick"]), "device:", idv.iterations, idv.stop,
          list(trd["pick"]))
    assert idv.launches == 1
    assert _info_tuple(idv) == _info_tuple(ih), (_info_tuple(idv), _info_tuple(ih))
    assert Rd.tobytes() == Rh.tobytes() and td.tobytes() == th.tobytes(), (Rd - Rh, td - th)
    assert len(trd) == len(trh) == ih.iterations
    for it in range(len(trh)):
        assert trd[it:it + 1].tobytes() == trh[it:it + 1].tobytes(), (it, trd[it], trh[it])
    n_eff = min(case[1], 700)
    batched = case[2] and case[2] < n_eff
    assert (trh["n"] == (case[2] if batched else n_eff)).all()


@pytest.mark.gpu
def test_gpu_case_list_reaches_every_branch_of_the_loop(solver):
    """read off the HOST path's traces: the three trials of the first round, the second round, both ways a registration ends
    early or late, and the alternating batch"""
    _, _, host, _ = solver
    picks, stops, alternates = set(), set(), False
    for case, (_, _, info, tr) in host.items():
        assert info.iterations == len(tr) and 1 <= info.iterations <= case[4]
        picks |= set(int(p) for p in tr["pick"])
        stops.add((info.stop, info.iterations < case[4]))
        if case[2] == 300 and len(tr) >= 4:
            alternates |= list(tr["offset"]) == [(it % 2) * 300 for it in range(len(tr))]
    print("picks", sorted(picks), "stops", sorted(stops))
    assert {0, 1, 2} <= picks and any(p >= 3 for p in picks)
    assert (2, True) in stops                     # no trial acceptable, before the iteration limit
    assert any(s == 0 for s, _ in stops)          # ran to the iteration limit
    assert alternates


@pytest.mark.gpu
def test_gpu_host_path_with_one_batch_is_track_register(solver):
    dev, _, host, starts = solver
    for case in CASES:
        s, n, b, huber, iters = case
        if b:
            continue
        R1, t1, rms1, it1 = dev.track_register(n, starts[s][0], starts[s][1], huber=huber, huber_threshold=50.0, max_iterations=iters,
                                               damping=1e-3)
        R0, t0, info, _ = host[case]
        assert R1.tobytes() == R0.tobytes() and t1.tobytes() == t0.tobytes(), case
        assert struct.pack("<d", rms1) == struct.pack("<d", info.rms) and it1 == info.iterations, case


@pytest.mark.gpu
def test_gpu_singular_damped_system_ends_both_paths_alike(solver):
    """A damped system the elimination refuses (here: a diagonal that overflows) with no acceptable trial before it ends the
    registration with ok = 0, stop = 3 and the start pose, on the host as in the kernel: as the first trial of an iteration
    (damping inf), and as the third one behind two trials whose steps are too small to pay."""
    dev, _, _, _ = solver
    H = dev.track_normal_equations(np.eye(3), np.zeros(3), 0, 700)[0]
    third = np.finfo(np.float64).max / (50.0 * np.diag(H).max())      # x 100 overflows, x 10 does not
    for damping, trials in ((np.inf, 0), (third, 2)):
        out = [dev.track_solve(700, np.eye(3), np.zeros(3), damping=damping, on_device=d) for d in (False, True)]
        (Rh, th, ih, trh), (Rd, td, idv, trd) = out
        assert (ih.ok, ih.stop, ih.iterations) == (0, 3, 1) and trh["pick"][0] == -1 and trh["trials"][0] == trials, (ih.stop, trh)
        assert np.array_equal(Rh, np.eye(3)) and not th.any()
        assert _info_tuple(idv) == _info_tuple(ih) and idv.launches == 1
        assert Rd.tobytes() == Rh.tobytes() and td.tobytes() == th.tobytes() and trd.tobytes() == trh.tobytes(), (trd, trh)


@pytest.mark.gpu
def test_gpu_optional_outputs_and_error_paths(solver):
    from esvo_amd import lib, params
    dev, _, host, _ = solver
    for on_device in (0, 1):
        for iters in (0, 65):
            with pytest.raises(lib.EsvoError) as e:
                dev.track_solve(700, np.eye(3), np.zeros(3), max_iterations=iters, on_device=on_device)
            assert e.value.code == -1            # ESVO_ERR_INVALID_ARG
        prm = abi.TrackSolveParamsStruct(700, 0, 7, 12, on_device, 0, 50.0, 1e-3)     # no such norm
        R, t = np.eye(3).reshape(9).copy(), np.zeros(3)
        assert dev.lib.esvo_track_solve(dev.h, C.addressof(prm), R.ctypes.data, t.ctypes.data, None, None, 0) == -1
        # info and trace may be NULL; at most trace_cap records are written
        prm = abi.TrackSolveParamsStruct(700, 0, 1, 12, on_device, 0, 50.0, 1e-3)
        assert dev.lib.esvo_track_solve(dev.h, C.addressof(prm), R.ctypes.data, t.ctypes.data, None, None, 0) == 0
        Rh, th, ih, trh = host[("I0", 700, 0, True, 12)]
        assert R.tobytes() == Rh.tobytes() and t.tobytes() == th.tobytes()
        R, t = np.eye(3).reshape(9).copy(), np.zeros(3)
        tr = np.zeros(3, abi.TRACK_ITER_DTYPE)
        tr["pick"] = 77
        assert dev.lib.esvo_track_solve(dev.h, C.addressof(prm), R.ctypes.data, t.ctypes.data, None, tr.ctypes.data, 2) == 0
        assert ih.iterations > 2 and tr[:2].tobytes() == trh[:2].tobytes() and tr["pick"][2] == 77
    g, rig, _, xyz = _problem()
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], rig)
    fresh = lib.Esvo(p, rig, device=0)
    fresh.track_set_reference(xyz, g["T_world_ref"])
    for on_device in (False, True):
        with pytest.raises(lib.EsvoError) as e:
            fresh.track_solve(700, np.eye(3), np.zeros(3), on_device=on_device)
        assert e.value.code == -6                # ESVO_ERR_STATE: no esvo_track_set_current yet
    fresh.close()


@pytest.mark.gpu
def test_gpu_closed_loop_with_the_device_registration_reproduces_the_host_one():
    from esvo_amd import closed_loop
    a = closed_loop.run(n_ticks=6, device_register=False)
    b = closed_loop.run(n_ticks=6, device_register=True)
    assert np.array(a["poses"]).tobytes() == np.array(b["poses"]).tobytes()
    assert a["points"] == b["points"] and a["map"].tobytes() == b["map"].tobytes()
