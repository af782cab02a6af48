"""Closed-loop harness: SGM bootstrap -> tracker -> mapper, all three on the device.

The tracker's optimiser is host-side C++ inside the library (esvo_track_register: a damped Gauss-Newton over
esvo_track_normal_equations -- the same residual and Jacobian RegProblemLM hands to Eigen's LM,
esvo_core/src/core/RegProblemLM.cpp:93-236, reduced to J^T J / J^T f on the device);
the poses the mapper fuses with are the tracker's estimates, never ground truth after the bootstrap pose.

Property of the formulation worth knowing when reading the bars: the map sits on the LEADING edge of the
Time Surface (the newest events), the blurred negative surface has its minimum about 0.4 trail lengths
BEHIND it, so the registered pose lags the true one by a constant ~1.2-1.7 ticks of motion.  With a fixed
reference map the lag stays bounded while the path grows; every re-reference to a map fused with lagged
poses adds one more lag.  The bars below are measured with that in mind.
"""
import time

import numpy as np

from esvo_amd import calib, lib, params, rostime, synth

TICK_NS = 10_000_000


def cayley2rot(c):
    s = 1 + c @ c
    R = np.array([[1 + c[0]**2 - c[1]**2 - c[2]**2, 2*(c[0]*c[1]-c[2]), 2*(c[0]*c[2]+c[1])],
                  [2*(c[0]*c[1]+c[2]), 1 - c[0]**2 + c[1]**2 - c[2]**2, 2*(c[1]*c[2]-c[0])],
                  [2*(c[0]*c[2]-c[1]), 2*(c[1]*c[2]+c[0]), 1 - c[0]**2 - c[1]**2 + c[2]**2]])
    return R / s


def orth(R):
    U, _, Vt = np.linalg.svd(R)
    return U @ Vt


def register(dev, n_points, R_, t_, iters=12, device_register=False):
    """The registration of one frame: the library's driver (esvo_track_register: host C++ over esvo_track_normal_equations,
    the three trial dampings of an iteration in one launch, 224 bytes back per trial).  device_register: the same loop in one
    kernel launch (esvo_track_solve, on_device) -- the same bits, without the host between dependent launches."""
    if device_register:
        R, t, info, _ = dev.track_solve(n_points, R_, t_, batch_size=0, huber=True, huber_threshold=50.0, max_iterations=iters,
                                        damping=1e-3, on_device=True)
        return R, t, info.rms
    R, t, rms, _ = dev.track_register(n_points, R_, t_, huber=True, huber_threshold=50.0, max_iterations=iters, damping=1e-3)
    return R, t, rms


def lm_gn_loop(evaluate, R_, t_, iters=12, damping=1e-3):
    """include/esvo_hip.hpp's gauss_newton_register in numpy (same batch every iteration): Levenberg-damped Gauss-Newton steps
    linearised at x = 0, each accepted only if actual / predicted reduction >= 1e-4 (cost evaluated at the trial pose), the
    damping raised tenfold otherwise (6 attempts), lowered tenfold (not below `damping`) after an accepted step and carried
    over.  The C++ driver evaluates three trial dampings per call; taking the first acceptable one in rising order is what this
    sequential loop does.  evaluate(R, t) -> (H, b, cost, n).  Returns (R, t, rms, iterations)."""
    H, b, cost, n = evaluate(R_, t_)
    it, lam = 0, damping
    for it in range(iters):
        accepted = False
        for _ in range(6):
            dx = np.linalg.solve(H + lam * np.diag(np.diag(H)) + 1e-9 * np.eye(6), -b)
            dR = cayley2rot(dx[:3])
            Rn, tn = orth(dR @ R_), dx[3:] + dR @ t_
            Ht, bt, cost_t, nt = evaluate(Rn, tn)
            pred = -(2.0 * b @ dx + dx @ H @ dx)
            if pred > 0 and (cost - cost_t) >= 1e-4 * pred:
                accepted = True
                break
            lam *= 10.0
        if not accepted:
            break
        R_, t_, H, b, cost, n = Rn, tn, Ht, bt, cost_t, nt
        lam = max(lam / 10.0, damping)
        if np.linalg.norm(dx) < 1e-6:
            break
    return R_, t_, float(np.sqrt(cost / n)) if n else 0.0, it + 1


def register_python(dev, n_points, R_, t_, iters=12):
    """The library's driver (esvo_track_register) restated in Python over esvo_track_residuals / esvo_track_jacobian (two
    synchronous calls and a count x 7 download per evaluation): the cross-check of the C++ one."""
    def evaluate(R, t):
        Tlr = np.eye(4)
        Tlr[:3, :3] = R.T
        Tlr[:3, 3] = -R.T @ t
        r = dev.track_residuals(Tlr, 0, n_points, huber=True, huber_threshold=50.0)
        J = dev.track_jacobian(R, t, 0, n_points)
        return J.T @ J, J.T @ r, float(r @ r), len(r)
    R, t, rms, _ = lm_gn_loop(evaluate, R_, t_, iters)
    return R, t, rms


class _OneGpu:
    """the calls of the loop on one plain handle"""

    def __init__(self, dev):
        self.dev = dev

    def full_left_ts(self):
        pass

    def pointcloud(self):
        return self.dev.get_pointcloud()

    def tick(self, t, stamps, poses):
        self.dev.tick(t, stamps, poses)

    def final_map(self):
        return self.dev.get_map()


class _Band:
    """... on one rank of a band-sharded run (every call here is collective: the ranks make them in the same order)"""

    def __init__(self, dev):
        self.dev = dev

    def full_left_ts(self):
        self.dev.comm_gather_ts(0)         # the tracker reads the WHOLE left Time Surface; a routed rank rendered its rows

    def pointcloud(self):
        return self.dev.comm_gather_pointcloud()   # the whole map's cloud on every rank, merged on the device

    def tick(self, t, stamps, poses):
        self.dev.comm_shard_tick(t, stamps, poses)

    def final_map(self):
        return self.dev.comm_gather_map()


def _loop(rig, st, p, ops, t0, T0, xyz0, n_ticks, reref, verbose=False, device_register=False, device_reference=False,
          reproj_map=False):
    """tracker -> mapper for n_ticks ticks after the bootstrap at t0 (pose T0, reference cloud xyz0); `ops`: _OneGpu / _Band.
    device_reference (one plain handle): a re-reference builds the map's cloud on the device (map_cloud_build) and the tracker
    gathers its 2000 points out of it (track_set_reference_from_cloud) -- the same rng.permutation(n)[:2000] indices as the
    host route takes out of the downloaded cloud, so both routes register against the same points, bit for bit.
    reproj_map: after each registration the tracker's Reproj_Map_Left is drawn on the device for the registered motion
    (track_reprojection_map, the image stays there); out["reproj_inside"] collects its n_inside per tick.  Outside the timed
    spans, and nothing else changes."""
    assert not device_reference or (xyz0 is None and isinstance(ops, _OneGpu)), "the device-resident cloud is a one-GPU handle's"
    dev = ops.dev
    T_est = {t0: T0}
    out = {"pos_err": [], "rot_err_deg": [], "cos": [], "est_len": [], "gt_len": [], "points": [],
           "cycle_ms": [], "track_ms": [], "map_ms": [], "poses": []}
    rng = np.random.default_rng(0)
    t_ref, xyz, sel, R_, t_ = t0, None, None, np.eye(3), np.zeros(3)
    for k in range(1, n_ticks + 1):
        t = t0 + k * TICK_NS
        c0 = time.perf_counter()
        dev.ts_render(0, t, download=False)
        dev.ts_render(1, t, download=False)
        ops.full_left_ts()
        if sel is None or (k - 1) % reref == 0:
            if device_reference:
                sel = rng.permutation(dev.map_cloud_build())[:2000]
            else:
                xyz = xyz0 if (xyz is None and xyz0 is not None) else ops.pointcloud()
                sel = rng.permutation(len(xyz))[:2000]
            t_ref = t - TICK_NS
            R_, t_ = np.eye(3), np.zeros(3)
        dev.track_set_current(None, 5)
        if device_reference:
            dev.track_set_reference_from_cloud(sel, T_est[t_ref])
        else:
            dev.track_set_reference(xyz[sel], T_est[t_ref])
        R_, t_, rms = register(dev, len(sel), R_, t_, device_register=device_register)
        Tw = np.eye(4)
        Tw[:3, :3] = T_est[t_ref][:3, :3] @ R_
        Tw[:3, 3] = T_est[t_ref][:3, :3] @ t_ + T_est[t_ref][:3, 3]
        T_est[t] = Tw
        c1 = time.perf_counter()
        if reproj_map:
            _, n_in = dev.track_reprojection_map(R_, t_, 2000, p.invdepth_min, p.invdepth_max, download=False)
            out.setdefault("reproj_inside", []).append(n_in)
        gt = st.pose(t)
        d_est = Tw[:3, 3] - T_est[t0][:3, 3]
        d_gt = gt[:3, 3] - st.pose(t0)[:3, 3]
        out["pos_err"].append(float(np.linalg.norm(Tw[:3, 3] - gt[:3, 3])))
        out["rot_err_deg"].append(float(np.degrees(np.arccos(np.clip((np.trace(Tw[:3, :3].T @ gt[:3, :3]) - 1) / 2, -1, 1)))))
        out["cos"].append(float(d_est @ d_gt / (np.linalg.norm(d_est) * np.linalg.norm(d_gt) + 1e-12)))
        out["est_len"].append(float(np.linalg.norm(d_est)))
        out["gt_len"].append(float(np.linalg.norm(d_gt)))
        out["poses"].append(Tw.copy())

        def pose_at(tq, a=T_est[t - TICK_NS], b=Tw, ta=t - TICK_NS):
            w = (tq - ta) / TICK_NS                       # tf-style interpolation between tracked poses
            T = np.eye(4)
            T[:3, 3] = (1 - w) * a[:3, 3] + w * b[:3, 3]
            T[:3, :3] = orth((1 - w) * a[:3, :3] + w * b[:3, :3])
            return T
        stamps, poses = rostime.pose_table(pose_at, t, p.bm_half_slice_thickness)
        c2 = time.perf_counter()
        dev.set_observation(t, None, None, Tw)
        ops.tick(t, stamps, poses)
        out["points"].append(int(dev.stats().last_points))   # (reading the statistics completes the tick)
        c3 = time.perf_counter()
        out["track_ms"].append((c1 - c0) * 1e3)               # both renders + reference upload + the registration
        out["map_ms"].append((c3 - c2) * 1e3)
        out["cycle_ms"].append((c1 - c0 + c3 - c2) * 1e3)
        if verbose:
            print(f"tick {k}: |r| {rms:.1f} pos err {out['pos_err'][-1]*1e3:.2f} mm of {out['gt_len'][-1]*1e3:.1f} mm, "
                  f"cos {out['cos'][-1]:.3f}, rot {out['rot_err_deg'][-1]:.3f} deg, points {out['points'][-1]}")
    mp = ops.final_map()
    u, v, rho = st.true_inv_depth_image(t)
    ok = (u >= 0) & (u < rig.width) & (v >= 0) & (v < rig.height)
    gtimg = {(int(b), int(a)): c for a, b, c in zip(u[ok], v[ok], rho[ok])}
    err = np.array([m["inv_depth"] - gtimg[(int(m["row"]), int(m["col"]))] for m in mp
                    if (int(m["row"]), int(m["col"])) in gtimg and m["inv_depth"] > 0])
    out["map"] = mp
    out["map_cells"] = len(mp)
    out["map_on_gt"] = len(err)
    out["map_median_abs_err"] = float(np.median(np.abs(err))) if len(err) else float("nan")
    return out


def _scene(seed, speed):
    rig = calib.dataset_rig("upenn")
    st = synth.make_stream(rig, 8000, 0.35, 0.16, 1.0, seed=seed, speed=speed)
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], rig)
    return rig, st, p, st.t0_ns + int(0.08e9)


def run(n_ticks=15, reref=10**9, speed=1.0, seed=20250419, verbose=False, device_register=False, device_reference=False,
        reproj_map=False):
    rig, st, p, t0 = _scene(seed, speed)
    dev = lib.Esvo(p, rig)
    dev.ts_push_events(0, st.ev_left)
    dev.ts_push_events(1, st.ev_right)
    dev.ts_render(0, t0, download=False)
    dev.ts_render(1, t0, download=False)
    T0 = st.pose(t0)                      # bootstrap pose given, as the reference's identity at start-up
    dev.set_observation(t0, None, None, T0)
    n_sgm, _ = dev.init_sgm(None, None, min_points=100)
    out = _loop(rig, st, p, _OneGpu(dev), t0, T0, None, n_ticks, reref, verbose, device_register, device_reference, reproj_map)
    out["sgm_points"] = n_sgm
    dev.close()
    return out


def run_bands(G, routing="y_rect", n_ticks=15, reref=10**9, speed=1.0, seed=20250419, transport=None, device_register=False):
    """The same loop with the mapper split over G row bands (BASELINE configs[2] on configs[3]'s partition): G ranks -- handles on
    ONE GPU here, driven from G threads through the library's collective calls with an in-process all-gather (`transport`:
    tests/test_gpu_comm.LocalTransport's interface) -- each ingesting its rows, rendering its band of the Time Surfaces, matching
    and refining its events, fusing and regularising its rows.  What the loop adds to the band mode: the tracker reads the
    WHOLE left Time Surface (esvo_comm_gather_ts) and registers against the WHOLE map's cloud (esvo_comm_gather_pointcloud_xyz,
    merged on the device); it runs replicated -- same inputs, same bits, same pose on every rank, nothing to exchange.
    The SGM bootstrap runs on one plain handle that sees the whole stream (initialisation precedes the sharded operation); its
    frame opens every rank's fusion window.  Returns rank 0's figures (+ "ranks_agree")."""
    import threading
    from esvo_amd import dist as edist
    transport = transport or edist.LocalTransport(G)
    rig, st, p, t0 = _scene(seed, speed)
    boot = lib.Esvo(p, rig)
    boot.ts_push_events(0, st.ev_left)
    boot.ts_push_events(1, st.ev_right)
    boot.ts_render(0, t0, download=False)
    boot.ts_render(1, t0, download=False)
    T0 = st.pose(t0)
    boot.set_observation(t0, None, None, T0)
    n_sgm, _ = boot.init_sgm(None, None, min_points=100)
    frame0, xyz0 = boot.get_last_frame(), boot.get_pointcloud()
    boot.close()
    outs, errs = [None] * G, []

    def rank_main(r):
        try:
            dev = lib.Esvo(p, rig)
            y0, y1 = edist.band_of(r, G, rig.height)
            dev.set_band(y0, y1, r, G, routing=routing)
            dev.comm_init_callbacks(r, G, lambda s, d, n, stream: transport.all_gather(r, s, d, n))
            dev.ts_push_events(0, st.ev_left)   # every rank is handed the whole stream; a routed handle keeps its rows
            dev.ts_push_events(1, st.ev_right)
            dev.push_frame(frame0, T0.reshape(1, 16))
            outs[r] = _loop(rig, st, p, _Band(dev), t0, T0, xyz0, n_ticks, reref, device_register=device_register)
            outs[r]["halo_violations"] = int(dev.stats().halo_violations)
            outs[r]["events_staged"] = [int(x) for x in dev.stats().events_staged]
            dev.close()
        except BaseException as e:  # noqa: BLE001
            errs.append((r, e))
            transport.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(G)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    if errs:
        raise errs[0][1]
    out = outs[0]
    out["sgm_points"] = n_sgm
    out["ranks_agree"] = all(np.array_equal(np.array(o["poses"]), np.array(out["poses"])) and np.array_equal(o["map"], out["map"]) for o in outs)
    out["events_staged_max_frac"] = max(o["events_staged"][0] for o in outs) / max(len(st.ev_left), 1)
    return out


def run_node_rates(n_frames=20, map_every=5, resident=True, history=100, speed=1.0, seed=20250419, verbose=False):
    """The loop at the reference's own rates on ONE handle: the Time Surfaces are rendered every 10 ms, the tracker registers
    every frame against the NEWEST retained frame (esvo_Tracking.cpp:241-247), the mapper ticks every `map_every` frames on the
    pair dataTransferring would take (esvo_Mapping.cpp:497-534): the second newest for which "a pose is known", i.e. that the
    tracker has registered -- nothing while fewer than eleven pairs are retained.  Each mapper tick is followed by a
    re-reference of the tracker to the new map.
    resident=True: the frames stay on the device (ts_history_configure; track_set_current_at, ts_history_select_observation,
    set_observation_at).  resident=False: the same loop the way it has to be done without the history -- every render is
    downloaded, the pairs are kept in a host dict with the same eviction, and the chosen ones are handed back with
    set_observation(t, left, right, T) and track_set_current(left, 5).  Both compute the same bits."""
    rig, st, p, t0 = _scene(seed, speed)
    if t0 + n_frames * TICK_NS > st.t1_ns:
        raise ValueError(f"the scene's stream ends after {(st.t1_ns - t0) // TICK_NS} frames")
    dev = lib.Esvo(p, rig)
    if resident:
        dev.ts_history_configure(history)
    dev.ts_push_events(0, st.ev_left)
    dev.ts_push_events(1, st.ev_right)
    host_ts = {}                           # resident=False: stamp -> (left, right), the node's TS_history_
    pair = (dev.ts_render(0, t0, download=not resident), dev.ts_render(1, t0, download=not resident))
    if not resident:
        host_ts[t0] = pair
    T0 = st.pose(t0)                       # bootstrap pose given, as the reference's identity at start-up
    dev.set_observation(t0, None, None, T0)
    n_sgm, _ = dev.init_sgm(None, None, min_points=100)
    T_est = {t0: T0}
    out = {"pos_err": [], "rot_err_deg": [], "points": [], "tick_frames": [], "tick_stamps": [], "track_ms": [], "map_ms": [],
           "poses": [], "n_inside": [], "sgm_points": n_sgm}
    rng = np.random.default_rng(0)
    xyz = dev.get_pointcloud()
    sel = rng.permutation(len(xyz))[:2000]
    t_ref, R_, t_ = t0, np.eye(3), np.zeros(3)
    for k in range(1, n_frames + 1):
        t = t0 + k * TICK_NS
        c0 = time.perf_counter()
        pair = (dev.ts_render(0, t, download=not resident), dev.ts_render(1, t, download=not resident))
        if resident:
            dev.track_set_current_at(t, 5)
        else:
            host_ts[t] = pair
            while len(host_ts) > history:
                del host_ts[min(host_ts)]
            dev.track_set_current(host_ts[max(host_ts)][0], 5)
        dev.track_set_reference(xyz[sel], T_est[t_ref])
        R_, t_, rms = register(dev, len(sel), R_, t_)
        Tw = np.eye(4)
        Tw[:3, :3] = T_est[t_ref][:3, :3] @ R_
        Tw[:3, 3] = T_est[t_ref][:3, :3] @ t_ + T_est[t_ref][:3, 3]
        T_est[t] = Tw
        c1 = time.perf_counter()
        out["track_ms"].append((c1 - c0) * 1e3)                # both renders (+ their download) + the registration
        out["n_inside"].append(dev.track_reprojection_map(R_, t_, 2000, p.invdepth_min, p.invdepth_max, download=False)[1])
        gt = st.pose(t)
        out["pos_err"].append(float(np.linalg.norm(Tw[:3, 3] - gt[:3, 3])))
        out["rot_err_deg"].append(float(np.degrees(np.arccos(np.clip((np.trace(Tw[:3, :3].T @ gt[:3, :3]) - 1) / 2, -1, 1)))))
        out["poses"].append(Tw.copy())
        if k % map_every:
            continue
        c2 = time.perf_counter()
        if resident:
            chosen = dev.ts_history_select_observation(T_est.get)
        else:
            stamps_h = sorted(host_ts)
            chosen = lib.ts_history_select(stamps_h, T_est.get)
            chosen = None if chosen is None else (stamps_h[chosen[0]], chosen[1])
        if chosen is None:                                     # the node's dataTransferring returns false: no tick
            continue
        t_obs, T_obs = chosen

        def pose_at(tq, a=T_est[t_obs - TICK_NS], b=T_obs, ta=t_obs - TICK_NS):
            w = (tq - ta) / TICK_NS                            # tf-style interpolation between tracked poses
            T = np.eye(4)
            T[:3, 3] = (1 - w) * a[:3, 3] + w * b[:3, 3]
            T[:3, :3] = orth((1 - w) * a[:3, :3] + w * b[:3, :3])
            return T
        c2b = time.perf_counter()
        stamps, poses = rostime.pose_table(pose_at, t_obs, p.bm_half_slice_thickness)
        c2c = time.perf_counter()
        if resident:
            dev.set_observation_at(t_obs, T_obs)
        else:
            dev.set_observation(t_obs, host_ts[t_obs][0], host_ts[t_obs][1], T_obs)
        dev.tick(t_obs, stamps, poses)
        out["points"].append(int(dev.stats().last_points))     # (reading the statistics completes the tick)
        c3 = time.perf_counter()
        out["map_ms"].append((c2b - c2 + c3 - c2c) * 1e3)       # the choice of the pair, the observation and the tick
        out["tick_frames"].append(k)
        out["tick_stamps"].append(int(t_obs))
        xyz = dev.get_pointcloud()                             # re-reference: the tracker registers against the new map
        sel = rng.permutation(len(xyz))[:2000]
        t_ref, R_, t_ = t, np.eye(3), np.zeros(3)
        if verbose:
            print(f"frame {k}: mapper tick at frame {(t_obs - t0) // TICK_NS}, {out['points'][-1]} points, pos err "
                  f"{out['pos_err'][-1] * 1e3:.2f} mm")
    mp = dev.get_map()
    t_map = out["tick_stamps"][-1] if out["tick_stamps"] else t0
    u, v, rho = st.true_inv_depth_image(t_map)
    ok = (u >= 0) & (u < rig.width) & (v >= 0) & (v < rig.height)
    gtimg = {(int(b), int(a)): c for a, b, c in zip(u[ok], v[ok], rho[ok])}
    err = np.array([m["inv_depth"] - gtimg[(int(m["row"]), int(m["col"]))] for m in mp
                    if (int(m["row"]), int(m["col"])) in gtimg and m["inv_depth"] > 0])
    out["map"] = mp
    out["map_cells"] = len(mp)
    out["map_median_abs_err"] = float(np.median(np.abs(err))) if len(err) else float("nan")
    dev.close()
    return out
