"""esvo_reset puts a handle back to "as created": a handle that ran one session, was reset and then ran a second session gives,
byte for byte, what a fresh handle gives for the second session alone.  The first session (A) is chosen so that every group of
session state (context.hpp: the structs esvo_reset assigns) is dirty when the reset comes; the second one (B) lies EARLIER in
the stream, as a replayed bag does, so stale ring bookkeeping, selection marks or stamps would show.  Configuration survives a
reset (Time-Surface history length, global-cloud parameters, bands and routing), so the fresh handle is configured alike."""
import numpy as np
import pytest

from esvo_amd import dist as edist, lib, params, rostime

pytestmark = pytest.mark.gpu
MS = 1_000_000
# esvo_stats_t fields that are timings or clocks, or say how many ticks recorded timings (stage timings are SAMPLED, and the
# sampling counters survive a reset on purpose: which ticks of B record theirs depends on how many ticks the handle has seen)
TIMING = {"ms_ts_scatter", "ms_ts_render", "ms_bm", "ms_refine", "ms_fusion", "ms_regularization", "ms_tick_total", "ms_kernel",
          "sum_ms_kernel", "clk_cycles", "clk_ref_ticks", "clk_samples", "clk_ref_khz", "stage_timing_samples", "pad_", "pad2_"}
SGM_COUNTS = ("events", "on_image", "matched_columns", "disp_ok", "points", "zero_disp")
# esvo_gpc_stats_t without ms_last (t_last_pub is the stamp of the last publication, not a measurement) -- and without `updates` and
# `refreshes`, the one output left out: GpcState::stats survives a reset except for total_points (gpc_reset, api_gpc.hip), so
# both go on counting from session A.  Observed before the session structs existed: updates 2 against 1, refreshes 2 against 1.
GPC_FIELDS = ("total_points", "last_near", "last_voxels", "last_added", "last_refreshed", "t_last_pub")


def _counts(s, skip=()):
    out = {}
    for k, _ in type(s)._fields_:
        if k in skip:
            continue
        v = getattr(s, k)
        out[k] = list(v) if hasattr(v, "__len__") else v
    return out


def _outputs(dev, unsharded=True):
    """every output the two handles are compared on, as bytes or plain values"""
    out = {"get_map": dev.get_map().tobytes()}
    m, t = dev.get_committed_map()
    out["get_committed_map"] = (m.tobytes(), t)
    out["get_pointcloud"] = dev.get_pointcloud().tobytes()
    out["get_last_frame"] = dev.get_last_frame().tobytes()
    out["stats"] = _counts(dev.stats(), TIMING)
    if unsharded:
        out["map_cloud"] = dev.map_cloud().tobytes()
        out["gpc_cloud"] = dev.gpc_cloud().tobytes()
        t, cams = dev.ts_history()
        out["ts_history"] = (t.tobytes(), cams.tobytes())
        g = dev.sgm_stats()
        out["sgm_stats"] = {k: int(getattr(g, k)) for k in SGM_COUNTS}
        g = dev.gpc_stats()
        out["gpc_stats"] = {k: getattr(g, k) for k in GPC_FIELDS}
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    bad = []
    for k in a:
        if a[k] != b[k]:
            bad.append(k)
            if isinstance(a[k], dict):
                print(what, k, {f: (a[k][f], b[k][f]) for f in a[k] if a[k][f] != b[k][f]})
            else:
                print(what, k, "differs:", [len(x) if isinstance(x, bytes) else x for x in (a[k] if isinstance(a[k], tuple) else (a[k],))],
                      [len(x) if isinstance(x, bytes) else x for x in (b[k] if isinstance(b[k], tuple) else (b[k],))])
    assert not bad, f"{what}: a reset handle and a fresh one differ in {bad}"


def _tick_args(st, p, t):
    stamps, poses = rostime.pose_table(st.pose, t, p.bm_half_slice_thickness)
    return t, st.pose(t), stamps, poses


def _configure(dev):
    dev.ts_history_configure(4)
    dev.gpc_configure(visualize_range=10.0, interval_s=0.005, num_added_per_refresh=1000, capacity_points=20000)


T_A = 120 * MS     # first tick of session A, from the stream's start
T_B = 50 * MS      # ... of session B
T_PUB_B = 400 * MS  # t_last_pub survives a reset as the reference's t_last_pub_pc_ does (api_gpc.hip), so B publishes behind A


def _session_a(dev, st, p):
    t0, ta = st.t0_ns, st.t0_ns + T_A
    pins = []
    # ---- async pushes on both cameras; the second packet of camera 0 arrives behind the third (out of order: merged into the ring)
    bounds = [t0, ta - 40 * MS, ta - 30 * MS, ta + 25 * MS]
    for cam in (0, 1):
        order = (0, 2, 1) if cam == 0 else (0, 1, 2)
        for k in order:
            ev = st.slice(cam, bounds[k], bounds[k + 1])
            pe = lib.PinnedEvents(len(ev))
            pe.array[:] = ev
            pins.append(pe)
            dev.ts_push_events_async(cam, pe.array)
    assert dev.stats().late_events[0] > 0
    # ---- renders: they fill the Time-Surface history
    for t in (ta - 20 * MS, ta - 10 * MS):
        dev.ts_render(0, t, download=False)
        dev.ts_render(1, t, download=False)
    assert len(dev.ts_history()[0]) == 2
    # ---- one SGM tick, the device cloud, the global cloud, the tracker's current image and its reference out of the cloud
    dev.set_observation(ta - 10 * MS, None, None, st.pose(ta - 10 * MS))
    n_sgm, _ = dev.tick_sgm(want_disp=False)
    n_cloud = dev.map_cloud_build()
    assert n_sgm > 0 and n_cloud > 0
    assert dev.gpc_update(ta - 10 * MS)
    dev.track_set_current(None, 5)
    dev.track_set_reference_from_cloud(None, st.pose(ta - 10 * MS), n=min(n_cloud, 100))
    # ---- three pipelined ticks: each is handed in while its predecessor is pending, the last one is still pending at the reset
    for k in range(3):
        dev.tick_resident(*_tick_args(st, p, ta + 10 * MS * k))
    return pins


def _session_b(dev, st, p):
    t0, tb = st.t0_ns, st.t0_ns + T_B
    for cam in (0, 1):
        dev.ts_push_events(cam, st.slice(cam, t0, tb + 25 * MS))
    dev.ts_render(0, tb - 10 * MS, download=False)
    dev.ts_render(1, tb - 10 * MS, download=False)
    for k in range(3):
        dev.tick_resident(*_tick_args(st, p, tb + 10 * MS * k))
    assert dev.map_cloud_build() > 0
    assert dev.gpc_update(t0 + T_PUB_B)
    n_sgm, _ = dev.tick_sgm(want_disp=False)
    assert n_sgm > 0
    return _outputs(dev)


def test_reset_then_session_equals_fresh_session(upenn_rig, upenn_stream):
    st = upenn_stream
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], upenn_rig, process_event_num=400, max_events_per_tick=4096,
                              event_ring_capacity=1 << 18)
    used, fresh = lib.Esvo(p, upenn_rig), lib.Esvo(p, upenn_rig)
    for d in (used, fresh):
        _configure(d)
    pins = _session_a(used, st, p)
    used.reset()
    for cam in (0, 1):
        used.ts_push_wait(cam)
    for pe in pins:
        pe.free()
    assert len(used.ts_history()[0]) == 0 and len(used.get_map()) == 0 and len(used.map_cloud()) == 0
    got, want = _session_b(used, st, p), _session_b(fresh, st, p)
    s = fresh.stats()
    assert s.ticks == 4 and s.last_points > 0 and len(fresh.get_map()) > 50 and len(fresh.gpc_cloud()) > 0
    assert len(fresh.ts_history()[0]) == 4
    _same(got, want, "unsharded")
    used.close()
    fresh.close()


def _shard_tick(ranks, st, p, t, t_prev):
    """one three-phase tick of row-routed ranks with Denoising (tests/test_gpu_lifecycle.py): the mask bits are exchanged first"""
    from test_gpu_shard import _emulated_gather
    stamps, poses = rostime.pose_table(st.pose, t, p.bm_half_slice_thickness)
    for d in ranks:
        for cam in (0, 1):
            d.ts_push_events(cam, st.slice(cam, t_prev, t + 2 * MS))
            d.ts_render(cam, t, download=False)
        d.set_observation(t, None, None, st.pose(t))
    assert all([d.shard_phase(0, t, stamps, poses) for d in ranks])
    _emulated_gather(ranks)
    assert not any([d.shard_phase(0) for d in ranks])
    for phase in (1, 2):
        _emulated_gather(ranks)
        for d in ranks:
            d.shard_phase(phase)


def _routed_pair(p, rig):
    ranks = [lib.Esvo(p, rig), lib.Esvo(p, rig)]
    for g, d in enumerate(ranks):
        d.set_band(*edist.band_of(g, 2, rig.height), g, 2, routing="y_rect")
    return ranks


def _session_b_sharded(ranks, st, p):
    t_prev = st.t0_ns
    for k in range(2):
        t = st.t0_ns + T_B + 10 * MS * k
        _shard_tick(ranks, st, p, t, t_prev)
        t_prev = t + 2 * MS
    return [_outputs(d, unsharded=False) for d in ranks]


def test_reset_then_session_equals_fresh_session_routed_bands(upenn_rig, upenn_stream):
    """two row bands with routing and Denoising (the set-up of tests/test_gpu_lifecycle.py): the routed ingest's host sequences, the
    pending-exchange flags.  8000 events per tick here: the 3 x 3 median of Denoising keeps nothing of a few hundred synthetic
    events (tests/scenarios.py), and empty maps would compare equal whatever a reset left behind."""
    st = upenn_stream
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], upenn_rig, process_event_num=8000, max_events_per_tick=8192,
                              event_ring_capacity=1 << 18, regularization=0)
    p.denoising = 1
    used, fresh = _routed_pair(p, upenn_rig), _routed_pair(p, upenn_rig)
    _shard_tick(used, st, p, st.t0_ns + T_A, st.t0_ns)
    assert all(d.stats().ticks == 1 and d.stats().events_staged[0] > 0 for d in used)
    for d in used:
        d.reset()
    got, want = _session_b_sharded(used, st, p), _session_b_sharded(fresh, st, p)
    print([(d.stats().ticks, d.stats().last_events_in, d.stats().last_matches, d.stats().last_points, len(d.get_map())) for d in fresh])
    assert all(d.stats().ticks == 2 and d.stats().last_points > 0 for d in fresh) and sum(len(d.get_map()) for d in fresh) > 50
    for g in range(2):
        _same(got[g], want[g], f"rank {g}")
    for d in used + fresh:
        d.close()
