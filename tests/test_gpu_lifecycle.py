"""What a handle allocates it frees: the ledger of esvo_amd/csrc/devmem.hpp (live allocations, live bytes of every device and
pinned buffer the library owns) around create / destroy cycles, every lazily allocating path, the regrow paths, a create that
fails midway and a reconfiguration.  Device-wide free memory says nothing on a shared card, so every assertion is a ledger
DELTA around this module's own handles (session fixtures of other modules may hold handles of their own)."""
import numpy as np
import pytest

import map_cloud_cases as MC
from esvo_amd import abi, dist as edist, lib, params, rostime

pytestmark = pytest.mark.gpu
MS = 1_000_000
EV = abi.EVENT_DTYPE.itemsize


def _params(rig, preset="mapping_upenn", **over):
    kw = dict(max_events_per_tick=4096, event_ring_capacity=8192, regularization=0)
    kw.update(over)
    return params.make_params(params.PRESETS[preset], rig, **kw)[0]


class Ledger:
    """deltas against the ledger at construction"""

    def __init__(self):
        self.base = lib.debug_live_allocations()

    def __call__(self):
        now = lib.debug_live_allocations()
        return now[0] - self.base[0], now[1] - self.base[1]

    def rose(self, what):
        """the live-allocation count is above the last call's (the path was reached and allocated)"""
        n = self()[0]
        assert n > getattr(self, "last", 0), f"{what}: the live-allocation count did not rise ({n})"
        self.last = n


def _stage_and_render(dev, stream, t_prev, t):
    for cam in (0, 1):
        dev.ts_push_events(cam, stream.slice(cam, t_prev, t))
        dev.ts_render(cam, t, download=False)


def test_create_destroy_cycles(upenn_rig):
    p = _params(upenn_rig, event_ring_capacity=1024)
    led = Ledger()
    for _ in range(20):
        dev = lib.Esvo(p, upenn_rig)
        assert led()[0] > 50
        dev.close()
    assert led() == (0, 0)


def test_every_lazy_path_then_destroy(upenn_rig, upenn_stream):
    import test_gpu_em as EM
    from test_gpu_shard import _emulated_gather
    st, t0 = upenn_stream, upenn_stream.t0_ns
    p = _params(upenn_rig)
    led = Ledger()
    dev = lib.Esvo(p, upenn_rig)
    led.rose("esvo_create")
    # ---- ingest: the wire format, an out-of-order packet (merge scratch)
    dev.ts_push_event_array(0, abi.serialize_event_array(st.slice(0, t0, t0 + 4 * MS), upenn_rig.width, upenn_rig.height))
    led.rose("wire staging")
    dev.ts_push_events(0, st.slice(0, t0 + 4 * MS, t0 + 10 * MS))
    dev.ts_push_events(0, st.slice(0, t0 + 2 * MS, t0 + 3 * MS))       # older than the newest staged event
    assert dev.stats().late_events[0] > 0
    led.rose("out-of-order merge scratch")
    dev.ts_push_events(1, st.slice(1, t0, t0 + 10 * MS))
    # ---- FORWARD-mode Time Surfaces
    for cam in (0, 1):
        dev.ts_render_forward(cam, t0 + 10 * MS)
        led.rose(f"forward lists of camera {cam}")
        dev.ts_render(cam, t0 + 10 * MS, download=False)
    # ---- ticks (they allocate nothing), debug images, the device cloud, the global cloud, the voxel filter
    t_prev = t0 + 10 * MS
    for k in range(3):
        before = led()
        t = t0 + (20 + 10 * k) * MS
        MC.tick_at(dev, st, p, t, t_prev)
        t_prev = t
        dev.synchronize()
        assert led() == before, "a tick allocated"
    dev.get_debug_images()
    led.rose("debug images")
    dev.map_cloud_build()
    led.rose("device cloud")
    dev.gpc_configure(capacity_points=20000)
    led.rose("global cloud")
    dev.gpc_update(t)
    dev.map_voxel_filter(np.random.default_rng(3).uniform(-2, 2, (500, 3)).astype(np.float32), 0.3)
    led.rose("voxel filter upload")
    # ---- SGM bootstrap and tick, event-to-event matching
    dev.init_sgm(None, None, min_points=1, want_disp=False)
    led.rose("SGM scratch")
    for cam in (0, 1):
        dev.ts_push_events(cam, st.slice(cam, t, t + 5 * MS))          # (the SGM tick wants events behind t)
    dev.tick_sgm(want_disp=False)
    em = params.make_em_params(params.PRESETS["mvstereo_upenn"])
    left, right, begin, count, T = EM.seam_case(st, t - 20 * MS, t, 3000, em.slice_thickness)
    dev.match_em(em, left, begin, count, T, right)
    led.rose("event matching")
    # ---- tracker
    dev.ts_render(0, t + 5 * MS, download=False)
    dev.track_set_current(None, 5)
    led.rose("tracker images")
    xyz = np.random.default_rng(5).uniform((-1, -1, 2), (1, 1, 5), (300, 3)).astype(np.float32)
    dev.track_set_reference(xyz, np.eye(4))
    led.rose("tracker reference")
    dev.track_normal_equations(np.eye(3), np.zeros(3), 0, 300)
    led.rose("tracker normal equations")
    R, tt, _, _ = dev.track_solve(300, np.eye(3), np.zeros(3), batch_size=100)
    led.rose("tracker solve")
    dev.track_reprojection_map(R, tt, 300, 0.2, 2.0)
    led.rose("tracker reprojection map")
    # ---- two row bands with routing and Denoising (the peer is a second handle inside the same ledger): the exchange blocks, the
    # routed staging, the denoise flags
    dev.reset()
    pd = type(p).from_buffer_copy(p)
    pd.denoising = 1
    dev.set_params(pd)
    peer = lib.Esvo(pd, upenn_rig)
    led.rose("the peer handle")
    ranks = [dev, peer]
    for g, d in enumerate(ranks):
        d.set_band(*edist.band_of(g, 2, upenn_rig.height), g, 2, routing="y_rect")
    led.rose("shard exchange blocks")
    t = t0 + 10 * MS
    stamps, poses = rostime.pose_table(st.pose, t, p.bm_half_slice_thickness)
    for d in ranks:
        _stage_and_render(d, st, t0, t)
        d.set_observation(t, None, None, st.pose(t))
    led.rose("routed staging")
    assert all([d.shard_phase(0, t, stamps, poses) for d in ranks])    # Denoising: the mask bits are exchanged first
    _emulated_gather(ranks)
    assert not any([d.shard_phase(0) for d in ranks])
    led.rose("denoise flags")
    for phase in (1, 2):
        _emulated_gather(ranks)
        for d in ranks:
            d.shard_phase(phase)
    peer.close()
    dev.close()
    assert led() == (0, 0)


def test_event_queue_copies_then_destroy(upenn_rig, upenn_stream):
    """max_event_queue_len = 3: the copies that stand in for late events are uploaded by the next scatter (d_tsq_dup)"""
    st, t0 = upenn_stream, upenn_stream.t0_ns
    led = Ledger()
    dev = lib.Esvo(_params(upenn_rig, max_event_queue_len=3), upenn_rig)
    dev.ts_push_events(0, st.slice(0, t0, t0 + 5 * MS))
    led.rose("esvo_create")
    dev.ts_push_events(0, st.slice(0, t0 + 2 * MS, t0 + 3 * MS))
    led.rose("out-of-order merge scratch")
    dev.ts_render(0, t0 + 5 * MS, download=False)
    led.rose("queue-mode copies")
    dev.close()
    assert led() == (0, 0)


def _regrow(led, small, large, want_bytes, what):
    """small() then large(): the count stays, the bytes rise by want_bytes(), evaluated behind large()"""
    small()
    n0, b0 = led()
    large()
    n1, b1 = led()
    want = want_bytes()
    print(f"{what}: allocations {n0} -> {n1}, bytes {b0} -> {b1} (+{b1 - b0}, expected +{want})")
    assert n1 == n0, what
    assert b1 - b0 == want, what


def test_regrow_frees_what_it_replaces(upenn_rig, upenn_stream, monkeypatch):
    """Ring of 128 Ki events here: the wire staging starts at 1 MiB, so only a message of more than 80 659 events regrows it."""
    st, t0 = upenn_stream, upenn_stream.t0_ns
    W, H = upenn_rig.width, upenn_rig.height
    monkeypatch.setenv("ESVO_POSE_SLOTS0", "2")
    p = _params(upenn_rig, event_ring_capacity=1 << 17)
    led = Ledger()
    dev = lib.Esvo(p, upenn_rig)
    # ---- the wire staging of camera 1: max(13 n, 1 MiB) bytes
    big = st.ev_right
    assert len(big) * 13 > 1 << 20
    _regrow(led, lambda: dev.ts_push_event_array(1, abi.serialize_event_array(big[:1000], W, H)),
            lambda: (dev.reset(), dev.ts_push_event_array(1, abi.serialize_event_array(big, W, H))),
            lambda: len(big) * 13 - (1 << 20), "wire staging")
    # ---- the merge scratch of an out-of-order packet: K staged events behind the packet's first stamp, n in the packet;
    # max(need + need / 2, 4096) elements of K, n, K + n (events, events, words)
    dev.reset()
    cap = lambda need: max(need + need // 2, 4096)  # noqa: E731
    K, n1, n2 = 3000, 100, 5000
    dev.ts_push_events(0, st.ev_left[20000:20000 + K])                 # both packets are older than all of these, the second than the first
    assert cap(K + n1) >= K + n1                                       # (the copy of the staged tail does not regrow: K + n1 fit behind K)
    _regrow(led, lambda: dev.ts_push_events(0, st.ev_left[n2:n2 + n1]), lambda: dev.ts_push_events(0, st.ev_left[:n2]),
            lambda: EV * (cap(n2) - cap(n1)) + 4 * (cap(K + n1 + n2) - cap(K + n1)), "merge scratch")
    # ---- the tracker's reference block: max(n, 4096) points of 3 floats pinned, 3 floats, 3 doubles, 6 doubles
    xyz = np.random.default_rng(5).uniform((-1, -1, 2), (1, 1, 5), (5000, 3)).astype(np.float32)
    _regrow(led, lambda: dev.track_set_reference(xyz[:100], np.eye(4)), lambda: dev.track_set_reference(xyz, np.eye(4)),
            lambda: (5000 - 4096) * (12 + 12 + 24 + 48), "tracker reference")
    # ---- the cloud id arrays (3 x cap ids + their scan scratch, cap = max(ids + ids / 4, 4096), ids = 4 per window point) and,
    # on the way, the pose-slot table: two slots at first, doubled whenever every slot holds a frame of the window
    dev.reset()
    state = dict(t_prev=t0, k=0, id_cap=0, frames=0)

    def tick_and_build():
        t = t0 + (60 + 10 * state["k"]) * MS
        MC.tick_at(dev, st, p, t, state["t_prev"])
        state.update(t_prev=t, k=state["k"] + 1)
        dev.map_cloud_build()
        s = dev.stats()
        state["frames"] = max(state["frames"], int(s.last_window_frames))
        return 4 * int(s.last_window_points)

    def id_bytes(cap_ids):
        return 4 * (3 * cap_ids + lib.debug_scan_predicates(cap_ids)[3] + 8)

    def first():
        state["id_cap"] = max(tick_and_build() * 5 // 4, 4096)

    def more():
        state["old"] = state["id_cap"]
        while state["id_cap"] == state["old"] and state["k"] < 12:
            ids = tick_and_build()
            if ids > state["id_cap"]:
                state["id_cap"] = max(ids + ids // 4, 4096)
        assert state["id_cap"] > state["old"], "the window never outgrew the first id arrays"

    def want():
        slots = 2
        while slots < state["frames"]:
            slots *= 2
        assert slots > 2, "the window never held more than two frames"
        return id_bytes(state["id_cap"]) - id_bytes(state["old"]) + (slots - 2) * p.max_poses_per_tick * 16 * 8

    _regrow(led, first, more, want, "cloud id arrays + pose-slot table")
    dev.close()
    assert led() == (0, 0)


def test_communicator_blocks_regrow(upenn_rig, upenn_stream, monkeypatch):
    """ESVO_COMM_STRIDE0 = 16 points per block: the first frame does not fit, the empty block and the two receive buffers are
    replaced by larger ones (2 + 13 stride words each, the receive buffers once per rank)."""
    from test_gpu_comm import _ticks
    monkeypatch.setenv("ESVO_COMM_STRIDE0", "16")
    p = _params(upenn_rig, event_ring_capacity=1 << 17)
    tr = edist.LocalTransport(1)
    led = Ledger()
    dev = lib.Esvo(p, upenn_rig)
    dev.comm_init_callbacks(0, 1, lambda s, d, n, st: tr.all_gather(0, s, d, n))
    dev.ts_push_events(0, upenn_stream.ev_left)
    dev.ts_push_events(1, upenn_stream.ev_right)

    def run():
        for t, stamps, poses, T in _ticks(upenn_stream, p, 4):
            dev.ts_render(0, t, download=False)
            dev.ts_render(1, t, download=False)
            dev.comm_tick(t, T, stamps, poses)
        dev.comm_newest_map()

    def want():
        cs = dev.comm_stats()
        assert cs.regrows >= 1 and cs.stride_cap_points > 16
        return 3 * 8 * 13 * (int(cs.stride_cap_points) - 16)

    _regrow(led, lambda: None, run, want, "communicator blocks")
    dev.comm_destroy()
    dev.close()
    assert led() == (0, 0)


def test_create_that_fails_midway(upenn_rig):
    """max_events_per_tick above the 4 M scan limit: refused behind the calibration, Time-Surface, ring and pose allocations"""
    p = _params(upenn_rig, event_ring_capacity=1024, max_events_per_tick=5_000_000)
    led = Ledger()
    with pytest.raises(lib.EsvoError, match="scan limit") as e:
        lib.Esvo(p, upenn_rig)
    assert f"({abi.ERR_CAPACITY})" in str(e.value)
    assert led() == (0, 0)


def test_reconfiguration(upenn_rig):
    p = _params(upenn_rig, event_ring_capacity=1024)
    H = upenn_rig.height
    led = Ledger()
    dev = lib.Esvo(p, upenn_rig)
    n_first = led()[0]
    SHARD_BLOCKS = 6                                                   # two code blocks, two point blocks, the kept counts, the ring's global indices
    steps = [lambda: dev.set_band(0, H // 2, 0, 2), lambda: dev.set_band(0, H // 2, 0, 2, routing="y_rect"),
             lambda: dev.set_band(0, H, 0, 1), dev.reset]
    for k, step in enumerate(steps):
        step()
        assert n_first <= led()[0] <= n_first + SHARD_BLOCKS, k
    assert led()[0] == n_first + SHARD_BLOCKS                          # (the blocks stay for the next band configuration)
    dev.close()
    assert led() == (0, 0)


@pytest.mark.parametrize("pinned", [False, True])
def test_the_owning_type(pinned):
    """alloc, grow smaller (same pointer), grow larger (exact capacity), move construction and assignment (source empty, one
    free), release twice, an empty buffer's destructor: each step against its ledger delta, inside the library (api_dev.hip)"""
    led = Ledger()
    assert lib.debug_devmem_selftest(pinned) == 0
    assert led() == (0, 0)
