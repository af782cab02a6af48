"""The Time-Surface history on the device (include/esvo_hip.h, "Time-Surface history"; esvo_amd/csrc/api_history.hip): frames
retained by stamp, the reference's eviction, and the mapper's and the tracker's calls on a retained stamp against the same
calls with the host images of those frames.  The feature adds no arithmetic, so every comparison is byte for byte; what the
tests look for is a wrong slot, a wrong stride, a frame read before it was stored or overwritten while it is read."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import scenarios as S
from esvo_amd import calib, lib, params, rostime, synth

pytestmark = pytest.mark.gpu
ERR_UNSUPPORTED = -5   # ESVO_ERR_UNSUPPORTED (include/esvo_hip.h)
STEP = 10_000_000
MAP_FIELDS = ["row", "col", "age", "inv_depth", "scale2", "nu", "variance", "residual", "x", "p_cam"]


def _small_rig(w, h):
    return calib.ideal_rig(w, h, 50.0, 0.1)


def _handle(rig, **over):
    p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], rig, **over)
    return lib.Esvo(p, rig), p


def _image(rig, i, cam):
    """a frame written from (stamp index, camera, pixel index): no two frames, rows or 256-byte blocks look alike"""
    px = np.arange(rig.width * rig.height, dtype=np.int64)
    return ((px * 7 + (px >> 8) * 13 + i * 31 + cam * 101 + (px // rig.width) * 3) & 255).astype(np.uint8).reshape(rig.height, rig.width)


def _refused(fn, code=lib.ERR_STATE):
    with pytest.raises(lib.EsvoError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def _same_map(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for f in MAP_FIELDS:
        assert np.array_equal(a[f], b[f]), f


class _Model:
    """TS_history_ as the reference keeps it: insert in stamp order, erase the smallest stamps beyond the length"""

    def __init__(self, length):
        self.length, self.frames, self.gone = length, {}, set()

    def put(self, t, cam, img):
        self.frames.setdefault(t, {})[cam] = img
        self.gone.discard(t)
        while len(self.frames) > self.length:
            t_min = min(self.frames)
            del self.frames[t_min]
            self.gone.add(t_min)

    def check(self, dev):
        t, cams = dev.ts_history()
        want = sorted(self.frames)
        assert t.dtype == np.uint64 and list(t) == want, (list(t), want)
        assert list(cams) == [sum(1 << c for c in self.frames[s]) for s in want]
        for s in want:
            for cam in (0, 1):
                if cam in self.frames[s]:
                    assert np.array_equal(dev.ts_history_get(s, cam), self.frames[s][cam]), (s, cam)
                else:
                    _refused(lambda: dev.ts_history_get(s, cam))
        for s in self.gone:
            for cam in (0, 1):
                msg = _refused(lambda: dev.ts_history_get(s, cam))
                assert str(s) in msg and (not want or (str(want[0]) in msg and str(want[-1]) in msg)), msg


# ---- B1: bytes and eviction --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(96, 64), (95, 63)])
@pytest.mark.parametrize("length", [1, 2, 3])
def test_put_get_and_eviction(size, length):
    rig = _small_rig(*size)
    dev, _ = _handle(rig)
    T = np.eye(4)
    for fn in (dev.ts_history, lambda: dev.ts_history_get(1, 0), lambda: dev.ts_history_put(1, 0, _image(rig, 0, 0)),
               lambda: dev.set_observation_at(1, T), lambda: dev.track_set_current_at(1, 5), dev.ts_history_select_observation):
        assert "history is off" in _refused(fn)
    dev.ts_history_configure(length)
    assert dev.ts_history()[0].size == 0
    _refused(lambda: dev.ts_history_get(1, 2), lib.ERR_INVALID_ARG)
    _refused(lambda: dev.ts_history_put(1, -1, _image(rig, 0, 0)), lib.ERR_INVALID_ARG)
    assert dev.lib.esvo_ts_history_put(dev.h, 1, 0, None) == lib.ERR_INVALID_ARG
    assert dev.lib.esvo_ts_history_list(dev.h, None, None, 0, None) == lib.ERR_INVALID_ARG
    m = _Model(length)
    t0 = 5_000_000_000
    stamps = [t0 + i * STEP for i in range(length + 2)]
    for i, t in enumerate(stamps):
        for cam in (0, 1):         # between the two puts the entry is left-only
            dev.ts_history_put(t, cam, _image(rig, i, cam))
            m.put(t, cam, _image(rig, i, cam))
            m.check(dev)
    assert sorted(m.frames) == stamps[-length:] and sorted(m.gone) == stamps[:2]
    # an overwrite of a retained stamp: the new frame, the same entries
    dev.ts_history_put(stamps[-1], 1, _image(rig, 77, 1))
    m.put(stamps[-1], 1, _image(rig, 77, 1))
    m.check(dev)
    # a stamp below every retained one on a full history is not retained
    dev.ts_history_put(t0 - STEP, 0, _image(rig, 50, 0))
    m.gone.add(t0 - STEP)
    m.check(dev)
    # a left-only entry: enough for the tracker, not for the mapper; nothing changes where a call is refused
    t_left = stamps[-1] + STEP
    dev.ts_history_put(t_left, 0, _image(rig, 60, 0))
    m.put(t_left, 0, _image(rig, 60, 0))
    m.check(dev)
    msg = _refused(lambda: dev.set_observation_at(t_left, T))
    assert str(t_left) in msg and "complete pair" in msg
    dev.track_set_current_at(t_left, 0)
    assert np.array_equal(dev.track_images()[0], 255 - _image(rig, 60, 0))
    _refused(lambda: dev.track_set_current_at(t_left + 1, 0))
    assert np.array_equal(dev.track_images()[0], 255 - _image(rig, 60, 0)), "the current frame stays in place"
    # reset and reconfiguration empty the history; the slots of a reset handle are still there
    dev.reset()
    assert dev.ts_history()[0].size == 0
    _refused(lambda: dev.ts_history_get(t_left, 0))
    m = _Model(length)
    dev.ts_history_put(t0, 1, _image(rig, 3, 1))
    m.put(t0, 1, _image(rig, 3, 1))
    m.check(dev)
    dev.ts_history_configure(length + 1)
    assert dev.ts_history()[0].size == 0
    m = _Model(length + 1)
    for i in range(length + 2):
        dev.ts_history_put(t0 + i * STEP, 0, _image(rig, i, 0))
        m.put(t0 + i * STEP, 0, _image(rig, i, 0))
    m.check(dev)
    dev.ts_history_configure(0)
    assert "history is off" in _refused(dev.ts_history)
    dev.close()


@pytest.fixture(scope="module")
def small_stream():
    rig = _small_rig(96, 64)
    return rig, synth.make_stream(rig, 400, 0.09, 0.3, 1.0, seed=20251019)


def test_queue_mode_renders_in_any_order(small_stream):
    """per-pixel queues (max_event_queue_len = 20): renders at t3, t1, t2 with two pairs retained leave {t2, t3}"""
    rig, st = small_stream
    dev, _ = _handle(rig, max_event_queue_len=20)
    dev.ts_history_configure(2)
    dev.ts_push_events(0, st.ev_left)
    dev.ts_push_events(1, st.ev_right)
    t1, t2, t3 = (st.t0_ns + k * STEP for k in (3, 4, 5))
    img = {}
    for t in (t3, t1, t2):
        img[t] = [dev.ts_render(cam, t) for cam in (0, 1)]
        want = {t3: [t3], t1: [t1, t3], t2: [t2, t3]}[t]
        assert list(dev.ts_history()[0]) == want and list(dev.ts_history()[1]) == [3] * len(want)
    for t in (t2, t3):
        for cam in (0, 1):
            assert np.array_equal(dev.ts_history_get(t, cam), img[t][cam])
    assert img[t2][0].any() and not np.array_equal(img[t2][0], img[t3][0])
    _refused(lambda: dev.ts_history_get(t1, 0))
    dev.close()


# ---- B2: renders are what is retained ----------------------------------------------------------------------------------------
def test_renders_are_retained(small_stream):
    rig, st = small_stream
    dev, p = _handle(rig)
    twin, _ = _handle(rig)
    dev.ts_history_configure(4)
    for d in (dev, twin):
        d.ts_push_events(0, st.ev_left)
        d.ts_push_events(1, st.ev_right)
    times = [st.t0_ns + (3 + k) * STEP for k in range(6)]
    seen = []
    for k, t in enumerate(times):
        want = [twin.ts_render(cam, t) for cam in (0, 1)]
        assert want[0].any() and want[1].any()
        if k < 4:      # esvo_ts_render, one camera at a time: the entry is left-only in between
            got0 = dev.ts_render(0, t)
            assert list(dev.ts_history()[0])[-1] == t and dev.ts_history()[1][-1] == 1
            got = [got0, dev.ts_render(1, t)]
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        elif k == 4:   # esvo_ts_render_forward: another image under its stamp
            got = [dev.ts_render_forward(cam, t) for cam in (0, 1)]
        else:          # both cameras of esvo_map_tick_resident: the frames esvo_ts_render makes on a twin handle
            stamps, poses = rostime.pose_table(st.pose, t, p.bm_half_slice_thickness)
            dev.tick_resident(t, st.pose(t), stamps, poses)
            got = want
        seen.append(t)
        assert list(dev.ts_history()[0]) == seen[-4:] and dev.ts_history()[1][-1] == 3
        for cam in (0, 1):
            assert np.array_equal(dev.ts_history_get(t, cam), got[cam]), (k, cam)
    # host images handed to the mapper or the tracker are not retained
    dev.set_observation(times[-1] + STEP, want[0], want[1], np.eye(4))
    dev.track_set_current(want[0], 5)
    assert list(dev.ts_history()[0]) == seen[-4:]
    # a render at a retained stamp overwrites its frame (stated deviation from the reference's emplace)
    dev.ts_history_put(times[-1], 0, _image(rig, 9, 0))
    assert np.array_equal(dev.ts_history_get(times[-1], 0), _image(rig, 9, 0))
    again = dev.ts_render(0, times[-1])
    assert np.array_equal(again, want[0]) and np.array_equal(dev.ts_history_get(times[-1], 0), want[0])
    assert np.array_equal(dev.ts_history_get(times[-1], 1), want[1]) and list(dev.ts_history()[0]) == seen[-4:]
    dev.close()
    twin.close()


# ---- B3: mapper by stamp -----------------------------------------------------------------------------------------------------
def _counters(dev):
    s = dev.stats()
    return {k: (list(getattr(s, k)) if hasattr(getattr(s, k), "__len__") else getattr(s, k))
            for k, _ in type(s)._fields_ if k.startswith("last_")}


@pytest.mark.parametrize("name", ["upenn", "dsec"])   # dsec: SmoothTimeSurface, 3 x 3 fusion, the regulariser
def test_mapper_by_stamp_equals_the_host_image_route(name):
    sc = S.Scenario(name, n_ticks=14)
    st, p, rig = sc.stream(), sc.params, sc.rig
    assert bool(p.smooth_time_surface) == (name == "dsec")
    a, b = lib.Esvo(p, rig), lib.Esvo(p, rig)
    a.ts_history_configure(12)
    for d in (a, b):
        d.ts_push_events(0, st.ev_left)
        d.ts_push_events(1, st.ev_right)
    times = [st.t0_ns + int(round(sc.spec["t_first"] * 1e9)) + k * STEP for k in range(14)]
    pairs, ticks = {}, 0
    for k, t in enumerate(times):
        pairs[t] = [a.ts_render(cam, t) for cam in (0, 1)]     # downloaded as they are made
        for cam in (0, 1):
            b.ts_render(cam, t, download=False)
        if k % 5 != 3:
            continue
        t_obs = times[k - 1]                                   # the second newest pair
        T = st.pose(t_obs)
        stamps, poses = rostime.pose_table(st.pose, t_obs, p.bm_half_slice_thickness)
        a.set_observation_at(t_obs, T)
        a.tick(t_obs, stamps, poses)
        b.set_observation(t_obs, pairs[t_obs][0], pairs[t_obs][1], T)
        b.tick(t_obs, stamps, poses)
        _same_map(a.get_map(), b.get_map())
        fa, fb = a.get_last_frame(), b.get_last_frame()
        assert len(fa) == len(fb) and fa.tobytes() == fb.tobytes()
        assert _counters(a) == _counters(b)
        ticks += 1
    assert ticks == 3 and len(a.get_map()) > 50 and a.stats().last_points > 0
    assert not np.array_equal(pairs[times[12]][0], pairs[times[13]][0]), "the observed pair is not the resident one"
    # an evicted stamp: refused, the observation stays in place, the next tick equals the other handle's
    assert list(a.ts_history()[0]) == times[2:]
    msg = _refused(lambda: a.set_observation_at(times[1], st.pose(times[1])))
    assert str(times[1]) in msg and str(times[2]) in msg and str(times[13]) in msg
    stamps, poses = rostime.pose_table(st.pose, times[13], p.bm_half_slice_thickness)
    a.tick(times[13], stamps, poses)
    b.tick(times[13], stamps, poses)
    _same_map(a.get_map(), b.get_map())
    assert a.get_last_frame().tobytes() == b.get_last_frame().tobytes() and _counters(a) == _counters(b)
    a.close()
    b.close()


# ---- B4: tracker by stamp ----------------------------------------------------------------------------------------------------
def _tracker_case(which):
    if which == "95x63":
        rig = _small_rig(95, 63)
        return rig, synth.make_stream(rig, 400, 0.08, 0.3, 1.0, seed=20251020), "mvstereo_upenn"
    rig = calib.dataset_rig("upenn")
    return rig, synth.make_stream(rig, 3000, 0.08, 0.16, 1.0, seed=20251021), "mapping_upenn"


@pytest.mark.parametrize("which", ["95x63", "upenn"])
def test_tracker_by_stamp_equals_the_host_image_route(which):
    rig, st, preset = _tracker_case(which)
    p, _ = params.make_params(params.PRESETS[preset], rig)
    dev, host = lib.Esvo(p, rig), lib.Esvo(p, rig)
    dev.ts_history_configure(4)
    dev.ts_push_events(0, st.ev_left)
    times = [st.t0_ns + (3 + k) * STEP for k in range(3)]
    imgs = {t: dev.ts_render(0, t) for t in times}             # left frames only: all the tracker needs
    assert list(dev.ts_history()[1]) == [1, 1, 1]
    assert imgs[times[0]].any() and not np.array_equal(imgs[times[0]], imgs[times[2]])
    # 300 reference points in front of the camera at the first frame
    rng = np.random.default_rng(5)
    P = np.asarray(rig.left.P, np.float64).reshape(3, 4)
    z = rng.uniform(1.5, 4.0, 300)
    u, v = rng.uniform(4, rig.width - 5, 300), rng.uniform(4, rig.height - 5, 300)
    cam_xyz = np.stack([(u - P[0, 2]) / P[0, 0] * z, (v - P[1, 2]) / P[1, 1] * z, z], 1)
    T_ref = st.pose(times[0])
    xyz = (cam_xyz @ T_ref[:3, :3].T + T_ref[:3, 3]).astype(np.float32)
    R, tr = np.eye(3), np.array([0.004, -0.002, 0.001])
    for d in (dev, host):
        d.track_set_reference(xyz, T_ref)
    for ks in (0, 5):
        for t in (times[2], times[0]):                         # the newest stamp, and an older one that is not the resident frame
            dev.track_set_current_at(t, ks)
            host.track_set_current(imgs[t], ks)
            for x, y in zip(dev.track_images(), host.track_images()):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (ks, t)
            ga, gb = dev.track_normal_equations(R, tr, 0, 300), host.track_normal_equations(R, tr, 0, 300)
            assert ga[3] == gb[3] == 300
            assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes() and ga[2] == gb[2], (ks, t)
    dev.track_set_current_at(times[0], 0)
    older = dev.track_images()[0]
    dev.track_set_current(None, 0)                             # the resident frame is still the newest render
    assert not np.array_equal(older, dev.track_images()[0]) and np.array_equal(dev.track_images()[0], 255 - imgs[times[2]])
    _refused(lambda: dev.track_set_current_at(times[2] + 1, 5))
    _refused(lambda: dev.track_set_current_at(times[2], 3), ERR_UNSUPPORTED)
    dev.close()
    host.close()


# ---- B5: three threads on one handle -----------------------------------------------------------------------------------------
def test_render_tracker_and_mapper_threads(small_stream):
    """a render thread, a tracker thread on the newest complete stamp and a mapper thread on the second newest, four pairs
    retained; the render thread is never more than two frames ahead of either reader, so no requested stamp can be evicted"""
    rig, st = small_stream
    n = 12
    times = [st.t0_ns + 25_000_000 + k * 5_000_000 for k in range(n)]

    def setup():
        dev, p = _handle(rig)
        dev.ts_history_configure(4)
        dev.ts_push_events(0, st.ev_left)
        dev.ts_push_events(1, st.ev_right)
        return dev, p

    def render(dev, k):
        dev.ts_render(0, times[k], download=False)
        dev.ts_render(1, times[k], download=False)

    def track(dev, k):
        dev.track_set_current_at(times[k], 5)
        return dev.track_images()

    def mapper(dev, p, k):
        if k == 0:
            return None
        t = times[k - 1]
        stamps, poses = rostime.pose_table(st.pose, t, p.bm_half_slice_thickness)
        dev.set_observation_at(t, st.pose(t))
        dev.tick(t, stamps, poses)
        return dev.get_map()

    dev, p = setup()
    want_trk, want_map = [], []
    for k in range(n):
        render(dev, k)
        want_trk.append(track(dev, k))
        want_map.append(mapper(dev, p, k))
    dev.close()
    assert len(want_map[-1]) > 20 and not np.array_equal(want_trk[0][0], want_trk[-1][0])

    dev, p = setup()
    errors, got_trk, got_map = [], [None] * n, [None] * n
    rendered = [-1]
    cv = threading.Condition()
    room = [threading.Semaphore(3), threading.Semaphore(3)]    # frame k + 3 is rendered only once both readers are done with frame k

    def render_main():
        try:
            for k in range(n):
                for s in room:
                    assert s.acquire(timeout=120) or errors
                render(dev, k)
                with cv:
                    rendered[0] = k
                    cv.notify_all()
        except BaseException as e:  # noqa: BLE001
            errors.append(("render", repr(e)))
            with cv:
                cv.notify_all()

    def reader_main(which, fn, out):
        try:
            for k in range(n):
                with cv:
                    assert cv.wait_for(lambda: rendered[0] >= k or errors, timeout=120) and not errors, errors
                out[k] = fn(k)
                room[which].release()
        except BaseException as e:  # noqa: BLE001
            errors.append((which, repr(e)))
            for _ in range(n):                                 # (the render thread must not wait for a reader that is gone)
                room[which].release()
            with cv:
                cv.notify_all()

    threads = [threading.Thread(target=render_main), threading.Thread(target=reader_main, args=(0, lambda k: track(dev, k), got_trk)),
               threading.Thread(target=reader_main, args=(1, lambda k: mapper(dev, p, k), got_map))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
    assert not errors, errors
    for k in range(n):
        for x, y in zip(got_trk[k], want_trk[k]):
            assert x.tobytes() == y.tobytes(), k
        if k:
            _same_map(got_map[k], want_map[k])
    assert list(dev.ts_history()[0]) == times[-4:]
    dev.close()


# ---- B6: the node-rate loop --------------------------------------------------------------------------------------------------
def test_node_rate_loop_resident_equals_host_route():
    from esvo_amd import closed_loop
    a = closed_loop.run_node_rates(n_frames=20, map_every=5, resident=True)
    b = closed_loop.run_node_rates(n_frames=20, map_every=5, resident=False)
    assert a["tick_frames"] == b["tick_frames"] and a["tick_stamps"] == b["tick_stamps"] and len(a["tick_frames"]) >= 2
    assert np.array_equal(np.array(a["poses"]), np.array(b["poses"])) and len(a["poses"]) == 20
    assert a["points"] == b["points"] and a["n_inside"] == b["n_inside"]
    _same_map(a["map"], b["map"])
    # loose sanity only: every mapper tick produced points, the tracker's reference lands inside the image
    assert all(n > 0 for n in a["points"]) and all(n > 0 for n in a["n_inside"])


# ---- B7: life cycle, refused handles, the C++ layer --------------------------------------------------------------------------
def test_slots_are_freed_and_the_ledger_balances():
    rig = _small_rig(95, 63)
    before = lib.debug_live_allocations()
    dev, _ = _handle(rig)
    created = lib.debug_live_allocations()
    stride = (95 * 63 + 255) // 256 * 256
    dev.ts_history_configure(100)
    n100, b100 = lib.debug_live_allocations()
    assert n100 == created[0] + 1 and b100 - created[1] >= 100 * 2 * stride
    dev.ts_history_put(1, 0, _image(rig, 0, 0))
    dev.ts_history_configure(3)
    n3, b3 = lib.debug_live_allocations()
    assert n3 == created[0] + 1 and 3 * 2 * stride <= b3 - created[1] < b100 - created[1]
    dev.ts_history_configure(0)
    assert lib.debug_live_allocations() == created
    dev.ts_history_configure(2)
    dev.close()                                                # esvo_destroy with the history on
    assert lib.debug_live_allocations() == before


def test_refused_on_sharded_and_tick_interleaved_handles():
    rig = _small_rig(96, 64)
    dev, _ = _handle(rig)
    dev.ts_history_configure(3)                                # history on: no band, no communicator
    for fn in (lambda: dev.set_band(0, 32, 0, 2), lambda: dev.comm_init_callbacks(0, 1, lambda s, d, n, stream: 0),
               lambda: dev.comm_init(bytes(128), 0, 1)):
        assert "Time-Surface history" in _refused(fn, ERR_UNSUPPORTED)
    dev.ts_history_configure(0)
    dev.set_band(0, 32, 0, 2)                                  # a band-sharded handle: no history
    assert "band-sharded" in _refused(lambda: dev.ts_history_configure(3), ERR_UNSUPPORTED)
    dev.ts_history_configure(0)                                # switching it off (again) is always possible
    dev.close()
    dev, _ = _handle(rig)
    dev.comm_init_callbacks(0, 1, lambda s, d, n, stream: 0)   # a tick-interleaved handle: no history
    _refused(lambda: dev.ts_history_configure(3), ERR_UNSUPPORTED)
    dev.close()


def test_cpp_layer(tmp_path):
    """tests/cpp/ts_history.cpp: esvo_hip::TimeSurfaceHistory, DepthFusion::setObservationAt and RegProblemLM::setCurrentAt against
    the host-image route on the same handle -- matches and normal equations equal as bytes"""
    sc = S.Scenario("upenn", n_ticks=12)
    st, p, rig = sc.stream(), sc.params, sc.rig
    src = lib.Esvo(p, rig)
    src.ts_push_events(0, st.ev_left)
    src.ts_push_events(1, st.ev_right)
    times = [st.t0_ns + int(round(sc.spec["t_first"] * 1e9)) + k * STEP for k in range(12)]
    left = np.stack([src.ts_render(0, t) for t in times])
    right = np.stack([src.ts_render(1, t) for t in times])
    t_obs = times[9]                                           # the pair the program's lookup leads to
    for k in (7, 8, 9):                                        # a map of three ticks: the tracker's reference cloud
        stamps, poses = rostime.pose_table(st.pose, times[k], p.bm_half_slice_thickness)
        src.set_observation(times[k], left[k], right[k], st.pose(times[k]))
        src.tick(times[k], stamps, poses)
    xyz = src.get_pointcloud()
    assert len(xyz) > 50                                       # (any cloud will do: the sums are compared as bytes)
    src.close()
    from oracle import oracle as O
    ev = st.ev_left[O.select_events(st.ev_left, t_obs, p.bm_half_slice_thickness, p.process_event_num)]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "ts_history")
    libdir = os.path.dirname(lib._LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "ts_history.cpp"), "-o", exe, "-L", libdir, "-lesvo_hip",
                           f"-Wl,-rpath,{libdir}"])
    d = tmp_path
    np.array(times, np.uint64).tofile(d / "stamps.bin")
    left.tofile(d / "left.bin")
    right.tofile(d / "right.bin")
    st.pose(t_obs).reshape(16).tofile(d / "Tobs.bin")
    np.ascontiguousarray(ev).tofile(d / "ev.bin")
    np.ascontiguousarray(stamps, np.uint64).tofile(d / "pose_stamps.bin")
    np.ascontiguousarray(poses, np.float64).tofile(d / "poses.bin")
    xyz.tofile(d / "xyz.bin")
    st.pose(times[8]).reshape(16).tofile(d / "Tref.bin")
    np.eye(3).tofile(d / "R.bin")
    np.array([0.004, -0.002, 0.001]).tofile(d / "tr.bin")
    for c, cal in ((0, rig.left), (1, rig.right)):
        cal.P.tofile(d / f"P{c}.bin")
        cal.rect_lut.tofile(d / f"lut{c}.bin")
        cal.map_x.tofile(d / f"mx{c}.bin")
        cal.map_y.tofile(d / f"my{c}.bin")
    (d / "params.bin").write_bytes(C.string_at(C.addressof(p), C.sizeof(p)))
    subprocess.check_call(["timeout", "-k", "10", "120", exe, str(d), str(rig.width), str(rig.height)])
    blob = (d / "out.bin").read_bytes()
    n_host, n_hist, k = np.frombuffer(blob[:24], np.uint64)
    sums = np.frombuffer(blob[24:], np.float64).reshape(5, 43)
    assert k == 9 and n_host == n_hist and n_host > 50
    assert (d / "emp_host.bin").read_bytes() == (d / "emp_hist.bin").read_bytes()
    assert sums[0].tobytes() == sums[1].tobytes() and sums[2].tobytes() == sums[3].tobytes()
    assert sums[0].tobytes() != sums[2].tobytes()              # the older frame is another image
    assert sums[4].tobytes() == sums[3].tobytes()              # a refused stamp leaves the current frame in place
