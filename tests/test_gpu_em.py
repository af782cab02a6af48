"""Event-to-event matching on the device (esvo_map_match_em / esvo_map_tick_em, esvo_MVStereo modes 0 and 2) against the CPU
restatement tests/em_restated.py, bit for bit, and the EM ticks against the pinned stage-wise calls they are built from."""
import os
import subprocess

import numpy as np
import pytest

import em_restated as R
from esvo_amd import calib, lib, params, synth

pytestmark = pytest.mark.gpu

NS = R.NS
STREAMS = {  # rig -> make_stream arguments (points, duration, rho range, speed)
    "upenn": (6000, 0.2, 0.16, 1.0, 1.0),
    "rpg": (4000, 0.2, 0.2, 2.0, 1.0),
    "dsec": (20000, 0.12, 0.02, 0.25, 2.0),
}
_cache = {}


def stream(name):
    if name not in _cache:
        rig = calib.dataset_rig(name)
        n, dur, r0, r1, sp = STREAMS[name]
        _cache[name] = (rig, synth.make_stream(rig, n, dur, r0, r1, seed=20250501, speed=sp))
    return _cache[name]


def make_dev(rig, **kw):
    over = dict(max_events_per_tick=4096, smooth_time_surface=0)
    over.update(kw)
    preset = "mapping_dsec" if rig.name == "dsec" else "mvstereo_upenn"  # the depth range sets the (unused) BM disparity range
    p, _ = params.make_params(params.PRESETS[preset], rig, **over)
    return lib.Esvo(p, rig, device=0), p


def observe(dev, st, t):
    dev.ts_push_events(0, st.ev_left)
    dev.ts_push_events(1, st.ev_right)
    g = [dev.ts_render(c, t) for c in (0, 1)]
    dev.set_observation(t, g[0], g[1], st.pose(t))
    return g


def stamps(ev):
    return ev["sec"].astype(np.uint64) * np.uint64(NS) + ev["nsec"].astype(np.uint64)


def seam_case(st, t_low, t_up, cap, thickness):
    """the node's side of the seam: dataTransferring + eventSlicingForEM, from the restatement"""
    sl, nl = R.select(stamps(st.ev_left), t_low, t_up, cap)
    sr, nr = R.select(stamps(st.ev_right), t_low, t_up, cap)
    left, right = st.ev_left[sl:sl + nl], st.ev_right[sr:sr + nr]
    slices = R.slice_events(stamps(left), t_low, t_up, thickness)
    begin = np.array([s[0] for s in slices], np.uint32)
    count = np.array([s[1] for s in slices], np.uint32)
    T = np.stack([np.asarray(st.pose(s[2]), np.float64).reshape(4, 4) for s in slices])
    return left, right, begin, count, T


def assert_same(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for f in R.MATCH_FIELDS:
        assert a[f].tobytes() == b[f].tobytes(), f


CASES = [  # rig, patch, epipolar threshold, threads, time threshold
    ("upenn", (15, 7), 1.0, 4, 5e-4),
    ("upenn", (25, 25), 0.5, 1, 5e-4),
    ("rpg", (10, 4), 1.0, 4, 5e-4),
    ("rpg", (15, 7), 0.5, 1, 5e-4),
    ("dsec", (15, 7), 1.0, 4, 5e-4),
    ("dsec", (25, 25), 0.5, 1, 5e-5),
]


@pytest.mark.parametrize("name,patch,epi,threads,time_thr", CASES)
def test_match_em_equals_restatement(name, patch, epi, threads, time_thr):
    rig, st = stream(name)
    dev, p = make_dev(rig, patch_size_x=patch[0], patch_size_y=patch[1], num_threads=threads)
    t = st.t0_ns + int(0.1e9)
    g = observe(dev, st, t)
    em = params.make_em_params(params.PRESETS["mvstereo_upenn"], epipolar_threshold=epi, time_threshold=time_thr)
    left, right, begin, count, T = seam_case(st, t - 20_000_000, t, 3000, em.slice_thickness)
    got = dev.match_em(em, left, begin, count, T, right)
    want, s = R.match(rig, patch[0], patch[1], threads, em, st.pose(t), g[0], g[1], left, begin, count, T, right, want_stats=True)
    assert len(want) > 0
    assert_same(got, want)
    es = dev.em_stats()
    assert (es.events, es.time_polarity, es.epipolar, es.patch_ok, es.matches) == \
        (s["events"], s["time_polarity"], s["epipolar"], s["patch_ok"], s["matches"])


def test_match_em_dsec_large():
    rig, st = stream("dsec")
    dev, p = make_dev(rig, num_threads=4)
    t = st.t0_ns + int(0.1e9)
    g = observe(dev, st, t)
    em = params.make_em_params(params.PRESETS["mvstereo_upenn"], time_threshold=5e-5)
    left, right, begin, count, T = seam_case(st, t - 60_000_000, t, 200_000, em.slice_thickness)
    assert count.sum() >= 100_000
    got = dev.match_em(em, left, begin, count, T, right)
    want = R.match(rig, 15, 7, 4, em, st.pose(t), g[0], g[1], left, begin, count, T, right)
    assert len(want) > 0
    assert_same(got, want)


def test_match_em_no_candidates_and_no_slices():
    rig, st = stream("upenn")
    dev, p = make_dev(rig)
    t = st.t0_ns + int(0.1e9)
    observe(dev, st, t)
    em = params.make_em_params(params.PRESETS["mvstereo_upenn"])
    left, right, begin, count, T = seam_case(st, t - 10_000_000, t, 3000, em.slice_thickness)
    later = right.copy()
    later["sec"] += 1  # no right event within any left event's time window
    assert len(dev.match_em(em, left, begin, count, T, later)) == 0
    s = dev.em_stats()
    assert s.time_polarity == 0 and s.events == count.sum() and s.matches == 0
    assert len(dev.match_em(em, left, begin[:0], count[:0], T[:0], right)) == 0
    assert len(dev.match_em(em, left, begin, count, T, right[:0])) == 0


def test_match_em_skips_events_off_the_sensor():
    """a left and a right event outside the image (u16 coordinates up to 65535) are never used to index the rectification
    tables: the left one keeps its position and gets no match, the right one is no candidate -- the matches equal the restatement
    with the right one dropped"""
    rig, st = stream("upenn")
    dev, p = make_dev(rig, num_threads=4)
    t = st.t0_ns + int(0.1e9)
    g = observe(dev, st, t)
    em = params.make_em_params(params.PRESETS["mvstereo_upenn"])
    left, right, begin, count, T = seam_case(st, t - 20_000_000, t, 3000, em.slice_thickness)
    bad_l = left[1:2].copy()
    bad_l["x"], bad_l["y"] = 65535, 65535
    left2 = np.concatenate([left[:1], bad_l, left[1:]])          # position 1, inside slice 0
    count2, begin2 = count.copy(), begin.copy()
    count2[0] += 1
    begin2[1:] += 1
    k = len(right) // 2
    bad_r = right[k:k + 1].copy()
    bad_r["x"], bad_r["y"] = rig.width + 3, 7
    right2 = np.concatenate([right[:k], bad_r, right[k:]])
    got = dev.match_em(em, left2, begin2, count2, T, right2)
    want = R.match(rig, 15, 7, 4, em, st.pose(t), g[0], g[1], left2, begin2, count2, T, right)
    assert len(want) > 0 and 1 not in set(want["event_idx"].tolist())
    assert_same(got, want)
    assert_same(got, R.match(rig, 15, 7, 4, em, st.pose(t), g[0], g[1], left2, begin2, count2, T, right2))


def test_match_em_threshold_one_keeps_the_references_corner_case():
    """EM_TS_NCC_THRESHOLD >= 1 and every candidate's patches outside the image: the reference emits candidate 0 with cost 1.0 and
    inv_depth = 1 / 0 = +inf (its best_depth keeps 0); next to it an ordinary match"""
    W, H = 80, 48
    rig = calib.ideal_rig(W, H, 50.0, 0.1)
    dev, p = make_dev(rig, num_threads=4)
    rng = np.random.default_rng(5)
    L = rng.integers(0, 256, (H, W)).astype(np.uint8)
    Rt = np.zeros_like(L)
    Rt[:, : W - 10] = L[:, 10:]
    dev.set_observation(10 * NS, L, Rt, np.eye(4))

    def ev(xs, ys, t_ns):
        e = np.zeros(len(xs), lib.EVENT_DTYPE)
        e["x"], e["y"], e["sec"], e["nsec"], e["polarity"] = xs, ys, t_ns // NS, t_ns % NS, 1
        return e
    T0 = 10 * NS
    left = np.concatenate([ev([3], [20], T0), ev([4], [30], T0 + 1_000_000), ev([40], [20], T0 + 2_000_000)])
    right = np.concatenate([ev([1, 2], [20, 20], T0), ev([0], [30], T0 + 1_000_000), ev([30, 35], [20, 20], T0 + 2_000_000)])
    em = params.make_em_params(params.PRESETS["mvstereo_upenn"], ncc_threshold=1.0)
    b, c, T = np.array([0], np.uint32), np.array([3], np.uint32), np.eye(4)[None]
    got = dev.match_em(em, left, b, c, T, right)
    want, s = R.match(rig, 15, 7, 4, em, np.eye(4), L, Rt, left, b, c, T, right, want_stats=True)
    assert s["epipolar"] == 5 and s["patch_ok"] == 2
    assert len(want) == 3 and int(np.isinf(want["inv_depth"]).sum()) == 2 and set(want["cost"][np.isinf(want["inv_depth"])]) == {1.0}
    assert_same(got, want)


def _pose_fn(st):
    return lambda t_ns: st.pose(t_ns)


def _check_selection(dev, st, t_low, t_up, cap, thickness):
    s = dev.em_selection()
    sl, nl = R.select(stamps(st.ev_left), t_low, t_up, cap)
    sr, nr = R.select(stamps(st.ev_right), t_low, t_up, cap)
    assert (s["left_first"], s["left_count"], s["right_first"], s["right_count"]) == (sl, nl, sr, nr)
    slices = R.slice_events(stamps(st.ev_left[sl:sl + nl]), t_low, t_up, thickness)
    assert [tuple(x) for x in zip(s["slice_begin"], s["slice_count"], s["slice_t_ns"])] == [tuple(x) for x in slices]
    for k, x in enumerate(slices):
        assert np.array_equal(s["slice_T"][k], np.asarray(st.pose(x[2]), np.float64).reshape(4, 4))
    return s


@pytest.mark.parametrize("mode", [0, 2])
def test_tick_em_equals_stagewise(mode):
    """mode 0: esvo_map_tick_em == esvo_map_match_em + esvo_map_fuse_matches_naive, window of maxNumFusionFrames frames.
    mode 2: esvo_map_tick_em == the pinned oracle's set_poses (slice table) + refine + push_frame + fuse on the restatement's
    matches."""
    from oracle import oracle
    rig, st = stream("upenn")
    dev, p = make_dev(rig, max_fusion_frames=3, num_threads=4)
    em = params.make_em_params(params.PRESETS["mvstereo_upenn"], num_event_matching=2000)
    if mode == 0:
        ref, _ = make_dev(rig, max_fusion_frames=3, num_threads=4)
        ref.ts_push_events(0, st.ev_left)
        ref.ts_push_events(1, st.ev_right)
    else:
        orc = oracle.OracleMapper(p, rig)
        orc.set_mode(True, True)
    dev.ts_push_events(0, st.ev_left)
    dev.ts_push_events(1, st.ev_right)
    for k in range(5):
        t = st.t0_ns + int(0.06e9) + k * 20_000_000
        g = [dev.ts_render(c, t) for c in (0, 1)]
        dev.set_observation(t, None, None, st.pose(t))
        t_low = t - 15_000_000
        dev.tick_em(em, mode, t_low, t, _pose_fn(st))
        s = _check_selection(dev, st, t_low, t, em.num_event_matching, em.slice_thickness)
        left = st.ev_left[s["left_first"]:s["left_first"] + s["left_count"]]
        right = st.ev_right[s["right_first"]:s["right_first"] + s["right_count"]]
        if mode == 0:
            for c in (0, 1):
                ref.ts_render(c, t)
            ref.set_observation(t, None, None, st.pose(t))
            m = ref.match_em(em, left, s["slice_begin"], s["slice_count"], s["slice_T"], right)
            assert dev.em_stats().matches == len(m) > 0
            ref.fuse_matches_naive(m, s["slice_T"])
            a, b = dev.get_map(), ref.get_map()
            assert a.tobytes() == b.tobytes(), k
            assert dev.stats().last_window_frames == min(k + 1, 3)
            assert dev.stats().last_matches == len(m)
        else:
            m = R.match(rig, 15, 7, 4, em, st.pose(t), g[0], g[1], left, s["slice_begin"], s["slice_count"], s["slice_T"], right)
            assert dev.em_stats().matches == len(m) > 0
            orc.set_observation(t, g[0], g[1], st.pose(t))
            orc.set_poses(s["slice_t_ns"], s["slice_T"])
            pts = orc.refine(m)
            orc.push_frame(pts, s["slice_T"])
            orc.fuse()
            a, b = dev.get_map(), orc.get_map()
            assert len(a) > 0
            assert a.tobytes() == b.tobytes(), k


def test_tick_em_edge_cases():
    rig, st = stream("upenn")
    dev, p = make_dev(rig, max_poses_per_tick=8, max_events_per_tick=32768)
    em = params.make_em_params(params.PRESETS["mvstereo_upenn"], num_event_matching=20000)
    t = st.t0_ns + int(0.1e9)
    dev.ts_push_events(0, st.ev_left)  # no right events staged: no tick
    for c in (0, 1):
        dev.ts_render(c, t)
    dev.set_observation(t, None, None, st.pose(t))
    dev.tick_em(em, 2, t - 5_000_000, t, _pose_fn(st))
    s = dev.em_selection()
    assert s["left_count"] > 0 and s["right_count"] == 0 and s["n_slices"] == 0
    assert len(dev.get_map()) == 0 and dev.stats().ticks == 0
    dev.ts_push_events(1, st.ev_right)
    dev.tick_em(em, 2, t - 5_000_000, t, _pose_fn(st))   # 5 slices: fits 8 poses
    assert 0 < dev.em_selection()["n_slices"] <= 8
    before, sel = dev.get_map(), dev.em_selection()
    with pytest.raises(lib.EsvoError) as e:
        dev.tick_em(em, 2, t - 20_000_000, t, _pose_fn(st))  # 20 slices > 8 poses
    assert e.value.code == -4  # ESVO_ERR_CAPACITY
    assert dev.get_map().tobytes() == before.tobytes()
    assert dev.em_selection()["left_first"] == sel["left_first"]
    with pytest.raises(lib.EsvoError):
        dev.tick_em(em, 1, t - 5_000_000, t, _pose_fn(st))  # modes 0 and 2 only


def test_cpp_event_matcher_class(tmp_path):
    """include/esvo_hip.hpp's EventMatcher (createMatchProblem + match_all_HyperThread) gives the C-ABI's matches"""
    rig, st = stream("rpg")
    dev, p = make_dev(rig, num_threads=4)
    t = st.t0_ns + int(0.1e9)
    g = observe(dev, st, t)
    em = params.make_em_params(params.PRESETS["mvstereo_rpg"])
    left, right, begin, count, T = seam_case(st, t - 10_000_000, t, 3000, em.slice_thickness)
    want = dev.match_em(em, left, begin, count, T, right)
    dev.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "em_class")
    libdir = os.path.dirname(lib._LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "em_class.cpp"), "-o", exe, "-L", libdir, "-lesvo_hip",
                           f"-Wl,-rpath,{libdir}"])
    d = tmp_path
    left.tofile(d / "left.bin")
    right.tofile(d / "right.bin")
    np.asarray(begin, np.uint32).tofile(d / "begin.bin")
    np.asarray(count, np.uint32).tofile(d / "count.bin")
    np.ascontiguousarray(T, np.float64).tofile(d / "T.bin")
    g[0].tofile(d / "tsl.bin")
    g[1].tofile(d / "tsr.bin")
    np.asarray(st.pose(t), np.float64).reshape(16).tofile(d / "Tobs.bin")
    for c, cal in ((0, rig.left), (1, rig.right)):
        cal.P.tofile(d / f"P{c}.bin")
        cal.rect_lut.tofile(d / f"lut{c}.bin")
        cal.map_x.tofile(d / f"mx{c}.bin")
        cal.map_y.tofile(d / f"my{c}.bin")
    import ctypes as C
    (d / "params.bin").write_bytes(C.string_at(C.addressof(p), C.sizeof(p)))
    (d / "em.bin").write_bytes(C.string_at(C.addressof(em), C.sizeof(em)))
    subprocess.check_call(["timeout", "-k", "10", "300", exe, str(d), str(rig.width), str(rig.height)])
    got = np.fromfile(d / "out.bin", dtype=want.dtype)
    assert len(want) > 0
    assert_same(got, want)
