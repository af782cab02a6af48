"""esvo_MVStereo mode 4 (PURE_SEMI_GLOBAL_MATCHING) on the device -- esvo_map_tick_sgm and its seam esvo_map_push_disparity_frame
-- against the CPU restatement tests/sgm_tick_restated.py (pinned to the reference's own mode-4 branch in
tests/test_sgm_tick_restated.py), byte for byte in every field of the frame and of the DepthMap, and the disparity image against
the oracle's StereoSGBM bit for bit.  "Byte for byte" treats two NaNs as equal (sgm_tick_restated.same_bits): the p_cam of a
zero-disparity point holds 0 * inf where the ray's component is 0, whose sign and payload differ between processors.

Not covered: the refusal "selected events already overwritten in the event ring".  It needs a pusher thread that holds a block
reserved while the tick selects (esvo_ts_push_events trims the host stamps to the ring, so a single thread cannot select an
overwritten event); the tick shares that check with esvo_map_init_sgm (one function).  "More selected events than
max_events_per_tick" cannot arise in the tick either (the handle sizes its buffers for PROCESS_EVENT_NUM + 1); it is checked on
the seam, which takes any number of events."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sgm_tick_cases as SC
import sgm_tick_restated as SR
from esvo_amd import abi, calib, lib, params

pytestmark = pytest.mark.gpu

ERR_CAPACITY, ERR_UNSUPPORTED, ERR_STATE = -4, -5, -6   # esvo_status_t
COUNTS = ("events", "on_image", "matched_columns", "disp_ok", "points", "zero_disp")
_runs = {}


def _stage(dev, stream):
    dev.ts_push_events(0, stream.ev_left)                             # the whole stream is staged: lower_bound(t) != end()
    dev.ts_push_events(1, stream.ev_right)


def run(name):
    """the case's ticks through esvo_map_tick_sgm with device-resident Time Surfaces, once per process:
    [dict(n, disp, frame, map, stats, sgm)]"""
    if name not in _runs:
        rig, stream, p, ticks = SC.case(name)
        dev = lib.Esvo(p, rig)
        _stage(dev, stream)
        out = []
        for tk in ticks:
            dev.ts_render(0, tk["t"], download=False)
            dev.ts_render(1, tk["t"], download=False)
            dev.set_observation(tk["t"], None, None, tk["T"])
            n, disp = dev.tick_sgm()
            frame, mp = dev.get_last_frame(), dev.get_map()
            s, g = dev.stats(), dev.sgm_stats()
            out.append(dict(n=n, disp=disp, frame=frame, map=mp, sgm={k: int(getattr(g, k)) for k in COUNTS},
                            ms=(g.ms_sgbm, g.ms_points, g.ms_propagate),
                            stats={k: int(getattr(s, k)) for k in ("ticks", "last_events_in", "last_points", "last_window_frames",
                                                                   "last_window_points", "last_map_size")}))
        dev.close()
        _runs[name] = out
    return _runs[name]


def test_upenn_ticks_equal_the_restatement():
    rig, stream, p, ticks = SC.case("upenn")
    zero = 0
    for k, (tk, got, (frame, mp, window, counts)) in enumerate(zip(ticks, run("upenn"), SC.restated("upenn"))):
        assert np.array_equal(got["disp"], tk["disp"]), k             # the whole disparity image, bit for bit
        assert got["n"] == len(frame) > 100
        assert SR.same_bits(got["frame"], frame) is None, (k, SR.same_bits(got["frame"], frame))
        assert not got["frame"]["scale2"].any() and not got["frame"]["nu"].any()
        assert SR.same_bits(got["map"], mp) is None, (k, SR.same_bits(got["map"], mp))
        assert got["stats"] == dict(ticks=k + 1, last_events_in=len(tk["idx"]), last_points=len(frame), last_window_frames=len(window),
                                    last_window_points=sum(window), last_map_size=len(mp)), k
        assert got["sgm"] == counts, k
        assert got["ms"][0] > 0 and got["ms"][1] > 0 and got["ms"][2] > 0
        zero += counts["zero_disp"]
    assert zero > 0                                                   # a disparity of exactly 0 is kept: the case holds such points
    assert window == [len(r[0]) for r in SC.restated("upenn")[-3:]]   # the window rolled: maxNumFusionFrames = 3


def test_seam_equals_tick():
    """a second handle fed push_disparity_frame(disp, staged[idx]) tick by tick has the same map bytes"""
    rig, stream, p, ticks = SC.case("upenn")
    dev = lib.Esvo(p, rig)
    for k, (tk, want) in enumerate(zip(ticks, run("upenn"))):
        dev.set_observation(tk["t"], tk["l"], tk["r"], tk["T"])
        assert dev.push_disparity_frame(tk["disp"], stream.ev_left[tk["idx"]]) == want["n"]
        assert dev.get_last_frame().tobytes() == want["frame"].tobytes(), k
        assert dev.get_map().tobytes() == want["map"].tobytes(), k
        assert {c: int(getattr(dev.sgm_stats(), c)) for c in COUNTS} == want["sgm"]
        assert dev.sgm_stats().ms_sgbm == 0
    assert dev.stats().last_window_frames == 3
    dev.close()


def test_seam_on_the_devices_last_disparity():
    """disp16 = NULL: the disparity image the last SGM run left on the device"""
    rig, stream, p, ticks = SC.case("upenn")
    tk = ticks[0]
    dev = lib.Esvo(p, rig)
    dev.set_observation(tk["t"], tk["l"], tk["r"], tk["T"])
    with pytest.raises(lib.EsvoError, match="no disparity image") as e:
        dev.push_disparity_frame(None, stream.ev_left[tk["idx"]])
    assert e.value.code == ERR_STATE
    _stage(dev, stream)
    n, disp = dev.tick_sgm(tk["l"], tk["r"])                         # host images
    assert np.array_equal(disp, tk["disp"]) and n == run("upenn")[0]["n"]
    first = dev.get_map()
    dev.reset()
    with pytest.raises(lib.EsvoError, match="set_observation|no disparity image"):
        dev.push_disparity_frame(None, stream.ev_left[tk["idx"]])
    dev.close()
    assert first.tobytes() == run("upenn")[0]["map"].tobytes()


def test_dsec_ticks_equal_the_restatement():
    """640 x 480, PROCESS_EVENT_NUM of the preset, a moving camera: the window's frames carry different poses"""
    rig, stream, p, ticks = SC.case("dsec")
    assert not np.array_equal(ticks[0]["T"], ticks[-1]["T"])
    for k, (tk, got, (frame, mp, window, counts)) in enumerate(zip(ticks, run("dsec"), SC.restated("dsec"))):
        assert np.array_equal(got["disp"], tk["disp"]), k
        assert got["n"] == len(frame) > 1000 and got["sgm"] == counts
        assert SR.same_bits(got["frame"], frame) is None, (k, SR.same_bits(got["frame"], frame))
        assert SR.same_bits(got["map"], mp) is None, (k, SR.same_bits(got["map"], mp))
        assert got["stats"]["last_window_frames"] == len(window) == k + 1


def _crafted(rig, p):
    """a disparity image of -16 except a handful of pixels, and events that exercise each rule"""
    W, H = rig.width, rig.height
    lut = np.asarray(rig.left.rect_lut, np.float32).reshape(H, W, 2)
    pix = np.floor(lut).astype(np.int64)

    def event_at(col, row):  # a sensor pixel whose rectified coordinate floors to (col, row)
        ys, xs = np.nonzero((pix[..., 0] == col) & (pix[..., 1] == row))
        return (int(xs[0]), int(ys[0])) if len(xs) else None
    outside = np.argwhere((pix[..., 0] < 0) | (pix[..., 0] >= W) | (pix[..., 1] < 0) | (pix[..., 1] >= H))
    assert len(outside)                                               # this rig's table maps sensor corners off the image
    def cut(col, row, d):  # does the 2 x 2 block of a point at this pixel cross the border?  (an integer pixel comes back from
        # cam2World -> world2Cam a last bit above or below itself: below, its block starts one cell earlier and fits)
        xy = event_at(col, row)
        if xy is None:
            return False
        one = np.full((H, W), -16, np.int16)
        one[row, col] = d
        fr, _ = SR.points(rig, p, one, abi.make_events([xy[0]], [xy[1]], [10_000_000_000]))
        return 1 <= len(SR.naive_propagation(rig, [(fr, np.eye(4))], np.eye(4))) < 4
    last_col = next((W - 1, r) for r in range(H // 4, H) if event_at(W - 1, r))   # (on this rig it comes back just below W - 1)
    last_row = next((c, H - 1) for c in range(W // 2, W) if cut(c, H - 1, 200))
    disp = np.full((H, W), -16, np.int16)
    cases = [((47, 100), 80),          # column 47: skipped whatever its disparity
             ((48, 100), 80),          # column 48: the first matched column
             ((120, 60), -16),         # no disparity
             ((125, 65), -5),          # a negative value other than "none"
             ((130, 70), 0),           # zero: a point of the frame that touches no cell
             ((140, 80), 33), ((140, 80), 33),   # two events on one pixel: two points, one owner
             (last_col, 160), (last_row, 200)]   # at the last column / row: the 2 x 2 block of the second crosses the border
    xy = []
    for (c, r), d in cases:
        disp[r, c] = d
        xy.append(event_at(c, r))
    xy.append((W, 7))                                                 # off the sensor
    xy.append((int(outside[0][1]), int(outside[0][0])))               # on the sensor, rectified pixel off the image
    ev = abi.make_events([a for a, _ in xy], [b for _, b in xy], 10_000_000_000 + 1000 * np.arange(len(xy)))
    return disp, ev


def test_crafted_disparity_through_the_seam(upenn_rig):
    rig = upenn_rig
    p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], rig, max_fusion_frames=3)
    disp, ev = _crafted(rig, p)
    T = np.eye(4)
    ref = SR.Mapper(rig, p)
    frame = ref.tick(disp, ev, T)
    assert ref.stats == dict(events=11, on_image=9, matched_columns=8, disp_ok=6, points=6, zero_disp=1)
    assert frame["row"][:4].tolist() == [48, 130, 140, 140] and frame["inv_depth"][1] == 0
    assert 1 <= len(SR.naive_propagation(rig, [(frame[5:6], T)], T)) < 4   # the block at the last row is cut
    assert len(ref.map) == 4 + 4 + len(SR.naive_propagation(rig, [(frame[4:6], T)], T))
    blank = np.zeros((rig.height, rig.width), np.uint8)
    dev = lib.Esvo(p, rig)
    dev.set_observation(10_000_000_000, blank, blank, T)
    assert dev.push_disparity_frame(disp, ev) == 6
    assert {c: int(getattr(dev.sgm_stats(), c)) for c in COUNTS} == ref.stats
    assert SR.same_bits(dev.get_last_frame(), frame) is None
    assert SR.same_bits(dev.get_map(), ref.map) is None
    # an empty selection: its empty frame still enters the window, and the third one evicts the crafted frame
    none = ev[:0]
    for k in range(3):
        ref.tick(disp, none, T)
        assert dev.push_disparity_frame(disp, none) == 0
        s = dev.stats()
        assert (s.last_window_frames, s.last_window_points, s.last_points) == (min(k + 2, 3), sum(ref.window_sizes()), 0)
        assert SR.same_bits(dev.get_map(), ref.map) is None
        assert len(dev.get_last_frame()) == 0
    assert len(ref.map) == 0 and ref.window_sizes() == [0, 0, 0]
    dev.close()


def _untouched(dev, before_map, before_stats):
    s = dev.stats()
    return (dev.get_map().tobytes() == before_map.tobytes()
            and (s.last_window_frames, s.last_window_points, s.ticks) == before_stats)


def test_refusals_change_nothing():
    rig, stream, p, ticks = SC.case("upenn")
    tk = ticks[0]
    ev = stream.ev_left[tk["idx"]]
    # no observation
    dev = lib.Esvo(p, rig)
    _stage(dev, stream)
    for call in (lambda: dev.tick_sgm(tk["l"], tk["r"]), lambda: dev.push_disparity_frame(tk["disp"], ev)):
        with pytest.raises(lib.EsvoError, match="set_observation") as e:
            call()
        assert e.value.code == ERR_STATE
    assert len(dev.get_map()) == 0 and dev.stats().last_window_frames == 0
    # one good tick, then every refusal against its map and window
    dev.set_observation(tk["t"], tk["l"], tk["r"], tk["T"])
    dev.tick_sgm(tk["l"], tk["r"])
    before = dev.get_map()
    state = (1, len(run("upenn")[0]["frame"]), 1)
    assert before.tobytes() == run("upenn")[0]["map"].tobytes()
    with pytest.raises(lib.EsvoError, match="esvo_ts_render") as e:  # no device-resident Time Surface
        dev.tick_sgm(None, None)
    assert e.value.code == ERR_STATE and _untouched(dev, before, state)
    max_ev = max(p.max_events_per_tick, p.process_event_num) + 1
    with pytest.raises(lib.EsvoError, match="max_events_per_tick") as e:
        dev.push_disparity_frame(tk["disp"], stream.ev_left[:max_ev + 1])
    assert e.value.code == ERR_CAPACITY and _untouched(dev, before, state)
    dev.set_band(0, rig.height // 2, 0, 2)                            # a sharded handle
    for call in (lambda: dev.tick_sgm(tk["l"], tk["r"]), lambda: dev.push_disparity_frame(tk["disp"], ev)):
        with pytest.raises(lib.EsvoError, match="sharded") as e:
            call()
        assert e.value.code == ERR_STATE
    dev.set_band(0, rig.height, 0, 1)
    assert _untouched(dev, before, state)
    dev.close()
    # a window ring too small for maxNumFusionFrames frames of PROCESS_EVENT_NUM + 1 points (the handle gives the ring at least three
    # frames of max_events_per_tick): the fourth frame of five is refused before anything changes
    q, _ = params.make_params(params.PRESETS["mvstereo_upenn"], rig, max_fusion_frames=5, max_window_points=1)
    dev = lib.Esvo(q, rig)
    _stage(dev, stream)
    for t_ in ticks[:3]:
        dev.set_observation(t_["t"], t_["l"], t_["r"], t_["T"])
        dev.push_disparity_frame(t_["disp"], stream.ev_left[t_["idx"]])
    before = dev.get_map()
    state = (3, sum(r["n"] for r in run("upenn")[:3]), 0)
    assert before.tobytes() == run("upenn")[2]["map"].tobytes()
    t3 = ticks[3]
    dev.set_observation(t3["t"], t3["l"], t3["r"], t3["T"])
    for call in (lambda: dev.tick_sgm(t3["l"], t3["r"]), lambda: dev.push_disparity_frame(t3["disp"], stream.ev_left[t3["idx"]])):
        with pytest.raises(lib.EsvoError, match="window ring") as e:
            call()
        assert e.value.code == ERR_CAPACITY and _untouched(dev, before, state)
    dev.close()
    # W <= 50: the SGM chain matches the columns x >= 48 only
    small = calib.ideal_rig(48, 32, 100.0, 0.1)
    ps, _ = params.make_params(params.PRESETS["mvstereo_upenn"], small)
    dev = lib.Esvo(ps, small)
    blank = np.zeros((32, 48), np.uint8)
    dev.set_observation(10_000_000_000, blank, blank, np.eye(4))
    for call in (lambda: dev.tick_sgm(blank, blank), lambda: dev.push_disparity_frame(np.zeros((32, 48), np.int16), ev[:0])):
        with pytest.raises(lib.EsvoError, match="numDisparities") as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED
    assert len(dev.get_map()) == 0 and dev.stats().last_window_frames == 0
    dev.close()


def test_cpp_semi_global_matching_layer(tmp_path):
    """include/esvo_hip.hpp's MappingAtTimeSemiGlobalMatching and DepthFusion::pushDisparityFrame give the C-ABI's map"""
    rig, stream, p, ticks = SC.case("upenn")
    n_ticks = 3
    want = run("upenn")[n_ticks - 1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "sgm_tick")
    libdir = os.path.dirname(lib._LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "sgm_tick.cpp"), "-o", exe, "-L", libdir, "-lesvo_hip",
                           f"-Wl,-rpath,{libdir}"])
    d = tmp_path
    stream.ev_left.tofile(d / "left.bin")
    for k, tk in enumerate(ticks[:n_ticks]):
        np.asarray([tk["t"]], np.uint64).tofile(d / f"t{k}.bin")
        tk["l"].tofile(d / f"tsl{k}.bin")
        tk["r"].tofile(d / f"tsr{k}.bin")
        tk["T"].reshape(16).tofile(d / f"Tobs{k}.bin")
        tk["disp"].tofile(d / f"disp{k}.bin")
        np.asarray(tk["idx"], np.uint32).tofile(d / f"sel{k}.bin")
    for c, cal in ((0, rig.left), (1, rig.right)):
        cal.P.tofile(d / f"P{c}.bin")
        cal.rect_lut.tofile(d / f"lut{c}.bin")
        cal.map_x.tofile(d / f"mx{c}.bin")
        cal.map_y.tofile(d / f"my{c}.bin")
    (d / "params.bin").write_bytes(C.string_at(C.addressof(p), C.sizeof(p)))
    subprocess.check_call(["timeout", "-k", "10", "300", exe, str(d), str(rig.width), str(rig.height), str(n_ticks)])
    got = np.fromfile(d / "map.bin", dtype=want["map"].dtype)
    counts = np.fromfile(d / "counts.bin", dtype=np.uint64)
    assert counts.tolist() == [r["n"] for r in run("upenn")[:n_ticks]]
    assert len(got) > 1000 and got.tobytes() == want["map"].tobytes()
