"""CPU tests of the event-matching restatement (tests/em_restated.py) on hand-built cases, the EM preset values and the ABI
mirrors of the new structs.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import em_restated as R
from esvo_amd import abi, calib, params

NS = R.NS


def _ev(xs, ys, t_ns, pol):
    n = len(xs)
    e = np.zeros(n, abi.EVENT_DTYPE)
    e["x"], e["y"] = xs, ys
    t = np.asarray(t_ns, np.uint64) if np.ndim(t_ns) else np.full(n, t_ns, np.uint64)
    e["sec"], e["nsec"] = t // np.uint64(NS), t % np.uint64(NS)
    e["polarity"] = pol
    return e


def _em(**kw):
    d = dict(time_threshold=5e-4, epipolar_threshold=1.0, ncc_threshold=0.1)
    d.update(kw)
    return d


T0 = 10 * NS


# ---- selection -----------------------------------------------------------------------------------------------------------
def test_selection_never_takes_the_last_event_before_t_up():
    st = np.array([T0 + k * 1000 for k in range(10)], np.uint64)
    lo, n = R.select(st, T0, T0 + 9000, 3000)   # lower_bound(t_up) = 9 -> up = 8: events 0..7
    assert (lo, n) == (0, 8)
    lo, n = R.select(st, T0 + 500, T0 + 8500, 3000)  # lo = 1, lower_bound = 9, up = 8 -> 1..7
    assert (lo, n) == (1, 7)


def test_selection_cap_is_num_event_matching_plus_one():
    st = np.array([T0 + k * 1000 for k in range(100)], np.uint64)
    assert R.select(st, T0, T0 + 99_000, 10) == (0, 11)


def test_selection_empty_range_is_no_tick():
    st = np.array([T0, T0 + 1000], np.uint64)
    assert R.select(st, T0, T0 + 500, 3000)[1] == 0          # lower_bound(t_up) = 1 -> up = lo
    assert R.select(st, T0 + 5000, T0 + 9000, 3000)[1] == 0  # nothing in the window


# ---- slicing -------------------------------------------------------------------------------------------------------------
def test_slices_are_inclusive_and_stop_after_num_slice():
    st = np.array([T0 + k * 250_000 for k in range(20)], np.uint64)  # 4 events per ms
    sl = R.slice_events(st, T0, T0 + 3_100_000, 1e-3)               # floor(3.1) = 3 slices
    assert len(sl) == 3
    # slice 0: ts0 .. lower_bound(ts0 + 1 ms) = event 4, inclusive -> 5 events; the next starts behind it
    assert sl[0][:2] == (0, 5) and sl[1][0] == 5 and sl[2][0] == sl[1][0] + sl[1][1]
    assert sl[0][2] == int(st[0 + 5 // 2])


def test_slicing_stops_at_the_end_of_the_selection():
    st = np.array([T0 + k * 250_000 for k in range(6)], np.uint64)
    sl = R.slice_events(st, T0, T0 + 10_000_000, 1e-3)  # 10 slices allowed, the events end first
    assert [s[:2] for s in sl] == [(0, 5), (5, 1)]      # lower_bound hits end() -> step back one


# ---- matching on an ideal rig --------------------------------------------------------------------------------------------
W, H, F, B = 80, 48, 50.0, 0.1


@pytest.fixture(scope="module")
def rig():
    return calib.ideal_rig(W, H, F, B)


def _surfaces(shift, seed=3):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (H, W)).astype(np.uint8)
    Rt = np.zeros_like(L)
    Rt[:, : W - shift] = L[:, shift:]  # right image: the left one moved by `shift` px (fronto-parallel plane)
    return L, Rt


def _run(rig, left, right, L, Rt, em=None, wx=15, wy=7, threads=1, stats=False):
    I = np.eye(4)
    return R.match(rig, wx, wy, threads, em or _em(), I, L, Rt, left, [0], [len(left)], [I], right, want_stats=stats)


def test_one_point_finds_the_true_inverse_depth(rig):
    L, Rt = _surfaces(10)
    left = _ev([40], [20], T0, 1)
    right = _ev([35, 30, 25], [20, 20, 20], T0 + 10_000, 1)  # true match: disparity 10 -> depth b f / 10 = 0.5
    m, st = _run(rig, left, right, L, Rt, stats=True)
    assert len(m) == 1 and st["epipolar"] == 3
    assert abs(m["disp"][0] - 10.0) < 1e-9
    assert abs(m["inv_depth"][0] - 2.0) < 1e-9
    assert m["cost"][0] < 1e-6 and m["event_idx"][0] == 0 and m["pose_idx"][0] == 0


def test_time_polarity_and_epipolar_filters(rig):
    L, Rt = _surfaces(10)
    left = _ev([40], [20], T0, 1)
    right = np.concatenate([
        _ev([30], [20], T0 - 400_000, 1),  # outside +-0.25 ms
        _ev([30], [20], T0, 0),            # same time, opposite polarity
        _ev([30], [23], T0, 1),            # 3 rows off the epipolar line
        _ev([40], [20], T0, 1),            # x_r == x_l: rejected (strict <)
    ])
    m, st = _run(rig, left, right, L, Rt, stats=True)
    assert st["time_polarity"] == 2 and st["epipolar"] == 0 and len(m) == 0


def test_cost_tie_keeps_the_lower_index(rig):
    L = np.zeros((H, W), np.uint8)
    L[:, ::2] = 200          # period-2 texture: candidates 2 px apart see the same patches
    left = _ev([40], [20], T0, 1)
    right = _ev([30, 28], [20, 20], [T0 + 100, T0 + 200], 1)
    m = _run(rig, left, right, L, L.copy(), em=_em(ncc_threshold=0.5))
    assert len(m) == 1 and m["disp"][0] == 10.0  # equal costs: the first candidate in queue order wins


def test_all_warps_failing_gives_no_match_unless_threshold_is_one(rig):
    L, Rt = _surfaces(10)
    left = _ev([3], [20], T0, 1)             # patches leave the image on the left
    right = _ev([1], [20], T0, 1)
    m, st = _run(rig, left, right, L, Rt, stats=True)
    assert st["epipolar"] == 1 and st["patch_ok"] == 0 and len(m) == 0
    m = _run(rig, left, right, L, Rt, em=_em(ncc_threshold=1.0))  # reference's corner: candidate 0, invDepth = 1 / 0
    assert len(m) == 1 and np.isinf(m["inv_depth"][0]) and m["cost"][0] == 1.0 and m["disp"][0] == 2.0


def test_events_off_the_sensor_are_skipped(rig):
    L, Rt = _surfaces(10)
    left = np.concatenate([_ev([W + 5], [20], T0, 1), _ev([40], [20], T0, 1)])
    right = np.concatenate([_ev([30], [H], T0, 1), _ev([30], [20], T0 + 1000, 1)])
    m, st = _run(rig, left, right, L, Rt, stats=True)
    assert st["time_polarity"] == 1 and list(m["event_idx"]) == [1]
    m2 = _run(rig, left, right[1:], L, Rt)
    assert m.tobytes() == m2.tobytes()


def test_output_is_stride_n_order(rig):
    L, Rt = _surfaces(10)
    xs = np.arange(25, 60, 3)
    left = _ev(xs, np.full(len(xs), 20), T0, 1)
    right = _ev(xs - 10, np.full(len(xs), 20), T0 + 1000, 1)
    m1 = _run(rig, left, right, L, Rt, threads=1)
    m4 = _run(rig, left, right, L, Rt, threads=4)
    assert len(m1) == len(xs)
    assert list(m4["event_idx"]) == list(R.stride_order(len(xs), 4))
    assert np.array_equal(np.sort(m4, order="event_idx"), m1)


def test_lower_bound_is_std_lower_bound_on_unsorted_keys():
    keys = np.array([5.0, 1.0, 7.0, 3.0, 9.0])
    import bisect
    for t in (0.0, 3.0, 4.0, 8.0, 10.0):
        # the halving of std::lower_bound, written out
        first, ln = 0, len(keys)
        while ln > 0:
            half = ln >> 1
            if keys[first + half] < t:
                first, ln = first + half + 1, ln - half - 1
            else:
                ln = half
        assert R.lower_bound(keys, t)[0] == first
    assert R.lower_bound(np.sort(keys), 4.0)[0] == bisect.bisect_left(sorted(keys), 4.0)


# ---- presets and ABI mirrors -----------------------------------------------------------------------------------------------
from oracle import ref as _ref  # noqa: E402

REF_CFG = os.path.join(_ref.REFERENCE, "esvo_core", "cfg", "mvstereo")


@pytest.mark.skipif(not os.path.isdir(REF_CFG), reason="reference tree absent")
@pytest.mark.parametrize("name", ["upenn", "rpg"])
def test_em_presets_equal_the_shipped_yaml(name):
    y = params.load_yaml_cfg(os.path.join(REF_CFG, f"mvstereo_{name}.yaml"))
    p = params.PRESETS[f"mvstereo_{name}"]
    for k in ("EM_Slice_Thickness", "EM_Time_THRESHOLD", "EM_EPIPOLAR_THRESHOLD", "EM_TS_NCC_THRESHOLD", "EM_NUM_EVENT_MATCHING",
              "EM_PATCH_INTENSITY_THRESHOLD", "EM_PATCH_VALID_RATIO", "MVStereoMode"):
        assert p[k] == y[k], k


def test_make_em_params():
    e = params.make_em_params(params.PRESETS["mvstereo_upenn"])
    assert (e.slice_thickness, e.time_threshold, e.epipolar_threshold, e.ncc_threshold, e.num_event_matching) == \
        (0.001, 0.0005, 1.0, 0.1, 3000)
    d = params.make_em_params({})  # esvo_MVStereo.cpp:81-89 code defaults
    assert (d.time_threshold, d.epipolar_threshold, d.patch_intensity_threshold) == (5e-5, 0.5, 125)


def test_em_struct_sizes_equal_the_ctypes_bindings():
    from esvo_amd import lib
    assert lib.em_sizes() == [C.sizeof(abi.EmParamsStruct), C.sizeof(abi.EmSelectionStruct), C.sizeof(abi.EmStatsStruct), 0]
    assert lib.abi_sizes()[7] == 8  # the ABI number is unchanged
