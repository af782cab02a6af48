"""The tracker's reprojection map drawn on the device (esvo_track_reprojection_map, kernels_track_viz.hip) against the restated
loop of tests/reproj_restated.py: the image is 8-bit and every f64 expression is formed in the restatement's order, so image and
counter must be equal byte for byte."""
import threading

import numpy as np
import pytest

import map_cloud_cases as MC
import reproj_cases as RC
import reproj_restated as RR
from esvo_amd import abi, calib, dist, lib, params

pytestmark = pytest.mark.gpu

I4 = np.eye(4)


def _small(W, H):
    rig = calib.ideal_rig(W, H, RC.FOCAL, 0.1)
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], rig)
    return lib.Esvo(p, rig), rig


def _P(rig):
    return np.asarray(rig.left.P, np.float64).reshape(3, 4)


def _code(fn, *a, **k):
    with pytest.raises(lib.EsvoError) as e:
        fn(*a, **k)
    return e.value.code


def _same(got, want, label):
    (g_img, g_n), (w_img, w_n) = got, want
    assert g_n == w_n, (label, g_n, w_n)
    assert g_img.shape == w_img.shape and g_img.dtype == np.uint8
    if g_img.tobytes() != w_img.tobytes():
        bad = np.argwhere((g_img != w_img).any(axis=2))
        raise AssertionError(f"{label}: {len(bad)} pixels differ, first (row, col) {bad[:5].tolist()}")


# ---- 1. crafted parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(96, 64), (95, 63)])   # 95 x 63: a pixel count that is no multiple of the paint pass' 4 pixels
def test_crafted_points_equal_the_restatement(W, H):
    rig = calib.ideal_rig(W, H, RC.FOCAL, 0.1)
    P = _P(rig)
    xyz = RC.crafted(W, H, P)
    pts_ref = RR.reference_points(xyz, I4)                     # T_world_ref = I: the f32 input widened (a row with an infinity: NaNs)
    finite = np.isfinite(xyz).all(axis=1)
    assert np.array_equal(pts_ref[finite], xyz[finite].astype(np.float64)) and 350 <= len(xyz) <= 450 and 0 < (~finite).sum() < 10
    ts = np.random.default_rng(W).integers(0, 256, (H, W)).astype(np.uint8)
    RC.check_power((255 - ts), pts_ref, P)                     # on the CPU, before anything runs on the device
    dev, _ = _small(W, H)
    dev.track_set_reference(xyz, I4)
    for ksize in (0, 5):
        dev.track_set_current(ts, ksize)
        neg = dev.track_images()[0]
        if ksize == 0:
            assert np.array_equal(neg, 255 - ts)
        for name, (R, t) in RC.MOTIONS.items():
            for n in RC.n_values(len(xyz)):
                want = RR.reprojection_map(neg, pts_ref, R, t, P, n, RC.INV_MIN, RC.INV_MAX, RC.JET)
                got = dev.track_reprojection_map(R, t, n, RC.INV_MIN, RC.INV_MAX)
                _same(got, want, f"kernelSize {ksize} {name} n {n}")
    dev.close()


# ---- 2. pipeline parity ----------------------------------------------------------------------------------------------------------
def _pipeline(request):
    """four mapper ticks on upenn, the device-resident cloud, a permuted reference out of it, the registration: (dev, the reference
    points restated, neg, R, t, P, ranges)"""
    dev, p, stream, t_ns, _ = MC.ticked(request, "upenn")
    n_cloud = dev.map_cloud_build()
    cloud = dev.map_cloud()
    order = np.random.default_rng(11).permutation(n_cloud)[:2000].astype(np.uint32)
    T_world_ref = stream.pose(t_ns)
    dev.track_set_reference_from_cloud(order, T_world_ref)
    dev.track_set_current(None, 5)
    R, t, info, _ = dev.track_solve(len(order), np.eye(3), np.zeros(3), batch_size=300)
    assert info.iterations >= 1
    pts_ref = RR.reference_points(cloud[order], T_world_ref)
    cfg = params.PRESETS["mapping_upenn"]
    rig = request.getfixturevalue("upenn_rig")
    return dev, pts_ref, dev.track_images()[0], R, t, _P(rig), float(cfg["invDepth_min_range"]), float(cfg["invDepth_max_range"])


def test_pipeline_equals_the_restatement(request):
    dev, pts_ref, neg, R, t, P, lo, hi = _pipeline(request)
    want = RR.reprojection_map(neg, pts_ref, R, t, P, 2000, lo, hi, RC.JET)
    got = dev.track_reprojection_map(R, t, 2000, lo, hi)
    _same(got, want, "pipeline")
    assert got[1] > 500                                         # most of the map reprojects into the image
    assert int((got[0] != np.repeat(neg[:, :, None], 3, axis=2)).any(axis=2).sum()) > 500


# ---- 3. the image stays on the device --------------------------------------------------------------------------------------------
def test_device_resident_image(request):
    dev, pts_ref, neg, R, t, P, lo, hi = _pipeline(request)
    img, n_in = dev.track_reprojection_map(R, t, 2000, lo, hi)
    none, n_dev = dev.track_reprojection_map(R, t, 2000, lo, hi, download=False)
    assert none is None and n_dev == n_in
    ptr = dev.track_reprojection_map_device()
    assert ptr != 0
    on_device = dist.device_tensor(ptr, img.size, "|u1").cpu().numpy()
    assert on_device.tobytes() == img.tobytes()


# ---- 4. repeatability: the owner words are clean after every call -----------------------------------------------------------------
def test_repeated_calls_and_shrinking_n():
    W, H = 96, 64
    dev, rig = _small(W, H)
    P = _P(rig)
    xyz = RC.crafted(W, H, P)
    pts_ref = RR.reference_points(xyz, I4)
    dev.track_set_reference(xyz, I4)
    dev.track_set_current(np.random.default_rng(5).integers(0, 256, (H, W)).astype(np.uint8), 5)
    neg = dev.track_images()[0]
    R, t = RC.MOTIONS["moved"]
    want = {n: RR.reprojection_map(neg, pts_ref, R, t, P, n, RC.INV_MIN, RC.INV_MAX, RC.JET) for n in (len(xyz), 5)}
    assert not np.array_equal(want[5][0], want[len(xyz)][0])
    a = dev.track_reprojection_map(R, t, len(xyz), RC.INV_MIN, RC.INV_MAX)
    b = dev.track_reprojection_map(R, t, len(xyz), RC.INV_MIN, RC.INV_MAX)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    for n in (len(xyz), 5, len(xyz), 5, 0, len(xyz)):
        got = dev.track_reprojection_map(R, t, n, RC.INV_MIN, RC.INV_MAX)
        _same(got, want[n] if n else (np.repeat(neg[:, :, None], 3, axis=2), 0), f"n {n}")
    dev.close()


# ---- 5. the tracker group next to the mapper group --------------------------------------------------------------------------------
def test_beside_the_mappers_debug_images(request):
    dev, pts_ref, neg, R, t, P, lo, hi = _pipeline(request)
    debug = [x.tobytes() for x in dev.get_debug_images()]
    assert len(set(debug)) > 1 and any(np.frombuffer(x, np.uint8).any() for x in debug)
    img, n_in = dev.track_reprojection_map(R, t, 2000, lo, hi)
    errs = []

    def mapper():
        try:
            for _ in range(20):
                assert [x.tobytes() for x in dev.get_debug_images()] == debug
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    def tracker():
        try:
            for _ in range(20):
                g, n = dev.track_reprojection_map(R, t, 2000, lo, hi)
                assert n == n_in and g.tobytes() == img.tobytes()
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=mapper), threading.Thread(target=tracker)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=60)
    assert not any(x.is_alive() for x in th), "a thread did not finish"
    if errs:
        raise errs[0]


# ---- 6. refusals and the empty reference ------------------------------------------------------------------------------------------
def test_errors_and_empty_reference():
    W, H = 96, 64
    dev, rig = _small(W, H)
    R, t = np.eye(3), np.zeros(3)
    assert _code(dev.track_reprojection_map, R, t, 10, 0.16, 1.0) == abi.ERR_STATE          # before track_set_current
    assert _code(dev.track_reprojection_map_device) == abi.ERR_STATE                        # before any map
    ts = np.random.default_rng(9).integers(0, 256, (H, W)).astype(np.uint8)
    dev.track_set_current(ts, 0)
    assert _code(dev.track_reprojection_map_device) == abi.ERR_STATE
    for lo, hi in ((0.5, 0.5), (float("nan"), 1.0), (0.16, float("nan")), (float("inf"), 1.0), (0.16, float("-inf"))):
        assert _code(dev.track_reprojection_map, R, t, 10, lo, hi) == abi.ERR_INVALID_ARG
    assert _code(dev.track_reprojection_map_device) == abi.ERR_STATE                        # a refused call leaves no image
    assert dev.lib.esvo_track_reprojection_map(dev.h, None, t.ctypes.data, 10, 0.16, 1.0, None, None) == abi.ERR_INVALID_ARG
    assert dev.lib.esvo_track_reprojection_map(dev.h, R.ctypes.data, None, 10, 0.16, 1.0, None, None) == abi.ERR_INVALID_ARG
    grey = np.repeat((255 - ts)[:, :, None], 3, axis=2)
    img, n_in = dev.track_reprojection_map(R, t, 2000, 0.16, 1.0)                           # no reference yet: the grey image
    assert np.array_equal(img, grey) and n_in == 0
    assert dev.track_reprojection_map_device() != 0
    dev.track_set_reference(np.zeros((0, 3), np.float32), I4)                               # an empty reference
    img, n_in = dev.track_reprojection_map(R, t, 2000, 0.16, 1.0)
    assert np.array_equal(img, grey) and n_in == 0
    dev.track_set_reference(np.array([[0.0, 0.0, 2.0]], np.float32), I4)
    img, n_in = dev.track_reprojection_map(R, t, 0, 0.16, 1.0)                              # n_points == 0
    assert np.array_equal(img, grey) and n_in == 0
    img, n_in = dev.track_reprojection_map(R, t, 2000, 1.0, 0.16)                           # a reversed range is a range
    want = RR.reprojection_map(255 - ts, np.array([[0.0, 0.0, 2.0]]), R, t, _P(rig), 1, 1.0, 0.16, RC.JET)
    _same((img, n_in), want, "reversed range")
    assert n_in == 1
    dev.close()


# ---- 7. the closed loop's opt-in ---------------------------------------------------------------------------------------------------
def test_closed_loop_collects_n_inside_and_changes_nothing_else():
    from esvo_amd import closed_loop
    plain = closed_loop.run(n_ticks=3)
    drawn = closed_loop.run(n_ticks=3, reproj_map=True)
    assert "reproj_inside" not in plain
    print("n_inside per tick:", drawn["reproj_inside"])
    assert len(drawn["reproj_inside"]) == 3 and all(0 < n <= 2000 for n in drawn["reproj_inside"])   # (the parity is tested above)
    assert np.array_equal(np.array(plain["poses"]), np.array(drawn["poses"])) and np.array_equal(plain["map"], drawn["map"])
