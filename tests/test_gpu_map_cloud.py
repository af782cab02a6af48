"""The map's point cloud built and kept on the device (esvo_map_cloud_build / _get / _device) against the host read-out
esvo_map_get_pointcloud_xyz, which downloads the elements and sorts them by creation id: same points, same order, same float
bits, on every route that leaves a DepthMap.  All comparisons are byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_cloud_cases as MC
from esvo_amd import abi, lib, params

pytestmark = pytest.mark.gpu


# ---- (a) the snapshot equals the host cloud -----------------------------------------------------------------------------------
def test_upenn_four_ticks_without_regulariser(request):
    dev, p, *_ = MC.ticked(request, "upenn")
    assert p.regularization == 0
    assert len(MC.same_cloud(dev)) > 300


def test_dsec_four_ticks_with_regulariser_reads_the_second_buffer(request):
    dev, p, *_ = MC.ticked(request, "dsec")
    assert p.regularization == 1 and p.reg_radius == 20 and p.fusion_radius == 1   # 9 records per point, owner elements only
    assert len(MC.same_cloud(dev)) > 300


def test_after_the_sgm_bootstrap_alone(upenn_rig, upenn_stream):
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], upenn_rig)
    dev = lib.Esvo(p, upenn_rig)
    dev.ts_push_events(0, upenn_stream.ev_left)
    dev.ts_push_events(1, upenn_stream.ev_right)
    t = upenn_stream.t0_ns + 80_000_000
    dev.ts_render(0, t, download=False)
    dev.ts_render(1, t, download=False)
    dev.set_observation(t, None, None, upenn_stream.pose(t))
    n_sgm, _ = dev.init_sgm(None, None, min_points=1, want_disp=False)
    assert n_sgm > 100
    assert len(MC.same_cloud(dev)) > 100
    assert dev.map_cloud_device()[2] == t          # the stamp of the tick the snapshot was built from
    dev.close()


def test_after_block_matching_only_ticks(request):
    dev, *_ = MC.ticked(request, "upenn", n_ticks=3, bm_only=True)   # the naive model: 4 records per point, never cleaned
    assert len(MC.same_cloud(dev)) > 300


def test_one_point_frame_is_the_smallest_map(request, upenn_rig):
    src, p, stream, t, ts_left = MC.ticked(request, "upenn")
    pt = src.get_last_frame()[:1].copy()
    assert len(pt) == 1
    pt["pose_idx"] = 0
    dev = lib.Esvo(p, upenn_rig)
    dev.set_observation(t, ts_left, ts_left, stream.pose(t))
    dev.push_frame(pt, stream.pose(t).reshape(1, 16))
    dev.fuse()
    cloud = MC.same_cloud(dev)
    assert 1 <= len(cloud) <= 4                    # fusion_radius 0: the point's 2 x 2 cells
    dev.close()


def test_fresh_handle_and_reset_give_an_empty_cloud(request, upenn_rig):
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], upenn_rig)
    dev = lib.Esvo(p, upenn_rig)
    assert dev.map_cloud().shape == (0, 3) and dev.map_cloud_device() == (0, 0, 0)   # before any build
    assert dev.map_cloud_build() == 0 and len(dev.get_pointcloud()) == 0
    assert dev.map_cloud().shape == (0, 3)
    dev.close()
    dev, p, stream, t, _ = MC.ticked(request, "upenn", fresh=True)
    assert dev.map_cloud_build() > 300
    dev.reset()
    assert dev.map_cloud().shape == (0, 3) and dev.map_cloud_device() == (0, 0, 0)   # the reset emptied the buffer
    assert dev.map_cloud_build() == 0 and len(dev.get_pointcloud()) == 0
    assert dev.map_cloud().shape == (0, 3)
    dev.close()


# ---- (b) the window shrinks between the fusion and the read-out ----------------------------------------------------------------
def test_window_shrunk_after_the_fusion(request):
    """CONST_FRAMES with two frames: after three ticks the window holds two large frames and the map carries creation ids up to
    (their points) x 4.  A one-point frame pushed WITHOUT a fusion makes the window policy pop a large frame, so window points x 4
    falls below the ids the map still holds: the id range must be the one the last fusion numbered.  The host path sorts and
    has no id bound: it is the yardstick."""
    dev, p, stream, t, _ = MC.ticked(request, "upenn", n_ticks=3, fresh=True, fusion_strategy=abi.FUSION_CONST_FRAMES,
                                     max_fusion_frames=2)
    st = dev.stats()
    assert st.last_window_frames == 2
    n_map_before = len(dev.get_pointcloud())
    pt = dev.get_last_frame()[:1].copy()
    pt["pose_idx"] = 0
    dev.push_frame(pt, stream.pose(t).reshape(1, 16))      # pops the older large frame: the window is now (newest frame, 1 point)
    cloud = MC.same_cloud(dev)
    assert len(cloud) == n_map_before > 50                 # no fusion ran: the map is the (cleaned) one of the third tick
    dev.close()


# ---- (c) the buffer is a snapshot ----------------------------------------------------------------------------------------------
def test_snapshot_survives_later_ticks(request):
    dev, p, stream, t, _ = MC.ticked(request, "upenn", fresh=True)
    kept = MC.same_cloud(dev).tobytes()
    stamp = dev.map_cloud_device()[2]
    assert stamp == t
    t_prev = t
    for k in (4, 5):
        t = stream.t0_ns + int((0.06 + 0.01 * k) * 1e9)
        MC.tick_at(dev, stream, p, t, t_prev)
        t_prev = t
    assert dev.stats().ticks == 6                          # (reading the statistics completes the last tick)
    assert dev.map_cloud().tobytes() == kept and dev.map_cloud_device()[2] == stamp
    now = dev.get_pointcloud()
    assert now.tobytes() != kept                           # the map has moved on ...
    assert dev.map_cloud().tobytes() == kept               # ... the host read-out does not touch the snapshot either
    assert dev.map_cloud_build() == len(now)
    assert dev.map_cloud().tobytes() == now.tobytes() and dev.map_cloud_device()[2] == t
    dev.close()


# ---- (d) refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(request, upenn_rig):
    src, p, stream, t, ts_left = MC.ticked(request, "upenn")
    T = stream.pose(t)
    dev = lib.Esvo(p, upenn_rig)
    with pytest.raises(lib.EsvoError) as e:                # before any build
        dev.track_set_reference_from_cloud(np.arange(4, dtype=np.uint32), T)
    assert e.value.code == abi.ERR_STATE
    with pytest.raises(lib.EsvoError) as e:
        dev.track_set_reference_from_cloud(None, T, n=10)
    assert e.value.code == abi.ERR_STATE
    dev.close()

    dev, p, stream, t, ts_left = MC.ticked(request, "upenn", fresh=True)
    n = dev.map_cloud_build()
    cloud = dev.map_cloud()
    dev.track_set_current(ts_left, 5)
    dev.track_set_reference(cloud[:500], T)
    Tlr = np.linalg.inv(T) @ stream.pose(t + 8_000_000)
    Tw = np.linalg.inv(Tlr)
    before = dev.track_residuals(Tw, 0, 500)
    assert len(before) == 500
    bad = np.arange(100, dtype=np.uint32)
    bad[37] = n                                            # an index equal to the count
    with pytest.raises(lib.EsvoError) as e:
        dev.track_set_reference_from_cloud(bad, T)
    assert e.value.code == abi.ERR_INVALID_ARG
    after = dev.track_residuals(Tw, 0, 500)                # still answers from the earlier reference
    assert after.tobytes() == before.tobytes()
    small = np.zeros((n - 1, 3), np.float32)               # cap_points too small
    cnt = lib.C.c_size_t()
    assert dev.lib.esvo_map_cloud_get(dev.h, small.ctypes.data, n - 1, lib.C.byref(cnt)) == abi.ERR_CAPACITY
    assert cnt.value == n
    assert dev.lib.esvo_map_cloud_get(dev.h, None, 0, lib.C.byref(cnt)) == 0 and cnt.value == n   # NULL: the count only
    dev.reset()
    with pytest.raises(lib.EsvoError) as e:                # after a reset
        dev.track_set_reference_from_cloud(np.arange(4, dtype=np.uint32), T)
    assert e.value.code == abi.ERR_STATE
    dev.close()

    rig = upenn_rig
    dev = lib.Esvo(p, rig)
    dev.set_band(0, rig.height // 2, 0, 2)
    with pytest.raises(lib.EsvoError, match="sharded") as e:
        dev.map_cloud_build()
    assert e.value.code == abi.ERR_STATE
    dev.close()


def test_c_entry_of_the_stochastic_order():
    """the library's C entry (which calls the C++ inline) against the Python function, whose literal-swap test needs no GPU"""
    rng = np.random.default_rng(5)
    for n_cloud, n_take in ((1, 1), (5, 5), (5, 12), (2000, 2000), (100_003, 2000), (7, 0)):
        draws = rng.integers(0, 2**31, size=max(n_take, 1), dtype=np.uint32)
        draws[0], draws[-1] = 0, 2**31 - 1
        a, b = lib.stochastic_order_c(n_cloud, n_take, draws), lib.stochastic_order(n_cloud, n_take, draws)
        assert a.dtype == np.uint32 and a.tobytes() == b.tobytes() and len(a) == min(n_take, n_cloud)


def test_cpp_layer(request, tmp_path, upenn_rig):
    """tests/cpp/map_cloud.cpp: DepthFusion::buildPointCloud + RegProblemLM::setProblemFromMap against getPointCloud + the swaps +
    setProblem on the same handle -- the normal equations are equal as bytes, with and without swaps"""
    src, p, stream, t, ts_left = MC.ticked(request, "upenn")
    rig = upenn_rig
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "map_cloud")
    libdir = os.path.dirname(lib._LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "map_cloud.cpp"), "-o", exe, "-L", libdir, "-lesvo_hip",
                           f"-Wl,-rpath,{libdir}"])
    d = tmp_path
    frame = src.get_map()[:3000].copy()        # the elements of a mapped DepthMap as one frame at the observation's pose
    assert len(frame) > 300
    frame["pose_idx"] = 0
    T = stream.pose(t)
    frame.tofile(d / "frame.bin")
    T.reshape(16).tofile(d / "poses.bin")
    np.asarray([t], np.uint64).tofile(d / "t.bin")
    ts_left.tofile(d / "tsl.bin")
    ts_left.tofile(d / "tsr.bin")
    T.reshape(16).tofile(d / "Tobs.bin")
    T.reshape(16).tofile(d / "Tref.bin")
    T_ref_left = np.linalg.inv(T) @ stream.pose(t + 8_000_000)
    np.ascontiguousarray(T_ref_left[:3, :3]).reshape(9).tofile(d / "R.bin")
    np.ascontiguousarray(T_ref_left[:3, 3]).tofile(d / "tr.bin")
    np.random.default_rng(3).integers(0, 2**31, size=2000, dtype=np.uint32).tofile(d / "draws.bin")
    for c, cal in ((0, rig.left), (1, rig.right)):
        cal.P.tofile(d / f"P{c}.bin")
        cal.rect_lut.tofile(d / f"lut{c}.bin")
        cal.map_x.tofile(d / f"mx{c}.bin")
        cal.map_y.tofile(d / f"my{c}.bin")
    (d / "params.bin").write_bytes(C.string_at(C.addressof(p), C.sizeof(p)))
    subprocess.check_call(["timeout", "-k", "10", "120", exe, str(d), str(rig.width), str(rig.height)])
    blob = (d / "out.bin").read_bytes()
    n_cloud, n_ref = np.frombuffer(blob[:16], np.uint64)
    sums = np.frombuffer(blob[16:], np.float64).reshape(4, 43)
    assert n_cloud > 300 and n_ref == min(n_cloud, 2000)
    assert sums[0].tobytes() == sums[1].tobytes() and sums[2].tobytes() == sums[3].tobytes()
    assert sums[0].tobytes() != sums[2].tobytes()          # the swaps chose other points
    assert np.abs(sums[0][:36]).max() > 0 and sums[0][42] > 0
