"""The mapper's global point cloud on the device (esvo_map_cloud_near, esvo_map_voxel_filter, esvo_map_gpc_*) against the host
yardsticks: esvo_map_get_pointcloud_near_xyz, esvo_voxel_filter_xyz == oracle.voxel_filter, and the branch restated in
tests/gpc_restated.py.  Every comparison is byte for byte; there is no tolerance in this feature."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpc_restated as G
import map_cloud_cases as MC
from esvo_amd import abi, lib, params

pytestmark = pytest.mark.gpu

LEAF = 0.3


@pytest.fixture(scope="module")
def dev(upenn_rig):
    """a handle whose map is never ticked: the voxel filter borrows its device and scratch only"""
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], upenn_rig)
    d = lib.Esvo(p, upenn_rig)
    yield d
    d.close()


def _same(dev, pts, leaf, reversed_differs=None):
    from oracle import oracle as O
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    want = lib.voxel_filter(pts, leaf)
    assert want.tobytes() == O.voxel_filter(pts, leaf).tobytes()
    got = dev.map_voxel_filter(pts, leaf)
    print(f"voxel filter: {len(pts)} rows, leaf {leaf}: {len(want)} voxels (device {len(got)})")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()
    if reversed_differs is not None:   # the case really exercises the order of the sum
        assert (G.voxel_filter_reversed(pts, leaf).tobytes() != want.tobytes()) == reversed_differs
    return got


def _shuffled(pts, seed):
    return np.ascontiguousarray(np.asarray(pts, np.float32)[np.random.default_rng(seed).permutation(len(pts))])


# ---- 1. the voxel filter -------------------------------------------------------------------------------------------------------
def test_voxel_filter_empty_single_and_non_finite(dev):
    assert _same(dev, np.zeros((0, 3)), LEAF).shape == (0, 3)
    assert _same(dev, [[0.7, -1.3, 2.2]], LEAF).tobytes() == np.array([[0.7, -1.3, 2.2]], np.float32).tobytes()
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    assert _same(dev, bad, LEAF).shape == (0, 3)                       # only non-finite rows
    rng = np.random.default_rng(3)
    pts = rng.normal(0, 1.0, (500, 3)).astype(np.float32)
    pts[::7, 0] = np.nan
    pts[3::11, 1] = np.inf
    pts[5::13, 2] = -np.inf
    pts[0] = np.nan                                                    # the first and the last row too
    pts[-1] = np.inf
    assert 0 < len(_same(dev, pts, LEAF)) < 400


def test_voxel_filter_one_long_chain(dev):
    rng = np.random.default_rng(4)
    pts = (rng.uniform(0.0, 0.29, (300, 3)) * np.where(rng.random((300, 3)) < 0.2, 1e-6, 1.0)).astype(np.float32)
    assert len(_same(dev, pts, LEAF, reversed_differs=True)) == 1     # 300 points in one voxel: one sequential chain


def test_voxel_filter_runs_across_wave_and_block_boundaries(dev):
    """sorted positions: 60 single voxels, a run of 10 (60..69 crosses lane 64), singles up to 250, a run of 20 (250..269
    crosses thread 256), singles up to 2040, a run of 20 across the scan tile at 2048; the input order is shuffled"""
    rng = np.random.default_rng(6)
    rows, key = [], 0
    for singles, run in ((60, 10), (180, 20), (1770, 20), (5, 0)):
        for _ in range(singles):
            rows.append([(key + 0.5) * LEAF, 0.1, 0.1])
            key += 1
        for _ in range(run):
            rows.append([key * LEAF + rng.uniform(0.01, 0.29), rng.uniform(0, 0.29) * (1e-5 if rng.random() < 0.3 else 1.0), 0.1])
        key += 1 if run else 0
    pts = _shuffled(rows, 7)
    assert len(_same(dev, pts, LEAF, reversed_differs=True)) == 60 + 180 + 1770 + 5 + 3


def test_voxel_filter_order_revealing_values_and_their_permutations(dev):
    """2^24 + 1 == 2^24 in float, 2^24 + 2 is not: the centroid tells in which order the four rows were summed, so an unstable
    sort or a tree sum changes the bytes; a second voxel in front keeps the run away from position 0"""
    a = [[16777216.0, 1e8 + 5, 3e8], [1.0, 1e8 + 7, 3e8], [1.0, 1e8 + 9, 3e8], [1.0, 1e8 + 11, 3e8]]
    seen = set()
    for perm in ((0, 1, 2, 3), (3, 2, 1, 0), (1, 0, 2, 3), (1, 2, 0, 3), (2, 3, 1, 0)):
        pts = np.array([[-5e8, -5e8, -5e8]] + [a[i] for i in perm], np.float32)
        got = _same(dev, pts, 1e9)
        assert len(got) == 2
        seen.add(got[1].tobytes())
    assert len(seen) >= 2
    # the same rows interleaved with rows of other voxels and with rows that are dropped
    pts = np.array([a[0], [np.nan, 0, 0], [-5e8, -5e8, -5e8], a[1], [2e9, 2e9, 2e9], a[2], [-5e8, -4e8, -5e8], a[3]], np.float32)
    assert len(_same(dev, pts, 1e9, reversed_differs=True)) == 3


def test_voxel_filter_on_cell_boundaries(dev):
    """coordinates exactly on k leaf (computed in float), at the float just below, at -0.0 and negative"""
    leaf32 = np.float32(LEAF)
    xs = []
    for k in range(-4, 5):
        e = np.float32(k) * leaf32
        xs += [e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))]
    xs += [np.float32(-0.0), np.float32(0.0), np.float32(-1e-30), np.float32(1e-30)]
    xs = np.array(xs, np.float32)
    pts = np.stack([xs, xs[::-1], np.roll(xs, 5)], 1)
    _same(dev, pts, LEAF)
    _same(dev, _shuffled(np.concatenate([pts, -pts, pts[:, ::-1]]), 8), LEAF)
    _same(dev, np.array([[-0.0, -0.0, -0.0], [0.0, 0.0, 0.0]], np.float32), LEAF)
    _same(dev, -np.abs(np.random.default_rng(9).normal(0, 2, (400, 3))).astype(np.float32), LEAF)   # all negative


def test_voxel_filter_every_point_in_its_own_voxel(dev):
    k = np.arange(1000, dtype=np.float32)
    pts = _shuffled(np.stack([(k + 0.5) * LEAF, ((k * 7) % 13 + 0.5) * LEAF, ((k * 3) % 5 + 0.5) * LEAF], 1), 10)
    assert len(_same(dev, pts, LEAF)) == 1000


def test_voxel_filter_seeded_clouds(dev):
    """four clouds drawn in this order from one generator; n > 65 536 so that a 16-bit index would show; 20 and 30 key bits (3 and 4 radix
    passes), one scan tile + 1 row, 8 cells"""
    rng = np.random.default_rng(1)
    a = rng.normal(0, 3, (70000, 3)).astype(np.float32)
    a2 = rng.normal(0, 3, (70000, 3)).astype(np.float32)
    b = rng.normal(0, 0.5, (2049, 3)).astype(np.float32)
    c = rng.normal(0, 0.05, (257, 3)).astype(np.float32)
    assert len(_same(dev, a, 0.3, reversed_differs=True)) == 40123
    assert len(_same(dev, a2, 0.03)) == 69949      # (order sensitivity not asserted: nearly every point has its own voxel)
    assert len(_same(dev, b, 0.3, reversed_differs=True)) == 444
    assert len(_same(dev, c, 0.3, reversed_differs=True)) == 8


def test_voxel_filter_errors(dev):
    pts = np.array([[0, 0, 0], [1000, 1000, 1000], [1, 2, 3]], np.float32)    # 3334^3 cells > 2^31 - 1
    out = np.full((8, 3), -77.0, np.float32)
    with pytest.raises(lib.EsvoError) as e:
        dev.map_voxel_filter(pts, LEAF, out=out)
    assert e.value.code == abi.ERR_CAPACITY and (out == -77.0).all()
    with pytest.raises(lib.EsvoError):
        lib.voxel_filter(pts, LEAF)                                           # the host helper refuses it as well
    pts = np.array([[0.1, 0.1, 0.1], [1, 1, 1], [2, 2, 2], [0.2, 0.1, 0.1]], np.float32)
    assert len(dev.map_voxel_filter(pts, LEAF, cap_points=3)) == 3
    with pytest.raises(lib.EsvoError) as e:
        dev.map_voxel_filter(pts, LEAF, cap_points=2)                         # one short
    assert e.value.code == abi.ERR_CAPACITY
    for leaf in (0.0, -0.3, float("nan")):
        with pytest.raises(lib.EsvoError) as e:
            dev.map_voxel_filter(pts, leaf)
        assert e.value.code == abi.ERR_INVALID_ARG
    _same(dev, pts, LEAF)                                                     # the handle still works


# ---- 2. the near cloud ---------------------------------------------------------------------------------------------------------
def _median_range(dev):
    m = dev.get_map()["p_cam"]
    return float(np.median(np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])))


@pytest.mark.parametrize("name", ["upenn", "dsec"])
def test_near_cloud_equals_the_host_read_out(request, name):
    dev, p, *_ = MC.ticked(request, name)
    assert p.regularization == (1 if name == "dsec" else 0)     # dsec: the map is read from the second buffer
    r = _median_range(dev)
    want, got, whole = dev.get_pointcloud_near(r), dev.map_cloud_near(r), dev.get_pointcloud()
    print(f"{name}: range {r}: {len(want)} of {len(whole)} points near")
    assert 0 < len(want) < len(whole)                            # both sides of the predicate are non-empty
    assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert dev.map_cloud_near(0.0).shape == (0, 3)
    assert dev.map_cloud_near(float("inf")).tobytes() == whole.tobytes() and len(dev.map_cloud_near(float("inf"))) == len(whole)
    MC.same_cloud(dev)                                           # the snapshot route is undisturbed


def test_near_cloud_of_a_fresh_handle_is_empty(upenn_rig):
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], upenn_rig)
    d = lib.Esvo(p, upenn_rig)
    assert d.map_cloud_near(5.0).shape == (0, 3)
    assert d.gpc_cloud().shape == (0, 3) and d.gpc_device() == (0, 0) and d.gpc_stats().total_points == 0   # before configure
    d.close()


# ---- 3. the accumulation -------------------------------------------------------------------------------------------------------
def _stats(st):
    return (st.updates, st.refreshes, st.total_points, st.last_near, st.last_voxels, st.last_added, st.last_refreshed, st.t_last_pub)


def _six_ticks(request, rig_name, stream_name, p, gpc=None):
    """six mapper ticks 10 ms apart on a fresh handle; gpc: (restated model, configure arguments) -> gpc_update after every tick"""
    rig, stream = request.getfixturevalue(rig_name), request.getfixturevalue(stream_name)
    d = lib.Esvo(p, rig)
    if gpc:
        d.gpc_configure(**gpc[1])
    flags, cut = [], 0
    t_prev = stream.t0_ns
    for k in range(6):
        t = stream.t0_ns + int((0.06 + 0.01 * k) * 1e9)
        MC.tick_at(d, stream, p, t, t_prev)
        t_prev = t
        if gpc:
            want = gpc[0].update(t, d.get_pointcloud_near)
            got = d.gpc_update(t)
            st = d.gpc_stats()
            print(f"tick {k}: refreshed {got}, near {st.last_near}, voxels {st.last_voxels}, added {st.last_added}, total {st.total_points}, "
                  f"{st.ms_last:.3f} ms")
            assert got == want
            assert d.gpc_cloud().tobytes() == gpc[0].cloud.tobytes() and len(d.gpc_cloud()) == len(gpc[0].cloud)
            assert _stats(st) == gpc[0].counts()
            flags.append(got)
            cut += int(got and st.last_voxels > gpc[1]["num_added_per_refresh"])
    out = (d.get_map().tobytes(), d.get_last_frame().tobytes(), flags, cut)
    d.close()
    return out


@pytest.fixture(scope="module")
def plain_six_ticks(request):
    """map and last frame after the six ticks on a handle that never called gpc_*"""
    _, p, *_ = MC.ticked(request, "upenn")
    return _six_ticks(request, "upenn_rig", "upenn_stream", p)


@pytest.mark.parametrize("leaf,added", [(0.3, 50), (0.03, 10**6)])
def test_accumulation_equals_the_restated_branch(request, plain_six_ticks, leaf, added):
    src, p, *_ = MC.ticked(request, "upenn")
    cfg = dict(visualize_range=_median_range(src), interval_s=0.015, num_added_per_refresh=added, leaf=leaf)
    model = G.Gpc(cfg["visualize_range"], cfg["interval_s"], added, leaf=leaf)
    m, f, flags, cut = _six_ticks(request, "upenn_rig", "upenn_stream", p, gpc=(model, cfg))
    assert True in flags and False in flags                      # some updates are gated and some are not
    assert len(model.cloud) > 0
    if added == 50:
        assert cut >= 1                                          # at least one refresh is cut by the tail rule
    else:
        assert cut == 0 and model.last_added == model.last_voxels - 1   # no cut, only the - 1
    assert (m, f) == plain_six_ticks[:2]                         # no tick output changed


# ---- 4. state rules ------------------------------------------------------------------------------------------------------------
def _code(call, *a, **k):
    with pytest.raises(lib.EsvoError) as e:
        call(*a, **k)
    return e.value.code


def test_state_rules(request, upenn_rig):
    d, p, stream, t, _ = MC.ticked(request, "upenn", fresh=True)
    assert _code(d.gpc_update, t) == abi.ERR_STATE                               # before configure
    cfg = dict(visualize_range=float("inf"), interval_s=0.0, num_added_per_refresh=10**6, leaf=LEAF)
    d.gpc_configure(**cfg)
    assert d.gpc_update(t)
    k1 = d.gpc_stats().last_added
    assert k1 > 1 and d.gpc_stats().total_points == k1
    ptr, n = d.gpc_device()
    assert ptr != 0 and n == k1
    d.gpc_configure(capacity_points=2 * k1 - 1, **cfg)                          # one point short of the second refresh
    assert d.gpc_stats().t_last_pub == 0.0 and len(d.gpc_cloud()) == 0          # configure restarts from 0.0
    assert d.gpc_update(t)
    before = (d.gpc_cloud().tobytes(), _stats(d.gpc_stats()))
    assert _code(d.gpc_update, t + 1000) == abi.ERR_CAPACITY
    assert (d.gpc_cloud().tobytes(), _stats(d.gpc_stats())) == before           # cloud, t_last_pub and total_points unchanged
    t_pub = d.gpc_stats().t_last_pub
    assert t_pub > 0
    d.reset()
    assert len(d.gpc_cloud()) == 0 and d.gpc_stats().total_points == 0 and d.gpc_stats().t_last_pub == t_pub
    assert d.gpc_update(t) is False                                             # the same stamp: not due
    assert _code(d.gpc_configure, num_added_per_refresh=0) == abi.ERR_INVALID_ARG
    assert _code(d.gpc_configure, leaf=0.0) == abi.ERR_INVALID_ARG
    d.close()
    b = lib.Esvo(p, upenn_rig)
    b.set_band(0, b.H // 2)
    assert _code(b.gpc_configure) == abi.ERR_STATE
    assert _code(b.gpc_update, t) == abi.ERR_STATE
    assert _code(b.map_cloud_near, 1.0) == abi.ERR_STATE
    b.close()


# ---- 5. the C++ layer ----------------------------------------------------------------------------------------------------------
def test_cpp_layer(request, tmp_path, upenn_rig):
    """tests/cpp/gpc.cpp: esvo_hip::GlobalPointCloud gives the C-ABI's cloud -- here, the restated branch's -- on a map fused from
    one frame"""
    src, p, stream, t, ts_left = MC.ticked(request, "upenn")
    rig = upenn_rig
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "gpc")
    libdir = os.path.dirname(lib._LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "gpc.cpp"), "-o", exe, "-L", libdir, "-lesvo_hip",
                           f"-Wl,-rpath,{libdir}"])
    d = tmp_path
    frame = src.get_map()[:3000].copy()        # the elements of a mapped DepthMap as one frame at the observation's pose
    assert len(frame) > 300
    frame["pose_idx"] = 0
    T = stream.pose(t)
    r = _median_range(src)
    frame.tofile(d / "frame.bin")
    T.reshape(16).tofile(d / "poses.bin")
    np.asarray([t], np.uint64).tofile(d / "t.bin")
    ts_left.tofile(d / "tsl.bin")
    ts_left.tofile(d / "tsr.bin")
    T.reshape(16).tofile(d / "Tobs.bin")
    np.asarray([r], np.float64).tofile(d / "range.bin")
    for c, cal in ((0, rig.left), (1, rig.right)):
        cal.P.tofile(d / f"P{c}.bin")
        cal.rect_lut.tofile(d / f"lut{c}.bin")
        cal.map_x.tofile(d / f"mx{c}.bin")
        cal.map_y.tofile(d / f"my{c}.bin")
    (d / "params.bin").write_bytes(C.string_at(C.addressof(p), C.sizeof(p)))
    subprocess.check_call(["timeout", "-k", "10", "120", exe, str(d), str(rig.width), str(rig.height)])
    head = np.fromfile(d / "out.bin", np.uint64, 4)
    n_near, n_global, refreshed_first, refreshed_second = (int(v) for v in head)
    body = np.fromfile(d / "out.bin", np.float32, offset=32)
    near, glob = body[:3 * n_near].reshape(-1, 3), body[3 * n_near:].reshape(-1, 3)
    assert len(glob) == n_global and (refreshed_first, refreshed_second) == (1, 0)
    # the same on a Python handle
    ref = lib.Esvo(p, rig)
    ref.set_observation(t, ts_left, ts_left, stream.pose(t))
    ref.push_frame(frame, T.reshape(1, 16))
    ref.fuse()
    want_near = ref.get_pointcloud_near(r)
    model = G.Gpc(r, 1.0, 40, leaf=LEAF)
    assert model.update(t, lambda _r: want_near)
    ref.close()
    assert 0 < len(want_near) and near.tobytes() == want_near.tobytes()
    assert 0 < len(model.cloud) and glob.tobytes() == model.cloud.tobytes()
