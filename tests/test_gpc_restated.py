"""The global point cloud's branch restated (tests/gpc_restated.py): tail rule, interval gate, reset; and the parts of the
device feature that need no GPU -- struct sizes, presets, the NULL-handle answer."""
import ctypes as C

import numpy as np

import gpc_restated as G
from esvo_amd import abi, lib, params


def _fake_filter(n):
    """a voxel filter that returns n numbered points whatever it is given"""
    return lambda xyz, leaf: np.arange(3 * n, dtype=np.float32).reshape(n, 3)


def _near(_range):
    return np.ones((4, 3), np.float32)


def test_tail_rule_on_hand_cases():
    assert G.tail_count(1, 1000) == 0
    assert G.tail_count(5, 3) == 2
    assert G.tail_count(3, 10) == 2
    assert G.tail_count(0, 1000) == 0
    for L, thr, want in ((1, 1000, []), (5, 3, [3, 4]), (3, 10, [1, 2]), (0, 1000, [])):
        g = G.Gpc(2.5, 0.0, thr, voxel_filter=_fake_filter(L))
        assert g.update(1_000_000_000, _near) is True
        assert g.cloud.tobytes() == _fake_filter(L)(None, 0)[want].tobytes(), (L, thr)   # the LAST points, in their order
        assert (g.last_voxels, g.last_added, g.refreshes) == (L, len(want), 1)             # L == 0 still counts as a refresh


def test_gate_is_a_strict_greater_than_from_zero():
    g = G.Gpc(2.5, 3.0, 1000, voxel_filter=_fake_filter(4))
    assert g.t_last_pub == 0.0
    assert g.update(1_000_000_000, _near) is False                  # 1 - 0 > 3 is false: the first update is not due
    assert len(g.cloud) == 0 and g.t_last_pub == 0.0 and (g.updates, g.refreshes) == (1, 0)
    assert g.update(3_000_000_000, _near) is False                  # now - t_last == interval: not due
    assert g.update(3_000_000_001, _near) is True
    assert g.t_last_pub == 3.000000001 and len(g.cloud) == 3
    assert g.update(6_000_000_001, _near) is False                  # == interval again, from the new t_last_pub
    assert g.update(6_000_000_002, _near) is True and len(g.cloud) == 6
    assert (g.updates, g.refreshes) == (5, 2)


def test_reset_empties_the_cloud_and_keeps_t_last_pub():
    g = G.Gpc(2.5, 1.0, 1000, voxel_filter=_fake_filter(4))
    assert g.update(2_000_000_000, _near) and len(g.cloud) == 3
    g.reset()
    assert len(g.cloud) == 0 and g.t_last_pub == 2.0
    assert g.update(2_000_000_000, _near) is False                  # the same stamp again: not due
    assert g.update(3_500_000_000, _near) is True and len(g.cloud) == 3


def test_capacity_error_changes_nothing():
    g = G.Gpc(2.5, 0.0, 1000, capacity_points=4, voxel_filter=_fake_filter(4))
    assert g.update(1_000_000_000, _near)
    before = (g.cloud.tobytes(), g.counts())
    try:
        g.update(2_000_000_000, _near)
        raise AssertionError("no capacity error")
    except G.CapacityError:
        pass
    assert (g.cloud.tobytes(), g.counts()) == before


def test_restated_branch_over_the_oracle_filter():
    """the default filter is oracle.voxel_filter, equal to the host helper; the reversed-order variant differs on an
    order-revealing voxel and not in which voxels come out"""
    from oracle import oracle as O
    pts = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.25], [5.0, 5.0, 5.0]], np.float32)   # two in voxel 0, one far away
    g = G.Gpc(2.5, 0.0, 1000)
    assert g.update(1_000_000_000, lambda r: pts)
    want = O.voxel_filter(pts, 0.3)
    assert len(want) == 2 and g.cloud.tobytes() == want[1:].tobytes()
    assert lib.voxel_filter(pts, 0.3).tobytes() == want.tobytes()
    big = np.array([[1e8, 0, 0]] + [[1, 0, 0]] * 8, np.float32)   # 1e8 + 1 == 1e8 in float, 1e8 + 8 is not
    fwd, rev = O.voxel_filter(big, 1e9), G.voxel_filter_reversed(big, 1e9)
    assert fwd.shape == rev.shape == (1, 3) and fwd.tobytes() != rev.tobytes()


def test_abi_number_and_struct_sizes():
    assert lib.abi_sizes()[7] == 8
    assert lib.gpc_sizes() == [C.sizeof(abi.GpcParamsStruct), C.sizeof(abi.GpcStatsStruct), 5_000_000, 0]
    assert C.sizeof(abi.GpcParamsStruct) == 40 and C.sizeof(abi.GpcStatsStruct) == 56


def test_presets_hold_the_shipped_yaml_values():
    want = {
        "mapping_upenn": dict(bVisualizeGlobalPC=True, visualizeGPC_interval=1, NumGPC_added_per_refresh=3000, visualize_range=5.0),
        "mapping_rpg": dict(bVisualizeGlobalPC=True, visualizeGPC_interval=3, NumGPC_added_per_refresh=1000, visualize_range=5.0),
        "mapping_hkust": dict(bVisualizeGlobalPC=True, visualizeGPC_interval=1, NumGPC_added_per_refresh=1500, visualize_range=2.5),
        "mapping_dsec": dict(bVisualizeGlobalPC=True, visualizeGPC_interval=0.5, NumGPC_added_per_refresh=10000, visualize_range=30),
        "code_defaults": dict(bVisualizeGlobalPC=False, visualizeGPC_interval=3, NumGPC_added_per_refresh=1000, visualize_range=2.5),
    }
    assert params.GPC_PRESETS == want
    assert not any(k in cfg for cfg in params.PRESETS.values() for k in want["code_defaults"])   # PRESETS got no new keys
    assert params.GPC_LEAF == 0.3


def test_library_loads_without_a_gpu_and_refuses_a_null_handle():
    so = lib.load()
    r = C.c_int(7)
    assert so.esvo_map_gpc_update(None, 1, C.byref(r)) == abi.ERR_INVALID_ARG and r.value == 7
    n = C.c_size_t(9)
    for rc in (so.esvo_map_gpc_configure(None, None), so.esvo_map_gpc_get(None, None, 0, C.byref(n)),
               so.esvo_map_gpc_stats(None, None), so.esvo_map_gpc_device(None, None, None),
               so.esvo_map_cloud_near(None, 1.0, None, 0, C.byref(n)), so.esvo_map_voxel_filter(None, None, 0, 0.3, None, 0, C.byref(n))):
        assert rc == abi.ERR_INVALID_ARG
    assert n.value == 9
