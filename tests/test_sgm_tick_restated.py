"""tests/sgm_tick_restated.py (esvo_MVStereo mode 4, PURE_SEMI_GLOBAL_MATCHING, behind the disparity image) pinned to the
reference's own compiled mode-4 branch, and its naive propagation cross-checked against the pinned oracle.

The reference node (oracle/ref.py: RefNode(..., mvstereo=True, extra={"MVStereoMode": 4})) runs dataTransferring's mode-4 branch
and MappingAtTime in mode 4 unmodified; the stand-in StereoSGBM::compute returns the disparity image injected through
initialization_at_time (which, in the MVStereo build, does nothing else).  Per tick: the SGM event list, the window's frame
sizes and every field of the newest frame are equal exactly; p_cam to 1e-12 (the reference inverts a 4x4 per cam2World call); the
map under the rule the bootstrap's pin uses (test_ref_pin._sgm_maps_agree): the node hands INTEGER pixel coordinates through
cam2World -> T_frame_obs -> world2Cam and floors the result, so the cell a point lands in depends on the last bit of that round
trip.  Measured on these inputs: frames equal, p_cam within 2.3e-15, map sizes within 1 %, agreement 98.6 - 100 % per tick.
"""
import ctypes
import os

import numpy as np
import pytest

import sgm_tick_cases as SC
import sgm_tick_restated as SR
from oracle import oracle as O


def test_sgm_sizes_match_bindings():
    from esvo_amd import abi, lib
    s = lib.sgm_sizes()
    assert s[0] == ctypes.sizeof(abi.SgmStatsStruct) == 64 and s[1] == SR.NUM_DISPARITIES and s[2] == s[3] == 0
    assert lib.abi_sizes()[7] == 8                                    # additive: the ABI number stays


def test_restated_naive_propagation_equals_the_pinned_oracle(upenn_rig, upenn_stream):
    """the single frame of OracleMapper.init_sgm through the restatement's naive_propagation gives the oracle's map bit for bit"""
    from esvo_amd import params
    rig, stream = upenn_rig, upenn_stream
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], rig)
    t = stream.t0_ns + int(0.08e9)
    ts = [O.OracleTS(rig.width, rig.height), O.OracleTS(rig.width, rig.height)]
    ts[0].push(stream.ev_left)
    ts[1].push(stream.ev_right)
    l = ts[0].render(t, map_x=rig.left.map_x, map_y=rig.left.map_y)
    r = ts[1].render(t, map_x=rig.right.map_x, map_y=rig.right.map_y)
    m = O.OracleMapper(p, rig)
    m.set_mode(True, True)
    T = np.asarray(stream.pose(t), np.float64).reshape(4, 4)
    m.set_observation(t, l, r, T)
    idx = O.select_events_sgm(stream.ev_left, t, p.bm_half_slice_thickness, p.process_event_num)
    n, _ = m.init_sgm(l, r, stream.ev_left[idx], min_points=50)
    frame, ref_map = m.get_last_frame(), m.get_map()
    assert len(frame) == n > 50 and len(ref_map) > n
    got = SR.naive_propagation(rig, [(frame, T)], T)
    assert SR.same_bits(got, ref_map, [f for f in SR.FIELDS if f not in ("pose_idx", "seq")]) is None


def test_restated_point_rule_on_a_crafted_disparity(upenn_rig):
    """the rules that differ from the bootstrap's, at the smallest size: column 47 / 48, a negative and a zero disparity, two events
    on one pixel, an event off the sensor"""
    from esvo_amd import abi, params
    rig = upenn_rig
    p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], rig)
    W, H = rig.width, rig.height
    lut = np.asarray(rig.left.rect_lut, np.float32).reshape(H, W, 2)
    pix = np.floor(lut).astype(np.int64)
    disp = np.full((H, W), -16, np.int16)

    def event_at(col, row):  # a sensor pixel whose rectified coordinate floors to (col, row)
        ys, xs = np.nonzero((pix[..., 0] == col) & (pix[..., 1] == row))
        assert len(xs), (col, row)
        return int(xs[0]), int(ys[0])
    targets = [(47, 100), (48, 100), (120, 60), (130, 70), (140, 80), (140, 80)]
    disp[100, 47], disp[100, 48], disp[60, 120], disp[70, 130], disp[80, 140] = 80, 80, -16, 0, 33
    xy = [event_at(c, r) for c, r in targets] + [(W, 5)]
    ev = abi.make_events([a for a, _ in xy], [b for _, b in xy], 10_000_000_000 + np.arange(len(xy)))
    fr, st = SR.points(rig, p, disp, ev)
    assert st == dict(events=7, on_image=6, matched_columns=5, disp_ok=4, points=4, zero_disp=1)
    assert fr["row"].tolist() == [48, 130, 140, 140] and fr["col"].tolist() == [100, 70, 80, 80]   # dp(x, y): row = x
    assert fr["inv_depth"][1] == 0 and not np.isfinite(fr["p_cam"][1]).all() and np.isfinite(fr["p_cam"][[0, 2, 3]]).all()
    mp = SR.naive_propagation(rig, [(fr, np.eye(4))], np.eye(4))
    assert len(mp) == 8                                               # the zero touches no cell, the pair has one owner


def test_restatement_equals_the_reference_mvstereo_node_in_mode_4():
    from oracle import ref as R
    if not os.path.isdir(os.path.join(R.REFERENCE, "esvo_core", "src")):
        pytest.skip("reference tree not present (GPU box)")
    from test_ref_pin import _sgm_maps_agree
    rig, stream, p, ticks = SC.case("upenn")
    node = R.RefNode(p, rig, stream.pose, mvstereo=True, extra={"MVStereoMode": 4})
    node.push_events(stream.ev_left)
    zero_points = 0
    for k, (tk, (frame, mp, window, stats)) in enumerate(zip(ticks, SC.restated("upenn"))):
        node.push_observation(tk["t"], tk["l"], tk["r"])
        assert node.data_transferring() and node.obs_time() == tk["t"]
        assert np.array_equal(node.sgm_events(), tk["idx"])
        assert node.initialization_at_time(tk["disp"]) is False     # MVStereo build: stores the disparity, nothing else
        node.mapping_at_time()
        assert node.window() == window, k
        ref = node.newest_frame()
        assert len(ref) == len(frame) > 0
        for f in ("row", "col", "x", "inv_depth", "variance", "residual", "age"):
            assert np.array_equal(ref[f], frame[f]), (k, f)
        fin = np.isfinite(frame["p_cam"]).all(axis=1)
        assert np.array_equal(fin, np.isfinite(ref["p_cam"]).all(axis=1))
        dp = np.abs(ref["p_cam"][fin] - frame["p_cam"][fin]).max()
        print(f"tick {k}: points {len(frame)}, p_cam max |diff| {dp:.3g}, map {len(mp)} vs reference {len(node.get_map())}")
        assert dp <= 1e-12, (k, dp)
        zero_points += int((frame["inv_depth"] == 0).sum())
        rm = node.get_map()
        _sgm_maps_agree(mp["row"], mp["col"], mp["inv_depth"], rm["row"], rm["col"], rm["inv_depth"])
    assert zero_points > 0 and len(window) == 3
