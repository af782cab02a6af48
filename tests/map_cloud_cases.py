"""Maps the device-resident point cloud tests run on (tests/test_gpu_map_cloud.py, tests/test_gpu_track_from_cloud.py): the
four-tick set-up of tests/test_gpu_track.py on the upenn and DSEC fixtures, built once per process and then only READ (read-outs,
cloud builds, tracker calls) -- a test that goes on ticking takes a handle of its own (fresh=True)."""
import numpy as np

from esvo_amd import lib, params, rostime

_maps = {}

CASES = {
    # upenn, no regulariser: the map is read from the first buffer
    "upenn": dict(preset="mapping_upenn", rig="upenn_rig", stream="upenn_stream", over=dict(regularization=0)),
    # DSEC with the shipped regulariser (radius 20): the map is read from the second buffer; 4000 events per tick
    "dsec": dict(preset="mapping_dsec", rig="dsec_rig", stream="dsec_stream", over=dict(process_event_num=4000)),
}


def tick_at(dev, stream, p, t, t_prev, bm_only=False):
    """stage the events of (t_prev, t], render both Time Surfaces, tick at t with ground-truth poses; returns the left surface"""
    for cam in (0, 1):
        dev.ts_push_events(cam, stream.slice(cam, t_prev, t))
    ts_left = dev.ts_render(0, t)
    dev.ts_render(1, t, download=False)
    stamps, poses = rostime.pose_table(stream.pose, t, p.bm_half_slice_thickness)
    dev.set_observation(t, None, None, stream.pose(t))
    (dev.tick_bm_only if bm_only else dev.tick)(t, stamps, poses)
    return ts_left


def ticked(request, name, n_ticks=4, fresh=False, bm_only=False, **over):
    """(dev, p, stream, t of the last tick, left Time Surface at t) after n_ticks mapper ticks 10 ms apart"""
    key = (name, n_ticks, bm_only, tuple(sorted(over.items())))
    if not fresh and key in _maps:
        return _maps[key]
    c = CASES[name]
    rig, stream = request.getfixturevalue(c["rig"]), request.getfixturevalue(c["stream"])
    p, _ = params.make_params(params.PRESETS[c["preset"]], rig, **dict(c["over"], **over))
    dev = lib.Esvo(p, rig)
    t_prev, t, ts_left = stream.t0_ns, stream.t0_ns, None
    for k in range(n_ticks):
        t = stream.t0_ns + int((0.06 + 0.01 * k) * 1e9)
        ts_left = tick_at(dev, stream, p, t, t_prev, bm_only)
        t_prev = t
    out = (dev, p, stream, t, ts_left)
    if not fresh:
        _maps[key] = out
    return out


def same_cloud(dev):
    """build the device-resident cloud and compare it with the host read-out: counts and bytes; returns the cloud"""
    want = dev.get_pointcloud()
    n = dev.map_cloud_build()
    got = dev.map_cloud()
    assert n == len(want) == len(got), (n, len(want), len(got))
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()
    ptr, n_dev, _ = dev.map_cloud_device()
    assert n_dev == n and (ptr != 0 or n == 0)
    return got
