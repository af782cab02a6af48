"""The Time-Surface raster on the crafted cases of tests/ts_cases.py (kernels_ts.hip through ts_push_events, ts_render,
ts_render_forward, track_set_current and track_images), held to the CPU oracle with np.array_equal on every mono8 image: there is
no tolerance.  What the cases reach, and that they reach it, is tested on the CPU (tests/test_ts_cases.py), where the oracle is
held to a plain restatement of the reference's TimeSurface.cpp and to the reference's own class (tests/test_ref_pin.py).

Cases that share an image size, a rig and a queue length share a handle: it is reset between cases, and decay_ms,
ignore_polarity and the median size change with esvo_set_params (the queue length is fixed at create).  The staging and geometry
cases run a second time in one fresh child process under ESVO_TS_STAGE_CAP=0, where every tile takes the direct path; both
runs must equal the oracle.  The queue cases overflow their tile lists by themselves (1088 and 1030 events in one batch): no
ESVO_TSQ_TILE_CAP.  eqpol_*: equal stamps of opposite polarity on one pixel follow the key-order rule of the kernel's comment
(the positive event wins), not the reference's arrival order.

What the module notices (scratch builds of kernels_ts.hip with one comparison flipped or one constant changed, none of which can
move an address; the new cases that turned red -- name: test_device_equals_the_oracle[name], name (direct): the child-process run
as well -- and whether the older Time-Surface tests noticed: test_gpu_parity::test_time_surface_* and ::test_bm_parity_dsec_smoothed,
test_gpu_fuzz's out-of-order ingest and tracker seeds, test_wire_golden, test_gpu_track):
  ts_decay_u8's guard `0.5f - 5e-4f` -> `0.5f`        all six sweep_*, both epoch_*, edges_d30_ip1, wide_k0 (direct)      older: 5 tests
                                                     (bit_exact[upenn], [ideal], both direct-path runs, fuzz seed 3081: a handful
                                                     of pixels of a bulk frame; the sweeps differ on hundreds)
  the fused render's `(acc + 16384) >> 15` -> `>> 15` every s70_*, mag128_*, wide_* (direct)                               older: 9 tests
  a tap outside the image returns the replicated     every s70_*, g33_*, mag128_* (direct)                                older: 9 tests
    pixel instead of 0
  median_by_rank's `le > n / 2` -> `>=`               median_k2_b, median_k3_b, s70_k2, s70_k3, g33_k2, g33_k3, mag128_k2,  older: 6 tests
                                                     wide_k2, wide_k3 (direct)
  the last exchange of median9 dropped               median_k1_b, every *_k1 and *_k1_pol case (direct), queue_L3_k1,     older: 13 tests
                                                     forward_ip1_k1, forward_ip0_k1
  tsq_view's `(k >> 1) < t_ns` -> `<=`                queue_L3, queue_L20, queue_L32, queue_L3_pol                         older: none
                                                     (the event at T above an older one: the view picks it, the decay refuses
                                                     it, the pixel renders empty; an event at T alone renders empty either way;
                                                     in queue_L3_k1 the 3 x 3 median filters the one pixel away)
  tsq_merge's `key >= mv` -> `>`                      none, and no input can: the two differ only where the arriving key EQUALS   older: none
                                                     the smallest key of a full queue, and replacing a key by itself leaves the
                                                     same set (keys that differ in the polarity bit alone are different keys)
  the overflow scan's `e.w == tile` dropped          queue_over_L3, queue_over_L20                                        older: 2 tests
                                                     (event_queues[4], the child process under ESVO_TSQ_TILE_CAP=4, and fuzz
                                                     seed 3081)
  FORWARD's clamp moved behind the loop              forward_ip0_k0 (with median 1 the one pixel is filtered away)        older: none
  gaussian5's `+ 128` dropped                        gauss_33x17, gauss_70x40                                             older: 6 tests
  staged against direct (ESVO_TS_STAGE_CAP, or the   none, by construction: both paths compute the same bytes; that they do is
    threshold `rw * rh <= stage_cap`)                what test_direct_path_equals_the_oracle and the boxes at 2560, 2562 and 2574 show"""
import copy
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import ts_cases as TC
import ts_restated as TR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HANDLES = {}


def _handle(c):
    """the handle of a case's rig and queue length, reset, under the case's parameters"""
    from esvo_amd import lib
    p = TC.case_params(c)
    key = TC.handle_key(c)
    if key not in _HANDLES:
        _HANDLES[key] = lib.Esvo(p, c["rig"])
    else:
        _HANDLES[key].reset()
        _HANDLES[key].set_params(copy.copy(p))
    return _HANDLES[key]


def run(name):
    """the mono8 image of every render / forward / gauss step of a case on the device, in script order"""
    c = TC.case(name)
    dev = _handle(c)

    def gauss(img):
        dev.track_set_current(img, 5)
        return dict(img=dev.track_images()[0].copy())

    out = TC.run_script(c, c["script"], dev.ts_push_events, lambda cam, T: dict(img=dev.ts_render(cam, T).copy()),
                        lambda cam, T: dict(img=dev.ts_render_forward(cam, T).copy()), gauss)
    return [o["img"] for o in out]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle on a case (eqpol_*: on the script the key-order rule leaves)"""
    return TC.oracle(name, expect=not TC.case(name)["oracle"])


def describe(name, i, o, got):
    """count and first differing pixel of output i, with what is known about it"""
    c = TC.case(name)
    d = np.argwhere(got != o["img"])
    y, x = (int(v) for v in d[0])
    msg = [f"{name} output {i} ({o['op']} cam {o['cam']} T {o['T']}): {len(d)} of {got.size} pixels differ; first (x {x}, y {y}): "
           f"device {int(got[y, x])} oracle {int(o['img'][y, x])}"]
    if c["group"] == "decay":      # identity map, no median: the output pixel is the raw pixel
        s = TC.decay_stats(name)[o["cam"]]
        k = np.flatnonzero((s["y"] == y) & (s["x"] == x))
        for j in k:
            msg.append(f"stamp {int(s['te'][j])} polarity {int(s['pol'][j])} dt {int(s['dt_ns'][j])} ns f64 value {s['g'][j]:.9f} "
                       f"distance to a half-integer {s['dist'][j]:.3g} inside the band {bool(s['in_band'][j])} float-only wrong {bool(s['float_wrong'][j])}")
        if not len(k):
            msg.append("no event before T on this pixel")
    elif o["op"] == "render":
        cam = TC.cams(c)[o["cam"]]
        t = TR.tile_boxes(cam.map_x, cam.map_y, c["W"], c["H"], c["median_k"])[(x // TR.TILE_X, y // TR.TILE_Y)]
        msg.append(f"map ({float(cam.map_x[y, x])!r}, {float(cam.map_y[y, x])!r}) tile {(x // TR.TILE_X, y // TR.TILE_Y)} {t}")
        te, pol, ys, xs = TC.found_events(c, o["cam"], o["T"])
        msg.append(f"events before T: {len(te)}")
    msg.append("tags: " + " ".join(sorted(TC.observe(name))))
    return "\n".join(msg)


def same(name, imgs, what):
    exp = expected(name)
    assert len(imgs) == len(exp) > 0
    for i, (got, o) in enumerate(zip(imgs, exp)):
        assert got.shape == o["img"].shape and got.dtype == np.uint8
        assert np.array_equal(got, o["img"]), what + ": " + describe(name, i, o, got)


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for dev in _HANDLES.values():
        dev.close()
    _HANDLES.clear()


def _dump(path):
    """(the child process) the staging and geometry cases on this process's handles"""
    flat = {}
    for name in TC.DIRECT_TWICE:
        for i, img in enumerate(run(name)):
            flat[f"{name}/{i}"] = img
    for dev in _HANDLES.values():
        dev.close()
    np.savez(path, **flat)


@pytest.fixture(scope="module")
def direct():
    """the staging and geometry cases in one fresh child process under ESVO_TS_STAGE_CAP=0: every tile on the direct path"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "direct.npz")
        code = f"import sys; sys.path.insert(0, 'tests'); import test_gpu_ts_cases as T; T._dump({path!r})"
        env = dict(os.environ, ESVO_DEV_SWITCHES="1", ESVO_TS_STAGE_CAP="0")
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        z = np.load(path)
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", TC.NAMES)
def test_device_equals_the_oracle(name):
    same(name, run(name), "default handle")


@pytest.mark.parametrize("name", TC.DIRECT_TWICE)
def test_direct_path_equals_the_oracle(name, direct):
    same(name, [direct[f"{name}/{i}"] for i in range(len(expected(name)))], "every tile direct (child process)")
