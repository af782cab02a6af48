"""The processing order of the narrow LM launch (kernels_lm.hip): grid position pos solves solver slot order[pos], the slots
sorted by their match's pixel, tile-major, stable.

* the order itself, through esvo_debug_lm_order: exactly numpy's stable argsort of the keys recomputed here from the match
  records, a permutation of [0, n) with the identity behind it, no guard word touched -- at the sizes where the radix sort
  changes path (its tile of 2048 rows +- 1, more than one tile, n = 0) and on the keys that break an unstable or a
  wrongly-ranked scatter (all equal, sorted, reversed, the image's last row and column, the smallest and largest patch SSD);
* bit identity of the mapper: the order changes WHERE in the grid a match is solved, never a bit of what comes out -- ticks of the
  smallest bound that takes the narrow layout against the same ticks of a handle created with ESVO_LM_ORDER=0 (a fresh child
  process: the switch is read at create), every field of every DepthMap element and frame point, `seq` included."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_LOG2 = 3          # kernels_lm.hip, LM_ORDER_TILE_LOG2: 8 x 8 pixel tiles, raster inside, tiles in raster order
PATCH_W, PATCH_H = 15, 7
SORT_TILE = 2048       # kernels_voxel.hip, VOX_TILE: rows per block and radix pass


# ---- the order primitive -------------------------------------------------------------------------------------------------
def _bits(v):
    return np.where(v > 0, np.floor(np.log2(np.maximum(v, 1))).astype(np.int64) + 1, 0)


def _pixel_key(x, y, W):
    m = (1 << TILE_LOG2) - 1
    tiles_x = (W + m) >> TILE_LOG2
    return ((((y >> TILE_LOG2) * tiles_x + (x >> TILE_LOG2)) << (2 * TILE_LOG2)) | ((y & m) << TILE_LOG2)) | (x & m)


def _ssd(x, y, disp, left, right, updown):
    H, W = left.shape
    out = np.zeros(len(x), np.int64)
    L, R = left.astype(np.int64), right.astype(np.int64)
    for dy in range(-(PATCH_H // 2), PATCH_H // 2 + 1):
        for dx in range(-(PATCH_W // 2), PATCH_W // 2 + 1):
            ly, lx = np.clip(y + dy, 0, H - 1), np.clip(x + dx, 0, W - 1)
            ry = np.clip(ly - (disp if updown else 0), 0, H - 1)
            rx = np.clip(lx - (0 if updown else disp), 0, W - 1)
            out += (L[ly, lx] - R[ry, rx]) ** 2
    return out


def _expected(matches, max_matches, left, right, T, updown, variant):
    """the order the library must return: slot s holds match stride_item(s, n, T) (the per-thread lists of the reference, back to back)"""
    n = len(matches)
    H, W = left.shape
    x = np.clip(np.floor(matches["x_left"][:, 0]), 0, W - 1).astype(np.int64)
    y = np.clip(np.floor(matches["x_left"][:, 1]), 0, H - 1).astype(np.int64)
    key = _pixel_key(x, y, W)
    if variant == 1:
        pixel_bits = int(_bits(np.array([_pixel_key(np.int64(W - 1), np.int64(H - 1), W)]))[0])
        disp = np.clip(matches["disp"], 0, 65535).astype(np.int64)
        key = ((31 - _bits(_ssd(x, y, disp, left, right, updown))) << pixel_bits) | key
    slot_match = np.concatenate([np.arange(t, n, T) for t in range(T)]).astype(np.int64) if n else np.zeros(0, np.int64)
    order = np.argsort(key[slot_match], kind="stable")
    return np.concatenate([order, np.arange(n, max_matches)]).astype(np.uint32)


def _matches(x, y, disp=None):
    from esvo_amd import lib
    m = np.zeros(len(x), lib.MATCH_DTYPE)
    m["x_left"][:, 0] = x
    m["x_left"][:, 1] = y
    m["disp"] = 7.0 if disp is None else disp
    m["inv_depth"] = 0.5
    m["event_idx"] = np.arange(len(x))
    return m


def _check(matches, max_matches, left, right, T=1, updown=False):
    from esvo_amd import lib
    H, W = left.shape
    r = lib.debug_lm_order(matches, max_matches, W, H, left, right, num_threads=T, updown=updown)
    assert r["guards"] == 0
    assert r["variant"] in (0, 1)
    n = len(matches)
    assert np.array_equal(np.sort(r["order"][:n]), np.arange(n, dtype=np.uint32))          # a permutation of [0, n)
    assert np.array_equal(r["order"][n:], np.arange(n, max_matches, dtype=np.uint32))     # the identity behind it
    assert np.array_equal(r["order"], _expected(matches, max_matches, left, right, T, updown, r["variant"]))
    return r


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(20250608)
    W, H = 346, 260    # (not a multiple of the tile in either direction)
    return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1])
def test_order_small_counts_and_sort_tile_edges(images, n):
    left, right = images
    H, W = left.shape
    rng = np.random.default_rng(n)
    # sub-pixel coordinates on few pixels: many equal keys, whose slots must stay in slot order
    m = _matches(rng.integers(0, 40, n) + rng.random(n), rng.integers(100, 130, n) + rng.random(n), rng.integers(0, 30, n))
    _check(m, n + 3, left, right, T=4)
    if n:
        _check(m, n, left, right, T=1)


def test_order_full_tick_size():
    rng = np.random.default_rng(45000)
    W, H = 640, 480
    left, right = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)
    n = 45000
    px = rng.integers(0, 30000, n)   # 45 000 matches on 30 000 pixels: a third share theirs, as in a tick
    pool_x, pool_y = rng.integers(0, W, 30000), rng.integers(0, H, 30000)
    m = _matches(pool_x[px] + 0.25, pool_y[px] + 0.75, rng.integers(0, 81, n))
    _check(m, n + 1234, left, right, T=4)


def test_order_equal_sorted_reversed_and_image_edges(images):
    left, right = images
    H, W = left.shape
    n = SORT_TILE * 2 + 77
    same = _matches(np.full(n, 17.5), np.full(n, 33.5))
    r = _check(same, n, left, right, T=4)
    assert np.array_equal(r["order"], np.arange(n, dtype=np.uint32))      # all keys equal: the identity
    # one match per pixel in key order (tile-major), and the same list reversed
    ys, xs = np.divmod(np.arange(W * H), W)
    by_key = np.argsort(_pixel_key(xs, ys, W), kind="stable")[:n]
    _check(_matches(xs[by_key] + 0.5, ys[by_key] + 0.5), n, left, right)
    _check(_matches(xs[by_key][::-1] + 0.5, ys[by_key][::-1] + 0.5), n, left, right)
    # the last row and the last column, beside the first ones
    ex = np.concatenate([np.arange(W), np.full(H, W - 1), np.arange(W), np.zeros(H, np.int64)])
    ey = np.concatenate([np.full(W, H - 1), np.arange(H), np.zeros(W, np.int64), np.arange(H)])
    _check(_matches(ex + 0.999, ey + 0.999, np.full(len(ex), 40)), len(ex) + 5, left, right, T=3)
    _check(_matches(ex + 0.999, ey + 0.999, np.full(len(ex), 40)), len(ex) + 5, left, right, T=3, updown=True)


def test_order_smallest_and_largest_patch_ssd():
    """(the SSD variant's extremes; with the pixel key alone the images are not read and the cases check the pixel order once more)"""
    W, H = 96, 64
    rng = np.random.default_rng(7)
    n = 300
    x, y = rng.integers(0, W, n) + 0.5, rng.integers(0, H, n) + 0.5
    flat = np.full((H, W), 90, np.uint8)
    _check(_matches(x, y, np.zeros(n)), n, flat, flat)                                             # SSD 0 everywhere
    _check(_matches(x, y, np.zeros(n)), n, np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8))  # 105 x 255^2 everywhere
    mixed = flat.copy()
    mixed[:, W // 2:] = 255    # both extremes and the octaves between them in one list
    _check(_matches(x, y, rng.integers(0, 20, n)), n + 1, mixed, np.zeros((H, W), np.uint8), T=2)


# ---- bit identity of the mapper -------------------------------------------------------------------------------------------
EVENTS_CAP = 45000   # the smallest bound in use that still takes the narrow layout (40 001 events and up)
N_TICKS = 6


def _fields(a):
    return {f: a[f].tobytes() for f in a.dtype.names}


def _result(dev):
    s = dev.stats()
    return dict(map=dev.get_map(), frame=dev.get_last_frame(),
                totals=np.array([s.total_matches, s.total_points, s.last_matches, s.last_solved, s.last_points], np.int64))


def _run_ticks(rig, stream, p, ticks, sync_each, ev_left=None, ev_right=None):
    from esvo_amd import lib
    dev = lib.Esvo(p, rig)
    dev.ts_push_events(0, stream.ev_left if ev_left is None else ev_left)
    dev.ts_push_events(1, stream.ev_right if ev_right is None else ev_right)
    for t, stamps, poses, T in ticks:
        dev.ts_render(0, t, download=False); dev.ts_render(1, t, download=False)
        dev.set_observation(t, None, None, T)
        dev.tick(t, stamps, poses)
        if sync_each:
            dev.synchronize()
    return _result(dev)


def _scenarios():
    """every scenario of this file on the handle the environment selects -> {name: result}"""
    import bench
    rig, stream, p, ticks = bench.make_workload("dsec640x480", N_TICKS, events_cap=EVENTS_CAP)
    out = {"pipelined": _run_ticks(rig, stream, p, ticks, False), "synchronised": _run_ticks(rig, stream, p, ticks, True)}
    t0 = ticks[0][0]
    hi = int(np.searchsorted(stream.ns_left, t0, side="left"))
    for cut in range(4):   # one tick whose newest events are cut off: four neighbouring match counts
        out[f"cut{cut}"] = _run_ticks(rig, stream, p, ticks[:1], True, ev_left=stream.ev_left[:hi - 37 * cut])
    # no match at all: a full launch bound of left events against an empty slice of the right camera, and an empty slice of both
    out["no_match"] = _run_ticks(rig, stream, p, ticks[:1], True, ev_right=stream.ev_right[:0])
    out["no_event"] = _run_ticks(rig, stream, p, ticks[:1], True, ev_left=stream.ev_left[:0], ev_right=stream.ev_right[:0])
    return out


def _dump(path):
    flat = {}
    for name, r in _scenarios().items():
        for k, v in r.items():
            flat[f"{name}/{k}"] = v
    np.savez(path, **flat)


@pytest.fixture(scope="module")
def both():
    """(ordered, identity): the scenarios on this process's default handle and on an ESVO_LM_ORDER=0 handle of a child process"""
    ordered = _scenarios()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "identity.npz")
        code = f"import sys; sys.path.insert(0, 'tests'); import test_gpu_lm_order as T; T._dump({path!r})"
        env = dict(os.environ, ESVO_DEV_SWITCHES="1", ESVO_LM_ORDER="0")
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        z = np.load(path)
        identity = {}
        for key in z.files:
            name, k = key.split("/")
            identity.setdefault(name, {})[k] = z[key]
    return ordered, identity


def _same(a, b):
    assert np.array_equal(a["totals"], b["totals"]), (a["totals"], b["totals"])
    for what in ("map", "frame"):
        assert len(a[what]) == len(b[what]), what
        fa, fb = _fields(a[what]), _fields(b[what])
        for f in fa:
            assert fa[f] == fb[f], (what, f)


@pytest.mark.parametrize("name", ["pipelined", "synchronised"])
def test_ordered_launch_changes_no_bit(both, name):
    ordered, identity = both
    assert ordered[name]["totals"][0] > N_TICKS * 4000 and len(ordered[name]["map"]) > 1000 and len(ordered[name]["frame"]) > 1000
    _same(ordered[name], identity[name])


def test_match_counts_around_a_wave(both):
    ordered, identity = both
    counts = [int(ordered[f"cut{c}"]["totals"][2]) for c in range(4)]
    assert any(c % 4 for c in counts), counts     # at least one launch ends inside a wave of four
    for c in range(4):
        _same(ordered[f"cut{c}"], identity[f"cut{c}"])
    for name in ("no_match", "no_event"):
        assert ordered[name]["totals"][2] == 0 and len(ordered[name]["frame"]) == 0, name
        _same(ordered[name], identity[name])
