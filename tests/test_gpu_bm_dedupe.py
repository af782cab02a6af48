"""Block matching once per distinct raw pixel (kernels_bm.hip, launch_bm_match_dedupe): the lowest slot of a pixel runs the
disparity search, every other event at the pixel copies its outcome with its own event_idx and its own pose look-up.  Nothing
that leaves the stage may change by a bit: the compacted match list, its count and the three failure counters.

The scenarios run on this process's handles with ESVO_BM_DEDUPE_MIN=1 (every launch shares) and once more in one fresh child
process with ESVO_BM_DEDUPE=0 (one search per event: the switches are read at create); the results are compared byte by byte.

* the match stage alone (dev.match on the 346 x 260 rig, a crafted observation pair): n = 0, 1, 7, 8, 9, 64 and 65 events on one
  pixel, no shared pixel at all, 3000 events on 1000 pixels, pairs 8 k slots apart / in neighbouring slots / in the last, partly
  filled wave, num_threads 1 and 4, shared pixels that fail each way (x >= W, masked, border patch, empty Time Surface, best cost
  above the threshold) and pose tables that end before the lowest or before a later slot of a pixel;
* the same list against the CPU oracle's exact-integer mode;
* two calls on one handle against the second call on a fresh handle (the owner table carries nothing over);
* the mapper: 6 ticks of dsec640x480 at 45 000 events per tick, pipelined and waited for one by one, and one denoised tick."""
import copy
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0_NS = 100_000_000_000
LATE_NS = T0_NS + 20_000_000          # behind the last pose stamp
EVENTS_CAP = 45000
N_TICKS = 6
CLASSES = ("good", "noise", "thresh", "border", "masked")


class _shared_env:
    """handles created inside take the shared path from one event on (a no-op where ESVO_BM_DEDUPE=0 is set: the child)"""

    def __enter__(self):
        self.old = os.environ.get("ESVO_BM_DEDUPE_MIN")
        os.environ["ESVO_BM_DEDUPE_MIN"] = "1"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("ESVO_BM_DEDUPE_MIN", None)
        else:
            os.environ["ESVO_BM_DEDUPE_MIN"] = self.old


# ---- the match stage alone ---------------------------------------------------------------------------------------------
_WORLD = {}


def _world():
    """rig, observation pair, pose stamps and the raw pixels of every outcome class (seeded: the same in the child process)"""
    if _WORLD:
        return _WORLD
    from esvo_amd import calib, params
    rig = copy.deepcopy(calib.dataset_rig("upenn"))
    W, H = rig.width, rig.height
    assert (W, H) == (346, 260)
    rig.left.rect_mask[:, W - 11:] = 0     # (the rig's own mask hides no pixel its look-up table keeps inside the image)
    p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], rig)
    dmax = p.bm_max_disparity
    d0 = (p.bm_min_disparity + dmax) // 2
    rng = np.random.default_rng(20250930)
    left = rng.integers(1, 256, (H, W), dtype=np.uint8)
    right = np.roll(left, -d0, axis=1)                               # right[:, x] = left[:, x + d0]: every patch matches at d0
    left[:70] = 0                                                    # an empty Time Surface region: the info-noise test fails
    right[70:140] = rng.integers(1, 256, (70, W), dtype=np.uint8)    # unrelated texture: no cost below the threshold
    lut = np.asarray(rig.left.rect_lut, np.float32).reshape(H, W, 2)
    xr, yr = lut[..., 0].astype(np.float64), lut[..., 1].astype(np.float64)
    inside = (xr >= 0) & (xr <= W - 1) & (yr >= 0) & (yr <= H - 1)
    xi, yi = np.clip(xr, 0, W - 1).astype(np.int64), np.clip(yr, 0, H - 1).astype(np.int64)
    mask = rig.left.rect_mask
    unmasked = inside & (np.ones((H, W), bool) if mask is None else mask[yi, xi] > 125)
    cols = (xr >= dmax + 9) & (xr < W - 10)                          # every candidate's patch lies inside the image
    sel = dict(good=unmasked & cols & (yr >= 150) & (yr < 250),
               noise=unmasked & cols & (yr >= 10) & (yr < 60),
               thresh=unmasked & cols & (yr >= 80) & (yr < 130),
               border=unmasked & (xr < 7) & (yr >= 10) & (yr < 250),
               masked=inside & ~unmasked)
    pix = {}
    for name, m in sel.items():
        ys, xs = np.nonzero(m)
        order = rng.permutation(len(xs))
        pix[name] = np.stack([xs[order], ys[order]], axis=1)        # (x, y) raw pixels, shuffled
    for name in CLASSES:
        assert len(pix[name]) >= 400, (name, len(pix[name]))
    stamps = (T0_NS + np.arange(6) * 2_000_000).astype(np.uint64)
    poses = np.tile(np.eye(4).reshape(16), (6, 1))
    _WORLD.update(rig=rig, W=W, H=H, d0=d0, left=left, right=right, pix=pix, stamps=stamps, poses=poses)
    return _WORLD


def _events(xy, t_ns):
    from esvo_amd import abi
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    return abi.make_events(xy[:, 0], xy[:, 1], np.asarray(t_ns, np.uint64))


def _times(rng, n):
    return T0_NS + rng.integers(100_000, 9_900_000, n)               # inside the pose table, spread over its stamps


def _cases():
    """name -> (num_threads, events, number of pose stamps handed over)"""
    w = _world()
    pix, W = w["pix"], w["W"]
    rng = np.random.default_rng(77)
    out = {}
    g = pix["good"]
    few = g[[0, 0, 1, 0, 2, 1, 3, 0, 4]]
    for n in (0, 1, 7, 8, 9):
        out[f"n{n}"] = (4, _events(few[:n], _times(rng, n)), 6)
    for n in (64, 65):
        out[f"one_pixel{n}"] = (4, _events(np.tile(g[5], (n, 1)), _times(rng, n)), 6)
    every = np.concatenate([pix[c][:200] for c in CLASSES if len(pix[c])])
    out["distinct"] = (4, _events(every[rng.permutation(len(every))[:500]], _times(rng, 500)), 6)
    pool = np.concatenate([g[:700], pix["noise"][:120], pix["thresh"][:120], pix["border"][:40], pix["masked"][:20]])[:1000]
    draw = pool[rng.integers(0, len(pool), 3000)]
    t3000 = _times(rng, 3000)
    out["pool3000"] = (4, _events(draw, t3000), 6)
    out["pool3000_t1"] = (1, _events(draw, t3000), 6)
    # pairs: slots i and i + 8 k (same wave of the search for no k, same 64-slot wave of the one-thread-per-slot kernels up to
    # k = 7, other waves beyond), neighbouring slots, and partners inside the last, partly filled wave (n = 8 * 37 + 3)
    n = 8 * 37 + 3
    base = np.concatenate([g[10:10 + n - 60], pix["thresh"][200:230], pix["noise"][200:230]])
    base = base[rng.permutation(n)]
    for i, j in [(0, 8), (1, 17), (2, 66), (3, 131), (20, 21), (63, 64), (70, 71), (100, n - 1), (n - 3, n - 2), (5, n - 2), (40, 296)]:
        base[j] = base[i]
    tp = _times(rng, n)
    out["pairs_t1"] = (1, _events(base, tp), 6)
    out["pairs_t4"] = (4, _events(base, tp), 6)
    # shared pixels that fail each way, five events apiece, interleaved with ones that match
    rows = [np.array([W + 5, 40])] + [pix[c][300 if len(pix[c]) > 300 else 0] for c in ("masked", "border", "noise", "thresh") if len(pix[c])]
    rows.append(g[300])
    fail = np.tile(np.stack(rows), (5, 1))
    out["failures"] = (4, _events(fail, _times(rng, len(fail))), 6)
    out["failures_t1"] = (1, _events(fail, _times(rng, len(fail))), 6)
    # a pose table that ends before some events: pixel A's lowest slot has no pose and a later one has, pixel B the other way
    # round (num_threads 1: slot = event index), then both patterns among duplicates of the whole pool
    a, b = g[310], g[311]
    out["pose_ab"] = (1, _events([a, a, b, b], [LATE_NS, T0_NS + 3_000_000, T0_NS + 5_000_000, LATE_NS]), 6)
    late = _times(rng, 3000)
    late[rng.random(3000) < 0.4] = LATE_NS
    out["pose_pool"] = (4, _events(draw, late), 6)
    out["pose_short_table"] = (4, _events(draw, t3000), 3)            # stamps up to 4 ms: most events lie behind the table
    return out


def _match_scenarios():
    from esvo_amd import lib, params
    w = _world()
    out = {}
    devs = {}
    for name, (T, ev, n_st) in _cases().items():
        if T not in devs:
            p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], w["rig"], num_threads=T, max_events_per_tick=4096)
            devs[T] = lib.Esvo(p, w["rig"])
            devs[T].set_observation(T0_NS, w["left"], w["right"], np.eye(4))
        dev = devs[T]
        rec = dev.match(ev, w["stamps"][:n_st], w["poses"][:n_st])
        s = dev.stats()
        cnt = np.array([len(rec), s.last_matches if len(ev) else 0, s.last_bm_info_noise_low if len(ev) else 0,
                        s.last_bm_coarse_fail if len(ev) else 0, s.last_bm_fine_fail if len(ev) else 0], np.int64)
        out[name] = dict(rec=rec.copy(), cnt=cnt)
    return out


# ---- the mapper --------------------------------------------------------------------------------------------------------
def _result(dev):
    s = dev.stats()
    return dict(map=dev.get_map(), frame=dev.get_last_frame(),
                totals=np.array([s.total_matches, s.total_points, s.last_matches, s.last_solved, s.last_points, s.total_events_in,
                                 s.total_bm_info_noise_low, s.total_bm_coarse_fail, s.total_bm_fine_fail], np.int64))


def _run_ticks(rig, stream, p, ticks, sync_each):
    from esvo_amd import lib
    dev = lib.Esvo(p, rig)
    dev.ts_push_events(0, stream.ev_left)
    dev.ts_push_events(1, stream.ev_right)
    for t, stamps, poses, T in ticks:
        dev.ts_render(0, t, download=False); dev.ts_render(1, t, download=False)
        dev.set_observation(t, None, None, T)
        dev.tick(t, stamps, poses)
        if sync_each:
            dev.synchronize()
    return _result(dev)


def _denoise_setup():
    """(the small sensor of tests/test_gpu_edge.py, whose rpg preset switches Denoising on, over a scene sparse enough for the
    kept events to match: about 3400 of 6800 events kept, 2600 distinct pixels, 800 matches)"""
    from esvo_amd import calib, params, rostime, synth
    rig = calib.ideal_rig(240, 180, 156.925, 0.14805)
    stream = synth.make_stream(rig, 4000, 0.10, 0.2, 2.0, seed=77, speed=1.5)
    p, den = params.make_params(params.PRESETS["mvstereo_rpg"], rig, process_event_num=12000)
    assert den and p.denoising == 1
    t = stream.t0_ns + int(0.07e9)
    stamps, poses = rostime.pose_table(stream.pose, t, p.bm_half_slice_thickness)
    return rig, stream, p, t, stamps, poses


def _denoise_tick():
    from esvo_amd import lib
    rig, stream, p, t, stamps, poses = _denoise_setup()
    dev = lib.Esvo(p, rig)
    for cam in (0, 1):
        dev.ts_push_events(cam, stream.slice(cam, stream.t0_ns, t + 2_000_000))
    dev.ts_render(0, t, download=False); dev.ts_render(1, t, download=False)
    dev.set_observation(t, None, None, stream.pose(t))
    dev.tick(t, stamps, poses)
    dev.synchronize()
    return _result(dev)


def _mapper_scenarios():
    import bench
    rig, stream, p, ticks = bench.make_workload("dsec640x480", N_TICKS, events_cap=EVENTS_CAP)
    return {"pipelined": _run_ticks(rig, stream, p, ticks, False), "synchronised": _run_ticks(rig, stream, p, ticks, True),
            "denoised": _denoise_tick()}


def _scenarios():
    with _shared_env():
        out = {f"match.{k}": v for k, v in _match_scenarios().items()}
        out.update({f"mapper.{k}": v for k, v in _mapper_scenarios().items()})
    return out


def _dump(path):
    flat = {}
    for name, r in _scenarios().items():
        for k, v in r.items():
            flat[f"{name}/{k}"] = v
    np.savez(path, **flat)


@pytest.fixture(scope="module")
def both():
    """(shared, per_event): the scenarios on this process's handles and on ESVO_BM_DEDUPE=0 handles of a child process"""
    shared = _scenarios()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "per_event.npz")
        code = f"import sys; sys.path.insert(0, 'tests'); import test_gpu_bm_dedupe as T; T._dump({path!r})"
        env = dict(os.environ, ESVO_DEV_SWITCHES="1", ESVO_BM_DEDUPE="0")
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        z = np.load(path)
        per_event = {}
        for key in z.files:
            name, k = key.split("/")
            per_event.setdefault(name, {})[k] = z[key]
    return shared, per_event


def _fields(a):
    return {f: np.ascontiguousarray(a[f]).tobytes() for f in a.dtype.names}


def _same_records(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    fa, fb = _fields(a), _fields(b)
    for f in fa:
        assert fa[f] == fb[f], (what, f)


MATCH_CASES = ["n0", "n1", "n7", "n8", "n9", "one_pixel64", "one_pixel65", "distinct", "pool3000", "pool3000_t1", "pairs_t1", "pairs_t4",
               "failures", "failures_t1", "pose_ab", "pose_pool", "pose_short_table"]


@pytest.mark.parametrize("name", MATCH_CASES)
def test_match_stage_changes_no_bit(both, name):
    shared, per_event = both
    a, b = shared[f"match.{name}"], per_event[f"match.{name}"]
    print(name, "shared", a["cnt"], "per event", b["cnt"])
    assert np.array_equal(a["cnt"], b["cnt"]), (a["cnt"], b["cnt"])       # records, last_matches, the three last_bm_* counters
    _same_records(a["rec"], b["rec"], name)


def test_match_cases_are_what_they_claim(both):
    """the crafted lists do share pixels and do fail the ways their names say (else the comparison above shows nothing)"""
    shared, _ = both
    d0 = _world()["d0"]
    cases = _cases()
    for name in ("pool3000", "pairs_t1", "failures", "pose_pool"):
        ev = cases[name][1]
        assert len(np.unique(ev["x"].astype(np.int64) | (ev["y"].astype(np.int64) << 16))) < len(ev), name
    ev = cases["distinct"][1]
    assert len(np.unique(ev["x"].astype(np.int64) | (ev["y"].astype(np.int64) << 16))) == len(ev)
    for n in (64, 65):    # every event of the one pixel matches, at the disparity the pair was built with, in event order
        r = shared[f"match.one_pixel{n}"]["rec"]
        assert len(r) == n and np.all(r["disp"] == d0) and np.array_equal(np.sort(r["event_idx"]), np.arange(n))
        assert len(np.unique(r["pose_idx"])) > 1          # ... each with its own pose
    f = shared["match.failures"]
    assert len(f["rec"]) == 5 and np.all(f["rec"]["disp"] == d0)         # the five events of the one matching pixel
    assert f["cnt"][2] == 5 and f["cnt"][3] == 5 and f["cnt"][4] == 0    # five info-noise failures, five above the threshold
    r = shared["match.pose_ab"]["rec"]    # pixel A: slot 0 has no pose, slot 1 has; pixel B: slot 2 has, slot 3 has none
    assert np.array_equal(r["event_idx"], [1, 2]) and np.array_equal(r["pose_idx"], [2, 3]) and np.all(r["disp"] == d0)
    short, full = shared["match.pose_short_table"]["rec"], shared["match.pool3000"]["rec"]
    assert 0 < len(short) < len(full)


def test_match_stage_against_the_oracle(both):
    """the fields and the tolerance of tests/test_gpu_parity.py's match records: exact against the oracle's integer mode"""
    from esvo_amd import params
    from oracle import oracle as O
    shared, _ = both
    w = _world()
    T, ev, n_st = _cases()["pool3000"]
    p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], w["rig"], num_threads=T, max_events_per_tick=4096)
    m = O.OracleMapper(p, w["rig"])
    m.set_mode(True, True)
    m.set_observation(T0_NS, w["left"], w["right"], np.eye(4))
    m.set_poses(w["stamps"][:n_st], w["poses"][:n_st])
    o, g = m.match(ev), shared["match.pool3000"]["rec"]
    assert len(g) == len(o) and len(g) > 1000, (len(g), len(o))
    for f in ("event_idx", "disp", "pose_idx", "x_left", "inv_depth", "cost"):
        assert np.array_equal(g[f], o[f]), f


def test_no_state_between_calls():
    """the second of two calls on one handle equals the same call on a fresh handle (no owner of an older call survives)"""
    from esvo_amd import lib, params
    w = _world()
    cases = _cases()
    first, second = cases["pool3000"][1], cases["pairs_t4"][1]
    p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], w["rig"], num_threads=4, max_events_per_tick=4096)
    res = []
    with _shared_env():
        for warm in (True, False):
            dev = lib.Esvo(p, w["rig"])
            dev.set_observation(T0_NS, w["left"], w["right"], np.eye(4))
            if warm:
                dev.match(first, w["stamps"], w["poses"])
                dev.match(second[::-1].copy(), w["stamps"], w["poses"])     # the same pixels owned by other slots
            rec = dev.match(second, w["stamps"], w["poses"])
            s = dev.stats()
            res.append((rec.copy(), (s.last_matches, s.last_bm_info_noise_low, s.last_bm_coarse_fail, s.last_bm_fine_fail)))
            # the searches that ran: one per distinct pixel (every event of the list lies inside the image)
            assert dev.debug_bm_owner_count() == len(np.unique(second["x"].astype(np.int64) | (second["y"].astype(np.int64) << 16)))
    assert res[0][1] == res[1][1] and len(res[0][0]) > 100
    _same_records(res[0][0], res[1][0], "second call")


@pytest.mark.parametrize("name", ["pipelined", "synchronised", "denoised"])
def test_mapper_changes_no_bit(both, name):
    shared, per_event = both
    a, b = shared[f"mapper.{name}"], per_event[f"mapper.{name}"]
    print(name, "shared", a["totals"], "per event", b["totals"])
    if name == "denoised":
        assert a["totals"][0] > 100 and len(a["frame"]) > 0
    else:
        assert a["totals"][0] > N_TICKS * 4000 and len(a["map"]) > 1000 and len(a["frame"]) > 1000
    assert np.array_equal(a["totals"], b["totals"]), (a["totals"], b["totals"])
    for what in ("map", "frame"):
        _same_records(a[what], b[what], (name, what))


def test_mapper_scenarios_share_pixels():
    """more events than distinct raw pixels in what the ticks hand to block matching"""
    import bench
    from oracle import oracle as O
    rig, stream, p, ticks = bench.make_workload("dsec640x480", N_TICKS, events_cap=EVENTS_CAP)
    idx = O.select_events(stream.ev_left, ticks[0][0], p.bm_half_slice_thickness, p.process_event_num)
    ev = stream.ev_left[idx]
    distinct = len(np.unique(ev["x"].astype(np.int64) | (ev["y"].astype(np.int64) << 16)))
    assert len(ev) > 40000 and distinct < len(ev), (len(ev), distinct)
    rig, stream, p, t, stamps, poses = _denoise_setup()
    staged = stream.slice(0, stream.t0_ns, t + 2_000_000)
    idx = O.select_events(staged, t, p.bm_half_slice_thickness, p.process_event_num)
    ev = staged[O.denoise_events(staged, idx, rig.width, rig.height, p.process_event_num)]
    distinct = len(np.unique(ev["x"].astype(np.int64) | (ev["y"].astype(np.int64) << 16)))
    assert len(ev) > 200 and distinct < len(ev), (len(ev), distinct)
