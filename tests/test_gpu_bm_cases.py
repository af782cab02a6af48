"""Block matching on the crafted events of tests/bm_cases.py (kernels_bm.hip through esvo_map_match), held to the CPU oracle's
exact-integer mode bit for bit: every field of every record (event_idx, pose_idx, disp, x_left, inv_depth, cost), the record count,
last_matches and the three last_bm_* failure counters.  What the cases reach, and that they reach it, is tested on the CPU
(tests/test_bm_cases.py).

Three paths: the one a default handle takes (every case, all patch sizes); handles created under ESVO_BM_DEDUPE_MIN=1, where every
launch runs one search per distinct raw pixel (the 15 x 7 cases; the searches that ran are counted); and one fresh child process
under ESVO_BM_DEDUPE=0 (one search per event: the switches are read at create), whose results for the 15 x 7 cases come back in
a file.  Cases that share an image size, a rig and a patch size share a handle: the other parameters change with
esvo_set_params.

What the module notices (scratch builds of kernels_bm.hip with one comparison flipped or one constant dropped, none of which can
move an address; the cases that turned red, and whether the older block-matching tests -- test_gpu_bm_dedupe, _ref, _parity,
_edge, _fuzz -- noticed):
  the lane's scan `cost <= best` -> `<`         tie_trips, tie_trips64; general kernel: any5x5_tie_trips            older: none
  grp_argmin `od > bestd` -> `<`               every tie_*, ud_tie*, coarse_tie, the *_up cases, any1x1, any5x5_tie   older: 2 tests
  `cnt > 0.95 N` -> `>=`                       general kernel: any5x4_noise, any10x4_noise, any10x10_noise            older: none
                                               (15 x 7: 0.95 x 105 = 99.75 is no integer -- the same function, nothing can notice)
  event gate `x1 + hx >= W - 1` -> `>`         gates, none_valid                                                      older: 30 tests
  `best < zncc_thr` -> `<=`                    flat_left, flat_right, flat_both, all255, thr_eq, ud_thr_eq;
                                               coarse pass: coarse_thr_eq; general kernel: any*_all255, any5x5_thr_eq older: none
  `& 0x00ffffff` dropped, left rows            186 tests: every case that matches on a texture                       older: 59 tests
  `& 0x00ffffff` dropped, candidate rows       171 tests                                                              older: 57 tests
  coarse neighbours' `< 1.0` removed           coarse2, coarse3, coarse4; general kernel: any*_coarse_border          older: 8 tests"""
import copy
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import bm_cases as BC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("event_idx", "pose_idx", "disp", "x_left", "inv_depth", "cost")


class _shared_env:
    """handles created inside take the shared path from one event on"""

    def __enter__(self):
        self.old = os.environ.get("ESVO_BM_DEDUPE_MIN")
        os.environ["ESVO_BM_DEDUPE_MIN"] = "1"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("ESVO_BM_DEDUPE_MIN", None)
        else:
            os.environ["ESVO_BM_DEDUPE_MIN"] = self.old


_HANDLES = {}


def _handle(c, shared):
    """the handle of a case's image size, rig and patch size on one path, under the case's parameters"""
    from esvo_amd import lib
    p = BC.case_params(c)
    key = (shared, c["W"], c["H"], id(c["rig"]), p.patch_size_x, p.patch_size_y)
    if key not in _HANDLES:
        if shared:
            with _shared_env():
                _HANDLES[key] = lib.Esvo(p, c["rig"])
        else:
            _HANDLES[key] = lib.Esvo(p, c["rig"])
    else:
        _HANDLES[key].set_params(copy.copy(p))
    return _HANDLES[key]


def run(name, shared=False):
    """(records, [record count, last_matches, last_bm_info_noise_low, last_bm_coarse_fail, last_bm_fine_fail], searches that ran
    once per pixel or None) of a case on the device"""
    c = BC.case(name)
    dev = _handle(c, shared)
    dev.set_observation(BC.T0_NS, c["left"], c["right"], np.eye(4))
    rec = dev.match(c["events"], c["stamps"], c["poses"])
    s = dev.stats()
    cnt = np.array([len(rec), s.last_matches, s.last_bm_info_noise_low, s.last_bm_coarse_fail, s.last_bm_fine_fail], np.int64)
    return rec.copy(), cnt, dev.debug_bm_owner_count()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's integer mode on a case: (records, the same five counts)"""
    c = BC.case(name)
    m = BC.oracle_for(c)
    rec = m.match(c["events"])
    return rec, np.array([len(rec), len(rec)] + list(m.bm_fail_counts()), np.int64)


def same(name, rec, cnt, what):
    exp, exp_cnt = expected(name)
    print(name, what, "device", cnt, "oracle", exp_cnt)
    assert np.array_equal(cnt, exp_cnt), (what, cnt, exp_cnt)
    for f in FIELDS:
        assert np.ascontiguousarray(rec[f]).tobytes() == np.ascontiguousarray(exp[f]).tobytes(), (what, f, rec[f], exp[f])


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for dev in _HANDLES.values():
        dev.close()
    _HANDLES.clear()


def _dump(path):
    """(the child process) every 15 x 7 case on this process's handles"""
    flat = {}
    for name in BC.REG_15x7:
        rec, cnt, owners = run(name)
        assert owners is None, "the child runs one search per event"
        flat[f"{name}/rec"], flat[f"{name}/cnt"] = rec, cnt
    np.savez(path, **flat)


@pytest.fixture(scope="module")
def per_event():
    """the 15 x 7 cases on ESVO_BM_DEDUPE=0 handles of one fresh child process"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "per_event.npz")
        code = f"import sys; sys.path.insert(0, 'tests'); import test_gpu_bm_cases as T; T._dump({path!r})"
        env = dict(os.environ, ESVO_DEV_SWITCHES="1", ESVO_BM_DEDUPE="0")
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        z = np.load(path)
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", BC.NAMES)
def test_default_handle_equals_the_oracle(name):
    rec, cnt, _ = run(name)
    same(name, rec, cnt, "default handle")


@pytest.mark.parametrize("name", BC.REG_15x7)
def test_one_search_per_pixel_equals_the_oracle(name):
    rec, cnt, owners = run(name, shared=True)
    e = BC.case(name)["events"]
    inside = (e["x"] < BC.case(name)["W"]) & (e["y"] < BC.case(name)["H"])
    pixels = len(np.unique(e["x"][inside].astype(np.int64) | (e["y"][inside].astype(np.int64) << 16)))
    assert owners == pixels + int((~inside).sum()), (owners, pixels)     # the shared path ran: one search per distinct pixel
    same(name, rec, cnt, "one search per pixel")


@pytest.mark.parametrize("name", BC.REG_15x7)
def test_one_search_per_event_equals_the_oracle(name, per_event):
    same(name, per_event[f"{name}/rec"], per_event[f"{name}/cnt"], "one search per event (child process)")
