"""esvo_ts_history_select against the reference's mapper node: which retained Time-Surface pair dataTransferring observes.

tests/golden/ref_ts_select.npz (tests/golden/make_ts_select_fixture.py) holds, for pushes of all-zero pairs 10 ms apart into
esvo_core/src/esvo_Mapping.cpp's node object, what dataTransferring() returned and the index (push order) of the pair it took:
fewer than eleven pairs, poses missing at the second newest / at several / everywhere but the oldest / everywhere but the
newest, the INITIALIZATION status, and a history trimmed to TS_HISTORY_LENGTH = 100 with the only pose just outside and just
inside what is retained.  The library's rule (host code) must give the same answer on the retained stamps.  Where the
reference tree is present the node is also run live against the fixture.
"""
import os
import sys

import numpy as np
import pytest

from esvo_amd import lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WORKING, INITIALIZATION = 0, 1


def _fixture():
    return np.load(os.path.join(GOLDEN, "ref_ts_select.npz"))


def _cases():
    g = _fixture()
    return list(range(len(g["n"])))


def _select(g, k):
    """the library's choice for case k -> (returned, index in push order or -1, pose or None, stamps the lookup was asked)"""
    n, length = int(g["n"][k]), int(g["history_length"])
    st = g["stamps"][:n]
    first = max(0, n - length)      # timeSurfaceCallback erases the smallest stamps beyond TS_HISTORY_LENGTH (esvo_Mapping.cpp:757-761)
    no_pose = {int(st[i]) for i in np.nonzero(g["no_pose"][k][:n])[0]}
    asked = []
    T_known = np.arange(16, dtype=np.float64).reshape(4, 4) + 1.0

    def pose(t):
        asked.append(int(t))
        return None if int(t) in no_pose else T_known + float(np.nonzero(st == np.uint64(t))[0][0])
    r = lib.ts_history_select(st[first:], pose, initialization=int(g["status"][k]) == INITIALIZATION)
    if r is None:
        return False, -1, None, asked
    return True, first + r[0], r[1], asked


@pytest.mark.parametrize("k", _cases())
def test_select_equals_the_reference_node(k):
    g = _fixture()
    ok, idx, T, asked = _select(g, k)
    assert ok == bool(g["returned"][k]), (k, ok)
    assert idx == int(g["index"][k]), (k, idx, int(g["index"][k]))
    n = int(g["n"][k])
    if int(g["status"][k]) == INITIALIZATION:
        assert asked == [], "poses are not consulted while the system initialises"
        if ok:
            assert np.array_equal(T, np.eye(4))
        return
    st = g["stamps"][:n]
    if n <= 10:
        assert asked == []
        return
    # the walk: from the second newest down, one stamp at a time, never the newest, ending at the stamp it took
    first = max(0, n - int(g["history_length"]))
    last = idx if ok else first
    assert asked == [int(st[i]) for i in range(n - 2, last - 1, -1)], k
    if ok:
        assert np.array_equal(T, np.arange(16, dtype=np.float64).reshape(4, 4) + 1.0 + idx), "the pose of the stamp it took"


def test_the_fixture_holds_the_cases_it_was_asked_for():
    g = _fixture()
    got = [(int(g["n"][k]), int(g["no_pose"][k].sum()), int(g["status"][k]), bool(g["returned"][k]), int(g["index"][k])) for k in _cases()]
    assert got == [(10, 0, 0, False, -1), (11, 0, 0, True, 9), (12, 0, 0, True, 10), (12, 1, 0, True, 9), (12, 3, 0, True, 7),
                   (12, 11, 0, True, 0), (12, 11, 0, False, -1), (12, 12, 0, False, -1), (12, 12, 1, True, 10), (101, 0, 0, True, 99),
                   (105, 1, 0, True, 102), (105, 104, 0, False, -1), (105, 104, 0, True, 5)]
    assert np.array_equal(np.diff(g["stamps"].astype(np.int64)), np.full(len(g["stamps"]) - 1, 10_000_000))


def test_select_argument_errors():
    st = np.arange(1, 13, dtype=np.uint64)
    with pytest.raises(lib.EsvoError) as e:
        lib.ts_history_select(st[::-1].copy(), lambda t: np.eye(4))
    assert e.value.code == lib.ERR_INVALID_ARG
    idx, T = lib.C.c_size_t(0), np.zeros(16)      # a NULL lookup is refused unless the system initialises
    raw = lib.load().esvo_ts_history_select
    assert raw(st.ctypes.data, len(st), 0, lib.EM_POSE_FN(), None, lib.C.byref(idx), T.ctypes.data) == lib.ERR_INVALID_ARG
    assert raw(st.ctypes.data, len(st), 1, lib.EM_POSE_FN(), None, lib.C.byref(idx), T.ctypes.data) == 0 and idx.value == 10
    assert lib.ts_history_select(np.zeros(0, np.uint64), lambda t: np.eye(4)) is None

    def boom(t):
        raise KeyError(t)
    with pytest.raises(KeyError):                 # an exception of the lookup reaches the caller, not the C frames
        lib.ts_history_select(st, boom)


def test_live_reference_node_reproduces_fixture():
    from oracle import ref as R
    if not os.path.isdir(os.path.join(R.REFERENCE, "esvo_core", "src")):
        pytest.skip("reference tree not present (GPU box): the fixtures are the pin")
    sys.path.insert(0, GOLDEN)
    import make_ts_select_fixture as M
    g = _fixture()
    assert len(M.CASES) == len(g["n"])
    for k, (n, missing, status) in enumerate(M.CASES):
        assert (n, status) == (int(g["n"][k]), int(g["status"][k]))
        assert sorted(missing) == [int(i) for i in np.nonzero(g["no_pose"][k])[0]]
        ok, idx = M.run_node(n, missing, status)
        assert (ok, idx) == (bool(g["returned"][k]), int(g["index"][k])), k
