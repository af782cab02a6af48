"""Records tests/golden/ref_ts_select.npz: which retained Time-Surface pair the reference's mapper node observes.

The node object (oracle/ref.py: RefNode = esvo_core/src/esvo_Mapping.cpp compiled as it is) receives n all-zero pairs
10 ms apart through timeSurfaceCallback; its pose lookup knows no pose for the chosen pushes; dataTransferring() then
picks TS_obs_ (esvo_Mapping.cpp:497-534).  Recorded per case: what it returned and the index, in push order, of the pair
it observed (-1: none).  Only stamps and indices are stored.  Needs the reference tree:

    python tests/golden/make_ts_select_fixture.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

W, H, FOCAL, BASELINE = 64, 48, 50.0, 0.1
T0_NS, STEP_NS = 1_000_000_000, 10_000_000
WORKING, INITIALIZATION = 0, 1
STATUS_NAMES = {WORKING: "WORKING", INITIALIZATION: "INITIALIZATION"}

# (pairs pushed, pushes without a pose, status)
CASES = [
    (10, [], WORKING),
    (11, [], WORKING),
    (12, [], WORKING),
    (12, [10], WORKING),
    (12, [10, 9, 8], WORKING),
    (12, list(range(1, 12)), WORKING),                   # all but the oldest
    (12, list(range(0, 11)), WORKING),                   # all but the newest: the newest is never taken
    (12, list(range(12)), WORKING),
    (12, list(range(12)), INITIALIZATION),               # identity pose, poses not consulted
    (101, [], WORKING),                                  # the history is trimmed to 100
    (105, [103], WORKING),
    (105, [i for i in range(105) if i != 4], WORKING),   # only push 4 has a pose: it is evicted
    (105, [i for i in range(105) if i != 5], WORKING),   # only push 5 has a pose: the oldest retained
]


def stamps(n):
    return T0_NS + STEP_NS * np.arange(n, dtype=np.uint64)


def run_node(n, missing, status):
    """(returned, index in push order or -1) from the reference's node"""
    from esvo_amd import calib, params
    from oracle import ref as R
    rig = calib.ideal_rig(W, H, FOCAL, BASELINE)
    p, _ = params.make_params(params.PRESETS["mapping_upenn"], rig)
    st = stamps(n)
    no_pose = {int(st[i]) for i in missing}
    node = R.RefNode(p, rig, lambda t: None if int(t) in no_pose else np.eye(4))
    img = np.zeros((H, W), np.uint8)
    for t in st:
        node.push_time_surfaces(int(t), img, img)
    node.set_status(STATUS_NAMES[status])
    ok = node.data_transferring()
    t_obs = node.obs_time()
    where = np.nonzero(st == np.uint64(t_obs))[0]
    return bool(ok), (int(where[0]) if len(where) else -1)


def main():
    n_max = max(c[0] for c in CASES)
    n = np.array([c[0] for c in CASES], np.int64)
    no_pose = np.zeros((len(CASES), n_max), np.uint8)
    status = np.array([c[2] for c in CASES], np.int64)
    returned, index = np.zeros(len(CASES), np.uint8), np.zeros(len(CASES), np.int64)
    for k, (nk, missing, s) in enumerate(CASES):
        no_pose[k, missing] = 1
        ok, idx = run_node(nk, missing, s)
        returned[k], index[k] = ok, idx
        print(f"n={nk:4d} without a pose: {len(missing):4d} {STATUS_NAMES[s]:15s} -> returned {ok}, index {idx}")
    np.savez_compressed(os.path.join(HERE, "ref_ts_select.npz"), n=n, no_pose=no_pose, status=status, returned=returned, index=index,
                        stamps=stamps(n_max), history_length=np.int64(100))


if __name__ == "__main__":
    main()
