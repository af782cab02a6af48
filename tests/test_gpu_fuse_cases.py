"""The back stage of the device (kernels_fuse.hip: propagate, tile lists, cell walk, clean, regulariser view and apply) on the crafted
cases of tests/fuse_cases.py, at production capacities: no environment switch shrinks a buffer here.  Per case and tick
set_observation (blank Time Surfaces), push_frame, fuse; then, exactly:
  * the fusion count is the oracle's;
  * get_map() equals the oracle's map element by element, in list order, on row, col, age and every f64 field;
  * the map's digest is the one recorded from the reference's own classes (tests/golden/ref_fuse_cases.npz): the device is held
    to the reference directly;
  * the per-cell record counts the tile kernel wrote (esvo_debug_fuse_cell_counts) equal the plan's n cell by cell -- the points
    landed where the case says, so the candidate counts and list lengths ARE the planned ones (tests/test_fuse_cases.py asserts
    what those reach: the four rank widths, the bitonic network, the dense path at P = 1025, the three list sorts, the
    global-memory cell, the overflow list, the record reservation, the length classes 0 to 12).
One oracle run per case serves its variants (ESVO_REG_SPARSE unset / 0 / 1, the row bands)."""
import functools
import os

import numpy as np
import pytest

import fuse_cases as FC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F64 = ["inv_depth", "scale2", "nu", "variance", "residual", "x", "p_cam"]
# Measured once on an MI355X (pytest --durations; the whole test: handle, three ticks of which only the last holds the full lists,
# read-outs, comparisons): the cases with four 3073-record cells, each ordered by one lane in global memory, take 3.6 s
# (lists_first), 3.8 s (lists_mid) and 3.8 s (lists_last); every other test of this file stays below 0.5 s.
DURATION_NOTE = "lists_first 3.6 s, lists_mid 3.8 s, lists_last 3.8 s; all others below 0.5 s"

FRONT = [n for n in FC.NAMES if not n.startswith("reg_")]
REG = [n for n in FC.NAMES if n.startswith("reg_")]


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "ref_fuse_cases.npz"))


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """per tick (fusions, map) of the oracle in the mode the device implements; computed once, read by every variant"""
    from oracle import oracle as O
    c = FC.case(name)
    p, rig = FC.case_params(c)
    m = O.OracleMapper(p, rig)
    m.set_mode(True, True)
    res = FC.run(m, c)
    for _, mp in res:
        mp.setflags(write=False)
    return res


def _same_map(g, o, what):
    assert len(g) == len(o), (what, len(g), len(o))
    for f in ("row", "col", "age"):
        assert np.array_equal(g[f], o[f]), (what, f)
    for f in F64:
        assert np.array_equal(g[f], o[f]), (what, f)


def _device(c, env=None):
    from esvo_amd import lib
    p, rig = FC.case_params(c)
    env = env or {}
    os.environ.update(env)
    try:
        return lib.Esvo(p, rig)   # the switches are read at esvo_create
    finally:
        for k in env:
            del os.environ[k]


def _check_case(name, env=None):
    c = FC.case(name)
    l2 = FC.is_l2(c)
    dev = _device(c, env)
    try:
        res = FC.run(_Counted(dev), c, want_cells=True)
    finally:
        dev.close()
    for k, ((nf, mp, counts), (o_nf, o_mp)) in enumerate(zip(res, oracle_run(name))):
        assert nf == o_nf, (k, nf, o_nf)
        _same_map(mp, o_mp, k)
        assert np.array_equal(FC.map_digest(mp, l2=l2), FC.recorded(golden(), name, k)["map_sha"]), k
        n = FC.plan(FC.window(c, k), c["over"]["fusion_radius"], c["W"], c["H"])["n"]
        assert np.array_equal(counts, n), (k, np.argwhere(counts != n)[:8])


class _Counted:
    """a device handle whose get_map_cells() is the tile kernel's per-cell record counts of the fusion just run"""

    def __init__(self, dev):
        self.dev = dev

    def __getattr__(self, a):
        return getattr(self.dev, a)

    def get_map_cells(self):
        return self.dev.debug_fuse_cell_counts()


@pytest.mark.parametrize("name", FRONT)
def test_fusion_front_and_clean_on_crafted_frames(name):
    _check_case(name)


@pytest.mark.parametrize("sparse", [None, "0", "1"], ids=["auto", "dense", "sparse"])
@pytest.mark.parametrize("name", REG)
def test_regulariser_on_the_crafted_map(name, sparse):
    """every instance of reg_apply_kernel -- <5>, <20> and <0> (radii 1, 12, 31), each in the dense and in the sparse layout --
    and reg_apply_l2_kernel (which has one layout: the switch must not matter)"""
    _check_case(name, None if sparse is None else {"ESVO_REG_SPARSE": sparse})


@pytest.mark.parametrize("name,edges", [("cand_p1025_r1", (0, 44, 100)), ("cand_p1025_r1", (0, 41, 46, 100)),
                                        ("reg_r20", (0, 8, 73, 100)), ("reg_r20", (0, 50, 100))])
def test_row_bands_merge_to_the_whole_map(name, edges):
    """The same frames pushed to two or three handles after set_band: the band edges cut through the dense tile (rows 40..47) and
    between the rows of displaced pairs (7 | 8, 72 | 73); the bands' maps merge to the oracle's, and every handle's tile kernel
    counted its own rows as planned."""
    from esvo_amd import dist
    c = FC.case(name)
    devs = [_device(c) for _ in edges[1:]]
    try:
        for g, (d, y0, y1) in enumerate(zip(devs, edges[:-1], edges[1:])):
            d.set_band(y0, y1, g, len(devs))
        runs = [FC.run(_Counted(d), c, want_cells=True) for d in devs]
    finally:
        for d in devs:
            d.close()
    for k, (o_nf, o_mp) in enumerate(oracle_run(name)):
        merged = dist.merge_band_maps([r[k][1] for r in runs])
        _same_map(merged, o_mp, k)
        n = FC.plan(FC.window(c, k), c["over"]["fusion_radius"], c["W"], c["H"])["n"]
        for r, y0, y1 in zip(runs, edges[:-1], edges[1:]):
            assert np.array_equal(r[k][2][y0:y1], n[y0:y1]), (k, y0, y1)
