"""The crafted back-stage cases (tests/fuse_cases.py) on the CPU: each case meets the targets its plan was written for, its frames
are the ones the fixture was recorded on, and the oracle -- in literal and in canonical mode -- reproduces what the reference's
own DepthFusion, SmartGrid::clean and DepthRegularization made of them (tests/golden/ref_fuse_cases.npz, recorded by
tests/golden/make_ref_fixtures.py --fuse-cases): fusion count, map length and the digest of every element with its true cell,
tick by tick, exactly.  Where oracle/_ref is present the reference is run live against the fixture.  The device side:
tests/test_gpu_fuse_cases.py."""
import copy
import os

import numpy as np
import pytest

import fuse_cases as FC
from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ref_fuse_cases.npz"))


def _neighbours(t, shape):
    return [(t[0] + dy, t[1] + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dy, dx) != (0, 0) and 0 <= t[0] + dy < shape[0] and 0 <= t[1] + dx < shape[1]]


def check_targets(c):
    """the plan of the case's last window against the targets the case states"""
    T = c["targets"]
    radius = c["over"]["fusion_radius"]
    last = len(c["frames"]) - 1
    pl = FC.plan(FC.window(c, last), radius, c["W"], c["H"])
    P, own, rec, n = pl["P"], pl["own"], pl["records"], pl["n"]
    if "P" in T:   # candidate counts
        t = T["tile"]
        assert P[t] == T["P"] and FC.rank_path(int(P[t])) == T["path"]
        assert 1 <= own[t] and (own[t] < P[t] or T["P"] == 1)          # the rest comes from the neighbours' rims ...
        assert all(own[nb] >= 3 for nb in _neighbours(t, own.shape))    # ... which also hold points that do not reach
        assert len(c["frames"]) == 3 and all(len(f) for f in c["frames"])
    if "n_values" in T:   # list lengths on the dense path
        t = T["tile"]
        cells = FC.tile_cells(n, *t)
        assert FC.rank_path(int(P[t])) == "dense" and rec[t] > FC.TILE_REC
        assert set(T["n_values"]) <= set(cells.tolist()) and cells[T["big_local"]] == 3073 == cells.max()
        assert {FC.sort_path(int(v)) for v in cells if v} == {"none", "insertion", "wave", "lane", "global"}
        busy = np.flatnonzero(cells)
        assert (cells[busy[0]:busy[-1]] == 0).any()                     # an empty cell between two busy ones
    if "overflow" in T:
        for t in T["overflow"]:
            assert own[t] > FC.TILE_CAP
            assert any(own[nb] < P[nb] <= FC.FUSE_PMAX for nb in _neighbours(t, own.shape))   # a fast-path tile reading its rim
        t = T["ordinary"]
        assert 0 < own[t] <= P[t] <= 64
        assert all(abs(t[0] - o[0]) > 1 or abs(t[1] - o[1]) > 1 for o in T["overflow"])
    if "region" in T:
        for t in T["region"]:
            assert rec[t] > FC.TILE_REC and P[t] <= FC.FUSE_PMAX
    if "classes" in T:
        tiles_x = own.shape[1]
        num = [t[0] * tiles_x + t[1] for t in T["classes"]]
        assert num[0] % 64 == num[1] % 64 != num[2] % 64
        for t in T["classes"]:
            cells = FC.tile_cells(n, *t)
            assert {FC.length_class(int(v)) for v in cells if v} == set(range(13))
    if "filled" in T:
        t = T["filled"]
        assert own[t] == FC.TILE_CAP
        assert sum(int((f["row"] == FC.REJECT).sum()) for f in c["frames"]) == T["rejected"]
        assert own[:, -1].sum() > 0 and own[-1, :].sum() > 0 and c["W"] % FC.FT and c["H"] % FC.FT   # partial tiles
        assert all(n[r, cc] > 0 for r in (0, c["H"] - 1) for cc in (0, c["W"] - 1))
    if "single_cells" in T:
        first = FC.plan(FC.window(c, 0), radius, c["W"], c["H"])["n"]
        assert all(first[r, cc] == 1 for r, cc in T["single_cells"])


@pytest.mark.parametrize("name", FC.NAMES)
def test_case_meets_its_plan(name):
    c = FC.case(name)
    _, rig = FC.case_params(c)
    for k, f in enumerate(c["frames"]):   # the propagation puts every point on its intended cell, or rejects it
        row, col = FC.landing(rig, f)
        assert np.array_equal(row, f["row"]) and np.array_equal(col, f["col"]), k
    check_targets(c)


def test_plan_on_a_hand_computed_window():
    rig = FC.rig()
    pts = FC.points_at(rig, [8, 0, 99, 47], [8, 0, 155, 79], 0.1, 1e-4, 5.0, 1, 4.0)
    rej = pts[:1].copy()
    rej["row"], rej["col"] = FC.REJECT, FC.REJECT
    for radius, n_cells in ((0, (4, 4, 1, 4)), (1, (9, 4, 4, 9))):
        pl = FC.plan([pts[:2], np.concatenate([pts[2:], rej])], radius, rig.width, rig.height)
        assert pl["n"].sum() == sum(n_cells) and pl["n"].max() == 1
        assert pl["own"][1, 1] == pl["own"][0, 0] == pl["own"][12, 19] == pl["own"][5, 9] == 1 and pl["own"].sum() == 4
        # (8, 8) is the first cell of tile (1, 1): radius 1 reaches the three tiles above and left of it as well
        assert pl["P"][1, 1] == 1 and pl["P"][0, 0] == (2 if radius else 1) and pl["P"][0, 1] == pl["P"][1, 0] == (1 if radius else 0)
        # (47, 79), the last cell of tile (5, 9), reaches right and below with either footprint
        assert pl["P"][5, 10] == pl["P"][6, 9] == pl["P"][6, 10] == 1
        assert pl["records"][1, 1] == (4 if radius else 4) and pl["records"][0, 0] == (4 + (1 if radius else 0))
    assert [FC.rank_path(p) for p in FC.CAND_P] == ["rank1", "rank1", "rank2", "rank2", "rank4", "rank4", "rank8", "rank8", "bitonic",
                                                   "bitonic", "dense"]
    assert [FC.sort_path(v) for v in FC.LIST_N] == ["none", "insertion", "insertion", "wave", "wave", "lane", "lane", "global"]
    assert [FC.length_class(v) for v in (1, 2, 3, 4, 5, 8, 9, 2049, 4096, 4097)] == [0, 1, 2, 2, 3, 3, 4, 12, 12, 13]


@pytest.mark.parametrize("name", FC.NAMES)
def test_frames_are_the_ones_the_fixture_was_recorded_on(name, golden):
    c = FC.case(name)
    assert FC.recorded(golden, name) == len(c["frames"])
    for k, f in enumerate(c["frames"]):
        assert np.array_equal(FC.frame_digest(f), FC.recorded(golden, name, k)["frame_sha"]), f"the generator of {name} drifted: frame {k}"


def check_against_fixture(name, res, golden):
    """per tick (fusions, map, true cells) of a run against the recorded reference"""
    l2 = FC.is_l2(FC.case(name))
    for k, (nf, mp, cells) in enumerate(res):
        ref = FC.recorded(golden, name, k)
        assert nf == ref["nf"], (k, nf, ref["nf"])
        assert len(mp) == ref["map_n"], (k, len(mp), ref["map_n"])
        assert np.array_equal(FC.map_digest(mp, l2=l2), ref["map_sha"]), k
        assert np.array_equal(FC.map_digest(mp, cells, l2=l2), ref["map_cells_sha"]), k


@pytest.mark.parametrize("canonical", [False, True], ids=["literal", "canonical"])
@pytest.mark.parametrize("name", FC.NAMES)
def test_oracle_equals_the_reference_on_the_crafted_cases(name, canonical, golden):
    c = FC.case(name)
    p, rig = FC.case_params(c)
    m = O.OracleMapper(p, rig)
    m.set_mode(canonical, canonical)
    res = FC.run(m, c, want_cells=True)
    check_against_fixture(name, res, golden)
    e, cnt = c["expect"], m.counters()
    if "nf" in e:   # the state-machine sequences: the branch order they were written for
        assert (res[0][0], cnt["replace"], cnt["replace_displaced"], len(res[0][1])) == (e["nf"], e["replace"], e["replace_displaced"], e["map_n"])
    if e.get("dangling"):
        assert FC.recorded(golden, name, len(res) - 1)["dangling"] > 0 and cnt["replace_displaced"] > 0
    if not FC.is_l2(c):   # the digest is test_ref_pin's
        from test_ref_pin import map_sha
        assert np.array_equal(map_sha(res[0][1], res[0][2]), FC.map_digest(res[0][1], res[0][2]))


@pytest.mark.parametrize("name", FC.NAMES)
def test_live_reference_reproduces_the_crafted_fixture(name, golden):
    from oracle import ref as R
    if not os.path.isdir(os.path.join(R.REFERENCE, "esvo_core", "src")):
        pytest.skip("reference tree not present (GPU box): the fixture is the pin")
    import sys
    sys.path.insert(0, GOLDEN)
    import make_ref_fixtures as mk
    res = mk.run_fuse_case(FC.case(name))
    check_against_fixture(name, [r[:3] for r in res], golden)
    assert [r[3] for r in res] == [FC.recorded(golden, name, k)["dangling"] for k in range(len(res))]


@pytest.mark.parametrize("radius,l2", [(R, False) for R in FC.REG_RADII] + [(R, True) for R in FC.REG_L2_RADII])
def test_regulariser_map_sits_on_its_switch_points(radius, l2):
    """The regulariser map at tick 1 (one frame, clean skipped), un-regularised, under a restatement of the two counts: it holds
    scanned elements with exactly RegularizationMinNeighbours neighbours and with one more (close count above its threshold, so
    the strict > decides), the same for RegularizationMinCloseNeighbours, taps at exactly 2 sigma, taps close by one side's sigma
    only, elements with row or col below the radius, displaced elements across the regulariser's tile seams, several elements
    believing one cell (the regularised map is shorter), the extreme scales and nu, and elements that are alive but not valid."""
    c = FC.case(f"reg_l2_r{radius}" if l2 else f"reg_r{radius}")
    p, rig = FC.case_params(c)
    W, H = rig.width, rig.height
    one = dict(c, frames=c["frames"][:1])
    p0 = copy.copy(p)
    p0.regularization = 0
    (_, mp, cells), = FC.run(O.OracleMapper(p0, rig), one, want_cells=True)
    (_, mp_reg, _), = FC.run(O.OracleMapper(p, rig), one, want_cells=True)
    assert len(mp_reg) < len(mp)                                       # several elements believed one cell
    k = FC.reg_counts(mp, cells, W, H, radius)
    nb, close = k["nb"], k["close"]
    N, C = p.reg_min_neighbours, p.reg_min_close_neighbours
    for v in (N, N + 1):
        assert ((nb == v) & (close > C)).any(), ("neighbours", v)
    for v in (C, C + 1):
        assert ((close == v) & (nb > N)).any(), ("close neighbours", v)
    assert k["at_edge"].max() > 0 and k["own_only"].max() > 0 and k["nb_only"].max() > 0
    # both outcomes occur among the scanned elements
    kept = (nb > N) & (close > C)
    assert kept.any() and ((nb >= 0) & ~kept).any()
    # a count that is never kept decides nothing: among the elements that ARE kept, some have a tap at exactly 2 sigma, equal
    # inverse depths in a row (a2 = +0), a far point, and close neighbours with scales on either side of the fast-division window
    # and with extreme nu
    for key in ("at_edge", "same_depth", "far") + (() if l2 else ("tiny", "huge", "nu_low", "nu_high")):
        assert (kept & (k[key] > 0)).any(), key
    row, col = mp["row"].astype(np.int64), mp["col"].astype(np.int64)
    t_row, t_col = np.asarray(cells, np.int64) // W, np.asarray(cells, np.int64) % W
    valid = mp["inv_depth"] > -1e-6
    for v in (radius - 1, radius):
        assert (valid & (row == v)).any() and (valid & (col == v)).any()
    assert (row == H - 1).any() and (col == W - 1).any()
    # displaced elements: true cell and believed cell on either side of a tile seam, both ways, and in the partial tile
    for a, b in ((63, 64), (64, 63), (127, 128), (128, 127)):
        assert ((t_col == a) & (col == b)).any(), (a, b)
    for a, b in ((7, 8), (8, 7)):
        assert ((t_row == a) & (row == b)).any(), (a, b)
    for d in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        assert ((row - t_row == d[0]) & (col - t_col == d[1])).any(), d
    assert ((t_col >= 128) & ((row != t_row) | (col != t_col))).any()
    if not l2:
        s2 = mp["scale2"]
        assert (s2 < 2.0 ** -332).any() and ((s2 > 2.0 ** -332) & (s2 < 1e-90)).any() and (s2 >= 2.0 ** 333).any() and ((s2 > 1e90) & (s2 < 2.0 ** 333)).any()
        assert (mp["nu"] < 2.1).any() and (mp["nu"] > 1e5).any()
    assert (valid & (mp["inv_depth"] < 1e-300)).any() and (~valid).any()
    assert (valid & (mp["variance"] > p.stdvar_vis_threshold ** 2)).any() and (valid & (mp["age"] < p.age_vis_threshold)).any()
    # neighbours with identical inverse depth (a2 = +0): two different cells, same bits
    u, cnt = np.unique(mp["inv_depth"][valid], return_counts=True)
    assert cnt.max() > 9
