"""Known answers for the restated reprojection map (tests/reproj_restated.py) on a 16 x 12 image: the sprite, the overlap
order, clipping at the border, truncation toward zero, the clamped colour index and the skipped points."""
import os

import numpy as np

import reproj_restated as RR

W, H = 16, 12
# x = 10 X / Z + 8, y = 10 Y / Z + 6
P = np.array([[10.0, 0.0, 8.0, 0.0], [0.0, 10.0, 6.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
JET = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jet256.npy")).reshape(256, 3)
NEG = (np.arange(W * H, dtype=np.uint32) * 7 % 251).astype(np.uint8).reshape(H, W)
GREY = np.repeat(NEG[:, :, None], 3, axis=2)
I3, Z3 = np.eye(3), np.zeros(3)


def at(x, y, z):
    """the reference point of depth z that the identity motion projects to (x, y)"""
    return [(x - 8.0) * z / 10.0, (y - 6.0) * z / 10.0, z]


def draw(pts, inv_min=0.0, inv_max=1.0, n=None, R=I3, t=Z3):
    pts = np.array(pts, np.float64).reshape(-1, 3)
    return RR.reprojection_map(NEG, pts, R, t, P, len(pts) if n is None else n, inv_min, inv_max, JET)


def painted(img):
    """{(x, y): colour} of the pixels that differ from the grey base"""
    ys, xs = np.nonzero((img != GREY).any(axis=2))
    return {(int(x), int(y)): tuple(int(c) for c in img[y, x]) for x, y in zip(xs, ys)}


def col(index):
    return tuple(int(c) for c in JET[index])


def test_jet_fixture_has_distinct_neighbours_for_these_cases():
    assert JET.shape == (256, 3) and JET.dtype == np.uint8
    assert len({col(0), col(63), col(127), col(255)}) == 4
    # the base image never equals the colours used below at the pixels they land on (else `painted` would miss a pixel)
    for c in (col(0), col(63), col(127), col(255)):
        assert not ((GREY == np.array(c, np.uint8)).all(axis=2)).any()


def test_one_point_is_the_five_pixel_plus():
    img, n_in = draw([at(5.3, 4.7, 2.0)])                    # val = 0.5: floor(0.5 * 255) = 127
    assert RR.color_index(2.0, 0.0, 1.0) == 127
    assert painted(img) == {q: col(127) for q in ((5, 4), (4, 4), (6, 4), (5, 3), (5, 5))}
    assert n_in == 1 and img.dtype == np.uint8 and img.shape == (H, W, 3)
    img0, n0 = draw([at(5.3, 4.7, 2.0)], n=0)                # n = 0: the grey image
    assert np.array_equal(img0, GREY) and n0 == 0
    assert np.array_equal(draw([at(5.3, 4.7, 2.0)], n=7)[0], img)   # n beyond the reference is clamped


def test_later_point_wins_the_overlap():
    a, b = at(5.5, 4.5, 2.0), at(6.5, 4.5, 4.0)              # indices 127 and floor(63.75) = 63, centres (5, 4) and (6, 4)
    assert RR.color_index(4.0, 0.0, 1.0) == 63
    ab, n_ab = draw([a, b])
    ba, n_ba = draw([b, a])
    assert n_ab == n_ba == 2
    only_a = {(4, 4): col(127), (5, 3): col(127), (5, 5): col(127)}
    only_b = {(7, 4): col(63), (6, 3): col(63), (6, 5): col(63)}
    assert painted(ab) == {**only_a, **only_b, (5, 4): col(63), (6, 4): col(63)}
    assert painted(ba) == {**only_a, **only_b, (5, 4): col(127), (6, 4): col(127)}
    assert not np.array_equal(ab, ba)


def test_centre_one_pixel_outside_paints_one_arm():
    img, n_in = draw([at(-1.5, 5.5, 2.0)])                   # (int)-1.5 = -1
    assert painted(img) == {(0, 5): col(127)} and n_in == 0
    img, n_in = draw([at(16.5, 5.5, 2.0)])                   # column W
    assert painted(img) == {(15, 5): col(127)} and n_in == 0
    img, n_in = draw([at(3.5, -1.5, 2.0), at(3.5, 12.5, 2.0)])
    assert painted(img) == {(3, 0): col(127), (3, 11): col(127)} and n_in == 0
    img, n_in = draw([at(-2.5, 5.5, 2.0), at(40.5, 70.5, 2.0)])   # two or more pixels outside: nothing
    assert painted(img) == {} and n_in == 0


def test_truncation_toward_zero():
    img, n_in = draw([at(-0.6, 5.5, 2.0)])                   # (int)-0.6 = 0, not floor's -1
    assert painted(img) == {q: col(127) for q in ((0, 5), (1, 5), (0, 4), (0, 6))} and n_in == 1
    img, n_in = draw([at(7.5, -0.9, 2.0)])
    assert painted(img) == {q: col(127) for q in ((7, 0), (6, 0), (8, 0), (7, 1))} and n_in == 1


def test_index_is_clamped_to_the_table():
    img, n_in = draw([at(5.5, 4.5, 10.0)], inv_min=0.2, inv_max=1.0)    # val = 0.1 below the range
    assert set(painted(img).values()) == {col(0)} and n_in == 1
    img, n_in = draw([at(5.5, 4.5, 0.5)], inv_min=0.2, inv_max=1.0)     # val = 2 above it
    assert set(painted(img).values()) == {col(255)} and n_in == 1
    assert RR.color_index(1e-300, 0.2, 1.0) == 255 and RR.color_index(-1e-300, 0.2, 1.0) == 0   # far beyond any int
    assert RR.color_index(0.0, 0.2, 1.0) == 255                         # 1 / 0 = +inf: clamped, not skipped
    assert RR.color_index(float("nan"), 0.2, 1.0) is None


def test_points_without_a_pixel_are_skipped():
    # warped z = 0 with a reference z of 2: t = (0, 0, 2) gives T_left_ref[2, 3] = -2, hm[2] = 0, x = +-inf or NaN
    t = np.array([0.0, 0.0, 2.0])
    assert RR.pose_left_ref(I3, t)[2, 3] == -2.0
    img, n_in = draw([[0.3, 0.2, 2.0], [0.0, 0.0, 2.0]], t=t)
    assert painted(img) == {} and n_in == 0
    # a NaN depth, and a coordinate of magnitude >= 2^30
    img, n_in = draw([[0.0, 0.0, float("nan")], at(2.0**30 + 8.0, 5.5, 1.0), at(5.5, -(2.0**31), 1.0)])
    assert painted(img) == {} and n_in == 0
    # behind the camera the reference still draws whatever world2Cam returns: (x, y) mirrored through the principal point
    img, n_in = draw([[0.5, 0.3, -2.0]], inv_min=0.2, inv_max=1.0)     # x = 8 - 2.5, y = 6 - 1.5; val = -0.5: index 0
    assert painted(img) == {q: col(0) for q in ((5, 4), (4, 4), (6, 4), (5, 3), (5, 5))} and n_in == 1
    # a skipped point between two drawn ones changes nothing
    a, b = at(5.5, 4.5, 2.0), at(9.5, 8.5, 4.0)
    with_skip, n_skip = draw([a, [0.0, 0.0, float("nan")], b])
    without, n_without = draw([a, b])
    assert np.array_equal(with_skip, without) and n_skip == n_without == 2


def test_motion_and_reference_frame():
    # the colour comes from z in the REFERENCE frame, the pixel from the warped point
    t = np.array([0.0, 0.0, -2.0])                           # p_left = p + (0, 0, 2)
    img, n_in = draw([[-0.5, -0.25, 2.0]], t=t)              # warped z = 4: x = 8 - 1.25, y = 6 - 0.625
    assert painted(img) == {q: col(127) for q in ((6, 5), (5, 5), (7, 5), (6, 4), (6, 6))} and n_in == 1
    # setProblem's line with T_world_ref = I widens the f32 input and nothing else
    xyz = np.array([[0.1, -0.2, 1.7], [3.0, 2.0, -1.0]], np.float32)
    assert RR.reference_points(xyz, np.eye(4)).tobytes() == xyz.astype(np.float64).tobytes()
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [1.0, 2.0, 3.0]
    want = (T[:3, :3].T @ (xyz.astype(np.float64) - T[:3, 3]).T).T
    assert np.array_equal(RR.reference_points(xyz, T), want)  # (a signed permutation: no rounding in either order)


def test_crafted_gpu_inputs_have_power():
    """the inputs of tests/test_gpu_track_reproj.py's crafted parity: enough painted pixels, an order-dependent image, every kind of
    point present -- checked here, where no GPU is needed"""
    import reproj_cases as RC
    from esvo_amd import calib
    for w, h in ((96, 64), (95, 63)):
        rig = calib.ideal_rig(w, h, RC.FOCAL, 0.1)
        Pm = np.asarray(rig.left.P, np.float64).reshape(3, 4)
        xyz = RC.crafted(w, h, Pm)
        assert xyz.dtype == np.float32 and 350 <= len(xyz) <= 450
        pts = RR.reference_points(xyz, np.eye(4))
        neg = np.random.default_rng(w).integers(0, 256, (h, w)).astype(np.uint8)
        RC.check_power(neg, pts, Pm)
        for name, (R, t) in RC.MOTIONS.items():
            xy = np.array([RR.project(q, RR.pose_left_ref(R, t), Pm) for q in pts])
            with np.errstate(invalid="ignore"):
                cx, cy = np.trunc(xy[:, 0]), np.trunc(xy[:, 1])
            for want in ((cx == -1) & (cy >= 0) & (cy < h), (cx == w) & (cy >= 0) & (cy < h), (cy == -1) & (cx >= 0) & (cx < w),
                         (cy == h) & (cx >= 0) & (cx < w), (xy[:, 0] > -1) & (xy[:, 0] < 0), (xy[:, 1] > -1) & (xy[:, 1] < 0),
                         cx == 0, cx == w - 1, cy == 0, cy == h - 1, ~np.isfinite(xy[:, 0])):
                assert want.sum() >= 1
            if name == "identity":                                     # (the tiny depths are tiny under the identity only)
                assert (np.abs(xy[:, 0]) >= 2.0**30).sum() >= 1 and (np.abs(xy[:, 1]) >= 2.0**30).sum() >= 1
                assert ((np.abs(xy[:, 0]) > 1e8) & (np.abs(xy[:, 0]) < 2.0**30)).sum() >= 1
        idx = [RR.color_index(z, RC.INV_MIN, RC.INV_MAX) for z in pts[:, 2]]
        assert idx.count(0) > 10 and idx.count(255) > 10 and sum(0 < i < 255 for i in idx if i is not None) > 64 and None in idx
        assert (pts[:, 2] < 0).sum() >= 3
