"""Crafted events for block matching (kernels_bm.hip: bm_match_kernel in its four group widths, its coarse and up-down instances,
bm_match_any_kernel, and the one-search-per-pixel path around them), pushed through esvo_map_match (tests/test_gpu_bm_cases.py; the
cases themselves are tested on the CPU in tests/test_bm_cases.py).

A stream almost never brings the search to a close decision.  Here every event is put where one is taken: raw and rectified
coordinates on the bounds of the image and on the floats beside them, patch centres on both sides of isValidPatch, left patches
with exactly as many zero pixels as the info-noise test allows and with one more, disparity ranges on both sides of every change of
the lane-group width and of the strip's staging width, true matches in the first and the last staged column at every byte phase,
exact ties from periodic strips (identical bytes, so the tie is exact however the moments are formed), costs of exactly 0.5 and
thresholds taken from a cost itself, the coarse-to-fine rule at both ends of its windows, the up-down variant, other patch sizes,
pose stamps one nanosecond around an event's, and lists that put an event into every position of a workgroup beside neighbours
that fail at each gate.

observe() says what an event really does: it runs the restated matcher (tests/bm_restated.py, which tests/test_bm_cases.py holds
to the oracle bit for bit) and turns its trace into tags.  Each case states the tags its events were written for, so a case that
drifts off its switch point fails as a test of the case; REQUIRED lists what the case list as a whole has to reach.

Small ideal rigs (identity look-up table; single entries of the table or the mask are rewritten on a deep copy); the poses of a
table differ by a millimetre each and the events by a nanosecond, so that the reference's records, which carry neither index, can
be told apart.
Images come from seeded generators and are stored nowhere; built once per process, read-only."""
import copy
import functools
import hashlib
import math

import numpy as np

import bm_restated as BR
from esvo_amd import abi, calib, params

FOCAL, BASELINE = 100.0, 0.1
T0_NS = 1_000_000_000
STAMPS = np.array([T0_NS, T0_NS + 1_000_000], np.uint64)
T_EV = T0_NS + 500_000          # between the two stamps: pose index 1
THR = 0.1
NZ = (1, 0x7f, 0x80, 0xff, 2, 0x81)   # the non-zero pixels of the info-noise patches


def below(v, t=np.float64):
    return t(np.nextafter(t(v), t(-np.inf)))


def above(v, t=np.float64):
    return t(np.nextafter(t(v), t(np.inf)))


@functools.lru_cache(maxsize=None)
def ideal(W, H):
    return calib.ideal_rig(W, H, FOCAL, BASELINE)


def own_rig(W, H):
    """a rig whose table and mask a case may write"""
    r = copy.deepcopy(ideal(W, H))
    if r.left.rect_mask is None:
        r.left.rect_mask = np.full((H, W), 255, np.uint8)
    return r


# ---- images -----------------------------------------------------------------------------------------------------------------------
def texture(W, H, seed):
    """white noise without a zero pixel"""
    return np.random.default_rng(seed).integers(1, 256, (H, W)).astype(np.uint8)


def span(c, n):
    """the n pixels of a patch side centred on c (block from the left-top corner: c - (n - 1) // 2 onwards)"""
    return slice(c - (n - 1) // 2, c - (n - 1) // 2 + n)


def banded(left, bands, wy=7, seed=99):
    """an unrelated texture whose patch rows around y1 are the left image's moved by d, for every y1: d of bands -- an event on
    row y1 matches at d exactly (right[y, x - d] = left[y, x]); d = (d_top, d_bottom, rows_top) moves the upper rows_top rows of
    the patch by d_top and the others by d_bottom"""
    H, W = left.shape
    right = texture(W, H, seed)
    for y1, d in bands.items():
        r = span(y1, wy)
        if isinstance(d, tuple):
            dt, db, k = d
            right[r.start:r.start + k] = np.roll(left[r.start:r.start + k], -dt, axis=1)
            right[r.start + k:r.stop] = np.roll(left[r.start + k:r.stop], -db, axis=1)
        else:
            right[r] = np.roll(left[r], -d, axis=1)
    return right


def banded_ud(left, bands, wx=15, seed=99):
    """the same for the up-down search: the patch columns around x1 moved along y (right[y - d, x] = left[y, x])"""
    H, W = left.shape
    right = texture(W, H, seed)
    for x1, d in bands.items():
        c = span(x1, wx)
        if isinstance(d, tuple):
            dl, dr, k = d
            right[:, c.start:c.start + k] = np.roll(left[:, c.start:c.start + k], -dl, axis=0)
            right[:, c.start + k:c.stop] = np.roll(left[:, c.start + k:c.stop], -dr, axis=0)
        else:
            right[:, c] = np.roll(left[:, c], -d, axis=0)
    return right


def periodic(W, H, P, r, seed, axis=1):
    """(left, right): a pattern of period P along the axis and itself moved by r -- the windows of the candidates d = r (mod P)
    are the left patch byte for byte"""
    rng = np.random.default_rng(seed)
    if axis == 1:
        left = np.tile(rng.integers(1, 256, (H, P)), (1, W // P + 1))[:, :W].astype(np.uint8)
    else:
        left = np.tile(rng.integers(1, 256, (P, W)), (H // P + 1, 1))[:H].astype(np.uint8)
    return left, np.roll(left, -r, axis=axis)


def checker(W, H):
    y, x = np.mgrid[:H, :W]
    return (((x + y) & 1) * 255).astype(np.uint8)


def noisy(a, n, seed):
    """a with n pixels changed"""
    a = a.copy()
    rng = np.random.default_rng(seed)
    flat = a.reshape(-1)
    idx = rng.choice(flat.size, n, replace=False)
    flat[idx] = rng.integers(1, 256, n)
    return a


# ---- a case -----------------------------------------------------------------------------------------------------------------------
def _case(left, right, events, dmin, dmax, tags=None, rig=None, stamps=STAMPS, doc="", **over):
    H, W = left.shape
    ev = [(tuple(e) + (T_EV + i,))[:3] for i, e in enumerate(events)]      # (distinct stamps: the reference's records carry no event index)
    events = abi.make_events([e[0] for e in ev], [e[1] for e in ev], np.array([e[2] for e in ev], np.uint64))
    stamps = np.ascontiguousarray(stamps, np.uint64)
    for a in (left, right, events, stamps):
        a.setflags(write=False)
    over = dict(dict(bm_min_disparity=dmin, bm_max_disparity=dmax, bm_zncc_threshold=THR, bm_step=1, bm_updown=0), **over)
    poses = np.tile(np.eye(4).reshape(16), (len(stamps), 1))
    poses[:, 3] = 1e-3 * np.arange(len(stamps))                            # (distinct poses: ... nor a pose index)
    return dict(W=W, H=H, rig=rig or ideal(W, H), left=left, right=right, events=events, stamps=stamps, poses=poses, over=over, tags=tags or {}, doc=doc)


def case_params(c, **more):
    """ParamsStruct of a case: mvstereo_upenn (no Time-Surface blur), a small event ring, the case's overrides"""
    p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], c["rig"], event_ring_capacity=4096, **dict(c["over"], **more))
    return p


def group_width(nd):
    """launch_bm_match's rule: the lane-group width that wastes the fewest candidate slots, a tie to the wider group"""
    best, slots = 64, 1 << 30
    for G in (64, 32, 16, 8):
        s = -(-nd // G) * G
        if s < slots:
            slots, best = s, G
    return best


def strip_dwords(nd):
    """(dwords staged per strip row, whether the row has no slack: ((nd + 2) >> 2) + 5 is a multiple of 4 already)"""
    need = ((nd + 2) >> 2) + 5
    return (need + 3) & ~3, need % 4 == 0


def oracle_for(c, exact=True, **more):
    from oracle import oracle as O
    m = O.OracleMapper(case_params(c, **more), c["rig"])
    m.set_mode(exact, exact)
    m.set_observation(T0_NS, c["left"], c["right"], np.eye(4))
    m.set_poses(c["stamps"], c["poses"])
    return m


def oracle_best(c, i=0, coarse=False):
    """the oracle's own integer-mode cost of event i's best candidate (of the coarse pass: of its best coarse candidate)"""
    row = oracle_for(c, bm_zncc_threshold=1.0).match_costs(c["events"][i], exact_int=True)
    row = row[~np.isnan(row)] if coarse else row
    return float(row[row < 1.0].min())


def with_threshold(c, thr, tags):
    return dict(c, over=dict(c["over"], bm_zncc_threshold=float(thr)), tags=tags)


# ---- event and coordinate gates ---------------------------------------------------------------------------------------------------
def _gates():
    """Raw coordinates W - 1, W and H; look-up values 0, -0.0, W - 1 (H - 1) and the floats beside the bounds; mask values 125 and
    126 under a fractional coordinate whose rounded index holds the other value; patch centres on both sides of isValidPatch.
    x1 = 8 with dmin = 0 leaves d = 0 as the only valid candidate: inv_depth is 1 / (bf / 0) = 0."""
    W, H = 61, 40
    r = own_rig(W, H)
    lut, mask = r.left.rect_lut, r.left.rect_mask
    f32 = np.float32
    xs = (f32(0.0), f32(-0.0), f32(W - 1), below(0.0, f32), above(W - 1, f32))
    ys = (f32(0.0), f32(-0.0), f32(H - 1), below(0.0, f32), above(H - 1, f32))
    for i, v in enumerate(xs):
        lut[28, 30 + i] = (v, 28.0)
    for i, v in enumerate(ys):
        lut[28, 40 + i] = (30.0, v)
    lut[28, 20] = (24.7, 28.6)
    lut[28, 21] = (34.7, 28.6)
    mask[28, 24], mask[28:30, 25], mask[29, 24] = 126, 125, 125
    mask[28, 34], mask[28:30, 35], mask[29, 34] = 125, 126, 126
    left = texture(W, H, 1)
    right = banded(left, {4: 1, 12: 0, 20: 2, 28: 1, 35: 3})
    ev = [(W - 1, 20), (W, 20), (20, H)] + [(30 + i, 28) for i in range(5)] + [(40 + i, 28) for i in range(5)] + [(20, 28), (21, 28)]
    ev += [(7, 12), (8, 12), (W - 9, 20), (W - 8, 20), (30, 3), (30, 4), (30, H - 5), (30, H - 4), (W - 9, H - 5)]
    tags = {"ex:W-1": [0], "ex:W": [1], "ey:H": [2], "gate:raw": [1, 2], "gate:border": [0, 3, 4, 5, 8, 9, 10, 15, 18, 19, 22],
            "lutx:0": [3], "lutx:-0": [4], "lutx:W-1": [5], "lutx:<0": [6], "lutx:>W-1": [7], "gate:lut": [6, 7, 11, 12],
            "luty:0": [8], "luty:-0": [9], "luty:H-1": [10], "luty:<0": [11], "luty:>H-1": [12],
            "mask:126": [13], "mask:125": [14], "gate:mask": [14], "matched": [13, 16, 17, 20, 21, 23],
            "x1:lo-1": [15], "x1:lo": [16], "x1:hi": [17], "x1:hi+1": [18], "y1:lo-1": [19], "y1:lo": [20], "y1:hi": [21], "y1:hi+1": [22],
            "one_valid:d0": [16], "inv_depth:0": [16], "last_valid_pixel": [23]}
    return _case(left, right, ev, 0, 3, tags, rig=r, doc=_gates.__doc__)


def _none_valid():
    """x1 = 8 with dmin = 1: no candidate is valid, which the reference counts as a coarse failure."""
    c = _gates()
    return dict(c, over=dict(c["over"], bm_min_disparity=1), tags={"none_valid": [16], "gate:coarse": [16]}, doc=_none_valid.__doc__)


def _first_pixel():
    """The first valid pixel under a range wider than the image: the strip starts before the image (a negative byte address, the
    clamped branch of the staging) and only d = 0 is valid; the last valid pixel in the same launch."""
    W, H = 61, 40
    left = texture(W, H, 2)
    right = banded(left, {4: 0, 35: 5})
    return _case(left, right, [(8, 4), (W - 9, H - 5)], 0, 80, {"clamp_lo": [0], "first_valid_pixel": [0], "one_valid:d0": [0], "last_valid_pixel": [1],
                                                                 "matched": [0, 1]}, doc=_first_pixel.__doc__)


def clamp_hi_reachable(W, H, dmax_to=400):
    """whether any valid event and any range (dmin = 0, the longest strip for its dmax) makes the horizontal 15 x 7 staging read
    past the image's last dword (the upper clamp of its slow branch).  A strip row starts at byte x1 - dmax - 7 of its image row
    and is 4 RD <= nd + 34 bytes long; the last patch row, H - 2, is followed by one more image row, so the end is passed only if
    x1 - dmax + nd + 27 > 2 W: with x1 <= W - 9 never for W >= 19, and by enumeration not for 17 and 18 either."""
    n_dw = (W * H + 3) >> 2
    for x1 in range(8, W - 8):
        for dmax in range(0, dmax_to):
            RD, _ = strip_dwords(dmax + 1)
            if (((H - 2) * W + x1 - dmax - 7) >> 2) + RD - 1 >= n_dw:
                return True
    return False


# ---- info-noise -------------------------------------------------------------------------------------------------------------------
def _sparse_patch(img, x1, y1, wx, wy, n_zero):
    """wx x wy patch at (x1, y1) of a black image with exactly n_zero zero pixels; the others hold 1, 0x7f, 0x80, 0xff, ... at
    positions spread over the patch (first and last column, both sides of the dword boundaries)"""
    N = wx * wy
    k = N - n_zero
    pos = [(i * 37 + 3 * (i // 2)) % N for i in range(4 * N)]
    seen = []
    for q in [0, N - 1, 3, 4, wx - 1, wx] + pos:
        if q not in seen and 0 <= q < N:
            seen.append(q)
    r, c = span(y1, wy), span(x1, wx)
    for j, q in enumerate(seen[:k]):
        img[r.start + q // wx, c.start + q % wx] = NZ[j % len(NZ)]


def _noise(wx=15, wy=7):
    """Left patches with exactly as many zero pixels as `cnt > 0.95 N` lets through and with one more, the other pixels 1, 0x7f,
    0x80 and 0xff; once in a black image and once with the bytes left and right of every patch row at 255 (the 16th byte of the
    packed rows and the zero pad byte must not be counted)."""
    N = wx * wy
    at = max(c for c in range(N + 1) if not float(c) > 0.95 * float(N))
    H = 4 * (wy + 2) + 5                      # odd, and W = 2 (mod 4): W H is no multiple of 4 (the image ends inside a dword)
    W = 2 * wx + 16 + (2 if (2 * wx + 16) % 4 == 0 else 0)
    x1 = W // 2
    left = np.zeros((H, W), np.uint8)
    ys = [2 + (wy - 1) // 2 + i * (wy + 2) for i in range(4)]
    for i, y1 in enumerate(ys):
        _sparse_patch(left, x1, y1, wx, wy, at + (i & 1))
        if i >= 2:
            c = span(x1, wx)
            left[span(y1, wy), c.start - 1] = left[span(y1, wy), c.stop] = 255
    right = banded(left, {y: 2 for y in ys}, wy)
    tags = {"cnt:at": [0, 2], "cnt:above": [1, 3], "matched": [0, 2], "gate:noise": [1, 3], "beside:0": [0, 1], "beside:255": [2, 3]}
    if N - at >= 4:
        tags.update({"nz:1": [0, 1], "nz:7f": [0, 1], "nz:80": [0, 1], "nz:ff": [0, 1]})
    return _case(left, right, [(x1, y) for y in ys], 1, 4, tags, patch_size_x=wx, patch_size_y=wy, doc=_noise.__doc__)


# ---- staging ----------------------------------------------------------------------------------------------------------------------
def _staging(nd):
    """The true match in the last staged column (d = dmin) and in the first (d = dmax) at all four byte phases of x1 - dmax - 7."""
    dmin = 2
    dmax = dmin + nd - 1
    H, x0 = 40, dmax + 8
    W = x0 + 3 + 9 + 1 + (nd & 3)
    left = texture(W, H, 100 + nd)
    right = banded(left, {8: dmin, 20: dmax, 32: dmin + nd // 2})
    ev = [(x0 + k, y) for y in (8, 20, 32) for k in range(4)]
    tags = {"matched": list(range(12)), "win:dmin": [0, 1, 2, 3], "win:dmax": [4, 5, 6, 7]}
    for k in range(4):
        tags[f"xphase:{(x0 + k - dmax - 7) & 3}"] = [k, 4 + k]
    return _case(left, right, ev, dmin, dmax, tags, doc=_staging.__doc__)


# ---- group width ------------------------------------------------------------------------------------------------------------------
def _group(nd):
    """The minimum in the first trip of its lane, in the last trip, and in the last lane of the last (where nd is no multiple of
    the group width: partly used) trip."""
    dmin = 1
    dmax = nd
    G = group_width(nd)
    last = dmin + ((nd - 1) // G) * G          # the first candidate of the last trip
    mid = last if last < dmax else dmin + (nd - 1) // 2
    H, x0 = 40, dmax + 8
    W = x0 + 1 + 9 + 1 + (nd % 3)
    left = texture(W, H, 200 + nd)
    right = banded(left, {8: dmin, 20: dmax, 32: mid})
    ev = [(x0, 8), (x0 + 1, 8), (x0, 20), (x0 + 1, 20), (x0, 32)]
    tags = {"matched": [0, 1, 2, 3, 4], f"nd{nd}:G{G}": [0], f"nd{nd}:first_trip": [0, 1], f"nd{nd}:last_trip": [2, 3], f"nd{nd}:at_dmax": [2, 3]}
    return _case(left, right, ev, dmin, dmax, tags, doc=_group.__doc__)


# ---- ties -------------------------------------------------------------------------------------------------------------------------
def _tie(dmin, dmax, P, r, x1=None, tags=(), updown=0, step=1, wx=15, wy=7, thr=THR):
    """A pattern of period P and itself moved by r: every valid candidate d = r (mod P) costs the same to the bit, the largest wins."""
    hx, hy = (wx - 1) // 2, (wy - 1) // 2
    if updown:
        y1 = dmax + hy + 1 if x1 is None else x1
        W, H = 61, max(y1 + hy + 3, 40)
        left, right = periodic(W, H, P, r, 300 + P, axis=0)
        ev = [(30, y1)]
    else:
        x1 = dmax + hx + 1 if x1 is None else x1
        W, H = max(x1 + hx + 3, 61), 40 if wy <= 25 else wy + 6
        left, right = periodic(W, H, P, r, 300 + P)
        ev = [(x1, H // 2)]
    return _case(left, right, ev, dmin, dmax, {t: [0] for t in tags + ("matched",)}, bm_updown=updown, bm_step=step, patch_size_x=wx, patch_size_y=wy,
                 bm_zncc_threshold=thr, doc=_tie.__doc__)


# ---- cost -------------------------------------------------------------------------------------------------------------------------
def _flat(kind, wx=15, wy=7):
    """Zero variance on either side: cov == 0 and the cost is exactly 0.5 for every candidate -- a tie over the whole range."""
    W, H = max(61, wx + 20), max(40, wy + 6)
    tex = texture(W, H, 5)
    left, right = dict(flat_left=(np.full((H, W), 100, np.uint8), tex), flat_right=(tex, np.full((H, W), 100, np.uint8)),
                       flat_both=(np.full((H, W), 100, np.uint8), np.full((H, W), 7, np.uint8)),
                       all255=(np.full((H, W), 255, np.uint8), np.full((H, W), 255, np.uint8)))[kind]
    return _case(left.copy(), right.copy(), [(W // 2, H // 2)], 1, 8, {kind: [0], "cost:half": [0], "thr:eq": [0], "gate:coarse": [0]}, bm_zncc_threshold=0.5,
                 patch_size_x=wx, patch_size_y=wy, doc=_flat.__doc__)


def _checker(compl, wx=15, wy=7):
    """A checkerboard of 0 and 255 against itself and against its complement: the largest N Sxx - Sx^2 and the most negative
    N Slr - Sl Sr a patch can give.  The complement's cost stays below 1.0 (the 1e-6 in both sigmas)."""
    W, H = max(61, wx + 20), max(40, wy + 6)
    left = checker(W, H)
    d = 1 if compl else 2
    tags = {"checker": [0], "matched": [0], ("cost:near_one" if compl else "cost:tiny"): [0]}
    return _case(left, left.copy(), [(W // 2, H // 2)], d, d, tags, bm_zncc_threshold=1.0, patch_size_x=wx, patch_size_y=wy, doc=_checker.__doc__)


def _one_off():
    """A flat patch in which one pixel differs by 1: the smallest non-zero variance."""
    W, H = 63, 40
    left = np.full((H, W), 100, np.uint8)
    left[20, 31] = 101
    right = np.roll(left, -3, axis=1)
    return _case(left, right, [(30, 20), (36, 21)], 1, 8, {"one_off": [0, 1], "matched": [0, 1]}, doc=_one_off.__doc__)


def _threshold_base(wx=15, wy=7, updown=0, step=1):
    W, H = max(64, wx + 30), max(40, wy + 16)
    left = texture(W, H, 6)
    if updown:
        right = noisy(banded_ud(left, {W // 2: 4}, wx), W * H // 12, 7)
    else:
        right = noisy(banded(left, {H // 2: 4}, wy), W * H // 12, 7)
    return _case(left, right, [(W // 2, H // 2)], 0 if step > 1 else 1, 8, bm_zncc_threshold=1.0, patch_size_x=wx, patch_size_y=wy, bm_updown=updown, bm_step=step)


def _threshold(up, **kw):
    """bm_zncc_threshold is the oracle's own integer-mode cost of the best candidate: `best < threshold` fails; on the next double
    it holds."""
    c = _threshold_base(**kw)
    best = oracle_best(c, coarse=kw.get("step", 1) > 1)
    if up:
        return with_threshold(dict(c, doc=_threshold.__doc__), above(best), {"thr:above": [0], "matched": [0]})
    return with_threshold(dict(c, doc=_threshold.__doc__), best, {"thr:eq": [0], "gate:coarse": [0]})


def _flat_up(kind, **kw):
    c = _flat(kind, **kw)
    return with_threshold(c, above(0.5), {kind: [0], "cost:half": [0], "thr:above": [0], "matched": [0], "win:dmax": [0]})


# ---- coarse to fine ---------------------------------------------------------------------------------------------------------------
def _coarse(step):
    """BM_step > 1 on patches whose upper three rows match at one disparity and whose lower four at another: the coarse minimum
    cd lies on the grid (three rows agree), the fine minimum at cd - (step - 1) or cd + (step - 1) (four agree); the dense
    minimum outside the fine window; the coarse minimum at dmin (no lower neighbour: the reference's size_t difference wraps),
    at the last coarse candidate of a range that is no multiple of the step, and beside a candidate the image border refuses."""
    dmin, dmax = 2, 31
    cd = dmin + 3 * step
    last = dmin + ((dmax - dmin) // step) * step
    assert (dmax - dmin) % step
    W, H, x1 = 64 + step, 48, dmax + 8
    left = texture(W, H, 400 + step)
    xb = cd + step + 7                     # candidate cd + step has its patch's first column on column 0
    right = banded(left, {5: (cd, cd - (step - 1), 3), 13: (cd, cd + (step - 1), 3), 21: (cd, cd + 2 * step + 1, 3), 29: dmin, 37: last, 43: cd})
    ev = [(x1, 5), (x1, 13), (x1, 21), (x1, 29), (x1, 37), (xb, 43), (x1, 43)]
    tags = {"fine:lo_end": [0], "fine:hi_end": [1], "coarse:not_dense_min": [2], "coarse:no_lower": [3], "coarse:at_dmin": [3], "coarse:no_upper": [4],
            "coarse:ragged_last": [4], "coarse:neighbour_invalid": [5], "matched": [0, 1, 2, 6], "gate:coarse": [3, 4, 5], f"step:{step}": [0]}
    return _case(left, right, ev, dmin, dmax, tags, bm_step=step, bm_zncc_threshold=0.45, doc=_coarse.__doc__)


def _coarse_border(wx, wy, step=2):
    """the coarse minimum beside a candidate that the image border refuses (its cost-row entry is 1.0: rejected), and the same
    patch further right, where both neighbours are valid -- at any patch size"""
    hx = (wx - 1) // 2
    dmin, dmax = 2, 31
    cd = dmin + 3 * step
    W, H = dmax + 2 * wx + 12, max(40, wy + 6)
    left = texture(W, H, 450 + wx)
    y1 = H // 2
    right = banded(left, {y1: cd}, wy)
    ev = [(cd + step + hx, y1), (dmax + hx + 1, y1)]
    tags = {"coarse:neighbour_invalid": [0], "gate:coarse": [0], "matched": [1], f"step:{step}": [0, 1]}
    return _case(left, right, ev, dmin, dmax, tags, bm_step=step, patch_size_x=wx, patch_size_y=wy, doc=_coarse_border.__doc__)


def _coarse_wide():
    """A step larger than the range: dmin is the only coarse candidate and has no lower neighbour."""
    W, H = 61, 40
    left = texture(W, H, 8)
    return _case(left, banded(left, {20: 2}), [(30, 20)], 2, 5, {"coarse:step_gt_range": [0], "coarse:no_lower": [0], "gate:coarse": [0]}, bm_step=6,
                 doc=_coarse_wide.__doc__)


# ---- up-down ----------------------------------------------------------------------------------------------------------------------
def _updown():
    """BM_bUpDownConfiguration: y1 = 4 (only d = 0 is valid), strips that start above the image (rows clamped; only invalid
    candidates read them), y1 = H - 5, the match at dmin and at dmax."""
    W, H, dmax = 61, 48, 12
    left = texture(W, H, 9)
    right = banded_ud(left, {10: 0, 28: 5, 46: dmax})
    ev = [(10, 4), (10, 30), (28, H - 5), (28, 10), (46, dmax + 4), (46, H - 5), (46, 9), (28, 3), (28, H - 4)]
    tags = {"ud": list(range(9)), "one_valid:d0": [0], "ud:clamp_lo": [0, 3, 6], "y1:lo": [0], "y1:hi": [2, 5], "win:dmin": [0, 1], "win:dmax": [4, 5],
            "matched": [0, 1, 2, 3, 4, 5], "gate:coarse": [6], "gate:border": [7, 8], "y1:lo-1": [7], "y1:hi+1": [8]}
    return _case(left, right, ev, 0, dmax, tags, bm_updown=1, doc=_updown.__doc__)


def _updown_coarse():
    """the coarse-to-fine rule along y: the left seven patch columns match at cd, the right eight at cd - 1 and cd + 1"""
    W, H, dmin, dmax, step = 62, 48, 1, 12, 2
    cd = dmin + 3 * step
    left = texture(W, H, 10)
    right = banded_ud(left, {10: (cd, cd - 1, 7), 28: (cd, cd + 1, 7), 46: dmin})
    ev = [(10, 30), (28, 30), (46, 30)]
    tags = {"ud": [0, 1, 2], "fine:lo_end": [0], "fine:hi_end": [1], "coarse:no_lower": [2], "matched": [0, 1], "gate:coarse": [2]}
    return _case(left, right, ev, dmin, dmax, tags, bm_updown=1, bm_step=step, bm_zncc_threshold=0.45, doc=_updown_coarse.__doc__)


# ---- other patch sizes ------------------------------------------------------------------------------------------------------------
def _any(wx, wy):
    """bm_match_any_kernel on a texture: patch centres on both sides of isValidPatch (even sizes take the block from the
    left-top corner: the right and lower margins are one pixel narrower), the match at dmin and at dmax."""
    hx, hy = (wx - 1) // 2, (wy - 1) // 2
    dmin, dmax = 0, 6
    H = 2 * (wy + 3) + 4
    W = 2 * wx + 24 + (wx & 3)
    left = texture(W, H, 500 + wx * wy)
    ya, yb = hy + 1, H - 2 - hy
    right = banded(left, {ya: dmin, yb: dmax}, wy)
    xl, xh = hx + 1, W - 2 - hx
    xm = xh - 2
    ev = [(xl, ya), (xl - 1, ya), (xh, yb), (xh + 1, yb), (xm, ya - 1), (xm, yb + 1), (xm, ya), (xm, yb)]
    tags = {"x1:lo": [0], "x1:lo-1": [1], "x1:hi": [2], "x1:hi+1": [3], "y1:lo-1": [4], "y1:hi+1": [5], "y1:lo": [0, 6], "y1:hi": [2, 7], "one_valid:d0": [0],
            "matched": [0, 2, 6, 7], "gate:border": [1, 3, 4, 5], "win:dmin": [0, 6], "win:dmax": [2, 7], f"patch:{wx}x{wy}": [0]}
    thr = THR
    if wx * wy == 1:     # N = 1: every cost is 0.5, every valid candidate ties and the largest wins
        thr = above(0.5)
        tags.update({"win:dmin": [0], "win:dmax": [2, 6, 7], "cost:half": [0, 2, 6, 7], "thr:above": [0, 2, 6, 7]})
    return _case(left, right, ev, dmin, dmax, tags, patch_size_x=wx, patch_size_y=wy, bm_zncc_threshold=float(thr), doc=_any.__doc__)


# ---- poses ------------------------------------------------------------------------------------------------------------------------
def _poses(n):
    """Event stamps equal to a pose stamp, one nanosecond before and behind it, before the first stamp and behind the last; tables
    of one stamp and of max_poses_per_tick stamps."""
    W, H = 61, 40
    left = texture(W, H, 11)
    right = banded(left, {20: 2})
    st = (T0_NS + np.arange(n) * 1_000_000).astype(np.uint64)
    k = n // 2
    ts = [int(st[k]), int(st[k]) - 1, int(st[k]) + 1, T0_NS - 5, int(st[-1]) + (2 if n == 1 else 1)] + ([int(st[-1]), int(st[0])] if n > 1 else [])
    ev = [(30, 20, t) for t in ts]
    gone = [4] + ([2] if n == 1 else [])
    tags = {"pose:eq": [0, 5, 6][:len(ts) - 4], "pose:-1ns": [1], "pose:+1ns": [2], "pose:before_first": [3], "pose:behind_last": [4], "gate:pose": gone,
            "matched": [i for i in range(len(ts)) if i not in gone], f"pose:table{n}": [0]}
    return _case(left, right, ev, 1, 4, tags, stamps=st, max_poses_per_tick=256, doc=_poses.__doc__)


# ---- placement --------------------------------------------------------------------------------------------------------------------
KINDS = ("good_dmin", "good_dmax", "good_mid", "outside", "masked", "border", "noise", "threshold")
N_GOOD, FAILING = 3, (3, 4, 5, 6, 7)


def stride_order(n, T):
    """slot -> event of the reference's thread-stride order (EventBM.cpp:289-308)"""
    return np.concatenate([np.arange(t, n, T) for t in range(T)])


def slot_plan(epb):
    """which of the KINDS each slot holds: for every matching kind, every position of a workgroup of epb events and every failing
    kind one workgroup that holds the matching event at that position among copies of the failing one; then a last workgroup
    that is only partly filled"""
    wgs = []
    for g in range(N_GOOD):
        for pos in range(epb):
            for f in FAILING:
                wg = [f] * epb
                wg[pos] = g
                wgs.append(wg)
    flat = [k for wg in wgs for k in wg] + [g % N_GOOD for g in range(max(1, epb // 2))]
    return np.array(flat, np.int64)


def _placement(nd, T):
    """One event of each kind -- three that match (at dmin, at dmax, between), and one stopped at each gate: outside the image, masked,
    border, info-noise, threshold -- copied into every position of a workgroup (slot_plan), under num_threads 1 and 4."""
    dmin, dmax = 1, nd
    W, H, x1 = dmax + 8 + 12, 48, dmax + 8
    r = own_rig(W, H)
    r.left.rect_mask[5, x1 + 1] = 0
    left = texture(W, H, 600 + nd)
    left[span(29, 7)] = 0
    right = banded(left, {5: dmin, 13: dmax, 21: (dmin + dmax) // 2, 29: dmin})
    kinds = [(x1, 5), (x1, 13), (x1, 21), (W, 5), (x1 + 1, 5), (3, 5), (x1, 29), (x1, 37)]
    plan = slot_plan(64 // group_width(nd))
    ev = np.zeros((len(plan), 2), np.int64)
    ev[stride_order(len(plan), T)] = np.array(kinds)[plan]
    c = _case(left, right, [tuple(e) for e in ev], dmin, dmax, rig=r, num_threads=T, doc=_placement.__doc__)
    c["plan"], c["kinds"] = plan, kinds
    return c


# ---- the list ---------------------------------------------------------------------------------------------------------------------
# 1 ... 72: both sides of every power of two; 41 / 48, 89 / 96 and 121 / 128: the ranges in which a 16-, 32- and 64-lane group makes
# more than one trip (a narrower group wastes as many slots there, and the tie goes to the wider one)
GROUP_ND = (1, 8, 9, 16, 17, 32, 33, 41, 48, 64, 65, 72, 89, 96, 121, 128)
NOSLACK_ND = (10, 11, 12, 13, 26, 27, 28, 29)
ANY_SIZES = ((5, 5), (25, 25), (10, 4), (1, 1), (13, 14), (14, 14), (5, 4), (10, 10), (64, 40))
COST_KINDS = ("flat_left", "flat_right", "flat_both", "all255")


def _builders():
    b = {"gates": _gates, "none_valid": _none_valid, "first_pixel": _first_pixel, "noise": _noise}
    for nd in NOSLACK_ND:
        b[f"staging{nd}"] = functools.partial(_staging, nd)
    for nd in GROUP_ND:
        b[f"group{nd}"] = functools.partial(_group, nd)
    # ties: (dmin, dmax, period, residue) -> the tie set; lane = (d - dmin) % G, trip = (d - dmin) // G
    b["tie_lanes"] = functools.partial(_tie, 1, 16, 9, 3, tags=("tie:lanes", "tie:2"))                      # {3, 12}: G = 16, one trip
    b["tie_three"] = functools.partial(_tie, 1, 16, 5, 3, tags=("tie:lanes", "tie:3"))                      # {3, 8, 13}
    b["tie_lanes64"] = functools.partial(_tie, 1, 64, 40, 5, tags=("tie:lanes", "tie:2"))                   # {5, 45}: G = 64
    b["tie_trips"] = functools.partial(_tie, 1, 72, 64, 3, tags=("tie:trips", "tie:2"))                     # {3, 67}: G = 8, lane 2, trips 0 and 8
    b["tie_lower_lane"] = functools.partial(_tie, 1, 72, 63, 3, tags=("tie:lanes+trips:lower", "tie:2"))    # {3, 66}: lanes 2 and 1
    b["tie_higher_lane"] = functools.partial(_tie, 1, 72, 65, 3, tags=("tie:lanes+trips:higher", "tie:2"))  # {3, 68}: lanes 2 and 3
    b["tie_trips64"] = functools.partial(_tie, 1, 121, 64, 3, tags=("tie:trips", "tie:2"))                  # {3, 67}: G = 64, lane 2, trips 0 and 1
    b["tie_lower_lane64"] = functools.partial(_tie, 1, 121, 63, 3, tags=("tie:lanes+trips:lower", "tie:2"))  # {3, 66}: lanes 2 and 1
    b["tie_invalid"] = functools.partial(_tie, 1, 16, 5, 3, x1=20, tags=("tie:invalid", "tie:2"))           # {3, 8}; 13 has its first column on column 0
    for kind in COST_KINDS:
        b[kind] = functools.partial(_flat, kind)
        b[f"{kind}_up"] = functools.partial(_flat_up, kind)
    b["checker_self"] = functools.partial(_checker, False)
    b["checker_compl"] = functools.partial(_checker, True)
    b["one_off"] = _one_off
    b["thr_eq"] = functools.partial(_threshold, False)
    b["thr_up"] = functools.partial(_threshold, True)
    for step in (2, 3, 4):
        b[f"coarse{step}"] = functools.partial(_coarse, step)
    b["coarse_wide"] = _coarse_wide
    b["coarse_tie"] = functools.partial(_tie, 2, 31, 3, 2, step=4, tags=("fine:tie", "fine:hi_end"))      # coarse ties {2, 14, 26}, fine ties {23, 26, 29}
    b["coarse_thr_eq"] = functools.partial(_threshold, False, step=2)
    b["coarse_thr_up"] = functools.partial(_threshold, True, step=2)
    b["ud"] = _updown
    b["ud_tie"] = functools.partial(_tie, 1, 16, 5, 3, updown=1, tags=("ud", "tie:lanes", "tie:3"))
    b["ud_tie_invalid"] = functools.partial(_tie, 1, 16, 5, 3, x1=16, updown=1, tags=("ud", "tie:invalid"))
    b["ud_coarse"] = _updown_coarse
    b["ud_thr_eq"] = functools.partial(_threshold, False, updown=1)
    b["ud_thr_up"] = functools.partial(_threshold, True, updown=1)
    # other patch sizes: bm_match_any_kernel
    for wx, wy in ANY_SIZES:
        s = f"any{wx}x{wy}"
        if (wx, wy) != (64, 40):
            b[s] = functools.partial(_any, wx, wy)
        if (wx, wy) in ((1, 1), (64, 40), (13, 14), (14, 14)):
            b[f"{s}_all255"] = functools.partial(_flat, "all255", wx=wx, wy=wy)
            b[f"{s}_all255_up"] = functools.partial(_flat_up, "all255", wx=wx, wy=wy)
        if (wx, wy) in ((64, 40), (13, 14), (14, 14)):
            b[f"{s}_checker_self"] = functools.partial(_checker, False, wx=wx, wy=wy)
            b[f"{s}_checker_compl"] = functools.partial(_checker, True, wx=wx, wy=wy)
    for wx, wy in ((5, 4), (10, 4), (10, 10), (25, 25)):
        b[f"any{wx}x{wy}_noise"] = functools.partial(_noise, wx, wy)
    b["any5x5_tie"] = functools.partial(_tie, 1, 16, 5, 3, wx=5, wy=5, tags=("tie:3", "tie:lanes"))
    b["any5x5_tie_trips"] = functools.partial(_tie, 1, 72, 64, 3, wx=5, wy=5, tags=("tie:2", "tie:trips"))       # {3, 67}: lane 2 of the wave, trips 0 and 1
    b["any10x4_tie_lower_lane"] = functools.partial(_tie, 1, 72, 63, 3, wx=10, wy=4, tags=("tie:2", "tie:lanes+trips:lower"))   # {3, 66}: lanes 2 and 1
    b["any5x5_coarse_border"] = functools.partial(_coarse_border, 5, 5)
    b["any10x4_coarse_border"] = functools.partial(_coarse_border, 10, 4, 3)
    b["any10x4_tie_invalid"] = functools.partial(_tie, 1, 16, 5, 3, x1=17, wx=10, wy=4, tags=("tie:invalid",))
    b["any5x5_thr_eq"] = functools.partial(_threshold, False, wx=5, wy=5)
    b["any5x5_thr_up"] = functools.partial(_threshold, True, wx=5, wy=5)
    b["any25x25_coarse_thr_eq"] = functools.partial(_threshold, False, wx=25, wy=25, step=2)
    b["any10x4_ud_thr_up"] = functools.partial(_threshold, True, wx=10, wy=4, updown=1)
    b["any5x5_flat_left"] = functools.partial(_flat, "flat_left", wx=5, wy=5)
    for n in (1, 4, 256):
        b[f"poses{n}"] = functools.partial(_poses, n)
    for nd in (8, 32):
        for T in (1, 4):
            b[f"place{nd}_t{T}"] = functools.partial(_placement, nd, T)
    return b


_BUILDERS = _builders()
NAMES = list(_BUILDERS)
ANY = [n for n in NAMES if n.startswith("any")]
REG_15x7 = [n for n in NAMES if not n.startswith("any")]
PLACEMENT = [n for n in NAMES if n.startswith("place")]


@functools.lru_cache(maxsize=None)
def case(name):
    c = dict(_BUILDERS[name]())
    c["name"] = name
    return c


def setup(c):
    p = case_params(c)
    return BR.Setup(c["rig"], c["left"], c["right"], p, baseline=oracle_for(c).baseline)


def input_digest(c):
    """sha256 over what a case feeds the search: both images, the table and the mask, the events, the stamps, the parameters"""
    p = case_params(c)
    h = hashlib.sha256()
    for a in (c["left"], c["right"], c["rig"].left.rect_lut, c["rig"].left.rect_mask, c["events"], c["stamps"]):
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.array([p.patch_size_x, p.patch_size_y, p.bm_min_disparity, p.bm_max_disparity, p.bm_step, p.bm_updown, p.num_threads, c["W"], c["H"]],
                      np.int64).tobytes())
    h.update(np.array([p.bm_zncc_threshold, FOCAL, BASELINE], np.float64).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def pinned_events(c):
    """the events of a case that the reference is run on: all but those outside the image, where the reference itself reads its
    look-up table out of bounds (EventBM.cpp:88; the oracle and the device refuse them)"""
    e = c["events"]
    keep = (e["x"] < c["W"]) & (e["y"] < c["H"])
    keep[list(UNPINNED_EVENTS.get(c["name"], ((), ""))[0])] = False
    return np.ascontiguousarray(e[keep])


# ---- what an event does -----------------------------------------------------------------------------------------------------------
def _edge(v, lo, hi, axis):
    return {lo - 1: f"{axis}:lo-1", lo: f"{axis}:lo", hi: f"{axis}:hi", hi + 1: f"{axis}:hi+1"}.get(v)


def event_tags(c, s, ev, t):
    """tags of one event from its trace (bm_restated.match)"""
    W, H = s.W, s.H
    p = c["over"]
    tags = {"matched" if t["gate"] is None else f"gate:{t['gate']}"}
    ex, ey = int(ev["x"]), int(ev["y"])
    tags |= {k for k, on in (("ex:W-1", ex == W - 1), ("ex:W", ex == W), ("ey:H", ey == H)) if on}
    if s.updown:
        tags.add("ud")
    if t["xr"] is None:
        return tags
    f32 = np.float32
    for axis, v, top in (("x", t["xr"], W - 1), ("y", t["yr"], H - 1)):
        name = {"x": "W-1", "y": "H-1"}[axis]
        if v == 0:
            tags.add(f"lut{axis}:-0" if math.copysign(1.0, v) < 0 else f"lut{axis}:0")
        tags |= {k for k, on in ((f"lut{axis}:{name}", v == top), (f"lut{axis}:<0", v == float(below(0.0, f32))),
                                 (f"lut{axis}:>{name}", v == float(above(top, f32)))) if on}
    if t["gate"] == "lut":
        return tags
    if s.mask is not None and (t["xr"] != int(t["xr"]) or t["yr"] != int(t["yr"])):
        m = int(s.mask[int(t["yr"]), int(t["xr"])])
        other = int(s.mask[int(round(t["yr"])), int(round(t["xr"]))])
        if m in (125, 126) and other == 251 - m:
            tags.add(f"mask:{m}")       # the truncated index holds the value, the rounded one the other
    if t["x1"] is None:
        return tags
    x1, y1 = t["x1"], t["y1"]
    tags |= {e for e in (_edge(x1, s.hx + 1, W - 2 - s.hx, "x1"), _edge(y1, s.hy + 1, H - 2 - s.hy, "y1")) if e}
    if (x1, y1) == (s.hx + 1, s.hy + 1):
        tags.add("first_valid_pixel")
    if (x1, y1) == (W - 2 - s.hx, H - 2 - s.hy):
        tags.add("last_valid_pixel")
    if t["cnt"] is None:
        return tags
    N = s.wx * s.wy
    at = max(k for k in range(N + 1) if not float(k) > 0.95 * float(N))
    L = s.block(s.left, x1, y1)
    if t["cnt"] in (at, at + 1):
        tags.add("cnt:at" if t["cnt"] == at else "cnt:above")
        tags |= {f"nz:{v:x}" for v in (1, 0x7f, 0x80, 0xff) if (L == v).any()}
        if float(at) == 0.95 * float(N):
            tags.add("cnt:bar_is_integer")
        cs, rs = span(x1, s.wx), span(y1, s.wy)
        beside = np.concatenate([s.left[rs, cs.start - 1], s.left[rs, cs.stop]])
        tags |= {f"beside:{v}" for v in (0, 255) if (beside == v).all()}
    if t["gate"] == "noise":
        return tags
    nd = s.dmax - s.dmin + 1
    valid, row = t["valid"], t["row"]
    if not valid:
        tags.add("none_valid")
    if valid == [0]:
        tags.add("one_valid:d0")
    flat_l = N * t["Sll"] - t["Sl"] ** 2 == 0 if t["Sl"] is not None else False
    vals = set(np.unique(L).tolist())
    if vals == {0, 255} and abs(int((L == 0).sum()) * 2 - N) <= 1:
        tags.add("checker")
    if t["Sl"] is not None and N * t["Sll"] - t["Sl"] ** 2 == N - 1:
        tags.add("one_off")
    if valid:
        x2, y2 = s.candidate(x1, y1, valid[-1])
        R = s.block(s.right, x2, y2)
        flat_r = len(np.unique(R)) == 1
        if flat_l and flat_r:
            tags.add("all255" if vals == {255} and int(R[0, 0]) == 255 else "flat_both")
        elif flat_l or flat_r:
            tags.add("flat_left" if flat_l else "flat_right")
        if all(v == 0.5 for v in row.values()):
            tags.add("cost:half")
    best, bestd = t["best"], t["bestd"]
    if best is not None and bestd is not None:
        if t["gate"] == "coarse" and best == s.thr and (s.step == 1 or t["coarse"]["why"] == "threshold"):
            tags.add("thr:eq")
        if t["gate"] is None and s.thr == float(above(best)):
            tags.add("thr:above")
        if t["gate"] is None:
            if best < 1e-6:
                tags.add("cost:tiny")
            if 0.999 < best < 1.0:
                tags.add("cost:near_one")
            if t["record"]["inv_depth"] == 0.0 and bestd == 0:
                tags.add("inv_depth:0")
            if bestd == s.dmin:
                tags.add("win:dmin")
            if bestd == s.dmax:
                tags.add("win:dmax")
    if t["gate"] is None and any(c == best for c in t["ghost"].values()):
        tags.add("tie:invalid")
    co = t["coarse"]
    if co is not None:
        tags.add(f"step:{s.step}")
        last = s.dmin + ((s.dmax - s.dmin) // s.step) * s.step
        if co["why"]:
            tags.add(f"coarse:{co['why']}")
        if co["cd"] == s.dmin:
            tags.add("coarse:at_dmin")
        if co["cd"] == last and (s.dmax - s.dmin) % s.step:
            tags.add("coarse:ragged_last")
        if s.step > s.dmax - s.dmin:
            tags.add("coarse:step_gt_range")
        if t["gate"] is None:
            if bestd == co["cd"] - (s.step - 1):
                tags.add("fine:lo_end")
            if bestd == co["cd"] + (s.step - 1):
                tags.add("fine:hi_end")
            if len(t["ties"]) >= 2:
                tags.add("fine:tie")
            if min(row, key=lambda d: (row[d], -d)) != bestd:
                tags.add("coarse:not_dense_min")
    # lanes and trips: G lanes share an event's search (the general kernel: the whole wave), lane l owns dmin + l, dmin + l + G, ...
    G = group_width(nd) if (s.wx, s.wy) == (15, 7) else 64
    lane, trip = (lambda d: (d - s.dmin) % G), (lambda d: (d - s.dmin) // G)
    if t["gate"] is None and s.step == 1 and len(t["ties"]) >= 2:
        tags.add(f"tie:{len(t['ties'])}" if len(t["ties"]) <= 3 else "tie:many")
        for d in t["ties"][:-1]:
            if trip(d) == trip(bestd):
                tags.add("tie:lanes")
            elif lane(d) == lane(bestd):
                tags.add("tie:trips")
            else:
                tags.add("tie:lanes+trips:" + ("lower" if lane(bestd) < lane(d) else "higher"))
    if (s.wx, s.wy) != (15, 7):
        tags.add(f"patch:{s.wx}x{s.wy}")
        return tags
    # ---- the 15 x 7 kernel's own geometry: lane groups, trips, the staged strip ----
    if s.updown:
        if y1 - s.dmax - s.hy < 0:
            tags.add("ud:clamp_lo")
    else:
        RD, noslack = strip_dwords(nd)
        n_dw = (W * H + 3) >> 2
        xs0 = x1 - s.dmax - s.hx
        tags.add(f"xphase:{xs0 & 3}")
        if noslack:
            tags.add("rd_noslack")
        for py in range(7):
            A = (y1 - 3 + py) * W + xs0
            a0 = A >> 2
            tags.add(f"rowphase:{A - (a0 << 2)}")
            if a0 < 0:
                tags.add("clamp_lo")
            if a0 + RD - 1 >= n_dw:
                tags.add("clamp_hi")
            if t["gate"] is None and s.step == 1 and ((A - (a0 << 2)) + (s.dmax - bestd) + 14) >> 2 == RD - 1:
                tags.add("last_dword")
    if t["gate"] is None and s.step == 1:
        tags.add(f"nd{nd}:G{G}")
        if trip(bestd) == 0:
            tags.add(f"nd{nd}:first_trip")
        if trip(bestd) == trip(s.dmax):
            tags.add(f"nd{nd}:last_trip")
        if bestd == s.dmax:
            tags.add(f"nd{nd}:at_dmax")
            if nd % G:
                tags.add("last_lane_of_partial_trip")
    return tags


def pose_tags(c, ev, t):
    st = [int(v) for v in c["stamps"]]
    ns = int(ev["sec"]) * 1_000_000_000 + int(ev["nsec"])
    tags = {k for k, on in (("pose:eq", ns in st), ("pose:-1ns", ns + 1 in st), ("pose:+1ns", ns - 1 in st), ("pose:before_first", ns < st[0]),
                            ("pose:behind_last", ns > st[-1])) if on}
    tags.add(f"pose:table{len(st)}")
    return tags


@functools.lru_cache(maxsize=None)
def observe(name):
    """(per event: dict(trace, tags); records in thread-stride order; the three failure counts) of a case under the restated matcher"""
    c = case(name)
    s = setup(c)
    T = case_params(c).num_threads
    cache = {}
    traces = []
    for e in c["events"]:       # (the placement lists repeat eight events)
        key = e.tobytes()
        if key not in cache:
            cache[key] = BR.match(s, e, c["stamps"])
        traces.append(cache[key])
    order = stride_order(len(traces), T)
    recs = [(int(i), traces[i]["record"]) for i in order if traces[i]["gate"] is None]
    fails = [sum(t["reason"] == r for t in traces) for r in (1, 2, 3)]
    tag_cache = {}
    obs = []
    for e, t in zip(c["events"], traces):
        key = e.tobytes()
        if key not in tag_cache:
            tag_cache[key] = event_tags(c, s, e, t) | pose_tags(c, e, t)
        obs.append(dict(trace=t, tags=tag_cache[key]))
    return obs, recs, fails


def records_array(recs):
    m = np.zeros(len(recs), abi.MATCH_DTYPE)
    for j, (i, r) in enumerate(recs):
        m["x_left"][j] = r["x_left"]
        m["inv_depth"][j], m["cost"][j], m["disp"][j], m["event_idx"][j], m["pose_idx"][j] = r["inv_depth"], r["cost"], r["disp"], i, r["pose_idx"]
    return m


# The targets the case list has to reach (tests/test_bm_cases.py asserts that it does), as tags of observe().
REQUIRED_15x7 = (
    "ex:W-1", "ex:W", "ey:H", "gate:raw", "gate:lut", "gate:mask", "gate:border", "gate:noise", "gate:coarse", "gate:pose",
    "lutx:0", "lutx:-0", "lutx:W-1", "lutx:<0", "lutx:>W-1", "luty:0", "luty:-0", "luty:H-1", "luty:<0", "luty:>H-1",
    "mask:125", "mask:126",
    "x1:lo-1", "x1:lo", "x1:hi", "x1:hi+1", "y1:lo-1", "y1:lo", "y1:hi", "y1:hi+1",
    "cnt:at", "cnt:above", "nz:1", "nz:7f", "nz:80", "nz:ff", "beside:0", "beside:255",
    "one_valid:d0", "inv_depth:0", "none_valid", "last_valid_pixel", "first_valid_pixel", "clamp_lo",
    "rd_noslack", "last_dword", "win:dmin", "win:dmax", "xphase:0", "xphase:1", "xphase:2", "xphase:3", "rowphase:0", "rowphase:1", "rowphase:2", "rowphase:3",
    "last_lane_of_partial_trip",
    "tie:lanes", "tie:trips", "tie:lanes+trips:lower", "tie:lanes+trips:higher", "tie:2", "tie:3", "tie:invalid",
    "flat_left", "flat_right", "flat_both", "all255", "cost:half", "checker", "cost:tiny", "cost:near_one", "one_off", "thr:eq", "thr:above",
    "step:2", "step:3", "step:4", "coarse:at_dmin", "coarse:no_lower", "coarse:no_upper", "coarse:ragged_last", "coarse:neighbour_invalid",
    "coarse:threshold", "coarse:step_gt_range", "coarse:not_dense_min", "fine:lo_end", "fine:hi_end", "fine:tie",
    "ud", "ud:clamp_lo",
    "pose:eq", "pose:-1ns", "pose:+1ns", "pose:before_first", "pose:behind_last", "pose:table1", "pose:table256",
) + tuple(f"nd{nd}:{w}" for nd in GROUP_ND for w in (f"G{group_width(nd)}", "first_trip", "last_trip", "at_dmax"))
# ... and per combination: (tags that one event has to show together)
REQUIRED_TOGETHER = (
    [("rd_noslack", "win:dmin", "xphase:3", "last_dword"), ("rd_noslack", "win:dmax")]
    + [("rd_noslack", "win:dmin", f"xphase:{k}") for k in range(4)] + [("rd_noslack", "win:dmax", f"xphase:{k}") for k in range(4)]
    + [("cnt:at", "beside:255", "matched"), ("cnt:above", "beside:255"), ("cnt:at", "beside:0", "matched"), ("cnt:above", "beside:0", "gate:noise")]
    + [(k, "thr:eq") for k in COST_KINDS] + [(k, "thr:above", "win:dmax") for k in COST_KINDS]
    + [("ud", t) for t in ("one_valid:d0", "y1:lo", "y1:hi", "tie:lanes", "tie:invalid", "fine:lo_end", "fine:hi_end", "coarse:no_lower", "thr:eq", "thr:above")]
    + [("coarse:threshold", "thr:eq"), ("fine:tie", "fine:hi_end"), ("checker", "cost:tiny"), ("checker", "cost:near_one")]
    + [(f"step:{s}", "fine:lo_end") for s in (2, 3, 4)]
)
REQUIRED_ANY = tuple(f"patch:{wx}x{wy}" for wx, wy in ANY_SIZES) + (
    "cnt:at", "cnt:above", "cnt:bar_is_integer", "x1:lo-1", "x1:lo", "x1:hi", "x1:hi+1", "y1:lo-1", "y1:lo", "y1:hi", "y1:hi+1", "one_valid:d0",
    "all255", "checker", "cost:tiny", "cost:near_one", "cost:half", "thr:eq", "thr:above", "tie:invalid", "flat_left", "ud", "coarse:threshold",
    "win:dmin", "win:dmax", "tie:lanes", "tie:trips", "tie:lanes+trips:lower", "coarse:neighbour_invalid")
REQUIRED = REQUIRED_15x7 + REQUIRED_ANY
# What cannot be reached, and why (tests/test_bm_cases.py asserts that no case reaches them either):
UNREACHED = {
    "gate:fine": "failure reason 3 (fineSearchingFailNum_): the fine window contains the coarse minimum cd itself, a valid candidate whose cost "
                 "passed `< threshold` in the coarse pass, and the fine pass carries that minimum in -- its result can only be lower",
    "cost:one": "a valid candidate whose cost ties with an invalid candidate's 1.0: |cov| / ((sigl + 1e-6)(sigr + 1e-6)) / N < 1 for every pair of "
                "patches, so a cost stays below 1.0 (checker_compl comes nearest); the tie with an invalid slot is taken where a periodic "
                "strip's next window is refused by the image border (tie:invalid)",
    "clamp_hi": "the staging's clamp at the END of the image: the up-down strip ends on row y1 - dmin + 3 <= H - 2, and the horizontal strip of the "
                "last patch row ends less than one image row behind it (clamp_hi_reachable: never, whatever the range); the clamp at the "
                "START is reached (clamp_lo, ud:clamp_lo)",
}
# Single events that are not handed to the reference (bm_cases.pinned_events), and why.
UNPINNED_EVENTS = {n: ((13, 14), "mask values 125 and 126: the reference's mask is a thresholded image that holds 0 and 255 only, and the stand-in that "
                                 "hands it the rig's mask carries zero / non-zero, no other value")
                   for n in ("gates", "none_valid")}
# Cases that are not held to the reference's recorded matches (tests/test_ref_pin.py), and why.  Every other case is, the periodic
# ties among them.
UNPINNED = {}
for _n in NAMES:
    if "thr_" in _n:
        UNPINNED[_n] = ("the threshold is the integer-mode cost of the best candidate (or the double above it); the reference forms the cost from "
                        "normalised patches and rounds it differently in the last bits, so which side of the threshold it falls on is not the reference's to say")
