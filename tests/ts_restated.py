"""A plain restatement of the Time-Surface node (test infrastructure), written from esvo_time_surface/src/TimeSurface.cpp and
include/esvo_time_surface/TimeSurface.h, not from the kernels: per-pixel deques of max_event_queue_len events kept literally
(append, trim from the front, walk back to the first event with ts < T: TimeSurface.h:39-75), dt formed like
(ros::Time - ros::Time).toSec(), exp(-dt / decay) in f64 through libm, the polarity sign, x 255 or x 255 (e + 1) / 2, convertTo,
medianBlur(2k + 1) by sorting, the fixed-point bilinear remap with BORDER_CONSTANT 0, the FORWARD splat in raster order of the
sources with its clamp after every addition (:85-116), and GaussianBlur(5) with BORDER_REFLECT_101.  The OpenCV stages reuse
tests/opencv_restated.py where it restates them already.  tests/test_ts_cases.py holds this module to oracle.OracleTS bit for bit
on every case of tests/ts_cases.py.

observe(case) says what a case really reaches -- per raw pixel whether a float evaluation of the decay would have decided the
quantised value alone and whether it would have decided it wrongly, per output tile the box of source pixels its taps cover and
whether that box fits the staging buffer, per queue tile the events of a batch -- as tags.  The tags only show that a case
reaches what it claims; no expected value comes from them."""
import collections
import math

import numpy as np

import opencv_restated as OR

NS = 1_000_000_000
TILE_X, TILE_Y, STAGE_CAP = 32, 16, 2560     # the fused render's output tile and its staging capacity in raw pixels
QTILE, QTILE_CAP = 8, 1024                   # queue mode: events are binned by 8 x 8 pixel tile, 1024 per tile and batch
GUARD = 5e-4                                 # the float shortcut's guard band around a half-integer


def stamp(e):
    return int(e["sec"]) * NS + int(e["nsec"])


def duration_to_sec(t_ns, te_ns):
    """(ros::Time(T) - ros::Time(te)).toSec(): seconds and nanoseconds subtracted separately, the nanoseconds normalised into
    [0, 1e9) by a borrow, then sec + 1e-9 nsec"""
    sec = t_ns // NS - te_ns // NS
    nsec = t_ns % NS - te_ns % NS
    while nsec < 0:
        nsec += NS
        sec -= 1
    while nsec >= NS:
        nsec -= NS
        sec += 1
    return float(sec) + 1e-9 * float(nsec)


class Node:
    """the node's state for one camera: EventQueueMat and the newest event (events_.back())"""

    def __init__(self, W, H, queue_len=20):
        self.W, self.H, self.L = W, H, queue_len
        self.q = [collections.deque() for _ in range(W * H)]
        self.newest = None

    def push(self, ev):
        """eventsCallback (:403-425): the arriving event is sorted into events_ behind every stamp <= its own, and events_.back()
        -- the event with the largest stamp so far, the later arrival on a tie -- goes into insertEvent"""
        for e in ev:
            rec = (int(e["x"]), int(e["y"]), stamp(e), int(e["polarity"]))
            if self.newest is None or rec[2] >= self.newest[2]:
                self.newest = rec
            x, y, t, p = self.newest
            if x >= self.W or y >= self.H:      # insideImage
                continue
            eq = self.q[x + self.W * y]
            eq.append((t, p))
            while len(eq) > self.L:
                eq.popleft()

    def most_recent_before(self, x, y, t_ns):
        for t, p in reversed(self.q[x + self.W * y]):
            if t < t_ns:
                return t, p
        return None

    def exp_plane(self, t_ns, decay_ms, ignore_polarity):
        """(expVal per raw pixel or NaN where :71-73 find nothing, the stamp found or -1)"""
        decay_sec = decay_ms / 1000.0
        e = np.full((self.H, self.W), np.nan)
        te = np.full((self.H, self.W), -1, np.int64)
        for y in range(self.H):
            for x in range(self.W):
                if not self.q[x + self.W * y]:
                    continue
                hit = self.most_recent_before(x, y, t_ns)
                if hit is None:
                    continue
                t, p = hit
                if not (float(t // NS) + 1e-9 * float(t % NS) > 0):      # toSec() > 0
                    continue
                v = math.exp(-duration_to_sec(t_ns, t) / decay_sec)
                if not ignore_polarity:
                    v *= 1.0 if p else -1.0
                e[y, x], te[y, x] = v, t
        return e, te

    def render_f64(self, t_ns, decay_ms, ignore_polarity):
        """BACKWARD mode: the f64 image handed to convertTo"""
        e, _ = self.exp_plane(t_ns, decay_ms, ignore_polarity)
        return scale(np.where(np.isnan(e), 0.0, e), ignore_polarity)

    def render(self, t_ns, decay_ms, ignore_polarity, median_k, map_x=None, map_y=None):
        """(the rectified mono8 image, the image behind convertTo)"""
        pre = OR.cv_convert_to_u8(self.render_f64(t_ns, decay_ms, ignore_polarity))
        img = median(pre, median_k)
        if map_x is not None:
            img = OR.cv_remap_linear_u8(img, map_x, map_y)
        return img, pre

    def forward_f64(self, t_ns, decay_ms, ignore_polarity, rect_lut):
        e, _ = self.exp_plane(t_ns, decay_ms, ignore_polarity)
        W, H = self.W, self.H
        lut = np.asarray(rect_lut, np.float32).reshape(H, W, 2)
        m = np.zeros((H, W))
        for y in range(H):
            for x in range(W):
                v = e[y, x]
                if v != v:
                    continue
                u, w = float(lut[y, x, 0]), float(lut[y, x, 1])
                if not (u >= 0 and w >= 0):
                    continue
                u_i, v_i = math.floor(u), math.floor(w)
                if not (u_i + 1 < W and v_i + 1 < H):
                    continue
                fu, fv = u - u_i, w - v_i
                fu1, fv1 = 1.0 - fu, 1.0 - fv
                m[v_i, u_i] += fu1 * fv1 * v
                m[v_i, u_i + 1] += fu * fv1 * v
                m[v_i + 1, u_i] += fu1 * fv * v
                m[v_i + 1, u_i + 1] += fu * fv * v
                for yy, xx in ((v_i, u_i), (v_i, u_i + 1), (v_i + 1, u_i), (v_i + 1, u_i + 1)):
                    if m[yy, xx] > 1:
                        m[yy, xx] = 1
        return scale(m, ignore_polarity)

    def render_forward(self, t_ns, decay_ms, ignore_polarity, median_k, rect_lut):
        """(the mono8 image, the f64 image handed to convertTo)"""
        f = self.forward_f64(t_ns, decay_ms, ignore_polarity, rect_lut)
        return median(OR.cv_convert_to_u8(f), median_k), f


def scale(m, ignore_polarity):
    return 255.0 * m if ignore_polarity else 255.0 * (m + 1.0) / 2.0      # :123-126


def median(img, k):
    """cv::medianBlur(2k + 1) on 8UC1: the middle of the sorted window, BORDER_REPLICATE; k = 0: no filter (:130-131)"""
    if k <= 0:
        return img
    H, W = img.shape
    p = np.pad(img, k, mode="edge")
    n = 2 * k + 1
    stack = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(n) for dx in range(n)], 0)
    return np.sort(stack, axis=0)[n * n // 2]


def window(img, x, y, k):
    """the sorted replicated window of (x, y)"""
    H, W = img.shape
    return np.sort(np.array([img[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)]
                             for dy in range(-k, k + 1) for dx in range(-k, k + 1)], np.int64))


def gaussian5_neg(img):
    """the tracker's negative of the blurred Time Surface: 255 - GaussianBlur(5 x 5)"""
    return (255 - OR.cv_gaussian5_u8(img).astype(np.int64)).astype(np.uint8)


# ---- what a case reaches ----------------------------------------------------------------------------------------------------------
def decay_tags(te, pol, t_ns, decay_ms, ignore_polarity):
    """per raw pixel with an event before T (arrays te, pol): the f64 value g, its distance to the nearest half-integer, whether a
    numpy float32 evaluation of the short form (exp of (float) dt * (float)(-1e-9 / decay); it stands in for the device's float
    exp and only classifies inputs) lies inside the guard band, and whether rounding that float value disagrees with f64"""
    decay_sec = decay_ms / 1000.0
    f32 = np.float32
    dt_ns = (t_ns - te).astype(np.uint64)
    g = np.array([math.exp(-duration_to_sec(t_ns, int(t)) / decay_sec) for t in te])
    sgn = np.where(pol > 0, 1.0, -1.0)
    g = 255.0 * g if ignore_polarity else 255.0 * (g * sgn + 1.0) / 2.0
    with np.errstate(under="ignore"):
        e32 = np.exp(dt_ns.astype(f32) * f32(-1e-9 / decay_sec)).astype(f32)
    g32 = f32(255.0) * e32 if ignore_polarity else f32(127.5) * np.where(pol > 0, f32(1.0) + e32, f32(1.0) - e32).astype(f32)
    q32 = np.rint(g32)
    in_band = ~(np.abs(g32 - q32) < f32(0.5) - f32(GUARD))
    dist = np.abs(g - (np.floor(g) + 0.5))
    return dict(g=g, dist=dist, in_band=in_band, float_wrong=q32.astype(np.int64) != np.rint(g).astype(np.int64),
                err32=np.abs(g32.astype(np.float64) - g), e32_zero=e32 == 0, dt_ns=dt_ns)


def tile_boxes(map_x, map_y, W, H, k):
    """per 32 x 16 output tile: the box of in-image source pixels that its bilinear taps of non-zero weight cover (None: no tap
    lies in the image), rw x rh with the median's ring, and whether that fits the staging buffer"""
    sx = OR.cv_round(np.asarray(map_x, np.float32) * np.float32(32)).astype(np.int64)
    sy = OR.cv_round(np.asarray(map_y, np.float32) * np.float32(32)).astype(np.int64)
    ix, iy, fx, fy = sx >> 5, sy >> 5, sx & 31, sy & 31
    out = {}
    for ty in range(-(-H // TILE_Y)):
        for tx in range(-(-W // TILE_X)):
            s = (slice(ty * TILE_Y, min((ty + 1) * TILE_Y, H)), slice(tx * TILE_X, min((tx + 1) * TILE_X, W)))
            lx, hx = np.maximum(ix[s], 0), np.minimum(ix[s] + (fx[s] != 0), W - 1)
            ly, hy = np.maximum(iy[s], 0), np.minimum(iy[s] + (fy[s] != 0), H - 1)
            ok = (lx <= hx) & (ly <= hy)
            rows = s[0].stop - s[0].start
            t = dict(rows=rows, cols=s[1].stop - s[1].start, inside=int(ok.sum()), pixels=int(ok.size))
            if not ok.any():
                t.update(box=None, rw=0, rh=0, staged=False, empty=True)
            else:
                x0, x1, y0, y1 = int(lx[ok].min()), int(hx[ok].max()), int(ly[ok].min()), int(hy[ok].max())
                rw, rh = x1 - x0 + 1 + 2 * k, y1 - y0 + 1 + 2 * k
                t.update(box=(x0, y0, x1, y1), rw=rw, rh=rh, staged=rw * rh <= STAGE_CAP, empty=False)
            out[(tx, ty)] = t
    return out


def queue_batches(ev, W, H):
    """per 8 x 8 tile: the events of one batch that queue mode bins into it (inside the sensor, stamp not zero)"""
    n = collections.Counter()
    for e in ev:
        x, y = int(e["x"]), int(e["y"])
        if x < W and y < H and stamp(e) > 0:
            n[(x // QTILE, y // QTILE)] += 1
    return n
