"""The event filter's rule with its burst stage (include/esvo_hip.h, esvo_ts_burst_configure) restated with Python ints: verdicts,
`bstamp`, `bflags`, `last` and both counts.

Events are (x, y, t_ns, polarity) tuples of Python ints in stream order; `bstamp`, `bflags` and `last` are lists of H rows of W ints;
mask is None or such rows (non-zero = masked).  Nothing here calls the library."""
import event_filter_restated as F

KEPT, OUTSIDE, MASKED, REFRACTORY, UNSUPPORTED, BURST = range(6)
NAMES = F.NAMES + ("burst",)
OFF, TRAIL, STC_CUT_TRAIL, STC_KEEP_TRAIL = range(4)
MODES = (TRAIL, STC_CUT_TRAIL, STC_KEEP_TRAIL)
ZERO_BURST = {"judged": 0, "passed": 0, "dropped": 0}


def fresh(W, H):
    return [[0] * W for _ in range(H)]


def run(events, W, H, mode, burst_ns, refractory_ns, support_ns, mask=None, bstamp=None, bflags=None, last=None):
    """-> (verdicts, bstamp, bflags, last, burst counts, filter counts): the state advances in copies; the counts as
    esvo_event_burst_counts_t and esvo_event_filter_counts_t name them (a burst-dropped event stands in none of the filter's)"""
    bstamp = fresh(W, H) if bstamp is None else [list(r) for r in bstamp]
    bflags = fresh(W, H) if bflags is None else [list(r) for r in bflags]
    last = fresh(W, H) if last is None else [list(r) for r in last]
    verdicts = []
    for (x, y, t, p) in events:
        p = 1 if p else 0
        if x >= W or y >= H:
            verdicts.append(OUTSIDE)
            continue
        if mask is not None and mask[y][x] != 0:
            verdicts.append(MASKED)
            continue
        if mode != OFF:
            T, P, K = bstamp[y][x], bflags[y][x] & 1, bflags[y][x] >> 1 & 1
            linked = T != 0 and p == P and t - T <= burst_ns
            passes = {TRAIL: not linked, STC_CUT_TRAIL: linked and not K, STC_KEEP_TRAIL: linked}[mode]
            bstamp[y][x], bflags[y][x] = t, p | (2 if linked else 0)        # always, whatever the verdict
            if not passes:
                verdicts.append(BURST)
                continue
        L = last[y][x]
        if refractory_ns > 0 and L != 0 and t - L < refractory_ns:
            verdicts.append(REFRACTORY)
            continue
        sup = False
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nx, ny = x + dx, y + dy
                if (dx or dy) and 0 <= nx < W and 0 <= ny < H:
                    Ln = last[ny][nx]
                    sup = sup or (Ln != 0 and t - Ln <= support_ns)
        last[y][x] = t
        verdicts.append(UNSUPPORTED if support_ns > 0 and not sup else KEPT)
    fc = {name: verdicts.count(v) for v, name in enumerate(F.NAMES)}
    fc["events_in"] = sum(fc.values())
    bc = dict(ZERO_BURST)
    if mode != OFF:
        bc["dropped"] = verdicts.count(BURST)
        bc["passed"] = fc["kept"] + fc["refractory"] + fc["unsupported"]
        bc["judged"] = bc["passed"] + bc["dropped"]
    return verdicts, bstamp, bflags, last, bc, fc


def kept(events, verdicts):
    return [e for e, v in zip(events, verdicts) if v == KEPT]


def shares(verdicts):
    return [verdicts.count(v) / len(verdicts) for v in range(6)]


def stamp_array(img):
    import numpy as np
    return np.array(img, dtype=np.uint64)


def flags_array(img):
    import numpy as np
    return np.array(img, dtype=np.uint8)


# ---- the bursty stream of the tests: 346x260, `bursts` bursts starting uniformly over `span_ns`, their pixels drawn as
# event_filter_restated.random_stream draws them (low / high 24 columns and rows, the high range reaching W and H themselves), 1..6
# events each with gaps of 20..600 us (whole us), the polarity flipping with probability 0.15 per step; all events merged and sorted
# by stamp; 15 % of the pixels masked
W, H, T_BASE = F.W, F.H, F.T_BASE
BURST_NS, REFRACTORY_NS, SUPPORT_NS = 300_000, 250_000, 1_500_000


def bursty_stream(seed, bursts=1500, span_ns=12_000_000, width=W, height=H, margin=24):
    """-> (events, mask rows)"""
    import numpy as np
    r = np.random.default_rng(seed)

    def coord(size):
        lo, hi = r.integers(0, margin, bursts), r.integers(size - margin, size + 1, bursts)
        return np.where(r.integers(0, 2, bursts) == 0, lo, hi)
    start = r.integers(0, span_ns // 1000, bursts) * 1000
    length = r.integers(1, 7, bursts)
    p0 = r.integers(0, 2, bursts)
    x, y = coord(width), coord(height)
    ev = []
    for b in range(bursts):
        t, p = T_BASE + int(start[b]), int(p0[b])
        for k in range(int(length[b])):
            if k:
                t += int(r.integers(20, 601)) * 1000
                if r.random() < 0.15:
                    p ^= 1
            ev.append((int(x[b]), int(y[b]), t, p))
    ev.sort(key=lambda e: e[2])          # (stable: equal stamps keep the order they were drawn in)
    mask = (r.random((height, width)) < 0.15).astype(int)
    return ev, mask.tolist()
