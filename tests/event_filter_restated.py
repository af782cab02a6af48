"""The event filter's rule (include/esvo_hip.h, esvo_ts_filter_configure) restated with Python ints: verdicts, `last` and counts.

Events are (x, y, t_ns, polarity) tuples of Python ints in stream order; `last` is a list of H rows of W ints (0: none); mask is
None or such rows (non-zero = masked).  Nothing here calls the library."""

KEPT, OUTSIDE, MASKED, REFRACTORY, UNSUPPORTED = range(5)
NAMES = ("kept", "outside", "masked", "refractory", "unsupported")


def fresh_last(W, H):
    return [[0] * W for _ in range(H)]


def run(events, W, H, refractory_ns, support_ns, mask=None, last=None):
    """-> (verdicts, last, counts): the state advances in a copy; counts as esvo_event_filter_counts_t names them"""
    last = fresh_last(W, H) if last is None else [list(row) for row in last]
    verdicts = []
    for (x, y, t, _p) in events:
        if x >= W or y >= H:
            verdicts.append(OUTSIDE)
            continue
        if mask is not None and mask[y][x] != 0:
            verdicts.append(MASKED)
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
                    sup = sup or (Ln != 0 and t - Ln <= support_ns)       # read BEFORE the pixel's own update
        last[y][x] = t
        verdicts.append(UNSUPPORTED if support_ns > 0 and not sup else KEPT)
    counts = {name: verdicts.count(v) for v, name in enumerate(NAMES)}
    counts["events_in"] = len(events)
    return verdicts, last, counts


def kept(events, verdicts):
    return [e for e, v in zip(events, verdicts) if v == KEPT]


def records(events):
    """the esvo_event_t array of events as the ring holds them (polarity 0 / 1, padding 0)"""
    import numpy as np
    from esvo_amd import abi
    ev = np.zeros(len(events), abi.EVENT_DTYPE)
    if events:   # (the values are split in Python ints; numpy only stores them)
        ev["x"], ev["y"] = [e[0] for e in events], [e[1] for e in events]
        ev["sec"], ev["nsec"] = [e[2] // 10 ** 9 for e in events], [e[2] % 10 ** 9 for e in events]
        ev["polarity"] = [1 if e[3] else 0 for e in events]
    return ev


def last_array(last):
    import numpy as np
    return np.array(last, dtype=np.uint64)


# ---- the random stream of the tests: 346x260, events drawn half from the low and half from the high 24 columns / rows (the high
# range reaches W and H themselves: outside), stamp steps from {0, 1, 2, 3} us above a 1.7e18 ns base; 15 % of the pixels masked
W, H = 346, 260
T_BASE = 1_700_000_000_000_000_000
REFRACTORY_NS, SUPPORT_NS = 300_000, 1_500_000


def random_stream(seed, n=6000):
    """-> (events, mask rows)"""
    import numpy as np
    r = np.random.default_rng(seed)

    def coord(size):
        lo, hi = r.integers(0, 24, n), r.integers(size - 24, size + 1, n)
        return np.where(r.integers(0, 2, n) == 0, lo, hi)
    x, y = coord(W), coord(H)
    t = T_BASE + np.cumsum(r.integers(0, 4, n)) * 1000
    p = r.integers(0, 2, n)
    mask = (r.random((H, W)) < 0.15).astype(int)
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(x, y, t, p)], mask.tolist()
