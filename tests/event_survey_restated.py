"""The event survey's rules (include/esvo_hip.h, esvo_ts_survey_begin / esvo_ts_survey_mask) restated with Python ints: the counts
and stats of a stream, and the hot-pixel rule on a count image.

Events are (x, y, t_ns, polarity) tuples of Python ints; counts is [2][H][W] nested lists (plane = polarity); stats a dict named as
esvo_event_survey_stats_t.  sorted() gives the order statistic.  Nothing here calls the library."""

U32_MAX = 2 ** 32 - 1
STATS0 = dict(events_in=0, outside=0, packets=0, t_first=0, t_last=0)
RULE0 = dict(min_count=1, factor=0, rank_permille=500, max_rate_hz=0)


def fresh_counts(W, H):
    return [[[0] * W for _ in range(H)] for _ in range(2)]


def count(events, W, H, counts=None, stats=None):
    """-> (counts, stats) behind one accepted packet; both advance in copies"""
    counts = fresh_counts(W, H) if counts is None else [[list(r) for r in plane] for plane in counts]
    stats = dict(STATS0 if stats is None else stats)
    if not events:
        return counts, stats
    assert stats["events_in"] + stats["outside"] + len(events) <= U32_MAX
    for (x, y, t, p) in events:
        if x >= W or y >= H:
            stats["outside"] += 1
            continue
        counts[1 if p else 0][y][x] += 1
        if stats["events_in"] == 0:
            stats["t_first"] = stats["t_last"] = t
        stats["t_first"], stats["t_last"] = min(stats["t_first"], t), max(stats["t_last"], t)
        stats["events_in"] += 1
    stats["packets"] += 1
    return counts, stats


def hot_pixels(counts, stats, W, H, min_count=1, factor=0, rank_permille=500, max_rate_hz=0):
    """-> (mask rows of 0 / 1, report dict named as esvo_hot_pixel_report_t)"""
    assert min_count >= 1 and 0 <= rank_permille <= 1000 and (factor > 0 or max_rate_hz > 0)
    c = [counts[0][y][x] + counts[1][y][x] for y in range(H) for x in range(W)]
    k = rank_permille * (W * H - 1) // 1000
    B = sorted(c)[k]
    duration = stats["t_last"] - stats["t_first"] if stats["events_in"] else 0
    rate_on = max_rate_hz > 0 and duration > 0
    R = min(U32_MAX, max_rate_hz * duration // 10 ** 9) if rate_on else 0
    hot = [v >= min_count and ((factor > 0 and v > factor * B) or (rate_on and v > R)) for v in c]
    top = max(c)
    report = dict(baseline=B, rate_count=R, n_hot=sum(hot), max_count=top, max_pixel=c.index(top), events_hot=sum(v for v, h in zip(c, hot) if h))
    return [[1 if hot[y * W + x] else 0 for x in range(W)] for y in range(H)], report


def counts_array(counts):
    import numpy as np
    return np.array(counts, dtype=np.uint32)


# ---- the crafted count images of the tests: (name, c per pixel as a flat list of W * H ints, stats, rule) ----------------------------
DIGIT_EDGES = (0, 1, 255, 256, 257, 65535, 65536, 65537, 2 ** 24, U32_MAX)


def split_planes(c, W, H, seed=0):
    """a count image c (flat) as two planes that add up to it, the split drawn per pixel"""
    import random
    r = random.Random(seed)
    off = [r.randint(0, v) for v in c]
    return [[[(off[y * W + x] if plane == 0 else c[y * W + x] - off[y * W + x]) for x in range(W)] for y in range(H)] for plane in range(2)]


def crafted_images(W, H, seed=5):
    """the cases of the issue: radix digit boundaries, all equal, dark, the ranks, factor * B beyond 2^32, at / above factor * B,
    min_count gating, the rate test alone / both / duration 0, two pixels tied for max_count"""
    import random
    r = random.Random(seed)
    n = W * H
    sec = 10 ** 9
    run = dict(STATS0, events_in=1, packets=1, t_first=5 * sec, t_last=7 * sec)        # 2 s
    still = dict(run, t_last=run["t_first"])                                             # duration 0
    cases = []
    edges = [r.choice(DIGIT_EDGES) for _ in range(n)]
    for rank in (0, 500, 999, 1000):
        cases.append((f"digit_edges_rank{rank}", edges, run, dict(RULE0, factor=1, rank_permille=rank)))
    cases.append(("digit_edges_factor_beyond_u32", edges, run, dict(RULE0, factor=U32_MAX, rank_permille=300, min_count=2)))
    big = [2 ** 24] * n
    big[3], big[n - 1] = U32_MAX, U32_MAX - 1
    cases.append(("factor_times_b_beyond_u32", big, run, dict(RULE0, factor=255)))       # 255 * 2^24 < 2^32 - 1 < 256 * 2^24
    cases.append(("factor_times_b_beyond_u32_none", big, run, dict(RULE0, factor=256)))
    cases.append(("all_equal", [7] * n, run, dict(RULE0, factor=1)))
    dark = [0] * n
    dark[0], dark[n // 2], dark[n - 1] = 1, 3, 2
    cases.append(("dark_b0", dark, run, dict(RULE0, factor=1000)))
    cases.append(("dark_b0_min_count", dark, run, dict(RULE0, factor=1000, min_count=3)))   # passes c > 0, gated by min_count
    level = [10] * n
    level[17], level[18], level[n - 2] = 30, 31, 31                                      # exactly factor * B, one above; tied for the max
    cases.append(("at_and_above_factor_b", level, run, dict(RULE0, factor=3)))
    cases.append(("rate_alone", level, run, dict(RULE0, max_rate_hz=15)))                # R = 30: 31 is hot, 30 is not
    cases.append(("rate_and_baseline", level, run, dict(RULE0, factor=3, max_rate_hz=5, min_count=11)))   # R = 10: 30 and 31 by rate
    cases.append(("rate_duration_0", level, still, dict(RULE0, max_rate_hz=1)))          # contributes nothing: nothing is hot
    cases.append(("rate_duration_0_with_baseline", level, still, dict(RULE0, factor=3, max_rate_hz=1)))
    cases.append(("rate_clamped", edges, dict(run, t_last=run["t_first"] + 4000 * sec), dict(RULE0, max_rate_hz=U32_MAX)))
    return cases
