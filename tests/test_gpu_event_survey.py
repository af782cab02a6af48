"""The event survey on the device (include/esvo_hip.h, esvo_ts_survey_begin / esvo_ts_survey_mask) against the Python-int restatement
(tests/event_survey_restated.py) and the host twins: counts and stats through every entry point, the contention shapes the counting
kernel exists for, a handle with a survey against one without, refusals, count-only mode, the rule on planted count images, the
mask's installation and the calibration flow end to end.  Equality everywhere.  346x260 (upenn rig), ring 2^16."""
import functools

import numpy as np
import pytest

import event_filter_restated as F
import event_survey_restated as S
import evt3_restated as R3
from esvo_amd import abi, lib
from test_gpu_event_filter import ERR_UNSUPPORTED, _params, columns, feed, filter_state, state

pytestmark = pytest.mark.gpu

W, H, T0 = F.W, F.H, F.T_BASE
HOWS = ("records", "async", "wire", "host_columns", "device_columns", "evt3", "evt2", "evt21")
CORNERS = ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (344, 256), (345, 100), (100, 259), (W, H), (W, 0), (0, H))


@functools.lru_cache(maxsize=None)
def stream(seed, n=6000):
    """the filter tests' random stream (events outside included); its first events moved onto the corner pixels, the last partial
    tile row and column and just outside"""
    ev, mask = F.random_stream(seed, n)
    ev = [(cx, cy, e[2], e[3]) for (cx, cy), e in zip(CORNERS, ev)] + ev[len(CORNERS):]
    return ev, mask


def make(rig, ring=1 << 16, refractory_ns=0, support_ns=0, mask=None):
    dev = lib.Esvo(_params(rig, ring), rig)
    dev.debug_evt3_device_min(0)
    dev.debug_evt2_device_min(0)
    dev.ts_filter_configure(0, refractory_ns, support_ns, mask)
    return dev


@pytest.fixture(scope="module")
def dev(upenn_rig):
    d = make(upenn_rig)
    yield d
    d.close()


def fresh(dev, count_only=False, refractory_ns=0, support_ns=0, mask=None):
    """the module's handle reset, its filter configured anew and a survey begun"""
    try:
        dev.ts_survey_end(0)
    except lib.EsvoError as e:
        assert e.code == abi.ERR_STATE
    dev.reset()
    dev.ts_filter_configure(0, refractory_ns, support_ns, mask)
    dev.ts_survey_begin(0, count_only=count_only)
    return dev


def survey(dev):
    return dev.ts_survey_state(0).tobytes(), dev.ts_survey_stats(0)


def check(dev, counts, stats):
    assert dev.ts_survey_stats(0) == stats
    assert np.array_equal(dev.ts_survey_state(0), S.counts_array(counts))


def device_columns(events):
    import torch
    x, y, t, p = columns(events)
    d = [torch.from_numpy(x.view(np.int16)).cuda(), torch.from_numpy(y.view(np.int16)).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda()]
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("how", HOWS)
def test_counts_through_every_entry_point(dev, how):
    ev, _ = stream(31)
    fresh(dev)
    counts, stats, a = None, None, 0
    for m in (1, 63, 64, 65, 255, 256, 257, len(ev)):
        counts, stats = S.count(ev[a:a + m], W, H, counts, stats)
        feed(dev, ev[a:a + m], how)
        assert dev.ts_survey_stats(0) == stats, (how, m)
        a += m
    assert a >= len(ev) and stats["packets"] == 8 and stats["outside"] > 100
    check(dev, counts, stats)
    got = dev.ts_survey_state(0)
    for x, y in CORNERS[:7]:
        assert got[:, y, x].sum() >= 1
    host, hstats = lib.event_survey_host(F.records(ev), W, H)
    assert np.array_equal(got, host) and dict(hstats, packets=8) == stats


def _contended(name):
    r = np.random.default_rng(7)
    if name == "one_pixel":
        return [(100, 100, T0 + 1000 * i, i & 1) for i in range(4096)]
    if name == "half_on_one_pixel":
        bg, _ = stream(32)
        return [(345, 259, e[2], 1) if i & 1 else e for i, e in enumerate(bg)]
    assert name == "one_tile"          # 5000 events inside one 8x8 tile: beyond the 1024 entries of a filter tile list
    xs, ys, ps = r.integers(40, 48, 5000), r.integers(56, 64, 5000), r.integers(0, 2, 5000)
    return [(int(x), int(y), T0 + 1000 * i, int(p)) for i, (x, y, p) in enumerate(zip(xs, ys, ps))]


@pytest.mark.parametrize("name", ("one_pixel", "half_on_one_pixel", "one_tile"))
def test_contention_shapes(dev, name):
    ev = _contended(name)
    fresh(dev)
    feed(dev, ev, "device_columns")
    counts, stats = S.count(ev, W, H)
    check(dev, counts, stats)
    if name == "one_pixel":
        assert counts[0][100][100] == counts[1][100][100] == 2048
    feed(dev, [(e[0], e[1], e[2] + 10 ** 7, e[3]) for e in ev[:1500]], "host_columns")      # and once more, on top
    counts, stats = S.count([(e[0], e[1], e[2] + 10 ** 7, e[3]) for e in ev[:1500]], W, H, counts, stats)
    check(dev, counts, stats)


def test_a_survey_changes_nothing(upenn_rig):
    ev, mask = stream(33)
    a, b = (make(upenn_rig, refractory_ns=F.REFRACTORY_NS, support_ns=F.SUPPORT_NS, mask=mask) for _ in range(2))
    try:
        b.ts_survey_begin(0)
        cuts = ((0, 1500, "records"), (1500, 1501, "device_columns"), (1501, 3000, "device_columns"), (3000, 4200, "evt3"), (4200, 5000, "wire"),
                (5000, 6000, "evt2"))
        for lo, hi, how in cuts:
            for d in (a, b):
                feed(d, ev[lo:hi], how)
            assert state(a) == state(b) and filter_state(a) == filter_state(b), how
        sa, sb = a.stats(), b.stats()
        for field in ("events_staged", "events_scattered", "late_events", "ts_frames"):     # (the rest of esvo_get_stats are timings)
            assert list(getattr(sa, field)) == list(getattr(sb, field)), field
        t = int(np.frombuffer(state(a)["stamps"], np.uint64)[-1]) + 1
        assert np.array_equal(a.ts_render(0, t), b.ts_render(0, t))
        counts, stats = S.count(ev, W, H)
        check(b, counts, dict(stats, packets=len(cuts)))
        assert a.ts_filter_stats(0)["masked"] > 100      # the survey counted masked pixels all the same
    finally:
        a.close(); b.close()


def test_refusals_are_transactional(upenn_rig):
    d = make(upenn_rig, ring=1024, refractory_ns=500, support_ns=0)
    try:
        d.ts_survey_begin(0)
        first = [(i % 100, i // 100, T0 + 1000 * i, i & 1) for i in range(800)]
        feed(d, first, "host_columns")
        counts, stats = S.count(first, W, H)
        check(d, counts, stats)
        before, ring = survey(d), state(d)
        x, y, t, p = columns([(5, 5, T0 + 900_000, 1), (6, 6, T0 + 900_001, 1)])
        t[1] = -5
        import torch
        bad_stamp = [torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for v in (x, y, t, p)]
        cases = (
            (lambda: feed(d, [(5, 5, T0 + 900_000, 1), (6, 6, T0 + 899_000, 1)], "device_columns"), ERR_UNSUPPORTED),   # not sorted in itself
            (lambda: feed(d, [(5, 5, T0 + 1000, 1), (6, 6, T0 + 2000, 1)], "records"), ERR_UNSUPPORTED),                # older than the staged events
            (lambda: feed(d, [(5, 5, T0 + 1000, 1), (6, 6, T0 + 2000, 1)], "evt3"), ERR_UNSUPPORTED),
            (lambda: feed(d, [(5, 5, T0 + 900_000 + i, 1) for i in range(300)], "device_columns"), abi.ERR_CAPACITY),   # a full ring
            (lambda: d.ts_push_columns(0, *bad_stamp), abi.ERR_INVALID_ARG),                                            # a bad stamp, judged on the device
            (lambda: d.ts_push_columns(0, x, y, t, p), abi.ERR_INVALID_ARG),
        )
        for k, (call, code) in enumerate(cases):
            with pytest.raises(lib.EsvoError) as e:
                call()
            assert e.value.code == code, k
            assert survey(d) == before and state(d) == ring, k
        more = [(5, 5, T0 + 900_000, 1), (W, 6, T0 + 900_001, 1)]                                                       # and the stream goes on
        feed(d, more, "device_columns")
        check(d, *S.count(more, W, H, counts, stats))
    finally:
        d.close()


def test_state_errors(upenn_rig):
    d = lib.Esvo(_params(upenn_rig, 1 << 16), upenn_rig)
    try:
        def fails(code, call, *a, **kw):
            with pytest.raises(lib.EsvoError) as e:
                call(*a, **kw)
            assert e.value.code == code, (call.__name__, a, kw)
        fails(abi.ERR_STATE, d.ts_survey_begin, 0)                     # no filter
        for call in (d.ts_survey_end, d.ts_survey_stats, d.ts_survey_state):
            fails(abi.ERR_STATE, call, 0)                               # no survey
        fails(abi.ERR_STATE, d.ts_survey_mask, 0, factor=1)
        d.ts_filter_configure(0, 0, 0)
        fails(abi.ERR_INVALID_ARG, d.ts_survey_begin, 0, reserved=(0, 1, 0))
        fails(abi.ERR_INVALID_ARG, d.ts_survey_begin, 0, flags=2)
        d.ts_survey_begin(0)
        fails(abi.ERR_STATE, d.ts_survey_begin, 0)                     # twice
        fails(abi.ERR_STATE, d.ts_survey_begin, 0, count_only=True)
        fails(abi.ERR_STATE, d.ts_filter_configure, 0, off=True)       # filter off while the survey is open
        fails(abi.ERR_STATE, d.ts_survey_begin, 1)                     # the other camera has no filter
        for bad in (dict(), dict(factor=1, min_count=0), dict(factor=1, rank_permille=1001), dict(factor=1, reserved=(1, 0, 0, 0)), dict(factor=1, install=3)):
            fails(abi.ERR_INVALID_ARG, d.ts_survey_mask, 0, **bad)
        planes = np.zeros((2, H, W), np.uint32)
        planes[:, 3, 3] = 2 ** 31
        fails(abi.ERR_INVALID_ARG, d.ts_survey_state, 0, set=planes)
        # the bound: events_in + outside may reach 2^32 - 1 and not pass it
        planes[:, 3, 3] = (S.U32_MAX - 3) // 2, (S.U32_MAX - 3) - (S.U32_MAX - 3) // 2
        near = dict(S.STATS0, events_in=S.U32_MAX - 3, outside=2, packets=9, t_first=T0, t_last=T0 + 5)
        d.ts_survey_state(0, set=planes, stats=near)
        assert d.ts_survey_stats(0) == near
        ring = state(d)
        fails(abi.ERR_CAPACITY, feed, d, [(3, 3, T0 + 10, 1), (3, 3, T0 + 11, 0)], "device_columns")
        assert d.ts_survey_stats(0) == near and state(d) == ring
        feed(d, [(3, 3, T0 + 10, 1)], "device_columns")
        assert d.ts_survey_stats(0) == dict(near, events_in=S.U32_MAX - 2, packets=10, t_last=T0 + 10)
        assert int(d.ts_survey_state(0)[:, 3, 3].astype(np.uint64).sum()) == S.U32_MAX - 2
        fails(abi.ERR_CAPACITY, feed, d, [(3, 3, T0 + 12, 1)], "records")
        d.ts_filter_configure(0, 1000, 0)                               # reconfiguring keeps the survey and its counts
        assert d.ts_survey_stats(0)["events_in"] == S.U32_MAX - 2
        d.ts_survey_end(0)
        d.ts_filter_configure(0, off=True)
    finally:
        d.close()


def test_count_only_mode(upenn_rig):
    ev, mask = stream(34)
    d, twin = (make(upenn_rig, ring=ring, refractory_ns=F.REFRACTORY_NS, support_ns=F.SUPPORT_NS, mask=mask) for ring in (1024, 1 << 16))
    try:
        feed(d, ev[:500], "device_columns")
        ring, flt = state(d), filter_state(d)
        d.ts_survey_begin(0, count_only=True)
        unsorted = ev[700:500:-1]                                       # stamps run backwards, and lie behind the staged ones' start
        feed(d, unsorted, "device_columns")
        counts, stats = S.count(unsorted, W, H)
        check(d, counts, stats)
        large = ev[1000:2000]                                           # the ring has room for 524 more at the most
        for how in ("records", "host_columns"):
            feed(d, large, how)
            counts, stats = S.count(large, W, H, counts, stats)
        check(d, counts, stats)
        us = [(x, y, (t - T0) // 1000, p) for x, y, t, p in ev[2000:3000]]
        words = np.array(R3.encode(us, vect=True), np.uint16)
        assert d.ts_push_evt3(0, words, T0 // 1000) == 1000 == twin.ts_push_evt3(0, words, T0 // 1000)
        assert d.evt3_state(0).as_tuple() == twin.evt3_state(0).as_tuple() and d.evt3_stats(0) == twin.evt3_stats(0)
        counts, stats = S.count(ev[2000:3000], W, H, counts, stats)
        check(d, counts, stats)
        x, y, t, p = columns(ev[3000:3100])
        t[40] = -5                                                      # a bad stamp: refused, nothing of the packet counted
        import torch
        for cols in ((x, y, t, p), [torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for v in (x, y, t, p)]):
            with pytest.raises(lib.EsvoError) as e:
                d.ts_push_columns(0, *cols)
            assert e.value.code == abi.ERR_INVALID_ARG and "element 40 " in str(e.value)
            check(d, counts, stats)
        assert state(d) == ring and filter_state(d) == flt             # nothing staged, the filter untouched
        d.ts_survey_end(0)
        feed(d, ev[500:600], "device_columns")                          # and the stream goes on where it stood
        assert d.ts_filter_stats(0)["events_in"] == 600
    finally:
        d.close(); twin.close()


def test_state_round_trip_and_reset(dev):
    ev, _ = stream(35)
    fresh(dev)
    feed(dev, ev[:3000], "device_columns")
    counts, stats = S.count(ev[:3000], W, H)
    got = dev.ts_survey_state(0)
    r = np.random.default_rng(3)
    planted = r.integers(0, 2 ** 31, (2, H, W), dtype=np.uint32)
    pstats = dict(events_in=12345, outside=6, packets=7, t_first=T0 - 5, t_last=T0 + 10 ** 10)
    assert np.array_equal(dev.ts_survey_state(0, set=planted, stats=pstats), got)      # get comes first
    assert dev.ts_survey_stats(0) == pstats
    assert np.array_equal(dev.ts_survey_state(0, set=got, stats=stats), planted)
    check(dev, counts, stats)
    feed(dev, ev[3000:4000], "evt3")                                                  # resumed
    check(dev, *S.count(ev[3000:4000], W, H, counts, stats))
    dev.reset()                                                                       # zeroes, keeps the survey open
    assert dev.ts_survey_stats(0) == S.STATS0 and not dev.ts_survey_state(0).any()
    feed(dev, ev[:100], "records")
    check(dev, *S.count(ev[:100], W, H))


@functools.lru_cache(maxsize=None)
def crafted():
    return {name: (c, stats, rule) for name, c, stats, rule in S.crafted_images(W, H)}


@pytest.mark.parametrize("name", [c[0] for c in S.crafted_images(8, 8)])
def test_the_rule_on_planted_count_images(dev, name):
    c, stats, rule = crafted()[name]
    counts = S.split_planes(c, W, H)
    want_mask, want = S.hot_pixels(counts, stats, W, H, **rule)
    if not dev_has_survey(dev):
        fresh(dev)
    dev.ts_survey_state(0, set=S.counts_array(counts), stats=stats)
    mask, rep = dev.ts_survey_mask(0, **rule)
    assert rep == want
    assert mask.tolist() == want_mask
    hmask, hrep = lib.hot_pixel_mask_host(S.counts_array(counts), stats, W, H, **rule)
    assert hrep == rep and np.array_equal(hmask, mask)
    assert dev.ts_survey_mask(0, want_mask=False, **rule) == (None, want)


def dev_has_survey(dev):
    try:
        dev.ts_survey_stats(0)
        return True
    except lib.EsvoError:
        return False


@pytest.mark.parametrize("install", (abi.MASK_REPLACE, abi.MASK_UNION))
def test_install(upenn_rig, install):
    ev, planted = stream(36)
    a, b = (make(upenn_rig, refractory_ns=F.REFRACTORY_NS, support_ns=F.SUPPORT_NS, mask=planted) for _ in range(2))
    try:
        a.ts_survey_begin(0)
        for d in (a, b):
            feed(d, ev[:4000], "device_columns")
        before = filter_state(a)
        learnt, rep = a.ts_survey_mask(0, install=install, factor=1, rank_permille=500, min_count=3)
        want_mask, want = S.hot_pixels(S.count(ev[:4000], W, H)[0], a.ts_survey_stats(0), W, H, factor=1, rank_permille=500, min_count=3)
        assert rep == want and learnt.tolist() == want_mask and 20 < rep["n_hot"] < W * H // 4
        assert (learnt.astype(bool) & ~np.array(planted, bool)).any() and (np.array(planted, bool) & ~learnt.astype(bool)).any()
        assert filter_state(a) == before == filter_state(b)            # `last` and totals untouched by the install itself
        in_force = learnt if install == abi.MASK_REPLACE else (learnt | np.array(planted, np.uint8))
        b.ts_filter_configure(0, F.REFRACTORY_NS, F.SUPPORT_NS, in_force)               # from the host: zeroes `last` ...
        b.ts_filter_state(0, set=a.ts_filter_state(0))                                  # ... which comes from a
        for d in (a, b):
            feed(d, ev[4000:], "device_columns")
        assert state(a) == state(b) and filter_state(a) == filter_state(b)
        _, _, c = F.run(ev[4000:], W, H, F.REFRACTORY_NS, F.SUPPORT_NS, in_force.tolist(), a_last_before(before))
        assert a.ts_filter_stats(0)["masked"] - before[0]["masked"] == c["masked"] > 0
        assert a.ts_survey_stats(0)["events_in"] == S.count(ev, W, H)[1]["events_in"]   # the survey went on counting
    finally:
        a.close(); b.close()


def a_last_before(before):
    return np.frombuffer(before[1], np.uint64).reshape(H, W).tolist()


def test_end_to_end_calibration(dev):
    """a dark recording -- background over the whole sensor plus five pixels firing 50 times as often -- surveyed count-only, the mask
    learnt and installed on the device, then the stream itself"""
    r = np.random.default_rng(41)
    hot = ((0, 0), (345, 259), (173, 130), (8, 7), (344, 3))
    n_bg, per_hot = W * H // 2, 25                                      # 0.5 events per pixel; 50 times that
    xs, ys = r.integers(0, W, n_bg).tolist(), r.integers(0, H, n_bg).tolist()
    for hx, hy in hot:
        xs += [hx] * per_hot; ys += [hy] * per_hot
    order = r.permutation(len(xs))
    dark = [(xs[k], ys[k], T0 + 20_000 * i, int(i & 1)) for i, k in enumerate(order)]
    rule = dict(min_count=13, factor=3, rank_permille=999)
    counts, stats = None, None
    fresh(dev, count_only=True)
    for a in range(0, len(dark), 16000):
        feed(dev, dark[a:a + 16000], "device_columns")
        counts, stats = S.count(dark[a:a + 16000], W, H, counts, stats)
    want_mask, want = S.hot_pixels(counts, stats, W, H, **rule)
    assert sorted((x, y) for y in range(H) for x in range(W) if want_mask[y][x]) == sorted(hot) and want["n_hot"] == 5    # on the CPU
    mask, rep = dev.ts_survey_mask(0, install=abi.MASK_REPLACE, **rule)
    assert rep == want and mask.tolist() == want_mask
    assert state(dev)["bounds"] == (0, 0) and dev.ts_filter_stats(0)["events_in"] == 0
    dev.ts_survey_end(0)
    live = dark[:6000]
    feed(dev, live, "device_columns")
    tot = dev.ts_filter_stats(0)
    assert tot["masked"] == sum(1 for e in live if (e[0], e[1]) in hot) > 0 and tot["kept"] == 6000 - tot["masked"]
