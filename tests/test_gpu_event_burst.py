"""The burst stage of the event filter on the device (include/esvo_hip.h, esvo_ts_burst_configure): a handle with filter and stage fed
the RAW stream against a handle without either fed the records the Python-int restatement (tests/event_burst_restated.py) keeps.
The two are compared byte for byte through esvo_debug_ts_ring (records, stamp mirror, ring_base / ring_next), esvo_get_stats and a
rendered Time Surface; the filtering handle's two totals, its `last` image and the stage's bstamp / bflags against the restatement's.
346x260 (upenn rig: 43 full tile columns + 2 pixels, 32 full tile rows + 4 pixels), ring 2^16."""
import functools

import numpy as np
import pytest

import event_burst_restated as B
import event_filter_restated as R
import test_gpu_event_filter as G
from esvo_amd import abi, lib, params

pytestmark = pytest.mark.gpu

W, H, T0 = B.W, B.H, B.T_BASE
ERR_UNSUPPORTED = -5
ZERO = G.ZERO
K, D, U, RF, M, O = B.KEPT, B.BURST, B.UNSUPPORTED, B.REFRACTORY, B.MASKED, B.OUTSIDE


@functools.lru_cache(maxsize=None)
def stream(seed):
    return B.bursty_stream(seed)


def feed(dev, events, how):
    if how == "i8_columns":       # polarity as -1 / +1 int8
        x, y, t, p = G.columns(events)
        dev.ts_push_columns(0, x, y, t, np.where(p != 0, 1, -1).astype(np.int8))
    else:
        G.feed(dev, events, how)


class Pair:
    """a: no filter, fed the records the restatement keeps; b: filter and burst stage, fed the raw stream"""

    def __init__(self, rig, ring=1 << 16):
        self.p = G._params(rig, ring)
        self.a, self.b = lib.Esvo(self.p, rig), lib.Esvo(self.p, rig)
        self.b.debug_evt3_device_min(0)
        self.b.debug_evt2_device_min(0)
        self.totals, self.btotals = dict(ZERO), dict(B.ZERO_BURST)

    def configure(self, mode, burst_ns=B.BURST_NS, refractory_ns=B.REFRACTORY_NS, support_ns=B.SUPPORT_NS, mask=None):
        """filter and stage anew: all three images zero, the totals kept"""
        self.cfg = (mode, burst_ns, refractory_ns, support_ns, mask)
        self.b.ts_filter_configure(0, refractory_ns, support_ns, mask)
        self.b.ts_burst_configure(0, mode, burst_ns)
        self.last, self.bstamp, self.bflags = B.fresh(W, H), B.fresh(W, H), B.fresh(W, H)
        return self

    def reset(self):
        self.a.reset(); self.b.reset()
        self.last, self.bstamp, self.bflags = B.fresh(W, H), B.fresh(W, H), B.fresh(W, H)
        self.totals, self.btotals = dict(ZERO), dict(B.ZERO_BURST)
        return self

    def plant(self, bstamp, bflags):
        self.b.ts_burst_state(0, set=(B.stamp_array(bstamp), B.flags_array(bflags)))
        self.bstamp, self.bflags = [list(r) for r in bstamp], [list(r) for r in bflags]

    def push(self, events, how="device_columns"):
        mode, burst_ns, refractory_ns, support_ns, mask = self.cfg
        v, self.bstamp, self.bflags, self.last, bc, fc = B.run(events, W, H, mode, burst_ns, refractory_ns, support_ns, mask, self.bstamp, self.bflags, self.last)
        for k in fc:
            self.totals[k] += fc[k]
        for k in bc:
            self.btotals[k] += bc[k]
        want = R.records(B.kept(events, v))
        if len(want):
            self.a.ts_push_events(0, want)
        feed(self.b, events, how)
        return v

    def close(self):
        self.a.close(); self.b.close()


def stage_state(dev):
    st, fl = dev.ts_burst_state(0)
    return dev.ts_filter_stats(0), dev.ts_filter_state(0).tobytes(), dev.ts_burst_stats(0), st.tobytes(), fl.tobytes()


def same(pr, render=False):
    sa, sb = G.state(pr.a), G.state(pr.b)
    for k in sa:
        assert sa[k] == sb[k], k
    assert pr.b.ts_filter_stats(0) == pr.totals
    assert pr.b.ts_burst_stats(0) == pr.btotals
    assert pr.b.ts_filter_state(0).tobytes() == R.last_array(pr.last).tobytes()
    st, fl = pr.b.ts_burst_state(0)
    assert st.tobytes() == B.stamp_array(pr.bstamp).tobytes()
    assert fl.tobytes() == B.flags_array(pr.bflags).tobytes()
    if render and sa["bounds"][1] > sa["bounds"][0]:
        t = int(np.frombuffer(sa["stamps"], np.uint64)[-1]) + 1
        img = [d.ts_render(0, t) for d in (pr.a, pr.b)]
        assert np.array_equal(img[0], img[1])
    return sa


@pytest.fixture(scope="module")
def pair(upenn_rig):
    pr = Pair(upenn_rig)
    yield pr
    pr.close()


def fresh(pair, mode, **kw):
    return pair.reset().configure(mode, **kw)


@pytest.mark.parametrize("how,mode", (("records", B.TRAIL), ("async", B.STC_CUT_TRAIL), ("wire", B.STC_KEEP_TRAIL), ("host_columns", B.TRAIL),
                                      ("device_columns", B.STC_CUT_TRAIL), ("evt3", B.STC_KEEP_TRAIL), ("evt2", B.TRAIL), ("evt21", B.STC_CUT_TRAIL),
                                      ("i8_columns", B.STC_KEEP_TRAIL), ("device_columns", B.TRAIL), ("evt3", B.STC_CUT_TRAIL), ("evt2", B.STC_KEEP_TRAIL)))
def test_bursty_stream_through_every_entry_point(pair, how, mode):
    ev, mask = stream(21)
    fresh(pair, mode, mask=mask)
    v = pair.push(ev, how)
    share = B.shares(v)
    assert min(s for k, s in enumerate(share) if not (mode == B.STC_CUT_TRAIL and k == RF)) >= 0.03      # (tests/test_event_burst_restated.py)
    st = same(pair, render=True)
    assert st["staged"] == pair.totals["kept"] == v.count(K)
    assert pair.totals["events_in"] + pair.btotals["dropped"] == len(ev)


@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("seed,sizes", ((22, (1, 63, 64, 65, 2047, 2048)), (23, (2049, 1, 65, 2047, 64))))
def test_stream_cut_into_packets(pair, seed, sizes, mode):
    ev, mask = stream(seed)
    whole = B.run(ev, W, H, mode, B.BURST_NS, B.REFRACTORY_NS, B.SUPPORT_NS, mask)[0]
    fresh(pair, mode, mask=mask)
    a, got = 0, []
    for m in sizes + (len(ev),):
        got += pair.push(ev[a:a + m])
        same(pair)
        a += m
    assert a >= len(ev) and got == whole       # however the stream is cut, the verdicts are those of one packet: `linked` and polarity carry
    same(pair, render=True)


# one-pixel chains: (gaps in ns behind the first event, polarities, the verdicts by mode); burst_ns = 1000, no other test on
CHAINS = (
    ((1000, 1001), (1, 1, 1), {B.TRAIL: [K, D, K], B.STC_CUT_TRAIL: [D, K, D], B.STC_KEEP_TRAIL: [D, K, D]}),                 # exactly burst_ns links, one more does not
    ((0, 0), (0, 0, 0), {B.TRAIL: [K, D, D], B.STC_CUT_TRAIL: [D, K, D], B.STC_KEEP_TRAIL: [D, K, K]}),                       # equal stamps link
    ((10, 10, 10), (1, 1, 0, 0), {B.TRAIL: [K, D, K, D], B.STC_CUT_TRAIL: [D, K, D, K], B.STC_KEEP_TRAIL: [D, K, D, K]}),     # a polarity flip inside the window
    ((100,) * 5, (1,) * 6, {B.TRAIL: [K] + [D] * 5, B.STC_CUT_TRAIL: [D, K] + [D] * 4, B.STC_KEEP_TRAIL: [D] + [K] * 5}),     # six linked events
    ((), (1,), {B.TRAIL: [K], B.STC_CUT_TRAIL: [D], B.STC_KEEP_TRAIL: [D]}),                                                # an isolated event
)
CHAIN_PIXELS = ((7, 7), (8, 8), (100, 100), (345, 259), (344, 255))      # both sides of a seam, a tile's middle, the last partial tiles


@pytest.mark.parametrize("mode", B.MODES)
def test_crafted_one_pixel_chains(pair, mode):
    fresh(pair, mode, burst_ns=1000, refractory_ns=0, support_ns=0)
    ev, who = [], []
    for c, ((gaps, pols, _), (x, y)) in enumerate(zip(CHAINS, CHAIN_PIXELS)):
        t = T0 + 37 * c
        for i, p in enumerate(pols):
            t += gaps[i - 1] if i else 0
            ev.append((x, y, t, p)); who.append(c)
    order = sorted(range(len(ev)), key=lambda i: ev[i][2])      # (stable)
    v = pair.push([ev[i] for i in order])
    for c, (_, _, want) in enumerate(CHAINS):
        assert [v[k] for k, i in enumerate(order) if who[i] == c] == want[mode], c
    same(pair, render=True)


def test_cut_meets_refractory_between_two_bursts_of_opposite_polarity(pair):
    ev = [(9, 9, T0, 1), (9, 9, T0 + 100, 1), (9, 9, T0 + 200, 0), (9, 9, T0 + 300, 0)]      # CUT passes the second of each burst, 200 ns apart
    fresh(pair, B.STC_CUT_TRAIL, burst_ns=1000, refractory_ns=500, support_ns=0)
    assert pair.push(ev) == [D, K, D, RF]
    same(pair)
    fresh(pair, B.STC_CUT_TRAIL, burst_ns=1000, refractory_ns=200, support_ns=0)
    assert pair.push(ev) == [D, K, D, K]
    same(pair, render=True)


def test_seams_dropped_events_support_nothing_and_restart_nothing(pair):
    mask = np.zeros((H, W), int)
    mask[30, 30] = 1
    fresh(pair, B.TRAIL, burst_ns=1000, refractory_ns=180, support_ns=120, mask=mask.tolist())
    ev, t = [], T0
    pairs = (((7, 7), (8, 8)), ((8, 7), (7, 8)), ((7, 20), (8, 20)), ((20, 8), (20, 7)), ((343, 255), (344, 256)), ((345, 257), (344, 258)),
             ((345, 259), (344, 259)), ((344, 256), (345, 256)))
    for a, b in pairs:
        # a passes (alone: unsupported), a again is burst-dropped, b 150 ns behind a's first finds no support (50 ns behind the dropped one it
        # would), a with the other polarity 190 ns behind its first is out of the refractory period (90 ns behind the dropped one it would not be)
        ev += [a + (t, 1), a + (t + 100, 1), b + (t + 150, 1), a + (t + 190, 0)]
        t += 10_000
    ev += [(30, 30, t, 1), (W, 30, t + 1, 1), (30, H, t + 2, 1), (30, 30, t + 3, 1)]
    v = pair.push(ev)
    assert v == [U, D, U, K] * len(pairs) + [M, O, O, M]
    assert pair.bstamp[30][30] == 0 and pair.bflags[30][30] == 0 and pair.btotals["judged"] == 4 * len(pairs)
    same(pair, render=True)


@pytest.mark.parametrize("mode,want", ((B.TRAIL, [K, D, K, D, D]), (B.STC_CUT_TRAIL, [D, K, D, D, K]), (B.STC_KEEP_TRAIL, [D, K, D, K, K])))
def test_planted_state_alone_decides_the_first_event(pair, mode, want):
    fresh(pair, mode, burst_ns=1000, refractory_ns=0, support_ns=0)
    S, F = B.fresh(W, H), B.fresh(W, H)
    px = ((7, 8), (8, 7), (200, 100), (345, 259), (344, 3))       # flags 0, 1, 2, 3 ten ns back; flags 1 at a stamp a second AHEAD of the stream
    for f, (x, y) in enumerate(px[:4]):
        S[y][x], F[y][x] = T0 - 10, f
    S[3][344], F[3][344] = T0 + 10 ** 9, 1
    pair.plant(S, F)
    got = pair.b.ts_burst_state(0)
    assert got[0].tobytes() == B.stamp_array(S).tobytes() and got[1].tobytes() == B.flags_array(F).tobytes()
    assert pair.push([(x, y, T0 + i, 1) for i, (x, y) in enumerate(px)]) == want
    same(pair, render=True)


@pytest.mark.parametrize("mode,kept", ((B.TRAIL, 1), (B.STC_CUT_TRAIL, 1), (B.STC_KEEP_TRAIL, 2048)))
def test_one_pixel_receives_a_whole_packet(pair, mode, kept):
    """2049 same-polarity events at one unmasked pixel: its tile's list overflows, and the chain crosses every batch of the overflow route"""
    fresh(pair, mode, refractory_ns=0, support_ns=0)
    v = pair.push([(101, 99, T0 + 1000 * i, 1) for i in range(2049)])
    assert v.count(K) == kept and v.count(D) == 2049 - kept and v[0 if mode == B.TRAIL else 1] == K       # TRAIL keeps #1, both STC modes keep #2
    same(pair, render=True)


def test_tile_list_capacity_forced_to_four(upenn_rig, monkeypatch):
    """ESVO_FLT_TILE_CAP = 4: nearly every tile reads the packet instead of its list, in the burst kernel and in the walk"""
    monkeypatch.setenv("ESVO_DEV_SWITCHES", "1")
    monkeypatch.setenv("ESVO_FLT_TILE_CAP", "4")
    pr = Pair(upenn_rig)
    try:
        ev, mask = stream(23)
        for mode in B.MODES:
            pr.reset().configure(mode, refractory_ns=0, support_ns=0)
            pr.push([(101, 99, T0 + 1000 * i, i // 700 & 1) for i in range(2049)])
            same(pr)
            pr.reset().configure(mode, mask=mask)
            pr.push(ev[:3000]); pr.push(ev[3000:])
            same(pr, render=True)
    finally:
        pr.close()


def test_a_packet_of_which_the_stage_drops_everything(pair):
    fresh(pair, B.STC_KEEP_TRAIL, burst_ns=1000, refractory_ns=0, support_ns=0)
    ev = [(10 + 3 * i, 10 + i, T0 + 10 * i, i & 1) for i in range(70)]           # isolated events: STC drops each
    assert pair.push(ev) == [D] * 70
    st = same(pair)
    assert st["bounds"] == (0, 0) and pair.bstamp[10][10] == T0 and pair.btotals == {"judged": 70, "passed": 0, "dropped": 70}
    assert pair.totals["events_in"] == 0
    assert pair.push([(10, 10, T0 + 900, 0), (13, 11, T0 + 901, 0)]) == [K, D]   # the first links to the state that packet left, the second's polarity differs
    same(pair, render=True)


def test_refusals_leave_everything_as_it_was(upenn_rig):
    pr = Pair(upenn_rig, 1024)
    try:
        mask = np.zeros((H, W), int)
        mask[:, 200:] = 1
        pr.configure(B.STC_KEEP_TRAIL, burst_ns=5000, refractory_ns=500, support_ns=0, mask=mask.tolist())
        pr.push([(i // 2 % 100, i // 200, T0 + 1000 * i, 1) for i in range(800)], "host_columns")      # pairs 1 us apart: the second of each passes
        before, sbefore = same(pr), stage_state(pr.b)
        assert pr.btotals["passed"] > 0 and pr.btotals["dropped"] > 0
        cases = (
            ([(5, 1, T0 + 900_000, 1), (6, 1, T0 + 899_000, 1)], "records", ERR_UNSUPPORTED),           # not sorted in itself
            ([(5, 1, T0 + 1000, 1), (6, 1, T0 + 2000, 1)], "device_columns", ERR_UNSUPPORTED),          # older than the newest staged stamp
            ([(5, 1, T0 + 900_000, 1), (6, 1, T0 + 899_000, 1)], "device_columns", ERR_UNSUPPORTED),    # the same two, judged on the device
            ([(5, 1, T0 + 1000, 1), (6, 1, T0 + 2000, 1)], "evt3", ERR_UNSUPPORTED),
            ([(250, 1, T0 + 900_000 + i, 1) for i in range(700)], "host_columns", abi.ERR_CAPACITY),   # all masked, yet judged unfiltered (400 are staged)
            ([(5, 1, T0 + 900_000 + i, 1) for i in range(1025)], "records", abi.ERR_CAPACITY),         # more than the ring holds
        )
        for ev, how, code in cases:
            with pytest.raises(lib.EsvoError) as e:
                feed(pr.b, ev, how)
            assert e.value.code == code, (how, code)
            assert G.state(pr.b) == before and stage_state(pr.b) == sbefore
        import torch
        x, y, t, p = G.columns([(5, 1, T0 + 900_000, 1), (5, 1, T0 + 900_001, 1)])
        t[1] = -5                                                                                      # a bad stamp, found on the device
        with pytest.raises(lib.EsvoError) as e:
            pr.b.ts_push_columns(0, *[torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for v in (x, y, t, p)])
        assert e.value.code == abi.ERR_INVALID_ARG
        assert G.state(pr.b) == before and stage_state(pr.b) == sbefore
        pr.push([(5, 1, T0 + 900_000, 1), (5, 1, T0 + 900_001, 1)])                                    # and the stream goes on
        same(pr)
    finally:
        pr.close()


def test_reset_against_a_fresh_configured_handle(pair, upenn_rig):
    ev, mask = stream(22)
    fresh(pair, B.STC_CUT_TRAIL, mask=mask)
    pair.push(ev[:2000])
    pair.a.reset(); pair.b.reset()               # keeps both configurations, zeroes the three images and both totals
    st, fl = pair.b.ts_burst_state(0)
    assert pair.b.ts_burst_stats(0) == B.ZERO_BURST and pair.b.ts_filter_stats(0) == ZERO and not st.any() and not fl.any()
    other = Pair(upenn_rig).configure(B.STC_CUT_TRAIL, mask=mask)
    try:
        for pr in (pair, other):
            feed(pr.b, ev[2000:4000], "device_columns")
        assert G.state(pair.b) == G.state(other.b) and stage_state(pair.b) == stage_state(other.b)
        bc = pair.b.ts_burst_stats(0)
        assert bc["dropped"] > 0 and pair.b.ts_filter_stats(0)["events_in"] + bc["dropped"] == 2000
    finally:
        other.close()


def test_configure_off_configure_frees_and_zeroes(upenn_rig):
    ev, mask = stream(23)
    dev = lib.Esvo(G._params(upenn_rig, 1 << 16), upenn_rig)
    try:
        dev.ts_filter_configure(0, B.REFRACTORY_NS, B.SUPPORT_NS, mask)
        feed(dev, ev[:500], "host_columns")
        base = lib.debug_live_allocations()

        def cycle():
            dev.ts_burst_configure(0, B.TRAIL, B.BURST_NS)
            st, fl = dev.ts_burst_state(0)
            assert not st.any() and not fl.any()
            feed(dev, ev[500:1000], "host_columns")
            assert dev.ts_burst_state(0)[0].any()
            on = lib.debug_live_allocations()
            dev.ts_burst_configure(0, B.OFF)
            dev.reset()
            return on, lib.debug_live_allocations()
        first = cycle()
        assert first[0][0] > first[1][0] and first[0][1] > first[1][1] and first[1] == base
        assert cycle() == first
        with pytest.raises(lib.EsvoError) as e:
            dev.ts_burst_state(0)
        assert e.value.code == abi.ERR_STATE
        dev.ts_filter_configure(0, off=True)       # the stage is off: the filter may go
    finally:
        dev.close()


def test_state_argument_and_routing_refusals(upenn_rig):
    p = params.make_params(params.PRESETS["mvstereo_upenn"], upenn_rig)[0]
    dev, routed = lib.Esvo(p, upenn_rig), lib.Esvo(p, upenn_rig)
    try:
        def code(fn, *a, **kw):
            with pytest.raises(lib.EsvoError) as e:
                fn(*a, **kw)
            return e.value.code
        assert code(dev.ts_burst_configure, 0, B.TRAIL, 1000) == abi.ERR_STATE              # no filter
        dev.ts_burst_configure(0, B.OFF)                                                    # off without a filter: nothing to do
        dev.ts_filter_configure(0, 0, 0)
        assert code(dev.ts_burst_configure, 0, 4, 1000) == abi.ERR_INVALID_ARG              # unknown mode
        assert code(dev.ts_burst_configure, 0, B.TRAIL, 0) == abi.ERR_INVALID_ARG           # no window
        assert code(dev.ts_burst_configure, 0, B.TRAIL, 1000, (0, 0, 1)) == abi.ERR_INVALID_ARG
        assert code(dev.ts_burst_state, 0) == abi.ERR_STATE
        dev.ts_burst_configure(0, B.TRAIL, 1000)
        assert code(dev.ts_filter_configure, 0, off=True) == abi.ERR_STATE                  # the stage is on
        assert code(dev.set_band, 0, H // 2, 0, 2, routing="y_rect") == ERR_UNSUPPORTED     # filter and stage need the whole stream
        feed(dev, [(5, 5, T0, 1), (5, 5, T0 + 10, 1), (6, 6, T0 + 20, 0)], "records")
        kept = stage_state(dev)
        assert kept[2] == {"judged": 3, "passed": 2, "dropped": 1} and kept[0]["events_in"] == 2
        dev.ts_filter_configure(0, 1000, 0)                                                 # a reconfiguration keeps the stage, its state and its totals
        now = stage_state(dev)
        assert now[2:] == kept[2:] and now[0] == kept[0] and not dev.ts_filter_state(0).any()
        feed(dev, [(5, 5, T0 + 30, 1)], "records")                                          # polarity 1 again, 20 ns behind (5, 5)'s last: linked
        assert dev.ts_burst_stats(0) == {"judged": 4, "passed": 2, "dropped": 2}
        S, F = dev.ts_burst_state(0)
        bad = F.copy()
        bad[3, 3] = 4
        assert code(dev.ts_burst_state, 0, set=(S, bad)) == abi.ERR_INVALID_ARG             # a flag byte above 3
        assert dev.lib.esvo_ts_burst_state(dev.h, 0, None, None, S.ctypes.data, None) == abi.ERR_INVALID_ARG
        assert dev.lib.esvo_ts_burst_state(dev.h, 0, None, None, None, F.ctypes.data) == abi.ERR_INVALID_ARG
        assert stage_state(dev)[3:] == (S.tobytes(), F.tobytes())
        routed.set_band(0, H // 2, 0, 2, routing="y_rect")
        assert code(routed.ts_filter_configure, 0, 1000, 1000) == ERR_UNSUPPORTED           # no filter on a row-routed handle,
        assert code(routed.ts_burst_configure, 0, B.TRAIL, 1000) == abi.ERR_STATE           # so no stage
    finally:
        dev.close(); routed.close()


def test_stage_configured_off_is_the_filter_alone(pair):
    ev, mask = R.random_stream(11)
    fresh(pair, B.OFF, burst_ns=0, refractory_ns=R.REFRACTORY_NS, support_ns=R.SUPPORT_NS, mask=mask)
    want_v, want_last, want_c = R.run(ev, W, H, R.REFRACTORY_NS, R.SUPPORT_NS, mask)
    pair.b.ts_burst_configure(0, B.TRAIL, 1000)      # on, then configured OFF again: the filter alone from here
    pair.b.ts_burst_configure(0, B.OFF)
    mode, burst_ns, refractory_ns, support_ns, _ = pair.cfg
    v = B.run(ev, W, H, mode, burst_ns, refractory_ns, support_ns, mask)[0]
    assert v == want_v
    want = R.records(R.kept(ev, want_v))
    pair.a.ts_push_events(0, want)
    feed(pair.b, ev, "device_columns")
    sa, sb = G.state(pair.a), G.state(pair.b)
    assert sa == sb
    assert pair.b.ts_filter_stats(0) == want_c and pair.b.ts_filter_state(0).tobytes() == R.last_array(want_last).tobytes()
    assert pair.b.ts_burst_stats(0) == B.ZERO_BURST
    with pytest.raises(lib.EsvoError) as e:
        pair.b.ts_burst_state(0)
    assert e.value.code == abi.ERR_STATE
