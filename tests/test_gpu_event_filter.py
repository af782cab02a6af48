"""The event filter on the device (include/esvo_hip.h, esvo_ts_filter_configure): a handle with the filter fed the RAW stream
against a handle without it fed the records the Python-int restatement (tests/event_filter_restated.py) keeps.  The two are
compared byte for byte through esvo_debug_ts_ring (records, stamp mirror, ring_base / ring_next), esvo_get_stats and a rendered
Time Surface; the filtering handle's totals and `last` image against the restatement's.  346x260 (upenn rig), ring 2^16."""
import functools

import numpy as np
import pytest

import event_filter_restated as R
import evt2_restated as R2
import evt3_restated as R3
from esvo_amd import abi, lib, params

pytestmark = pytest.mark.gpu

W, H, T0 = R.W, R.H, R.T_BASE
ERR_UNSUPPORTED = -5
ZERO = dict.fromkeys(R.NAMES + ("events_in",), 0)


def _params(rig, ring):
    return params.make_params(params.PRESETS["mapping_upenn"], rig, max_events_per_tick=4096, event_ring_capacity=ring, regularization=0)[0]


@functools.lru_cache(maxsize=None)
def stream(seed, n=6000):
    return R.random_stream(seed, n)


def columns(events):
    return (np.array([e[0] for e in events], np.uint16), np.array([e[1] for e in events], np.uint16),
            np.array([e[2] for e in events], np.int64), np.array([e[3] for e in events], np.uint8))


def feed(dev, events, how):
    """the raw events to camera 0 of `dev` through one entry point"""
    if how == "records":
        dev.ts_push_events(0, R.records(events))
    elif how == "async":
        ev = R.records(events)
        dev.ts_push_events_async(0, ev)
        dev.ts_push_wait(0)
    elif how == "wire":
        assert dev.ts_push_event_array(0, abi.serialize_event_array(R.records(events), W, H)) == len(events)
    elif how == "host_columns":
        dev.ts_push_columns(0, *columns(events))
    elif how == "device_columns":
        import torch
        x, y, t, p = columns(events)
        d = [torch.from_numpy(x.view(np.int16)).cuda(), torch.from_numpy(y.view(np.int16)).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda()]
        torch.cuda.synchronize()
        dev.ts_push_columns(0, *d)
    elif how == "evt3":
        us = [(x, y, (t - T0) // 1000, p) for x, y, t, p in events]
        assert dev.ts_push_evt3(0, np.array(R3.encode(us, vect=True), np.uint16), T0 // 1000) == len(events)
    elif how in ("evt2", "evt21"):
        fmt = R2.EVT_2_0 if how == "evt2" else R2.EVT_2_1
        us = [(x, y, (t - T0) // 1000, p) for x, y, t, p in events]
        assert dev.ts_push_evt2(0, np.array(R2.encode(us, fmt), np.uint32), fmt, T0 // 1000) == len(events)
    else:
        raise AssertionError(how)


class Pair:
    """a: no filter, fed the records the restatement keeps; b: the filter, fed the raw stream"""

    def __init__(self, rig, ring=1 << 16, refractory_ns=R.REFRACTORY_NS, support_ns=R.SUPPORT_NS, mask=None):
        self.p = _params(rig, ring)
        self.a, self.b = lib.Esvo(self.p, rig), lib.Esvo(self.p, rig)
        self.b.debug_evt3_device_min(0)
        self.b.debug_evt2_device_min(0)
        self.configure(refractory_ns, support_ns, mask)

    def configure(self, refractory_ns, support_ns, mask=None, keep_totals=False):
        self.cfg = (refractory_ns, support_ns, mask)
        self.b.ts_filter_configure(0, refractory_ns, support_ns, mask)
        self.last = R.fresh_last(W, H)
        if not keep_totals:
            self.totals = dict(ZERO)
        return self

    def reset(self):
        self.a.reset(); self.b.reset()
        self.last, self.totals = R.fresh_last(W, H), dict(ZERO)
        return self

    def plant(self, last):
        self.b.ts_filter_state(0, set=R.last_array(last))
        self.last = [list(r) for r in last]

    def push(self, events, how="device_columns"):
        v, self.last, c = R.run(events, W, H, self.cfg[0], self.cfg[1], self.cfg[2], self.last)
        for k in c:
            self.totals[k] += c[k]
        want = R.records(R.kept(events, v))
        if len(want):
            self.a.ts_push_events(0, want)
        feed(self.b, events, how)
        return v

    def close(self):
        self.a.close(); self.b.close()


def state(dev, cam=0):
    ev, st, b0, b1 = dev.debug_ts_ring(cam)
    s = dev.stats()
    return dict(records=ev.tobytes(), stamps=st.tobytes(), bounds=(b0, b1), staged=int(s.events_staged[cam]), late=int(s.late_events[cam]))


def filter_state(dev):
    return dev.ts_filter_stats(0), dev.ts_filter_state(0).tobytes()


def same(pr, render=False):
    sa, sb = state(pr.a), state(pr.b)
    for k in sa:
        assert sa[k] == sb[k], k
    assert pr.b.ts_filter_stats(0) == pr.totals
    assert pr.b.ts_filter_state(0).tobytes() == R.last_array(pr.last).tobytes()
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


def fresh(pair, refractory_ns=R.REFRACTORY_NS, support_ns=R.SUPPORT_NS, mask=None):
    return pair.reset().configure(refractory_ns, support_ns, mask)


@pytest.mark.parametrize("how", ("records", "async", "wire", "host_columns", "device_columns", "evt3", "evt2", "evt21"))
def test_random_stream_through_every_entry_point(pair, how):
    ev, mask = stream(11)
    fresh(pair, mask=mask)
    v = pair.push(ev, how)
    assert min(v.count(k) for k in range(5)) >= 0.03 * len(ev)
    st = same(pair, render=True)
    assert st["staged"] == pair.totals["kept"] == v.count(R.KEPT)


@pytest.mark.parametrize("seed,sizes", ((11, (1, 63, 64, 65, 2047, 2048)), (12, (2049, 1, 65, 2047, 64))))
def test_stream_cut_into_packets(pair, seed, sizes):
    ev, mask = stream(seed)
    whole, _, _ = R.run(ev, W, H, R.REFRACTORY_NS, R.SUPPORT_NS, mask)
    fresh(pair, mask=mask)
    a, got = 0, []
    for m in sizes + (len(ev),):
        got += pair.push(ev[a:a + m])
        same(pair)
        a += m
    assert a >= len(ev) and got == whole       # however the stream is cut, the verdicts are those of one packet
    same(pair, render=True)


@pytest.mark.parametrize("kept", (0, 1, 63, 64, 65, 2049))
def test_kept_counts_at_the_compaction_seams(pair, kept):
    """4096 events over `kept` pixels under a refractory period longer than the packet: the first event of every pixel is kept"""
    r = np.random.default_rng(kept)
    mask = None
    if kept == 0:
        mask, ids = np.ones((H, W), int).tolist(), r.integers(0, 3000, 4096)
    else:
        ids = np.concatenate([r.permutation(kept), r.integers(0, kept, 4096 - kept)])
        r.shuffle(ids)
    ev = [(int(k) % W, int(k) // W, T0 + 1000 * i, i & 1) for i, k in enumerate(ids)]
    fresh(pair, 10 ** 9, 0, mask)
    v = pair.push(ev)
    assert v.count(R.KEPT) == kept
    same(pair, render=True)


def _one_pixel_chain():
    return [(100, 100, T0 + 1000 * i, i & 1) for i in range(4096)]


def test_one_pixel_with_a_refractory_chain(pair):
    fresh(pair, 10_000, 0)
    v = pair.push(_one_pixel_chain())
    assert v.count(R.KEPT) == 410 and v.count(R.REFRACTORY) == 4096 - 410
    same(pair, render=True)


def test_tile_list_capacity_forced_to_four(upenn_rig, monkeypatch):
    """ESVO_FLT_TILE_CAP = 4: nearly every tile reads the packet instead of its list"""
    monkeypatch.setenv("ESVO_FLT_TILE_CAP", "4")
    pr = Pair(upenn_rig)
    try:
        pr.configure(10_000, 0)
        pr.push(_one_pixel_chain())
        same(pr)
        ev, mask = stream(13)
        pr.reset().configure(R.REFRACTORY_NS, R.SUPPORT_NS, mask)
        pr.push(ev[:3000]); pr.push(ev[3000:])
        same(pr, render=True)
    finally:
        pr.close()


def test_support_across_tile_seams_and_partial_tiles(pair):
    fresh(pair, 0, 1000)
    ev, t = [], T0
    for (ax, ay), (bx, by) in (((7, 7), (8, 8)), ((8, 7), (7, 8)), ((7, 20), (8, 20)), ((20, 8), (20, 7)), ((15, 15), (16, 16)),
                               ((343, 255), (344, 256)), ((345, 257), (344, 258)), ((345, 259), (344, 259)), ((344, 256), (345, 256)),
                               ((40, 40), (42, 40))):
        ev += [(ax, ay, t, 1), (bx, by, t + 500, 0)]
        t += 10_000
    v = pair.push(ev)
    assert v == [R.UNSUPPORTED, R.KEPT] * 9 + [R.UNSUPPORTED, R.UNSUPPORTED]     # (the last pair lies two columns apart)
    same(pair, render=True)


def test_support_that_comes_only_from_a_planted_state(pair):
    fresh(pair, 2000, 1000)
    last = R.fresh_last(W, H)
    last[8][7] = T0 - 400         # neighbour of (8, 8) across the seam 7 | 8
    last[50][50] = T0 - 1500      # its own pixel: still refractory
    last[259][345] = T0 - 1000    # the last pixel of the last partial tile, support_ns away
    pair.plant(last)
    assert pair.b.ts_filter_state(0).tobytes() == R.last_array(last).tobytes()
    v = pair.push([(8, 8, T0, 1), (50, 50, T0, 1), (344, 258, T0, 0), (100, 100, T0 + 1, 1)])
    assert v == [R.KEPT, R.REFRACTORY, R.KEPT, R.UNSUPPORTED]
    same(pair, render=True)


def test_a_packet_of_which_nothing_is_kept(pair):
    fresh(pair, 0, 2000)
    ev = [(10 + 3 * i, 10, T0 + 1000 * i, 1) for i in range(70)] + [(W, 5, T0 + 70_000, 1)]
    v = pair.push(ev)
    assert v.count(R.KEPT) == 0 and v.count(R.UNSUPPORTED) == 70
    st = same(pair)
    assert st["bounds"] == (0, 0) and pair.last[10][10] == T0     # nothing staged, `last` advanced all the same
    v = pair.push([(218, 11, T0 + 70_500, 0)])    # supported by the last of them alone
    assert v == [R.KEPT]
    same(pair, render=True)


def test_refusals_leave_everything_as_it_was(upenn_rig):
    pr = Pair(upenn_rig, 1024, 0, 0, None)
    try:
        mask = np.zeros((H, W), int)
        mask[:, 200:] = 1
        pr.configure(500, 1000, mask.tolist())
        pr.push([(i % 100, i // 100, T0 + 1000 * i, 1) for i in range(800)], "host_columns")
        before, fbefore = same(pr), filter_state(pr.b)
        decoders = lambda: (pr.b.evt3_state(0).as_tuple(), pr.b.evt3_stats(0), pr.b.evt2_state(0).as_tuple(), pr.b.evt2_stats(0))  # noqa: E731
        dbefore = decoders()
        cases = (
            ([(5, 5, T0 + 900_000, 1), (6, 6, T0 + 899_000, 1)], "records", ERR_UNSUPPORTED),           # not sorted in itself
            ([(5, 5, T0 + 1000, 1), (6, 6, T0 + 2000, 1)], "device_columns", ERR_UNSUPPORTED),          # older than the newest staged stamp
            ([(5, 5, T0 + 900_000, 1), (6, 6, T0 + 899_000, 1)], "device_columns", ERR_UNSUPPORTED),    # the same two, judged on the device
            ([(5, 5, T0 + 1000, 1), (6, 6, T0 + 2000, 1)], "host_columns", ERR_UNSUPPORTED),
            ([(5, 5, T0 + 1000, 1), (6, 6, T0 + 2000, 1)], "evt3", ERR_UNSUPPORTED),                    # decoded words: the decoder state stays too
            ([(5, 5, T0 + 3000, 1), (6, 6, T0 + 2000, 1)], "evt2", ERR_UNSUPPORTED),
            ([(250, 5, T0 + 900_000 + i, 1) for i in range(300)], "host_columns", abi.ERR_CAPACITY),   # all masked, yet judged unfiltered
            ([(5, 5, T0 + 900_000 + i, 1) for i in range(1025)], "records", abi.ERR_CAPACITY),         # more than the ring holds
        )
        for ev, how, code in cases:
            with pytest.raises(lib.EsvoError) as e:
                feed(pr.b, ev, how)
            assert e.value.code == code, (how, code)
            assert state(pr.b) == before and filter_state(pr.b) == fbefore and decoders() == dbefore
        x, y, t, p = columns([(5, 5, T0 + 900_000, 1), (6, 6, T0 + 900_001, 1)])
        t[1] = -5                                                                                      # a bad column stamp
        with pytest.raises(lib.EsvoError) as e:
            pr.b.ts_push_columns(0, x, y, t, p)
        assert e.value.code == abi.ERR_INVALID_ARG
        assert state(pr.b) == before and filter_state(pr.b) == fbefore
        import torch
        with pytest.raises(lib.EsvoError) as e:                                                        # the same in device memory
            pr.b.ts_push_columns(0, *[torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for v in (x, y, t, p)])
        assert e.value.code == abi.ERR_INVALID_ARG and "element 1 " in str(e.value)
        assert state(pr.b) == before and filter_state(pr.b) == fbefore
        pr.push([(5, 5, T0 + 900_000, 1), (6, 6, T0 + 900_001, 1)])                                    # and the stream goes on
        same(pr)
    finally:
        pr.close()


def test_reset_against_a_fresh_configured_handle(pair, upenn_rig):
    ev, mask = stream(12)
    fresh(pair, mask=mask)
    pair.push(ev[:2000])
    pair.a.reset(); pair.b.reset()               # keeps the configuration, zeroes `last` and the totals
    assert pair.b.ts_filter_stats(0) == ZERO and not pair.b.ts_filter_state(0).any()
    other = Pair(upenn_rig, mask=mask)
    try:
        for pr in (pair, other):
            feed(pr.b, ev[2000:4000], "device_columns")
        assert state(pair.b) == state(other.b) and filter_state(pair.b) == filter_state(other.b)
        assert pair.b.ts_filter_stats(0)["events_in"] == 2000
    finally:
        other.close()


def test_configure_off_configure_frees_its_memory(upenn_rig):
    ev, mask = stream(13)
    dev = lib.Esvo(_params(upenn_rig, 1 << 16), upenn_rig)
    try:
        def cycle():
            dev.ts_filter_configure(0, R.REFRACTORY_NS, R.SUPPORT_NS, mask)
            feed(dev, ev[:500], "host_columns")
            on = lib.debug_live_allocations()
            dev.ts_filter_configure(0, off=True)
            dev.reset()
            return on, lib.debug_live_allocations()
        first = cycle()
        assert first[0][0] > first[1][0] and first[0][1] > first[1][1]
        assert cycle() == first
        feed(dev, ev[:500], "host_columns")       # off: the unfiltered path
        assert int(dev.stats().events_staged[0]) == 500 and dev.ts_filter_stats(0) == ZERO
        with pytest.raises(lib.EsvoError) as e:
            dev.ts_filter_state(0)
        assert e.value.code == abi.ERR_STATE
    finally:
        dev.close()


def test_row_routed_handles_refuse(upenn_rig):
    p = params.make_params(params.PRESETS["mvstereo_upenn"], upenn_rig)[0]
    routed, filtering = lib.Esvo(p, upenn_rig), lib.Esvo(p, upenn_rig)
    try:
        routed.set_band(0, H // 2, 0, 2, routing="y_rect")
        with pytest.raises(lib.EsvoError) as e:
            routed.ts_filter_configure(0, 1000, 1000)
        assert e.value.code == ERR_UNSUPPORTED
        filtering.ts_filter_configure(0, 1000, 1000)
        with pytest.raises(lib.EsvoError) as e:
            filtering.set_band(0, H // 2, 0, 2, routing="y_rect")
        assert e.value.code == ERR_UNSUPPORTED
        filtering.set_band(0, H // 2, 0, 2, routing="broadcast")      # every rank sees the whole stream: fine
        feed(filtering, [(5, 5, T0, 1), (6, 6, T0 + 10, 1)], "records")
        assert filtering.ts_filter_stats(0)["kept"] == 1
    finally:
        routed.close(); filtering.close()
