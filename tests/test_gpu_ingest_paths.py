"""Every ingest format and every scatter walk where the event ring wraps (esvo_amd/csrc/api_ingest.hip, api_words.hip; the scatter: api_ts.hip): handles that are fed the
same events by different routes, or hold them in rings of different size, must end in the same state.  Built like
tests/test_gpu_event_columns.py (whose packets and state comparison are used here): upenn rig, a ring of 1024 slots, crafted
packets in a small pixel box so that the median filter keeps them, the state read through esvo_debug_ts_ring."""
import numpy as np
import pytest

from esvo_amd import abi, lib
from test_gpu_event_columns import RING, T0_US, W, H, Packet, _params, _unsorted_packet, state

pytestmark = pytest.mark.gpu

BIG = 4096            # a ring in which nothing of these tests wraps
FORMATS = ("wire", "async", "columns")


def full_state(dev, cam=0):
    st = state(dev, cam)
    st["scattered"] = int(dev.stats().events_scattered[cam])
    return st


def push_as(dev, fmt, cam, pk, pins):
    """the packet's events by one route; records: the normalised esvo_event_t of the columns, synchronously"""
    cols, want = pk.columns()
    if fmt == "records":
        dev.ts_push_events(cam, want)
    elif fmt == "wire":
        assert dev.ts_push_event_array(cam, abi.serialize_event_array(want, W, H)) == pk.n
    elif fmt == "async":
        pe = lib.PinnedEvents(pk.n)
        pe.array[:] = want
        pins.append(pe)
        dev.ts_push_events_async(cam, pe.array)
        dev.ts_push_wait(cam)
    else:
        dev.ts_push_columns(cam, *cols)
    return want


@pytest.fixture(scope="module")
def handles(upenn_rig):
    """a, b: ring 1024; c: ring 4096 -- and the same three in queue mode"""
    made = {}

    def get(queue):
        if queue not in made:
            over = dict(max_event_queue_len=3) if queue else {}
            made[queue] = [lib.Esvo(_params(upenn_rig, process_event_num=200, event_ring_capacity=cap, **over), upenn_rig) for cap in (RING, RING, BIG)]
        for d in made[queue]:
            d.reset()
        return made[queue]
    yield get
    for devs in made.values():
        for d in devs:
            d.close()


# ---- case 1: every format at the ring's end -----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_at_the_rings_end(handles, fmt):
    rng = np.random.default_rng(1201)
    pins = []
    for first_n in (924, 925, 1000, 1001, 1002, 1003, 1023, 1024):   # 924: the second packet ends at the last slot; 1024: it starts at slot 0
        a, b, _ = handles(False)
        first = Packet(rng, first_n, T0_US * 1000 + 999_000_000, box=6)
        second = Packet(rng, 100, first.t_ns[-1] + 5, box=6)
        for pk in (first, second):
            want = push_as(a, "records", 0, pk, pins)
            push_as(b, fmt, 0, pk, pins)
            sa, sb = full_state(a), full_state(b)
            assert sa == sb, (first_n, pk.n)
            assert sa["records"][-pk.n * 16:] == want.tobytes()
            if pk is first:   # everything staged is scattered: the ring may evict
                img = [d.ts_render(0, first.t_ns[-1] + 1) for d in (a, b)]
                assert np.array_equal(img[0], img[1]) and img[0].any()
                assert full_state(a)["scattered"] == first_n and full_state(b)["scattered"] == first_n
        assert sa["bounds"] == (max(0, first_n + 100 - RING), first_n + 100) and sa["staged"] == first_n + 100 and sa["late"] == 0
    for pe in pins:
        pe.free()


# ---- case 2: an out-of-order packet whose merged tail wraps -------------------------------------------------------------
@pytest.mark.parametrize("queue", [False, True])
def test_out_of_order_packet_whose_merged_tail_wraps(handles, queue):
    rng = np.random.default_rng(1202)
    a, b, c = handles(queue)
    base = Packet(rng, 1000, T0_US * 1000 + 999_000_000, box=6)
    more = Packet(rng, 60, base.t_ns[-1] + 5, box=6)
    late = _unsorted_packet(rng, more.t_ns[-1] - 64_000)
    staged = np.array(base.t_ns + more.t_ns)
    pos = int(np.searchsorted(staged, min(late.t_ns), side="right"))   # the first staged event the packet is merged in front of
    assert 1000 < pos < RING - 2 and 1060 - pos >= 30                  # the rewritten tail crosses slot 1023 -> 0; nothing of it is scattered
    t_end = max(late.t_ns + more.t_ns) + 1
    results = []
    for dev, fmt in ((a, "records"), (b, "wire"), (b, "columns"), (c, "records")):
        dev.reset()
        for pk, how in ((base, "records"), (more, "records"), (late, fmt)):
            push_as(dev, how, 0, pk, None)
            if pk is base:
                assert dev.ts_render(0, base.t_ns[-1] + 1).any()
        assert dev.debug_ts_ring(0)[2:] == (0 if dev is c else 1110 - RING, 1110)
        ev, st = dev.debug_ts_ring(0, 1110 - RING, RING)[:2]
        assert (np.diff(st.astype(np.int64)) >= 0).all() and (abi.event_ns(ev) == st).all()
        s = dev.stats()
        img = dev.ts_render(0, t_end)
        results.append(dict(records=ev.tobytes(), stamps=st.tobytes(), late=int(s.late_events[0]), staged=int(s.events_staged[0]),
                            image=img.tobytes(), scattered=int(dev.stats().events_scattered[0])))
        assert img.any()
    assert results[0]["late"] > 0 and results[0]["staged"] == 1110
    for k, r in enumerate(results[1:]):
        for key in r:
            assert r[key] == results[0][key], (k + 1, key)


# ---- case 3: scatter ranges that wrap -----------------------------------------------------------------------------------
def _scatter_packets():
    rng = np.random.default_rng(1203)
    # (16 x 16 pixels: in queue mode a pixel keeps its newest 3 events, staged future ones included -- most pixels still hold one below t)
    pk = Packet(rng, 1200, T0_US * 1000 + 999_000_000, box=16)
    if pk.t_ns[1024] == pk.t_ns[1023]:   # a render at t_ns[1024] takes exactly the events below absolute index 1024
        pk.t_ns[1024:] = [t + 1 for t in pk.t_ns[1024:]]
    ev = pk.columns()[1]
    return pk, ev[:900], ev[900:]


def _render_walk(small, big, render, exact):
    pk, ev0, ev1 = _scatter_packets()
    devs = (small, big)

    def step(t, upto):
        for cam in (0, 1):
            img = [render(d, cam, t) for d in devs]
            assert np.array_equal(img[0], img[1]) and img[0].any(), (cam, t)
            sc = [int(d.stats().events_scattered[cam]) for d in devs]
            assert sc[0] == sc[1] and (not exact or sc[0] == upto), (cam, t, sc)
    for d in devs:
        for cam in (0, 1):
            d.ts_push_events(cam, ev0)
    step(pk.t_ns[899] + 1, 900)
    for d in devs:
        for cam in (0, 1):
            d.ts_push_events(cam, ev1)
    step(pk.t_ns[1024], 1024)      # the range ends exactly at the last slot
    step(pk.t_ns[-1] + 1, 1200)    # ... and the next one starts at slot 0
    for cam in (0, 1):
        assert state(small, cam)["bounds"] == (1200 - RING, 1200) and state(big, cam)["bounds"] == (0, 1200)


def test_scatter_walk_of_ts_render(handles):
    a, _, c = handles(False)
    _render_walk(a, c, lambda d, cam, t: d.ts_render(cam, t), True)


def test_scatter_walk_of_ts_render_forward(handles):
    a, _, c = handles(False)
    _render_walk(a, c, lambda d, cam, t: d.ts_render_forward(cam, t), True)


def test_scatter_walk_of_ts_render_with_event_queues(handles):
    a, _, c = handles(True)
    _render_walk(a, c, lambda d, cam, t: d.ts_render(cam, t), False)   # (queue mode inserts everything staged at every render)


@pytest.mark.parametrize("at_boundary", [False, True])
def test_scatter_walk_of_the_pair_render(handles, at_boundary):
    """esvo_map_tick_resident renders both cameras at once; at_boundary False: both cameras' ranges [900, 1200) wrap: four segments"""
    a, _, c = handles(False)
    devs = (a, c)
    pk, ev0, ev1 = _scatter_packets()
    from esvo_amd import rostime
    pose = lambda t: np.eye(4)
    for d in devs:
        for cam in (0, 1):
            d.ts_push_events(cam, ev0)
            assert d.ts_render(cam, pk.t_ns[899] + 1).any()
        for cam in (0, 1):
            d.ts_push_events(cam, ev1)
    for t, upto in ([(pk.t_ns[1024], 1024)] if at_boundary else []) + [(pk.t_ns[-1] + 1, 1200)]:
        stamps, poses = rostime.pose_table(pose, t, a.params.bm_half_slice_thickness)
        for d in devs:
            d.tick_resident(t, pose(t), stamps, poses)
        for cam in (0, 1):
            assert [int(d.stats().events_scattered[cam]) for d in devs] == [upto, upto]
            img = [d.ts_render(cam, t) for d in devs]
            assert np.array_equal(img[0], img[1]) and img[0].any()
            assert [int(d.stats().events_scattered[cam]) for d in devs] == [upto, upto]
        assert a.get_map().tobytes() == c.get_map().tobytes()
