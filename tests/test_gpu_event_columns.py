"""esvo_ts_push_event_columns on the device (include/esvo_hip.h): a handle fed COLUMNS against a handle fed the RECORDS the
Python-int restatement (tests/columns_restated.py) makes of them.  The two are compared through esvo_debug_ts_ring on all 16 bytes
of every record the ring holds, the host's stamp mirror, ring_base / ring_next, events_staged and late_events -- a render would
hide the nanoseconds behind a 30 ms decay rounded to u8.  Ring of 1024 slots, upenn rig, unless a case says otherwise."""
import ctypes

import numpy as np
import pytest

import columns_restated as R
import scenarios as S
from esvo_amd import abi, dist as edist, lib, params, rostime

pytestmark = pytest.mark.gpu

RING = 1024
W, H = 346, 260
T0_US = 1_700_000_000_000_000   # stamps of the crafted packets start here (microseconds): sec and nsec are both in use


def _params(rig, **over):
    kw = dict(max_events_per_tick=4096, event_ring_capacity=RING, regularization=0)
    kw.update(over)
    return params.make_params(params.PRESETS["mapping_upenn"], rig, **kw)[0]


class Pair:
    """a: fed records; b: fed columns"""

    def __init__(self, rig, **over):
        self.p = _params(rig, **over)
        self.a, self.b = lib.Esvo(self.p, rig), lib.Esvo(self.p, rig)

    def reset(self):
        self.a.reset(); self.b.reset()
        return self

    def close(self):
        self.a.close(); self.b.close()


@pytest.fixture(scope="module")
def pair(upenn_rig):
    pr = Pair(upenn_rig)
    yield pr
    pr.close()


@pytest.fixture(scope="module")
def qpair(upenn_rig):
    pr = Pair(upenn_rig, max_event_queue_len=3)
    yield pr
    pr.close()


def state(dev, cam=0):
    ev, st, b0, b1 = dev.debug_ts_ring(cam)
    s = dev.stats()
    return dict(records=ev.tobytes(), stamps=st.tobytes(), bounds=(b0, b1), staged=int(s.events_staged[cam]), late=int(s.late_events[cam]))


def same(pr, cam=0):
    sa, sb = state(pr.a, cam), state(pr.b, cam)
    for k in sa:
        assert sa[k] == sb[k], k
    return sa


class Packet:
    """n events: x, y inside the sensor, stamps in NANOSECONDS as Python ints (ascending unless shuffled), polarity bytes"""

    def __init__(self, rng, n, t_first_ns, whole_us=False, p_bytes=(0, 1, 2, 255), box=None):
        """box: the events fall into a box x box block of pixels (a render's median filter erases isolated ones)"""
        self.n = n
        self.x = (rng.integers(0, W, n) if box is None else rng.integers(100, 100 + box, n)).astype(np.uint16)
        self.y = (rng.integers(0, H, n) if box is None else rng.integers(100, 100 + box, n)).astype(np.uint16)
        gaps = rng.integers(0, 3000, n)          # ties included
        gaps[0] = 0
        self.t_ns = [int(t_first_ns) + int(g) for g in np.cumsum(gaps)]
        if whole_us:
            self.t_ns = [t - t % 1000 for t in self.t_ns]
        self.p = rng.choice(np.array(p_bytes, np.uint8), n)

    def columns(self, t_type=abi.T_NS_I64, p_type=abi.P_U8, with_p=True):
        """-> (x, y, t, p, unit, t_offset) as host arrays of the asked types, and the records they stand for"""
        k = R.UNIT[t_type]
        assert all(t % k == 0 for t in self.t_ns)
        # DSEC: a u32 of microseconds that starts near 0, + t_offset; the i64 types: none / a negative one
        off = {abi.T_NS_I64: 0, abi.T_US_I64: -123_456, abi.T_US_U32: min(self.t_ns) // k - 11}[t_type]
        t = np.array([s // k - off for s in self.t_ns], R.T_DTYPE[t_type])
        p = self.p.view(R.P_DTYPE[p_type]) if with_p else None
        want, bad = R.columns_to_events(self.x, self.y, t, self.p if with_p else None, t_type, p_type, off)
        assert bad is None
        assert [int(s) * 10 ** 9 + int(ns) for s, ns in zip(want["sec"], want["nsec"])] == self.t_ns
        return (self.x, self.y, t, p, R.T_UNIT[t_type], off), want


class Cai:
    """device memory of a torch tensor under another element type (__cuda_array_interface__): u16 / u32 columns"""

    def __init__(self, tensor, typestr):
        self.tensor = tensor
        self.__cuda_array_interface__ = dict(shape=(tensor.numel(),), typestr=typestr, data=(tensor.data_ptr(), True), version=2, strides=None)


def to_device(cols, pad=(0, 0, 0, 0)):
    """the same columns in device memory; pad[k]: elements in front of column k inside its allocation (an unaligned slice)"""
    import torch
    x, y, t, p, unit, off = cols

    def up(a, lead, as_int=None, typestr=None):
        if a is None:
            return None
        host = np.concatenate([np.zeros(lead, a.dtype), a, np.zeros(3, a.dtype)])
        d = torch.from_numpy(host.view(as_int) if as_int else host).cuda()[lead:lead + len(a)]
        return Cai(d, typestr) if typestr else d
    dx, dy = up(x, pad[0], np.int16), up(y, pad[1], np.int16, "<u2")   # (an int16 tensor's bits; a u16 view through the interface)
    dt = up(t, pad[2], np.int32, "<u4") if t.dtype == np.uint32 else up(t, pad[2])
    dp = up(p, pad[3])
    torch.cuda.synchronize()
    return dx, dy, dt, dp, unit, off


def host_slices(cols, pad):
    """host columns that start pad[k] elements into a larger array"""
    x, y, t, p, unit, off = cols
    out = []
    for a, lead in zip((x, y, t, p), pad):
        if a is None:
            out.append(None)
            continue
        big = np.concatenate([np.zeros(lead, a.dtype), a, np.zeros(3, a.dtype)])
        out.append(big[lead:lead + len(a)])
    return (*out, unit, off)


def push_both(pr, cols, want, cam=0):
    pr.a.ts_push_events(cam, want)
    pr.b.ts_push_columns(cam, *cols)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_lengths(pair, n):
    rng = np.random.default_rng(n)
    pk = Packet(rng, n, T0_US * 1000 + 999_999_000)    # crosses a second boundary within the first microseconds
    cols, want = pk.columns()
    push_both(pair.reset(), cols, want)
    st = same(pair)
    assert st["bounds"] == (0, n) and st["staged"] == n and st["records"] == want.tobytes()
    # the same from device memory
    pair.reset()
    pair.a.ts_push_events(0, want)
    pair.b.ts_push_columns(0, *to_device(cols))
    assert same(pair)["records"] == want.tobytes()


def test_one_event_too_many(pair):
    pk = Packet(np.random.default_rng(5), RING + 1, T0_US * 1000)
    cols, want = pk.columns()
    pair.reset()
    before = same(pair)
    for c in (cols, to_device(cols)):
        with pytest.raises(lib.EsvoError) as e:
            pair.b.ts_push_columns(0, *c)
        assert e.value.code == abi.ERR_CAPACITY
    with pytest.raises(lib.EsvoError) as e:
        pair.a.ts_push_events(0, want)
    assert e.value.code == abi.ERR_CAPACITY
    assert same(pair) == before
    pair.b.ts_push_columns(0, np.zeros(0, np.uint16), np.zeros(0, np.uint16), np.zeros(0, np.int64))   # n == 0: a no-op
    assert same(pair) == before


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("p_type", [abi.P_U8, abi.P_I8, None])
@pytest.mark.parametrize("t_type", [abi.T_NS_I64, abi.T_US_I64, abi.T_US_U32])
def test_types(pair, t_type, p_type, memory):
    rng = np.random.default_rng(100 + 10 * t_type + (p_type or 0))
    pk = Packet(rng, 257, T0_US * 1000 + 999_000_000, whole_us=t_type != abi.T_NS_I64, p_bytes=(0, 1, 2, 128, 255))
    cols, want = pk.columns(t_type, p_type if p_type is not None else abi.P_U8, with_p=p_type is not None)
    if p_type is None:
        assert (want["polarity"] == 1).all()
    pair.reset()
    pair.a.ts_push_events(0, want)
    pair.b.ts_push_columns(0, *(to_device(cols) if memory == "device" else cols))
    assert same(pair)["records"] == want.tobytes()
    # the right camera has a ring and a staging buffer of its own
    pair.a.ts_push_events(1, want)
    pair.b.ts_push_columns(1, *(to_device(cols) if memory == "device" else cols))
    assert same(pair, 1)["records"] == want.tobytes()


@pytest.mark.parametrize("memory", ["host", "device"])
def test_column_bases_inside_larger_allocations(pair, memory):
    rng = np.random.default_rng(77)
    for t_type in (abi.T_NS_I64, abi.T_US_U32):
        pk = Packet(rng, 65, T0_US * 1000, whole_us=True)
        cols, want = pk.columns(t_type, abi.P_I8)
        for col in range(4):
            for lead in range(4):
                pad = tuple(lead if k == col else 0 for k in range(4))
                pair.reset()
                pair.a.ts_push_events(0, want)
                pair.b.ts_push_columns(0, *(to_device(cols, pad) if memory == "device" else host_slices(cols, pad)))
                assert same(pair)["records"] == want.tobytes(), (t_type, col, lead)


@pytest.mark.parametrize("memory", ["host", "device"])
def test_ring_wrap_at_every_position(pair, memory):
    rng = np.random.default_rng(88)
    for k in range(8):
        first = Packet(rng, 1000 + k, T0_US * 1000)
        second = Packet(rng, 100, first.t_ns[-1] + 5)
        pair.reset()
        for pk in (first, second):
            cols, want = pk.columns()
            pair.a.ts_push_events(0, want)
            pair.b.ts_push_columns(0, *(to_device(cols) if memory == "device" else cols))
            if pk is first:   # everything staged is scattered: the ring may evict
                img = [d.ts_render(0, first.t_ns[-1] + 1) for d in (pair.a, pair.b)]
                assert np.array_equal(img[0], img[1])
        st = same(pair)
        assert st["bounds"] == (1100 + k - RING, 1100 + k)
        assert st["records"][-100 * 16:] == want.tobytes()


def test_order_at_the_newest_stamp_and_one_below(pair):
    rng = np.random.default_rng(99)
    base = Packet(rng, 10, T0_US * 1000 + 123, box=4)
    newest = base.t_ns[-1]
    pair.reset()
    push_both(pair, *base.columns())
    tie = Packet(rng, 6, newest, box=4)          # first stamp == the newest staged one: in order
    push_both(pair, *tie.columns())
    st = same(pair)
    assert st["late"] == 0 and st["bounds"] == (0, 16)
    late = Packet(rng, 6, tie.t_ns[-1] - 1, box=4)  # one nanosecond below it: late; the next one ties with the newest: not late
    late.t_ns = [tie.t_ns[-1] - 1 + i for i in range(6)]
    push_both(pair, *late.columns())
    st = same(pair)
    assert st["late"] == 1 and st["bounds"] == (0, 22) and st["staged"] == 22
    stamps = np.frombuffer(st["stamps"], np.uint64)
    assert (np.diff(stamps.astype(np.int64)) >= 0).all()
    img = [d.ts_render(0, late.t_ns[-1] + 1) for d in (pair.a, pair.b)]
    assert np.array_equal(img[0], img[1]) and img[0].any()


def _unsorted_packet(rng, t_first_ns):
    pk = Packet(rng, 50, t_first_ns, box=6)
    order = rng.permutation(50)
    pk.x, pk.y, pk.p, pk.t_ns = pk.x[order], pk.y[order], pk.p[order], [pk.t_ns[i] for i in order]
    pk.t_ns[7] = pk.t_ns[3]; pk.t_ns[20] = pk.t_ns[3]; pk.t_ns[41] = pk.t_ns[40]   # ties, apart and adjacent
    return pk


@pytest.mark.parametrize("memory", ["host", "device"])
def test_packet_unsorted_inside_itself(pair, memory):
    rng = np.random.default_rng(111)
    base = Packet(rng, 30, T0_US * 1000, box=6)
    pk = _unsorted_packet(rng, base.t_ns[-1] - 20_000)    # reaches back into the staged events as well
    pair.reset()
    push_both(pair, *base.columns())
    cols, want = pk.columns()
    pair.a.ts_push_events(0, want)
    pair.b.ts_push_columns(0, *(to_device(cols) if memory == "device" else cols))
    st = same(pair)
    assert st["late"] > 0 and st["bounds"] == (0, 80)
    img = [d.ts_render(0, max(pk.t_ns) + 1) for d in (pair.a, pair.b)]
    assert np.array_equal(img[0], img[1]) and img[0].any()


@pytest.mark.parametrize("memory", ["host", "device"])
def test_packet_unsorted_inside_itself_with_event_queues(qpair, memory):
    rng = np.random.default_rng(112)
    base = Packet(rng, 30, T0_US * 1000, box=6)
    pk = _unsorted_packet(rng, base.t_ns[-1] - 20_000)
    after = Packet(rng, 20, max(pk.t_ns) + 10, box=6)
    qpair.reset()
    push_both(qpair, *base.columns())
    img = [d.ts_render(0, base.t_ns[-1] - 5_000) for d in (qpair.a, qpair.b)]
    assert np.array_equal(img[0], img[1]) and img[0].any()
    cols, want = pk.columns()
    qpair.a.ts_push_events(0, want)
    qpair.b.ts_push_columns(0, *(to_device(cols) if memory == "device" else cols))
    assert same(qpair)["late"] > 0
    push_both(qpair, *after.columns())
    same(qpair)
    for t in (max(pk.t_ns) + 1, after.t_ns[-1] + 1):
        img = [d.ts_render(0, t) for d in (qpair.a, qpair.b)]
        assert np.array_equal(img[0], img[1]) and img[0].any()


def _raw_push(dev, s, n, cam=0):
    return lib.load().esvo_ts_push_event_columns(dev.h, cam, ctypes.addressof(s), n)


def test_refusals_change_nothing(pair):
    import torch
    rng = np.random.default_rng(121)
    base = Packet(rng, 40, T0_US * 1000)
    nxt = Packet(rng, 33, base.t_ns[-1] + 1)
    pair.reset()
    push_both(pair, *base.columns())
    before = same(pair)

    def refused(s, n, keep):
        assert _raw_push(pair.b, s, n) == abi.ERR_INVALID_ARG
        assert state(pair.b) == before

    cols, _ = nxt.columns()
    # an invalid element first, in the middle and last: host and device columns, every t_type's way of being invalid
    for where in (0, 16, 32):
        for t_type, bad_t, off in ((abi.T_NS_I64, -1, 0), (abi.T_US_I64, R.STAMP_END // 1000, 0), (abi.T_US_U32, 5, -6)):
            t = np.array([s // R.UNIT[t_type] for s in nxt.t_ns], np.int64)
            t = (t - (t.min() if t_type == abi.T_US_U32 else 0)).astype(R.T_DTYPE[t_type])
            t_off = off if t_type == abi.T_US_U32 else 0
            if t_type == abi.T_US_U32:
                t = t + np.uint32(10)           # valid under the offset -6 everywhere else
            t[where] = bad_t
            c = (nxt.x, nxt.y, t, nxt.p, R.T_UNIT[t_type], t_off)
            assert R.columns_to_events(nxt.x, nxt.y, t, nxt.p, t_type, abi.P_U8, t_off)[1] == where
            for cc in (c, to_device(c)):
                s, (n, keep) = lib.event_columns_struct(*cc)
                refused(s, n, keep)
                assert f"element {where} " in lib.load().esvo_last_error(pair.b.h).decode()
    # pinned host memory labelled DEVICE
    pin = lib.PinnedEvents(nxt.n)
    s, (n, keep) = lib.event_columns_struct(*cols)
    s.x = s.y = s.t = s.p = pin.ptr.value
    s.memory = abi.MEM_DEVICE
    refused(s, n, keep)
    # pageable host memory labelled DEVICE
    s, (n, keep) = lib.event_columns_struct(*cols)
    s.memory = abi.MEM_DEVICE
    refused(s, n, keep)
    # device memory labelled HOST; one device column among host columns, either label
    s, (n, keep) = lib.event_columns_struct(*to_device(cols))
    s.memory = abi.MEM_HOST
    refused(s, n, keep)
    sd, (_, keep_d) = lib.event_columns_struct(*to_device(cols))
    for label in (abi.MEM_HOST, abi.MEM_DEVICE):
        s, (n, keep) = lib.event_columns_struct(*cols)
        s.p, s.memory = sd.p, label
        refused(s, n, keep)
    # unknown types
    for field, value in (("t_type", 3), ("p_type", 2), ("memory", 2), ("t_type", -1)):
        s, (n, keep) = lib.event_columns_struct(*cols)
        setattr(s, field, value)
        refused(s, n, keep)
    # a missing column
    s, (n, keep) = lib.event_columns_struct(*cols)
    s.t = None
    refused(s, n, keep)
    pin.free()
    torch.cuda.synchronize()
    # the next valid push lands where it would have
    assert same(pair) == before
    push_both(pair, *nxt.columns())
    st = same(pair)
    assert st["bounds"] == (0, 73) and st["late"] == 0


def test_out_of_order_on_a_routed_handle_and_routed_maps(upenn_rig, upenn_stream):
    """two logical row-band shards per side, as tests/test_gpu_shard.py sets them up: one side fed records, one fed columns"""
    from test_gpu_shard import _emulated_gather
    rig, stream = upenn_rig, upenn_stream
    p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], rig)
    G = 2
    sides = [[lib.Esvo(p, rig) for _ in range(G)] for _ in range(2)]
    for shards in sides:
        for g, d in enumerate(shards):
            y0, y1 = edist.band_of(g, G, rig.height)
            d.set_band(y0, y1, g, G, routing="y_rect")
    t_prev = stream.t0_ns
    for k in range(3):
        t = stream.t0_ns + int((0.07 + 0.01 * k) * 1e9)
        stamps, poses = rostime.pose_table(stream.pose, t, p.bm_half_slice_thickness)
        for side, shards in enumerate(sides):
            for g, d in enumerate(shards):
                for cam in (0, 1):
                    ev = stream.slice(cam, t_prev, t + 5_000_000)
                    if side == 0:
                        d.ts_push_events(cam, ev)
                    else:
                        cols = (ev["x"].copy(), ev["y"].copy(), abi.event_ns(ev).astype(np.int64), ev["polarity"].copy(), "ns", 0)
                        d.ts_push_columns(cam, *(to_device(cols) if g == 1 else cols))
                d.ts_render(0, t, download=False); d.ts_render(1, t, download=False)
                d.set_observation(t, None, None, stream.pose(t))
            for d in shards:
                d.shard_phase(0, t, stamps, poses)
            _emulated_gather(shards)
            for d in shards:
                d.shard_phase(1)
            _emulated_gather(shards)
            for d in shards:
                d.shard_phase(2)
        t_prev = t + 5_000_000
        for g in range(G):
            for cam in (0, 1):
                sa, sb = state(sides[0][g], cam), state(sides[1][g], cam)
                assert sa == sb, (k, g, cam)
        maps = [edist.merge_band_maps([d.get_map() for d in shards]) for shards in sides]
        assert maps[0].tobytes() == maps[1].tobytes(), k
    assert len(maps[0]) > 50
    # a packet that reaches back: refused on a routed handle, by both calls alike, nothing consumed
    ev = stream.slice(0, t_prev - 2_000_000, t_prev - 1_000_000)
    assert len(ev) > 1
    before = [state(sides[s][0]) for s in range(2)]
    with pytest.raises(lib.EsvoError) as ea:
        sides[0][0].ts_push_events(0, ev)
    with pytest.raises(lib.EsvoError) as eb:
        sides[1][0].ts_push_columns(0, ev["x"].copy(), ev["y"].copy(), abi.event_ns(ev).astype(np.int64), ev["polarity"].copy())
    assert ea.value.code == eb.value.code and str(ea.value) == str(eb.value)
    assert [state(sides[s][0]) for s in range(2)] == before
    for shards in sides:
        for d in shards:
            d.close()


def test_end_to_end_dsec_typed_columns():
    """the small upenn scenario staged as DSEC's files hold events: x, y u16, t u32 microseconds + t_offset, p u8"""
    sc = S.Scenario("upenn")
    rig, p, st = sc.rig, sc.params, sc.stream()
    a, b = lib.Esvo(p, rig), lib.Esvo(p, rig)
    off_us = st.t0_ns // 1000 - 1000
    done = [0, 0]
    for k in range(sc.n_ticks):
        t = st.t0_ns + int(round((sc.spec["t_first"] + sc.spec["dt"] * k) * 1e9))
        for cam, (ev, ns) in enumerate(((st.ev_left, st.ns_left), (st.ev_right, st.ns_right))):
            hi = int(np.searchsorted(ns, t + 5_000_000, side="left"))
            sl = ev[done[cam]:hi]
            done[cam] = hi
            t_us = abi.event_ns(sl) // np.uint64(1000)
            a.ts_push_events(cam, abi.make_events(sl["x"], sl["y"], t_us * np.uint64(1000), sl["polarity"]))
            b.ts_push_columns(cam, sl["x"].copy(), sl["y"].copy(), (t_us.astype(np.int64) - off_us).astype(np.uint32), sl["polarity"].copy(),
                              unit="us", t_offset=off_us)
        stamps, poses = rostime.pose_table(st.pose, t, p.bm_half_slice_thickness)
        for d in (a, b):
            d.ts_render(0, t, download=False); d.ts_render(1, t, download=False)
            d.set_observation(t, None, None, st.pose(t))
            d.tick(t, stamps, poses)
        fa, fb = a.get_last_frame(), b.get_last_frame()
        assert len(fa) > 0 and fa.tobytes() == fb.tobytes(), k
    for cam in (0, 1):
        assert state(a, cam) == state(b, cam)
    ma, mb = a.get_map(), b.get_map()
    assert len(ma) > 50 and ma.tobytes() == mb.tobytes()
    a.close(); b.close()


def test_staging_memory(upenn_rig):
    from test_gpu_lifecycle import Ledger
    rng = np.random.default_rng(131)
    p = _params(upenn_rig)
    led = Ledger()
    dev = lib.Esvo(p, upenn_rig)
    created = led()
    small, large = Packet(rng, 100, T0_US * 1000), Packet(rng, 1000, T0_US * 1000)
    cs, ws = small.columns()
    cl, wl = large.columns()
    dev.ts_push_columns(0, *cs)
    first = led()
    assert first[0] == created[0] + 2                                  # the device staging and its pinned stamps
    assert first[1] == created[1] + 256 * 13 + 256 * 8
    dev.reset()                                                        # the staging survives a reset
    assert led() == first
    dev.ts_push_columns(0, *cs)
    dev.reset()
    dev.ts_push_columns(0, *to_device(cs))
    assert led() == first                                              # a second push of the same size allocates nothing
    dev.reset()
    dev.ts_push_columns(0, *cl)                                        # regrow: the same two buffers, larger, the old ones freed
    grown = led()
    assert grown[0] == first[0] and grown[1] == created[1] + 1536 * 21
    dev.reset()
    dev.ts_push_columns(0, *to_device(cl))
    dev.ts_push_columns(1, *cs)                                        # the right camera's own pair
    assert led() == (grown[0] + 2, grown[1] + 256 * 21)
    # a handle that pushed columns and was reset equals a fresh one
    dev.reset()
    fresh = lib.Esvo(p, upenn_rig)
    assert state(dev) == state(fresh) and state(dev)["bounds"] == (0, 0) and state(dev)["staged"] == 0
    for d in (dev, fresh):
        d.ts_push_events(0, ws)
    assert state(dev) == state(fresh)
    assert np.array_equal(dev.ts_render(0, small.t_ns[-1] + 1), fresh.ts_render(0, small.t_ns[-1] + 1))
    fresh.close()
    dev.close()
    assert led() == (0, 0)
