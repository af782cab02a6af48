"""esvo_ts_push_evt3 on the device (include/esvo_hip.h): a handle fed EVT 3.0 WORDS against a handle fed the RECORDS the Python-int
restatement (tests/evt3_restated.py) decodes from them.  The two are compared byte for byte through esvo_debug_ts_ring (the ring's
records, the host's stamp mirror, ring_base / ring_next), esvo_get_stats (events_staged, late_events) and a rendered Time Surface;
the decoder state and the totals of the words-fed handle against the restatement's.  The words-fed handle decodes EVERY packet on
the device (esvo_debug_evt3_device_min 0) unless a case says otherwise: the shapes below are the wave and tile seams of the scans.
346x260 (upenn rig)."""
import ctypes

import numpy as np
import pytest

import evt3_restated as R
import scenarios as S
from esvo_amd import abi, dist as edist, lib, params, rostime

pytestmark = pytest.mark.gpu

W, H = 346, 260
TILE = 2048                       # words per tile of the device decode
T0_US = 1_700_000_000_000_000     # t_offset_us of the crafted streams: sec and nsec are both in use
TH, TL, AY, AX, VB, V12, V8, EXT = (R.TIME_HIGH << 12, R.TIME_LOW << 12, R.ADDR_Y << 12, R.ADDR_X << 12, R.VECT_BASE_X << 12, R.VECT_12 << 12,
                                     R.VECT_8 << 12, R.EXT_TRIGGER << 12)


def _params(rig, ring, **over):
    kw = dict(max_events_per_tick=4096, event_ring_capacity=ring, regularization=0)
    kw.update(over)
    return params.make_params(params.PRESETS["mapping_upenn"], rig, **kw)[0]


class Pair:
    """a: fed records; b: fed EVT3 words, every packet decoded on the device"""

    def __init__(self, rig, ring, **over):
        self.p = _params(rig, ring, **over)
        self.a, self.b = lib.Esvo(self.p, rig), lib.Esvo(self.p, rig)
        self.b.debug_evt3_device_min(0)
        self.model = R.fresh_state()          # the restatement's state of b's left camera
        self.totals = dict.fromkeys(R.COUNTS, 0)

    def reset(self, state=None):
        self.a.reset(); self.b.reset()
        self.model, self.totals = R.fresh_state(), dict.fromkeys(R.COUNTS, 0)
        if state is not None:
            st = abi.Evt3State()
            st.flags, st.y, st.base_x, st.time_high, st.time_low, st.loops = R.state_tuple(state)
            self.b.evt3_state(0, set=st)
            self.model = dict(state)
        return self

    def push(self, words, memory="host", lead=0, off=T0_US):
        """the words to b, the records they decode to (restatement) to a; -> the records"""
        words = np.asarray(words, np.uint16)
        ev, self.model, c = R.decode(words.tolist(), self.model, off)
        for k in c:
            self.totals[k] += c[k]
        want = R.records(ev)
        if len(want):
            self.a.ts_push_events(0, want)
        n = self.b.ts_push_evt3(0, to_device(words, lead) if memory == "device" else words, off)
        assert n == len(want)
        return want

    def close(self):
        self.a.close(); self.b.close()


def to_device(words, lead=0):
    """the words in device memory, `lead` words into a larger int16 tensor"""
    import torch
    host = np.concatenate([np.full(lead, 0x2FFF, np.uint16), words, np.full(3, 0x2FFF, np.uint16)])
    d = torch.from_numpy(host.view(np.int16)).cuda()[lead:lead + len(words)]
    torch.cuda.synchronize()
    return d


def state(dev, cam=0):
    ev, st, b0, b1 = dev.debug_ts_ring(cam)
    s = dev.stats()
    return dict(records=ev.tobytes(), stamps=st.tobytes(), bounds=(b0, b1), staged=int(s.events_staged[cam]), late=int(s.late_events[cam]))


def same(pr, cam=0, render_at=None):
    sa, sb = state(pr.a, cam), state(pr.b, cam)
    for k in sa:
        assert sa[k] == sb[k], k
    if cam == 0:
        assert pr.b.evt3_state(0).as_tuple() == R.state_tuple(pr.model)
        assert pr.b.evt3_stats(0) == pr.totals
    if render_at is not None:   # "newest": just behind the newest staged stamp
        t = newest_ns(sa) + 1 if render_at == "newest" else render_at
        img = [d.ts_render(cam, t) for d in (pr.a, pr.b)]
        assert np.array_equal(img[0], img[1])
        return sa, img[0]
    return sa


def newest_ns(st):
    return int(np.frombuffer(st["stamps"], np.uint64)[-1])


class Gen:
    """words of a stream whose time never steps back, so that every packet cut from it takes the in-order path; events fall into
    the sensor (mostly into a block of it: a render's median filter erases isolated ones)"""
    START = dict(R.fresh_state(), have_th=1, have_y=1, have_base=1, time_high=3500, time_low=7, y=100, base_x=100, vect_pol=1)
    KINDS = ("ax", "ay", "vb", "v12", "v8", "tl", "th", "tlth", "ext", "res")
    WEIGHTS = np.array([30, 10, 10, 12, 8, 10, 6, 4, 3, 7]) / 100.0

    def __init__(self, seed, complete=True):
        """complete: the stream continues START (set it on the handle); else it starts from nothing and opens with the words that
        complete the state one by one"""
        self.rng = np.random.default_rng(seed)
        self.th, self.lo = (3500, 7) if complete else (3500, 0)
        self.words = [] if complete else [AX | 5, V8 | 0x11, TH | 3500, AX | 6, AY | 100, V12 | 0x3, VB | 0x800 | 100]

    def word(self, kind, wrap=False, to=None, least=0):
        """one more word; TIME_HIGH: wrap makes it a time loop, to jumps ahead to (at least) that value"""
        r = self.rng
        if kind == "ax":
            self.words.append(AX | int(r.integers(0, 2)) << 11 | int(r.integers(100, 112)))
        elif kind == "ay":
            self.words.append(AY | int(r.integers(100, 112)))
        elif kind == "vb":
            self.words.append(VB | int(r.integers(0, 2)) << 11 | int(r.integers(0, 300)))
        elif kind == "v12":
            self.words.append(V12 | int(r.integers(0, 4096)))
        elif kind == "v8":
            self.words.append(V8 | int(r.integers(0, 256)))
        elif kind == "tl":
            self.lo = min(4095, self.lo + int(r.integers(0, 3)))
            self.words.append(TL | self.lo)
        elif kind == "th":
            if to is not None:
                self.th = max(self.th, to)
            elif wrap or self.th >= 4090:   # a time loop: the step back is 2048 or more
                assert self.th >= 3000
                self.th -= 3000
            else:
                self.th += int(r.integers(least, 4))
            self.words.append(TH | self.th)
        elif kind == "tlth":                # TIME_LOW falls, TIME_HIGH rises right behind it: no event sees the time between them
            self.lo = int(r.integers(0, 50))
            self.words.append(TL | self.lo)
            self.word("th", least=1)
        elif kind == "ext":
            self.words.append(EXT | int(r.integers(0, 4096)))
        else:
            self.words.append(int(r.choice(R.RESERVED)) << 12 | int(r.integers(0, 4096)))
        return self

    def fill(self, upto):
        """random words until the stream has `upto` words"""
        while len(self.words) < upto:
            kind = str(self.rng.choice(self.KINDS, p=self.WEIGHTS))
            self.word("ax" if kind == "tlth" and len(self.words) + 2 > upto else kind)
        return self

    def array(self):
        return np.array(self.words, np.uint16)


@pytest.fixture(scope="module")
def pair(upenn_rig):
    pr = Pair(upenn_rig, 1 << 18)
    yield pr
    pr.close()


@pytest.fixture(scope="module")
def small(upenn_rig):
    pr = Pair(upenn_rig, 1024)
    yield pr
    pr.close()


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 70001])
def test_lengths(pair, n, memory):
    words = Gen(n).word("ax").fill(n).array()
    assert len(words) == n
    want = pair.reset(Gen.START).push(words, memory)
    st, img = same(pair, render_at="newest")
    assert st["bounds"] == (0, len(want)) and st["records"] == want.tobytes() and st["late"] == 0
    assert len(want) >= 1
    if n == 70001:
        assert pair.totals["time_loops"] >= 1 and pair.totals["ext_triggers"] > 0 and pair.totals["ignored_words"] > 0
    # the same stream from nothing: the words in front of the complete state are dropped and counted
    if n >= 63:
        words = Gen(n, complete=False).fill(n).array()
        want = pair.reset().push(words, memory)
        assert same(pair)["records"] == want.tobytes() and pair.totals["dropped_events"] == 1 + 2 + 1 + 2


SETTERS = {"ay": ("ax", "v12"), "th": ("ax", "v8"), "tl": ("ax", "v12"), "vb": ("v12", "v8")}


@pytest.mark.parametrize("seam", [TILE, 2 * TILE, 33 * TILE])
@pytest.mark.parametrize("setter", sorted(SETTERS))
def test_state_word_ends_a_tile_and_its_consumer_opens_the_next(pair, setter, seam):
    for consumer in SETTERS[setter]:
        g = Gen(seam + len(setter)).fill(seam - 1).word(setter).word(consumer).fill(seam + 70)
        words = g.array()
        assert words[seam - 1] >> 12 == {"ay": R.ADDR_Y, "th": R.TIME_HIGH, "tl": R.TIME_LOW, "vb": R.VECT_BASE_X}[setter]
        want = pair.reset(Gen.START).push(words)
        assert same(pair)["records"] == want.tobytes()


@pytest.mark.parametrize("seam", [TILE, 3 * TILE])
def test_time_loop_at_a_tile_seam(pair, seam):
    # the looping TIME_HIGH is the tile's last word (its events open the next tile) / the next tile's first word (the TIME_HIGH
    # it is compared with is the last word of the tile in front) / alone in its tile with the one before it tiles away
    for at in (seam - 1, seam):
        g = Gen(at).fill(at - 1).word("th", to=3500).word("th", wrap=True).word("ax").word("v12").fill(seam + 40)
        words = g.array()
        assert words[at] >> 12 == R.TIME_HIGH and (words[at - 1] & 0xFFF) - (words[at] & 0xFFF) >= 2048
        want = pair.reset(Gen.START).push(words)
        assert same(pair)["records"] == want.tobytes() and pair.totals["time_loops"] >= 1
    quiet = [AX | 100 | (i & 1) << 11 for i in range(2 * TILE)]            # two tiles without any TIME_HIGH word
    words = np.array([TH | 3000] + quiet + [TH | 900, AX | 101, TH | 3000, AX | 102], np.uint16)   # 900 -> 3000 is no loop
    want = pair.reset(Gen.START).push(words)
    assert same(pair)["records"] == want.tobytes() and pair.totals["time_loops"] == 1 and pair.model["loops"] == 1


def test_full_vector_straddles_the_end_of_the_ring(small):
    first = np.array([w for i in range(1018) for w in ([AY | 100 + i // 8 % 8] if i % 8 == 0 else []) + [AX | 100 + i % 8]], np.uint16)   # a block of 8 x 8
    for memory in ("host", "device"):
        small.reset(Gen.START).push(first, memory)
        st, _ = same(small, render_at="newest")                           # everything staged is scattered: the ring may evict
        assert st["bounds"] == (0, 1018)
        want = small.push([TL | 9, VB | 0x800 | 104, V12 | 0xFFF, V8 | 0xFF], memory)
        st, img = same(small, render_at="newest")
        assert st["bounds"] == (1038 - 1024, 1038) and st["records"][-20 * 16:] == want.tobytes() and img.any()


def test_a_packet_that_only_sets_state(pair):
    pair.reset()
    assert len(pair.push([TH | 77, TL | 5, EXT | 1])) == 0
    assert len(pair.push([AY | 101, VB | 0x800 | 102, 0x1000])) == 0
    st = same(pair)
    assert st["bounds"] == (0, 0) and pair.totals["words"] == 6 and pair.b.evt3_state(0).as_tuple() == (0xF, 101, 102, 77, 5, 0)
    want = pair.push([AX | 103, V12 | 0x801])
    st = same(pair)
    assert st["records"] == want.tobytes() and [int(x) for x in want["x"]] == [103, 102, 113]
    assert [int(s) * 10 ** 9 + int(ns) for s, ns in zip(want["sec"], want["nsec"])] == [(T0_US + (77 << 12 | 5)) * 1000] * 3
    # esvo_reset clears the state and the totals
    pair.reset()
    assert pair.b.evt3_state(0).as_tuple() == (0, 0, 0, 0, 0, 0) and pair.b.evt3_stats(0) == dict.fromkeys(R.COUNTS, 0)
    assert len(pair.push([AX | 1])) == 0 and pair.totals["dropped_events"] == 1
    same(pair)


def test_whole_and_in_chunks_cut_between_every_pair_of_word_types(pair):
    kinds = ("ay", "ax", "vb", "v12", "tl", "th", "ext")       # VECT_12 stands for both vector types, EXT for the ignored ones
    g, cuts = Gen(49), []
    for a in kinds:
        for b in kinds:
            g.fill(len(g.words) + 37).word(a)
            cuts.append(len(g.words))
            g.word(b)
    words = g.fill(len(g.words) + 2100).array()
    assert len(cuts) == 49
    want = pair.reset(Gen.START).push(words)
    whole = same(pair)
    assert whole["records"] == want.tobytes() and len(want) > 1000
    whole_state, whole_totals = pair.b.evt3_state(0).as_tuple(), dict(pair.totals)
    for memory in ("host", "device"):
        pair.reset(Gen.START)
        for lo, hi in zip([0] + cuts, cuts + [len(words)]):
            pair.push(words[lo:hi], memory, lead=lo % 8)
        assert same(pair) == whole
        assert pair.b.evt3_state(0).as_tuple() == whole_state and pair.totals == whole_totals


@pytest.mark.parametrize("n", [5, 2049])
def test_device_words_at_every_offset_into_a_larger_tensor(pair, n):
    words = Gen(n + 1).word("ax").fill(n).array()
    want = pair.reset(Gen.START).push(words)
    host = same(pair)
    assert host["records"] == want.tobytes()
    for lead in (1, 2, 3, 5, 7, 8, 9):            # an odd word offset: 2 bytes into a 4-byte word of the tensor
        pair.reset(Gen.START).push(words, "device", lead)
        assert same(pair) == host, lead
    big = np.concatenate([np.zeros(3, np.uint16), words])        # a host slice as well
    pair.reset(Gen.START)
    pair.a.ts_push_events(0, want)
    assert pair.b.ts_push_evt3(0, big[3:], T0_US) == len(want)
    pair.model, pair.totals = R.decode(words.tolist(), Gen.START, T0_US)[1:]
    assert same(pair) == host


@pytest.mark.parametrize("queues", [0, 3])
@pytest.mark.parametrize("memory", ["host", "device"])
def test_out_of_order_falls_back_to_the_record_paths(upenn_rig, memory, queues):
    pr = Pair(upenn_rig, 4096, **(dict(max_event_queue_len=queues) if queues else {}))
    base = Gen(1).fill(200).array()
    pr.reset(Gen.START).push(base, memory)
    t_render = newest_ns(same(pr)) - 2000
    same(pr, render_at=t_render)
    # TIME_LOW steps back inside the packet (late events, and the packet reaches back behind the newest staged stamp)
    words = [AX | 100, AX | 0x800 | 101, TL | 2, AX | 102, V12 | 0x3F, TL | 1, AX | 103, TL | 3000, AX | 104, AX | 105, TL | 2999, AX | 106]
    want = pr.push(words, memory)
    st = same(pr)
    assert st["late"] > 0 and len(want) == 13
    stamps = np.frombuffer(st["stamps"], np.uint64).astype(np.int64)
    assert (np.diff(stamps) >= 0).all()
    # in order inside itself, but behind what is staged
    pr.push([TL | 2500, AX | 107, AX | 108], memory)
    after = Gen(2)
    after.th, after.lo = pr.model["time_high"] + 1, 0
    pr.push(after.word("th").word("tl").fill(300).array(), memory)
    same(pr, render_at="newest")
    pr.close()


def _fast_words(ev, base_us):
    """events (microsecond stamps above base_us, ascending) as TIME_HIGH (where it changes) / TIME_LOW / ADDR_Y / ADDR_X words, in
    numpy; the restatement's encoder says the same of a short stream (asserted where this is used)"""
    t = (abi.event_ns(ev) // np.uint64(1000)).astype(np.int64) - base_us
    assert len(t) == 0 or (t[0] >= 0 and t[-1] < 2 ** 24 and (np.diff(t) >= 0).all())
    hi = t >> 12
    quad = np.stack([TH | hi, TL | (t & 0xFFF), AY | ev["y"].astype(np.int64), AX | (ev["polarity"] != 0).astype(np.int64) << 11 | ev["x"].astype(np.int64)], 1)
    keep = np.ones(quad.shape, bool)
    keep[1:, 0] = hi[1:] != hi[:-1]
    return quad[keep].astype(np.uint16)


def _us_records(ev):
    return abi.make_events(ev["x"], ev["y"], abi.event_ns(ev) // np.uint64(1000) * np.uint64(1000), (ev["polarity"] != 0).astype(np.uint8))


def test_fast_words_say_what_the_restated_encoder_says(upenn_stream):
    ev = upenn_stream.ev_left[:300]
    base = int(abi.event_ns(ev)[0] // 1000) - 3
    words = _fast_words(ev, base)
    got, _, _ = R.decode(words.tolist(), None, base)
    assert R.records(got).tobytes() == _us_records(ev).tobytes()
    E = [(int(e["x"]), int(e["y"]), int(abi.event_ns(ev[i:i + 1])[0] // 1000) - base, int(e["polarity"] != 0)) for i, e in enumerate(ev)]
    assert R.decode(R.encode(E), None, base)[0] == got


def test_routed_handles_and_their_refusal(upenn_rig, upenn_stream):
    """two logical row-band shards per side, as tests/test_gpu_shard.py sets them up: one side fed records, one fed EVT3 words"""
    from test_gpu_shard import _emulated_gather
    rig, stream = upenn_rig, upenn_stream
    p, _ = params.make_params(params.PRESETS["mvstereo_upenn"], rig)
    G = 2
    sides = [[lib.Esvo(p, rig) for _ in range(G)] for _ in range(2)]
    for shards in sides:
        for g, d in enumerate(shards):
            y0, y1 = edist.band_of(g, G, rig.height)
            d.set_band(y0, y1, g, G, routing="y_rect")
    base = stream.t0_ns // 1000 - 10
    t_prev = stream.t0_ns
    for k in range(3):
        t = stream.t0_ns + int((0.07 + 0.01 * k) * 1e9)
        stamps, poses = rostime.pose_table(stream.pose, t, p.bm_half_slice_thickness)
        for side, shards in enumerate(sides):
            for g, d in enumerate(shards):
                for cam in (0, 1):
                    ev = stream.slice(cam, t_prev, t + 5_000_000)
                    if side == 0:
                        d.ts_push_events(cam, _us_records(ev))
                    else:
                        words = _fast_words(ev, base)
                        assert d.ts_push_evt3(cam, to_device(words, 1) if g == 1 else words, base) == len(ev)
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
                assert state(sides[0][g], cam) == state(sides[1][g], cam), (k, g, cam)
        maps = [edist.merge_band_maps([d.get_map() for d in shards]) for shards in sides]
        assert maps[0].tobytes() == maps[1].tobytes(), k
    assert len(maps[0]) > 50
    # a packet that reaches back: refused on a routed handle, by both calls alike; nothing consumed, the decoder state included
    ev = stream.slice(0, t_prev - 2_000_000, t_prev - 1_000_000)
    assert len(ev) > 1
    before = [state(sides[s][0]) for s in range(2)]
    dec = (sides[1][0].evt3_state(0).as_tuple(), sides[1][0].evt3_stats(0))
    with pytest.raises(lib.EsvoError) as ea:
        sides[0][0].ts_push_events(0, _us_records(ev))
    with pytest.raises(lib.EsvoError) as eb:
        sides[1][0].ts_push_evt3(0, _fast_words(ev, base), base)
    assert ea.value.code == eb.value.code and str(ea.value) == str(eb.value)
    assert [state(sides[s][0]) for s in range(2)] == before
    assert (sides[1][0].evt3_state(0).as_tuple(), sides[1][0].evt3_stats(0)) == dec
    for shards in sides:
        for d in shards:
            d.close()


def _raw_push(dev, addr, n_bytes, memory, off=T0_US, cam=0):
    n = ctypes.c_size_t(123)
    rc = lib.load().esvo_ts_push_evt3(dev.h, cam, addr, n_bytes, memory, off, ctypes.byref(n))
    assert rc == 0 or n.value == 0
    return rc


def test_refusals_change_nothing(small):
    import torch
    small.reset(Gen.START).push(Gen(5).fill(300).array())
    before = same(small)
    dec = (small.b.evt3_state(0).as_tuple(), small.b.evt3_stats(0))

    def unchanged():
        assert state(small.b) == before and (small.b.evt3_state(0).as_tuple(), small.b.evt3_stats(0)) == dec

    nxt = Gen(6)
    nxt.th, nxt.lo = small.model["time_high"], small.model["time_low"]
    words = nxt.fill(200).array()
    dwords = to_device(words)
    # capacity: more events than the ring holds, from either memory, at either side of the host / device decode bound
    many = np.array([V12 | 0xFFF] * 86, np.uint16)                        # 1032 events
    for bound in (0, 1 << 20):
        small.b.debug_evt3_device_min(bound)
        for w in (many, to_device(many)):
            with pytest.raises(lib.EsvoError) as e:
                small.b.ts_push_evt3(0, w, T0_US)
            assert e.value.code == abi.ERR_CAPACITY
            unchanged()
        # a bad stamp: the offset puts the time below zero from event 0 on; above 2^32 s from the first event behind a far TIME_HIGH
        for w, off, bad in ((words, -(1 << 40), 0), (np.array([AX | 1, AX | 2, TH | 4095, AX | 3], np.uint16), R.STAMP_END // 1000 - (4000 << 12), 2)):
            assert small.model["loops"] == 0 and small.model["time_high"] < 4000
            for ww in (w, to_device(w)):
                with pytest.raises(lib.EsvoError) as e:
                    small.b.ts_push_evt3(0, ww, off)
                assert e.value.code == abi.ERR_INVALID_ARG and f"event {bad} " in str(e.value)
                unchanged()
    small.b.debug_evt3_device_min(0)
    # mislabelled pointers: refused by the attribute check, before any launch or copy
    pin = lib.PinnedEvents(64)
    assert _raw_push(small.b, pin.ptr.value, 256, abi.MEM_DEVICE) == abi.ERR_INVALID_ARG       # pinned host memory labelled DEVICE
    assert _raw_push(small.b, words.ctypes.data, 2 * len(words), abi.MEM_DEVICE) == abi.ERR_INVALID_ARG   # pageable labelled DEVICE
    assert _raw_push(small.b, dwords.data_ptr(), 2 * len(words), abi.MEM_HOST) == abi.ERR_INVALID_ARG    # device labelled HOST
    unchanged()
    # arguments
    assert _raw_push(small.b, words.ctypes.data, 2 * len(words) - 1, abi.MEM_HOST) == abi.ERR_INVALID_ARG   # an odd number of bytes
    assert _raw_push(small.b, words.ctypes.data + 1, 2 * len(words) - 2, abi.MEM_HOST) == abi.ERR_INVALID_ARG  # an odd address
    assert _raw_push(small.b, dwords.data_ptr() + 1, 2 * len(words) - 2, abi.MEM_DEVICE) == abi.ERR_INVALID_ARG
    assert _raw_push(small.b, words.ctypes.data, 2 * len(words), 2) == abi.ERR_INVALID_ARG
    assert _raw_push(small.b, None, 2, abi.MEM_HOST) == abi.ERR_INVALID_ARG
    assert _raw_push(small.b, words.ctypes.data, 2 ** 32, abi.MEM_HOST) == abi.ERR_INVALID_ARG             # 2^31 words
    assert _raw_push(small.b, None, 0, abi.MEM_HOST) == 0                                                   # no words: a no-op
    unchanged()
    pin.free()
    torch.cuda.synchronize()
    # the next valid push lands where it would have
    small.push(words, "device")
    st = same(small)
    assert st["late"] == 0 and st["bounds"][1] > before["bounds"][1]


def test_host_decode_below_the_bound_equals_the_device_decode(upenn_rig):
    pr = Pair(upenn_rig, 8192)
    words = Gen(11).word("ax").fill(3000).array()
    prev = pr.b.debug_evt3_device_min(1 << 20)
    assert prev == 0
    want = pr.reset(Gen.START).push(words)
    host = same(pr)
    pr.b.debug_evt3_device_min(0)
    pr.reset(Gen.START).push(words)
    assert same(pr) == host and host["records"] == want.tobytes()
    pr.close()


def test_end_to_end_twenty_ticks_fed_as_evt3():
    sc = S.Scenario("upenn", n_ticks=20)
    rig, p, st = sc.rig, sc.params, sc.stream()
    a, b = lib.Esvo(p, rig), lib.Esvo(p, rig)
    base = st.t0_ns // 1000 - 1000
    done = [0, 0]
    for k in range(sc.n_ticks):
        t = st.t0_ns + int(round((sc.spec["t_first"] + sc.spec["dt"] * k) * 1e9))
        for cam, (ev, ns) in enumerate(((st.ev_left, st.ns_left), (st.ev_right, st.ns_right))):
            hi = int(np.searchsorted(ns, t + 5_000_000, side="left"))
            sl = ev[done[cam]:hi]
            done[cam] = hi
            a.ts_push_events(cam, _us_records(sl))
            words = _fast_words(sl, base)
            assert b.ts_push_evt3(cam, to_device(words, k % 3) if k % 2 else words, base) == len(sl)
        stamps, poses = rostime.pose_table(st.pose, t, p.bm_half_slice_thickness)
        for d in (a, b):
            d.ts_render(0, t, download=False); d.ts_render(1, t, download=False)
            d.set_observation(t, None, None, st.pose(t))
            d.tick(t, stamps, poses)
        fa, fb = a.get_last_frame(), b.get_last_frame()
        assert len(fa) > 0 and fa.tobytes() == fb.tobytes(), k
    for cam in (0, 1):
        assert state(a, cam) == state(b, cam)
        assert b.evt3_stats(cam)["events"] == done[cam] and b.evt3_stats(cam)["dropped_events"] == 0
    ma, mb = a.get_map(), b.get_map()
    assert len(ma) > 50 and ma.tobytes() == mb.tobytes()
    a.close(); b.close()


def test_staging_memory(upenn_rig):
    from test_gpu_lifecycle import Ledger
    led = Ledger()
    dev = lib.Esvo(_params(upenn_rig, 1 << 19), upenn_rig)
    dev.debug_evt3_device_min(0)
    created = led()
    words = Gen(21).word("ax").fill(500).array()

    def push(w, memory="host", cam=0):
        st = abi.Evt3State()
        st.flags, st.y, st.base_x, st.time_high, st.time_low, st.loops = R.state_tuple(Gen.START)
        dev.evt3_state(cam, set=st)
        return dev.ts_push_evt3(cam, to_device(w) if memory == "device" else w, T0_US)

    n = push(words)
    first = led()
    assert n > 0 and first[0] == created[0] + 6      # the words, the tile tuples, the header (device and pinned), the column staging (2)
    dev.reset()                                      # the staging survives a reset
    assert led() == first
    push(words)
    dev.reset()
    push(words, "device")
    assert led() == first                            # a second push of the same size allocates nothing
    dev.reset()
    push(Gen(22).word("ax").fill(200_000).array())   # regrow: the same buffers, larger, the old ones freed
    grown = led()
    assert grown[0] == first[0] and grown[1] > first[1]
    push(words, cam=1)                               # the right camera's own set
    assert led()[0] == grown[0] + 6
    dev.close()
    assert led() == (0, 0)
