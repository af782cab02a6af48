"""esvo_ts_push_evt2 on the device (include/esvo_hip.h): a handle fed EVT 2.0 / 2.1 WORDS against a handle fed the RECORDS the
Python-int restatement (tests/evt2_restated.py) decodes from them.  The two are compared byte for byte through esvo_debug_ts_ring
(the ring's records, the host's stamp mirror, ring_base / ring_next), esvo_get_stats (events_staged, late_events) and a rendered
Time Surface; the decoder state and the totals of the words-fed handle against the restatement's.  The words-fed handle decodes
EVERY packet on the device (esvo_debug_evt2_device_min 0) unless a case says otherwise: the shapes below are the wave, round and
tile seams of the scans and of the expansion.  346x260 (upenn rig)."""
import ctypes

import numpy as np
import pytest

import evt2_restated as R
import scenarios as S
from esvo_amd import abi, dist as edist, lib, params, rostime

pytestmark = pytest.mark.gpu

W, H = 346, 260
TILE = 2048                       # words per tile of the device decode, walked in 8 rounds of 256 (a wave: 64 of them)
T0_US = 1_700_000_000_000_000     # t_offset_us of the crafted streams: sec and nsec are both in use
F20, F21, F21L = R.FORMATS
FULL = 0xFFFFFFFF
TH_TOP = 2 ** 28


def per(fmt):
    """uint32 per word"""
    return 1 if fmt == F20 else 2


def _params(rig, ring, **over):
    kw = dict(max_events_per_tick=4096, event_ring_capacity=ring, regularization=0)
    kw.update(over)
    return params.make_params(params.PRESETS["mapping_upenn"], rig, **kw)[0]


def c_state(s):
    st = abi.Evt2State()
    st.flags, st.time_high, st.loops = R.state_tuple(s)
    return st


class Pair:
    """a: fed records; b: fed EVT 2.x words, every packet decoded on the device"""

    def __init__(self, rig, ring, **over):
        self.p = _params(rig, ring, **over)
        self.a, self.b = lib.Esvo(self.p, rig), lib.Esvo(self.p, rig)
        self.b.debug_evt2_device_min(0)
        self.model = R.fresh_state()          # the restatement's state of b's left camera
        self.totals = dict.fromkeys(R.COUNTS, 0)

    def reset(self, state=None):
        self.a.reset(); self.b.reset()
        self.model, self.totals = R.fresh_state(), dict.fromkeys(R.COUNTS, 0)
        if state is not None:
            self.b.evt2_state(0, set=c_state(state))
            self.model = dict(state)
        return self

    def push(self, u32, fmt, memory="host", lead=0, off=T0_US):
        """the words (their memory image) to b, the records they decode to (restatement) to a; -> the records"""
        u32 = np.asarray(u32, np.uint32)
        ev, self.model, c = R.decode(u32.tolist(), fmt, self.model, off)
        for k in c:
            self.totals[k] += c[k]
        want = R.records(ev)
        if len(want):
            self.a.ts_push_events(0, want)
        n = self.b.ts_push_evt2(0, to_device(u32, lead) if memory == "device" else u32, fmt, off)
        assert n == len(want)
        return want

    def close(self):
        self.a.close(); self.b.close()


def to_device(u32, lead=0):
    """the words in device memory, `lead` 4-byte words into a larger int32 tensor (an odd lead: an EVT 2.1 base that is 4- but not
    8-byte aligned)"""
    import torch
    host = np.concatenate([np.full(lead, 0x1FFFFFFF, np.uint32), u32, np.full(3, 0x1FFFFFFF, np.uint32)])
    d = torch.from_numpy(host.view(np.int32)).cuda()[lead:lead + len(u32)]
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
        assert pr.b.evt2_state(0).as_tuple() == R.state_tuple(pr.model)
        assert pr.b.evt2_stats(0) == pr.totals
    if render_at is not None:   # "newest": just behind the newest staged stamp
        t = newest_ns(sa) + 1 if render_at == "newest" else render_at
        img = [d.ts_render(cam, t) for d in (pr.a, pr.b)]
        assert np.array_equal(img[0], img[1])
        return sa, img[0]
    return sa


def newest_ns(st):
    return int(np.frombuffer(st["stamps"], np.uint64)[-1])


def cd(fmt, pol, ts6, x, y, valid=1):
    """the image of one event word: EVT 2.0 has no mask (valid must be 1)"""
    if fmt == F20:
        assert valid == 1
        return [R.cd_word(pol, ts6, x, y)]
    return R.image([R.vector_word(pol, ts6, x, y, valid)], fmt)


class Gen:
    """words of a stream whose time never steps back, so that every packet cut from it takes the in-order path; events fall into
    a block of the sensor (a render's median filter erases isolated ones).  self.words: one list of uint32 per word."""
    START = dict(have_th=1, time_high=TH_TOP - 9000, loops=0)   # a long stream meets a time loop
    KINDS = ("cd", "th", "ext", "res")
    WEIGHTS = np.array([70, 14, 6, 10]) / 100.0

    def __init__(self, seed, fmt, complete=True):
        """complete: the stream continues START (set it on the handle); else it starts from nothing: two event words (dropped:
        2 events in EVT 2.0, 3 + 1 in EVT 2.1), then the first TIME_HIGH"""
        self.rng, self.fmt = np.random.default_rng(seed), fmt
        self.th, self.ts6, self.words = self.START["time_high"], 0, []
        if not complete:
            self.word("cd", valid=1 if fmt == F20 else 0x7).word("cd", valid=1).word("th", to=self.th)

    def word(self, kind, wrap=False, to=None, least=0, valid=None):
        """one more word; TIME_HIGH: wrap makes it a time loop, to jumps ahead to (at least) that value; cd: valid gives the mask"""
        r, fmt = self.rng, self.fmt
        if kind == "cd":
            self.ts6 = min(63, self.ts6 + int(r.integers(0, 3)))
            if valid is None:
                u, bits = float(r.random()), [int(b) for b in r.integers(0, 32, 3)]   # 15 % empty, 50 % one bit, 30 % up to three, 5 % full
                valid = 1 if fmt == F20 else 0 if u < 0.15 else 1 << bits[0] if u < 0.65 else 1 << bits[0] | 1 << bits[1] | 1 << bits[2] if u < 0.95 else FULL
            self.words.append(cd(fmt, int(r.integers(0, 2)), self.ts6, int(r.integers(96, 112)), int(r.integers(100, 112)), valid))
        elif kind == "th":
            before = self.th
            if to is not None:
                self.th = max(self.th, to)
            elif wrap or self.th >= TH_TOP - 8:      # a time loop: the step back is 2^27 or more
                assert self.th >= 2 ** 27 + 5000
                self.th -= 2 ** 27 + 5000
            else:
                self.th += int(r.integers(least, 4))
            if self.th != before:
                self.ts6 = 0
            self.words.append(R.time_high_word(self.th, fmt))
        else:
            typ = R.EXT_TRIGGER if kind == "ext" else int(r.choice(R.OTHER))
            payload = int(r.integers(0, 2 ** 28))
            self.words.append([typ << 28 | payload] if fmt == F20 else R.image([typ << 60 | payload << 32 | int(r.integers(0, 2 ** 32))], fmt))
        return self

    def fill(self, upto):
        """random words until the stream has `upto` words"""
        if upto > len(self.words):
            for k in self.rng.choice(len(self.KINDS), upto - len(self.words), p=self.WEIGHTS).tolist():
                self.word(self.KINDS[k])
        return self

    def array(self):
        return np.array([u for w in self.words for u in w], np.uint32)

    def type_at(self, i):
        return next(R.words_of(self.words[i], self.fmt))[0]


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


_LENGTHS = {}


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 70001])
def test_lengths(pair, n, memory, fmt):
    if (n, fmt) not in _LENGTHS:                  # (one stream serves both memories)
        _LENGTHS[n, fmt] = Gen(n, fmt).word("cd", valid=1).fill(n).array()
    words = _LENGTHS[n, fmt]
    assert len(words) == n * per(fmt)
    want = pair.reset(Gen.START).push(words, fmt, memory)
    st, img = same(pair, render_at="newest")
    assert st["bounds"] == (0, len(want)) and st["records"] == want.tobytes() and st["late"] == 0
    assert len(want) >= 1
    if n == 70001:
        assert pair.totals["time_loops"] >= 1 and pair.totals["ext_triggers"] > 0 and pair.totals["ignored_words"] > 0
        assert fmt == F20 or len(want) > n          # the output is larger than the input
    # the same stream from nothing: the words in front of the first TIME_HIGH are dropped and counted
    if 63 <= n <= 4097:
        words = Gen(n, fmt, complete=False).fill(n).array()
        want = pair.reset().push(words, fmt, memory)
        assert same(pair)["records"] == want.tobytes() and pair.totals["dropped_events"] == (2 if fmt == F20 else 4)


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("seam", [TILE, 2 * TILE, 33 * TILE])
def test_time_high_ends_a_tile_and_its_consumer_opens_the_next(pair, seam, fmt):
    g = Gen(seam, fmt).fill(seam - 1).word("th", least=1).word("cd", valid=1 if fmt == F20 else 0x80000001).fill(seam + 70)
    assert g.type_at(seam - 1) == R.TIME_HIGH and g.type_at(seam) <= R.CD_ON
    want = pair.reset(Gen.START).push(g.array(), fmt)
    assert same(pair)["records"] == want.tobytes()


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("seam", [TILE, 3 * TILE])
def test_time_loop_at_a_tile_seam(pair, seam, fmt):
    # the looping TIME_HIGH is the tile's last word (its events open the next tile) / the next tile's first word (the TIME_HIGH
    # it is compared with is the last word of the tile in front)
    for at in (seam - 1, seam):
        g = Gen(at, fmt).fill(at - 1).word("th", to=TH_TOP - 100).word("th", wrap=True).word("cd", valid=1).word("cd").fill(seam + 40)
        assert g.type_at(at) == g.type_at(at - 1) == R.TIME_HIGH
        want = pair.reset(Gen.START).push(g.array(), fmt)
        assert same(pair)["records"] == want.tobytes() and pair.totals["time_loops"] >= 1
    # two tiles without any TIME_HIGH word between two TIME_HIGH words; the second loops, the third (a step ahead) does not
    quiet = [u for i in range(2 * TILE) for u in cd(fmt, i & 1, 0, 100 + i % 8, 100 + i // 8 % 8, 1 if fmt == F20 else (1, 0x5, 0)[i % 3])]
    words = R.time_high_word(TH_TOP - 50, fmt) + quiet + R.time_high_word(100, fmt) + cd(fmt, 1, 0, 101, 101) + R.time_high_word(TH_TOP - 50, fmt) + cd(fmt, 1, 0, 102, 102)
    want = pair.reset(Gen.START).push(words, fmt)
    assert same(pair)["records"] == want.tobytes() and pair.totals["time_loops"] == 1 and pair.model["loops"] == 1


@pytest.mark.parametrize("fmt", [F21, F21L])
@pytest.mark.parametrize("at", [63, 64, 255, 256, TILE - 1, TILE])
def test_full_word_at_the_end_of_a_waves_share_of_a_round_and_of_a_tile(pair, at, fmt):
    """all 32 bits set in the last word of a wave's 64, of a round's 256, of a tile's 2048 -- and in the word behind each"""
    for memory in ("host", "device"):
        g = Gen(at, fmt).fill(at).word("cd", valid=FULL).fill(at + 200)
        want = pair.reset(Gen.START).push(g.array(), fmt, memory)
        st, img = same(pair, render_at="newest")
        assert st["records"] == want.tobytes() and len(want) >= 32 and img.any()
    # ... as the packet's last word
    g = Gen(at, fmt).fill(at).word("cd", valid=FULL)
    want = pair.reset(Gen.START).push(g.array(), fmt)
    assert same(pair)["records"] == want.tobytes() and [int(v) for v in want["x"][-32:]] == list(range(int(want["x"][-32]), int(want["x"][-32]) + 32))


@pytest.mark.parametrize("fmt", [F21, F21L])
def test_runs_of_full_words_and_empty_masks_between_them(pair, fmt):
    # 64 full words: 2048 events from 64 words, the output tile is 32 times the input
    run = [u for i in range(64) for u in cd(fmt, i & 1, i // 8, 100, 100 + i % 8, FULL)]
    want = pair.reset(Gen.START).push(run, fmt)
    st, img = same(pair, render_at="newest")
    assert len(want) == 2048 and st["records"] == want.tobytes() and img.any()
    # a whole tile of them, and beyond: every step of every wave writes 64 events
    run = [u for i in range(TILE + 70) for u in cd(fmt, i & 1, min(63, i // 40), 100, 100 + i % 8, FULL)]
    want = pair.reset(Gen.START).push(run, fmt, "device", lead=1)
    assert len(want) == 32 * (TILE + 70) and same(pair)["records"] == want.tobytes()
    # words with an empty mask between full ones, in every pairing of a step's two words
    masks = [FULL, 0, FULL, 0, 0, FULL, FULL, 0, 0, 0, FULL, 0x80000000, 0, 1, FULL] * 40
    mixed = [u for i, m in enumerate(masks) for u in cd(fmt, i & 1, min(63, i // 10), 96 + i % 5, 100 + i % 8, m)]
    want = pair.reset(Gen.START).push(mixed, fmt)
    assert len(want) == 40 * (6 * 32 + 2) and same(pair)["records"] == want.tobytes()


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_full_word_straddles_the_end_of_the_ring(small, fmt):
    first = np.array([u for i in range(1010) for u in cd(fmt, i & 1, min(63, i // 16), 100 + i % 8, 100 + i // 8 % 8)], np.uint32)   # a block of 8 x 8
    for memory in ("host", "device"):
        small.reset(Gen.START).push(first, fmt, memory)
        st, _ = same(small, render_at="newest")                           # everything staged is scattered: the ring may evict
        assert st["bounds"] == (0, 1010)
        more = R.time_high_word(TH_TOP - 8000, fmt) + (cd(fmt, 1, 0, 100, 104, FULL) if fmt != F20 else [u for i in range(32) for u in cd(fmt, 1, 0, 100 + i, 104)])
        want = small.push(more, fmt, memory)
        st, img = same(small, render_at="newest")
        assert st["bounds"] == (1042 - 1024, 1042) and st["records"][-32 * 16:] == want.tobytes() and img.any()


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_a_packet_that_only_sets_state(pair, fmt):
    pair.reset()
    ext = [R.EXT_TRIGGER << 28 | 1] if fmt == F20 else R.image([R.EXT_TRIGGER << 60 | 1], fmt)
    assert len(pair.push(R.time_high_word(77, fmt) + ext, fmt)) == 0
    assert len(pair.push(ext + R.time_high_word(78, fmt) + (cd(fmt, 1, 0, 5, 5, 0) if fmt != F20 else []), fmt)) == 0
    st = same(pair)
    assert st["bounds"] == (0, 0) and pair.totals["words"] == (4 if fmt == F20 else 5) and pair.b.evt2_state(0).as_tuple() == (1, 78, 0)
    want = pair.push(cd(fmt, 1, 9, 103, 50) + cd(fmt, 0, 9, 104, 51), fmt)
    st = same(pair)
    assert st["records"] == want.tobytes() and [int(x) for x in want["x"]] == [103, 104] and [int(p) for p in want["polarity"]] == [1, 0]
    assert [int(s) * 10 ** 9 + int(ns) for s, ns in zip(want["sec"], want["nsec"])] == [(T0_US + (78 << 6 | 9)) * 1000] * 2
    # esvo_reset clears the state and the totals
    pair.reset()
    assert pair.b.evt2_state(0).as_tuple() == (0, 0, 0) and pair.b.evt2_stats(0) == dict.fromkeys(R.COUNTS, 0)
    assert len(pair.push(cd(fmt, 1, 0, 1, 1), fmt)) == 0 and pair.totals["dropped_events"] == 1
    same(pair)
    # the set masks: flags to bit 0, time_high to 28 bits
    st = abi.Evt2State()
    st.flags, st.time_high, st.loops, st.reserved = 0xFF, 0xF0000005, 9, 3
    pair.b.evt2_state(0, set=st)
    got = pair.b.evt2_state(0)
    assert got.as_tuple() == (1, 5, 9) and got.reserved == 0


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_whole_and_in_chunks_cut_between_every_pair_of_word_types(pair, fmt):
    g, cuts = Gen(49, fmt), []
    for a in Gen.KINDS:
        for b in Gen.KINDS:
            g.fill(len(g.words) + 37).word(a)
            cuts.append(len(g.words) * per(fmt))
            g.word(b)
    words = g.fill(len(g.words) + 2100).array()
    assert len(cuts) == 16
    want = pair.reset(Gen.START).push(words, fmt)
    whole = same(pair)
    assert whole["records"] == want.tobytes() and len(want) > 1000
    whole_state, whole_totals = pair.b.evt2_state(0).as_tuple(), dict(pair.totals)
    for memory in ("host", "device"):
        pair.reset(Gen.START)
        for lo, hi in zip([0] + cuts, cuts + [len(words)]):
            pair.push(words[lo:hi], fmt, memory, lead=lo % 8)
        assert same(pair) == whole
        assert pair.b.evt2_state(0).as_tuple() == whole_state and pair.totals == whole_totals


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("n", [5, 2049])
def test_device_words_at_offsets_into_a_larger_tensor(pair, n, fmt):
    words = Gen(n + 1, fmt).word("cd", valid=1).fill(n).array()
    want = pair.reset(Gen.START).push(words, fmt)
    host = same(pair)
    assert host["records"] == want.tobytes()
    for lead in (1, 2, 3, 5, 7):                  # an odd lead: an EVT 2.1 base that is 4- but not 8-byte aligned
        pair.reset(Gen.START).push(words, fmt, "device", lead)
        assert same(pair) == host, lead
    big = np.concatenate([np.zeros(3, np.uint32), words])        # a host slice as well
    assert big[3:].ctypes.data % 8 == 4 or big.ctypes.data % 8 == 4
    pair.reset(Gen.START)
    pair.a.ts_push_events(0, want)
    assert pair.b.ts_push_evt2(0, big[3:], fmt, T0_US) == len(want)
    pair.model, pair.totals = R.decode(words.tolist(), fmt, Gen.START, T0_US)[1:]
    assert same(pair) == host


@pytest.mark.parametrize("fmt", [F20, F21])
@pytest.mark.parametrize("queues", [0, 3])
@pytest.mark.parametrize("memory", ["host", "device"])
def test_out_of_order_falls_back_to_the_record_paths(upenn_rig, memory, queues, fmt):
    pr = Pair(upenn_rig, 4096, **(dict(max_event_queue_len=queues) if queues else {}))
    base = Gen(1, fmt).fill(200).array()
    pr.reset(Gen.START).push(base, fmt, memory)
    t_render = newest_ns(same(pr)) - 2000
    same(pr, render_at=t_render)
    th = pr.model["time_high"]
    wide = 1 if fmt == F20 else 0x3F
    # ts6 and TIME_HIGH step back inside the packet (late events, and the packet reaches back behind the newest staged stamp)
    words = (R.time_high_word(th + 2, fmt) + cd(fmt, 0, 20, 100, 100) + cd(fmt, 1, 21, 101, 100) + cd(fmt, 1, 3, 102, 100) + cd(fmt, 1, 2, 103, 101, wide)
             + cd(fmt, 0, 40, 104, 101) + R.time_high_word(th + 1, fmt) + cd(fmt, 1, 63, 105, 101) + R.time_high_word(th + 3, fmt) + cd(fmt, 1, 0, 106, 102))
    want = pr.push(words, fmt, memory)
    st = same(pr)
    assert st["late"] > 0 and len(want) == (7 if fmt == F20 else 12)
    stamps = np.frombuffer(st["stamps"], np.uint64).astype(np.int64)
    assert (np.diff(stamps) >= 0).all()
    # in order inside itself, but behind what is staged
    pr.push(R.time_high_word(th + 2, fmt) + cd(fmt, 1, 1, 107, 102) + cd(fmt, 0, 2, 108, 102, wide), fmt, memory)
    after = Gen(2, fmt)
    after.th = th + 3
    pr.push(after.word("th", least=1).fill(300).array(), fmt, memory)
    same(pr, render_at="newest")
    pr.close()


def _fast_words(ev, base_us, fmt):
    """events (microsecond stamps above base_us, ascending, below 2^34) as the memory image of TIME_HIGH words (where it changes)
    and event words, in numpy: EVT 2.0 one word per event; EVT 2.1 one word per run of ADJACENT events of equal (us, y, polarity,
    x >> 5) with ascending x (so the decoded order is the events' order).  The restatement says the same of a short stream
    (asserted where this is used)."""
    t = (abi.event_ns(ev) // np.uint64(1000)).astype(np.int64) - base_us
    assert len(t) == 0 or (t[0] >= 0 and t[-1] < 2 ** 34 and (np.diff(t) >= 0).all())
    x, y, pol = ev["x"].astype(np.uint64), ev["y"].astype(np.uint64), (ev["polarity"] != 0).astype(np.uint64)
    t = t.astype(np.uint64)
    hi, ts6 = t >> np.uint64(6), t & np.uint64(63)
    u = np.uint64
    if fmt == F20:
        quad = np.stack([u(R.TIME_HIGH << 28) | hi, pol << u(28) | ts6 << u(22) | x << u(11) | y], 1)
        keep = np.ones(quad.shape, bool)
        keep[1:, 0] = hi[1:] != hi[:-1]
        return quad[keep].astype(np.uint32)
    if len(t) == 0:
        return np.zeros(0, np.uint32)
    merge = np.zeros(len(t), bool)
    merge[1:] = (t[1:] == t[:-1]) & (y[1:] == y[:-1]) & (pol[1:] == pol[:-1]) & (x[1:] > x[:-1]) & (x[1:] >> u(5) == x[:-1] >> u(5))
    first = np.flatnonzero(~merge)
    valid = np.bitwise_or.reduceat(u(1) << (x & u(31)), first)
    vec = pol[first] << u(60) | ts6[first] << u(54) | (x[first] >> u(5) << u(5)) << u(43) | y[first] << u(32) | valid
    quad = np.stack([u(R.TIME_HIGH << 60) | hi[first] << u(32), vec], 1)
    keep = np.ones(quad.shape, bool)
    keep[1:, 0] = hi[first][1:] != hi[first][:-1]
    halves = quad[keep].astype("<u8").view("<u4").reshape(-1, 2)
    return (halves if fmt == F21 else halves[:, ::-1]).reshape(-1).copy()


def _us_records(ev):
    return abi.make_events(ev["x"], ev["y"], abi.event_ns(ev) // np.uint64(1000) * np.uint64(1000), (ev["polarity"] != 0).astype(np.uint8))


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_fast_words_say_what_the_restatement_says(upenn_stream, fmt):
    ev = upenn_stream.ev_left[:300].copy()
    ev[11:14] = ev[10]                      # a run for EVT 2.1: four events of one microsecond and row, x ascending in one block of 32
    ev["x"][10:14] = (ev["x"][10] >> 5 << 5) + np.array([1, 2, 9, 31], np.uint16)
    base = int(abi.event_ns(ev)[0] // 1000) - 3
    words = _fast_words(ev, base, fmt)
    got, _, c = R.decode(words.tolist(), fmt, None, base)
    assert R.records(got).tobytes() == _us_records(ev).tobytes()
    assert fmt == F20 or c["words"] < len(_fast_words(ev, base, F20))      # the run is one word
    if fmt != F21L:
        E = [(int(e["x"]), int(e["y"]), int(abi.event_ns(ev[i:i + 1])[0] // 1000) - base, int(e["polarity"] != 0)) for i, e in enumerate(ev)]
        assert R.decode(R.encode(E, fmt), fmt, None, base)[0] == got


def test_routed_handles_and_their_refusal(upenn_rig, upenn_stream):
    """two logical row-band shards per side, as tests/test_gpu_shard.py sets them up: one side fed records, one fed words (the left
    camera EVT 2.1, the right EVT 2.0)"""
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
    fmts = (F21, F20)
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
                        words = _fast_words(ev, base, fmts[cam])
                        assert d.ts_push_evt2(cam, to_device(words, 1) if g == 1 else words, fmts[cam], base) == len(ev)
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
    dec = (sides[1][0].evt2_state(0).as_tuple(), sides[1][0].evt2_stats(0))
    with pytest.raises(lib.EsvoError) as ea:
        sides[0][0].ts_push_events(0, _us_records(ev))
    with pytest.raises(lib.EsvoError) as eb:
        sides[1][0].ts_push_evt2(0, _fast_words(ev, base, F21), F21, base)
    assert ea.value.code == eb.value.code and str(ea.value) == str(eb.value)
    assert [state(sides[s][0]) for s in range(2)] == before
    assert (sides[1][0].evt2_state(0).as_tuple(), sides[1][0].evt2_stats(0)) == dec
    for shards in sides:
        for d in shards:
            d.close()


def _raw_push(dev, addr, n_bytes, fmt, memory, off=T0_US, cam=0):
    n = ctypes.c_size_t(123)
    rc = lib.load().esvo_ts_push_evt2(dev.h, cam, addr, n_bytes, fmt, memory, off, ctypes.byref(n))
    assert rc == 0 or n.value == 0
    return rc


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_refusals_change_nothing(small, fmt):
    import torch
    small.b.debug_evt2_device_min(0)
    small.reset(Gen.START).push(Gen(5, fmt).fill(300).array(), fmt)
    before = same(small)
    dec = (small.b.evt2_state(0).as_tuple(), small.b.evt2_stats(0))

    def unchanged():
        assert state(small.b) == before and (small.b.evt2_state(0).as_tuple(), small.b.evt2_stats(0)) == dec

    nxt = Gen(6, fmt)
    nxt.th = small.model["time_high"]
    words = nxt.word("th", least=1).fill(200).array()
    dwords = to_device(words)
    # capacity: more events than the ring holds, from either memory, at either side of the host / device decode bound
    many = np.array([u for i in range(1032) for u in cd(fmt, 1, 0, 100, 100)] if fmt == F20 else [u for i in range(33) for u in cd(fmt, 1, 0, 100, 100, FULL)], np.uint32)
    th = small.model["time_high"]
    assert small.model["loops"] == 0 and th < TH_TOP - 200
    far = np.array(cd(fmt, 1, 0, 1, 1) + cd(fmt, 1, 0, 2, 1) + R.time_high_word(TH_TOP - 1, fmt) + cd(fmt, 1, 0, 3, 1), np.uint32)
    for bound in (0, 1 << 30):
        small.b.debug_evt2_device_min(bound)
        for w in (many, to_device(many)):
            with pytest.raises(lib.EsvoError) as e:
                small.b.ts_push_evt2(0, w, fmt, T0_US)
            assert e.value.code == abi.ERR_CAPACITY
            unchanged()
        # a bad stamp: the offset puts the time below zero from event 0 on; above 2^32 s from the first event behind a far TIME_HIGH
        for w, off, bad in ((words, -(1 << 50), 0), (far, R.STAMP_END // 1000 - ((TH_TOP - 100) << 6), 2)):
            for ww in (w, to_device(w)):
                with pytest.raises(lib.EsvoError) as e:
                    small.b.ts_push_evt2(0, ww, fmt, off)
                assert e.value.code == abi.ERR_INVALID_ARG and f"event {bad} " in str(e.value)
                unchanged()
    small.b.debug_evt2_device_min(0)
    # mislabelled pointers: refused by the attribute check, before any launch or copy
    pin = lib.PinnedEvents(64)
    nb = 4 * len(words)
    assert nb % 8 == 0 or fmt == F20
    assert _raw_push(small.b, pin.ptr.value, 256, fmt, abi.MEM_DEVICE) == abi.ERR_INVALID_ARG       # pinned host memory labelled DEVICE
    assert _raw_push(small.b, words.ctypes.data, nb, fmt, abi.MEM_DEVICE) == abi.ERR_INVALID_ARG     # pageable labelled DEVICE
    assert _raw_push(small.b, dwords.data_ptr(), nb, fmt, abi.MEM_HOST) == abi.ERR_INVALID_ARG      # device labelled HOST
    unchanged()
    # arguments
    for cut in (1, 2, 3) + (() if fmt == F20 else (4,)):                                             # n_bytes % 4 (EVT 2.0) / % 8 (EVT 2.1)
        assert _raw_push(small.b, words.ctypes.data, nb - cut, fmt, abi.MEM_HOST) == abi.ERR_INVALID_ARG
    assert _raw_push(small.b, words.ctypes.data + 2, nb - 8, fmt, abi.MEM_HOST) == abi.ERR_INVALID_ARG    # an address = 2 mod 4
    assert _raw_push(small.b, dwords.data_ptr() + 2, nb - 8, fmt, abi.MEM_DEVICE) == abi.ERR_INVALID_ARG
    for unknown in (0, 2, 22, 30, 120):                                                               # 30: that is esvo_ts_push_evt3's
        assert _raw_push(small.b, words.ctypes.data, 8, unknown, abi.MEM_HOST) == abi.ERR_INVALID_ARG
    assert _raw_push(small.b, words.ctypes.data, nb, fmt, 2) == abi.ERR_INVALID_ARG
    assert _raw_push(small.b, None, 8, fmt, abi.MEM_HOST) == abi.ERR_INVALID_ARG
    assert _raw_push(small.b, words.ctypes.data, 4 * per(fmt) * 2 ** 31, fmt, abi.MEM_HOST) == abi.ERR_INVALID_ARG   # 2^31 words
    assert _raw_push(small.b, None, 0, fmt, abi.MEM_HOST) == 0                                        # no words: a no-op
    unchanged()
    pin.free()
    torch.cuda.synchronize()
    # the next valid push lands where it would have
    small.push(words, fmt, "device")
    st = same(small)
    assert st["late"] == 0 and st["bounds"][1] > before["bounds"][1]


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_host_decode_below_the_bound_equals_the_device_decode(upenn_rig, fmt):
    pr = Pair(upenn_rig, 16384)
    words = Gen(11, fmt).word("cd", valid=1).fill(3000).array()
    prev = pr.b.debug_evt2_device_min(1 << 30)
    assert prev == 0
    want = pr.reset(Gen.START).push(words, fmt)
    host = same(pr)
    assert pr.b.debug_evt2_device_min(0) == 1 << 30
    pr.reset(Gen.START).push(words, fmt)
    assert same(pr) == host and host["records"] == want.tobytes()
    pr.close()


def test_default_bounds_send_small_packets_to_the_host_decoder(upenn_rig):
    """a fresh handle's bounds: a packet of a few words allocates what a push of its records allocates and no device staging (the
    host decoder took it)"""
    from test_gpu_lifecycle import Ledger
    led = Ledger()
    grew = []
    for feed_words in (False, True):
        dev = lib.Esvo(_params(upenn_rig, 4096), upenn_rig)
        created = led()
        for fmt in R.FORMATS:
            words = Gen(3, fmt).word("cd", valid=1).fill(50).array()
            if feed_words:
                dev.evt2_state(0, set=c_state(Gen.START))
                assert dev.ts_push_evt2(0, words, fmt, T0_US) > 0
            else:
                dev.ts_push_events(0, R.records(R.decode(words.tolist(), fmt, Gen.START, T0_US)[0]))
            dev.reset()
        grew.append(led()[0] - created[0])
        dev.close()
    assert grew[0] == grew[1]


def test_end_to_end_five_ticks_fed_as_evt2():
    sc = S.Scenario("upenn", n_ticks=5)
    rig, p, st = sc.rig, sc.params, sc.stream()
    a, b = lib.Esvo(p, rig), lib.Esvo(p, rig)
    b.debug_evt2_device_min(0)
    base = st.t0_ns // 1000 - 1000
    done = [0, 0]
    fmts = (F21, F20)                                # the left camera EVT 2.1, the right EVT 2.0
    for k in range(sc.n_ticks):
        t = st.t0_ns + int(round((sc.spec["t_first"] + sc.spec["dt"] * k) * 1e9))
        for cam, (ev, ns) in enumerate(((st.ev_left, st.ns_left), (st.ev_right, st.ns_right))):
            hi = int(np.searchsorted(ns, t + 5_000_000, side="left"))
            sl = ev[done[cam]:hi]
            done[cam] = hi
            a.ts_push_events(cam, _us_records(sl))
            words = _fast_words(sl, base, fmts[cam])
            assert b.ts_push_evt2(cam, to_device(words, k % 3) if k % 2 else words, fmts[cam], base) == len(sl)
        stamps, poses = rostime.pose_table(st.pose, t, p.bm_half_slice_thickness)
        for d in (a, b):
            d.ts_render(0, t, download=False); d.ts_render(1, t, download=False)
            d.set_observation(t, None, None, st.pose(t))
            d.tick(t, stamps, poses)
        fa, fb = a.get_last_frame(), b.get_last_frame()
        assert len(fa) > 0 and fa.tobytes() == fb.tobytes(), k
    for cam in (0, 1):
        assert state(a, cam) == state(b, cam)
        assert b.evt2_stats(cam)["events"] == done[cam] and b.evt2_stats(cam)["dropped_events"] == 0
    ma, mb = a.get_map(), b.get_map()
    assert ma.tobytes() == mb.tobytes()
    a.close(); b.close()


def test_staging_memory(upenn_rig):
    from test_gpu_lifecycle import Ledger
    led = Ledger()
    dev = lib.Esvo(_params(upenn_rig, 1 << 19), upenn_rig)
    dev.debug_evt2_device_min(0)
    created = led()
    words = Gen(21, F21).word("cd", valid=1).fill(500).array()

    def push(w, fmt, memory="host", cam=0):
        dev.evt2_state(cam, set=c_state(Gen.START))
        return dev.ts_push_evt2(cam, to_device(w) if memory == "device" else w, fmt, T0_US)

    n = push(words, F21)
    first = led()
    assert n > 0 and first[0] == created[0] + 6      # the words, the tile tuples, the header (device and pinned), the column staging (2)
    dev.reset()                                      # the staging survives a reset
    assert led() == first
    push(words, F21)
    dev.reset()
    push(words.reshape(-1, 2)[:, ::-1].reshape(-1).copy(), F21L, "device")   # the same words, the upper half first
    dev.reset()
    push(Gen(23, F20).word("cd").fill(400).array(), F20)   # one set serves the three formats
    assert led() == first                            # a second push of the same size allocates nothing
    dev.reset()
    push(Gen(22, F20).word("cd").fill(200_000).array(), F20)   # regrow: the same buffers, larger, the old ones freed
    grown = led()
    assert grown[0] == first[0] and grown[1] > first[1]
    push(words, F21, cam=1)                          # the right camera's own set
    assert led()[0] == grown[0] + 6
    dev.close()
    assert led() == (0, 0)
