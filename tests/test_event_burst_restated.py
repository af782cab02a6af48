"""esvo_event_burst_filter_host (include/esvo_hip.h) against the Python-int restatement of the two-stage rule
(tests/event_burst_restated.py): verdict for verdict, `bstamp`, `bflags` and `last` byte for byte, count for count.  Host only."""
import ctypes

import numpy as np
import pytest

import event_burst_restated as B
import event_filter_restated as R
from esvo_amd import abi, lib

T0 = B.T_BASE
SEEDS = (21, 22, 23)
NS = 1000          # burst_ns of the crafted chains


def both(events, W, H, mode, burst_ns, refractory_ns=0, support_ns=0, mask=None, bstamp=None, bflags=None, last=None):
    """the rule by the restatement and by the library, compared; -> the restatement's result"""
    want = B.run(events, W, H, mode, burst_ns, refractory_ns, support_ns, mask, bstamp, bflags, last)
    v, S, G, L, bc, fc = want
    gv, gk, gS, gG, gL, gbc, gfc = lib.event_burst_filter_host(
        R.records(events), W, H, mode, burst_ns, refractory_ns, support_ns, mask,
        None if bstamp is None else B.stamp_array(bstamp), None if bflags is None else B.flags_array(bflags), None if last is None else R.last_array(last))
    assert gv.tolist() == v
    assert gS.tobytes() == B.stamp_array(S).tobytes() and gG.tobytes() == B.flags_array(G).tobytes() and gL.tobytes() == R.last_array(L).tobytes()
    assert gbc == bc and bc["judged"] == bc["passed"] + bc["dropped"]
    assert gfc == fc and fc["events_in"] == sum(fc[k] for k in R.NAMES) == len(events) - bc["dropped"]
    assert gk.tobytes() == R.records(B.kept(events, v)).tobytes()
    return want


def chain(gaps, pols=None, x=5, y=5):
    t, ev = T0, []
    for i, g in enumerate([0] + list(gaps)):
        t += g
        ev.append((x, y, t, 1 if pols is None else pols[i]))
    return ev


def test_sizes_and_bindings():
    assert lib.event_burst_sizes() == [ctypes.sizeof(abi.EventBurstStruct), ctypes.sizeof(abi.EventBurstCounts), 0, 0] == [24, 24, 0, 0]
    assert lib.event_filter_sizes() == [40, 48, 0, 0] and lib.abi_sizes()[7] == 8       # additive: nothing else moved
    assert (abi.BURST_OFF, abi.BURST_TRAIL, abi.BURST_STC_CUT_TRAIL, abi.BURST_STC_KEEP_TRAIL) == (B.OFF, B.TRAIL, B.STC_CUT_TRAIL, B.STC_KEEP_TRAIL)
    assert abi.FILTER_BURST == B.BURST == 5
    assert {"esvo_ts_burst_configure", "esvo_ts_burst_stats", "esvo_ts_burst_state", "esvo_event_burst_filter_host", "esvo_event_burst_sizes"} <= set(lib.SYMBOLS)


K, D = B.KEPT, B.BURST


@pytest.mark.parametrize("mode,want", ((B.TRAIL, [K, D, K]), (B.STC_CUT_TRAIL, [D, K, D]), (B.STC_KEEP_TRAIL, [D, K, D])))
def test_gap_of_exactly_burst_ns_links_and_one_more_does_not(mode, want):
    v, S, G, _, _, _ = both(chain([NS, NS + 1]), 16, 12, mode, NS)
    assert v == want
    assert S[5][5] == T0 + 2 * NS + 1 and G[5][5] == 1           # the state is the last event's, whatever its verdict: polarity 1, not linked


@pytest.mark.parametrize("mode,want", ((B.TRAIL, [K, D, D]), (B.STC_CUT_TRAIL, [D, K, D]), (B.STC_KEEP_TRAIL, [D, K, K])))
def test_equal_stamps_link(mode, want):
    v, _, G, _, _, _ = both(chain([0, 0]), 16, 12, mode, NS)
    assert v == want and G[5][5] == 3


@pytest.mark.parametrize("mode,want", ((B.TRAIL, [K, D, K, D]), (B.STC_CUT_TRAIL, [D, K, D, K]), (B.STC_KEEP_TRAIL, [D, K, D, K])))
def test_polarity_flip_inside_the_window_ends_the_burst(mode, want):
    v, _, G, _, _, _ = both(chain([10, 10, 10], pols=[1, 1, 0, 0]), 16, 12, mode, NS)
    assert v == want and G[5][5] == 2                              # polarity 0, linked


@pytest.mark.parametrize("mode,want", ((B.TRAIL, [K, D, D, D, D, D]), (B.STC_CUT_TRAIL, [D, K, D, D, D, D]), (B.STC_KEEP_TRAIL, [D, K, K, K, K, K])))
def test_long_chain(mode, want):
    v, _, _, L, bc, fc = both(chain([100] * 5), 16, 12, mode, NS)
    assert v == want
    assert bc == {"judged": 6, "passed": want.count(K), "dropped": want.count(D)} and fc["events_in"] == want.count(K)
    assert L[5][5] == T0 + 100 * max(i for i, w in enumerate(want) if w == K)      # a burst-dropped event never reaches `last`


@pytest.mark.parametrize("mode,want", ((B.TRAIL, K), (B.STC_CUT_TRAIL, D), (B.STC_KEEP_TRAIL, D)))
def test_isolated_event(mode, want):
    v, _, _, _, _, _ = both([(3, 3, T0, 0)], 16, 12, mode, NS)
    assert v == [want]


def test_cut_meets_refractory_between_two_bursts_of_opposite_polarity():
    # burst A (polarity 1) at T0, T0 + 100; burst B (polarity 0) at T0 + 200, T0 + 300: CUT passes #2 of each, 200 ns apart
    ev = chain([100, 100, 100], pols=[1, 1, 0, 0])
    v, _, _, L, _, _ = both(ev, 16, 12, B.STC_CUT_TRAIL, NS, refractory_ns=500)
    assert v == [D, K, D, B.REFRACTORY] and L[5][5] == T0 + 100
    v, _, _, _, _, _ = both(ev, 16, 12, B.STC_CUT_TRAIL, NS, refractory_ns=200)
    assert v == [D, K, D, K]


def test_burst_dropped_event_neither_supports_nor_restarts_the_refractory_period():
    # TRAIL: (5, 5) fires at T0 (passes, unsupported), T0 + 100 (burst-dropped); the neighbour (6, 5) at T0 + 150 finds last = T0: 150 > support 120
    v, _, _, L, _, _ = both([(5, 5, T0, 1), (5, 5, T0 + 100, 1), (6, 5, T0 + 150, 1)], 16, 12, B.TRAIL, NS, support_ns=120)
    assert v == [B.UNSUPPORTED, D, B.UNSUPPORTED] and L[5][5] == T0
    # refractory 180: the opposite-polarity event at T0 + 190 is beyond it counted from T0, within it counted from the dropped T0 + 100
    v, _, _, _, _, _ = both([(5, 5, T0, 1), (5, 5, T0 + 100, 1), (5, 5, T0 + 190, 0)], 16, 12, B.TRAIL, NS, refractory_ns=180)
    assert v == [K, D, K]


def test_masked_and_outside_events_leave_the_burst_state_alone():
    mask = R.fresh_last(16, 12)
    mask[4][4] = 1
    v, S, G, _, bc, fc = both([(4, 4, T0, 1), (16, 3, T0 + 1, 1), (3, 12, T0 + 2, 1), (4, 4, T0 + 3, 1)], 16, 12, B.STC_KEEP_TRAIL, NS, mask=mask)
    assert v == [B.MASKED, B.OUTSIDE, B.OUTSIDE, B.MASKED]
    assert not np.any(B.stamp_array(S)) and not np.any(B.flags_array(G)) and bc == B.ZERO_BURST and fc["events_in"] == 4


def test_planted_state():
    W, H = 16, 12
    for mode in B.MODES:
        for flags in range(4):
            for p in (0, 1):
                S, G = B.fresh(W, H), B.fresh(W, H)
                S[2][3], G[2][3] = T0 - 10, flags
                v, _, G2, _, _, _ = both([(3, 2, T0, p)], W, H, mode, NS, bstamp=S, bflags=G)
                linked = p == (flags & 1)
                want = {B.TRAIL: not linked, B.STC_CUT_TRAIL: linked and not flags >> 1, B.STC_KEEP_TRAIL: linked}[mode]
                assert v == [K if want else D] and G2[2][3] == p | (2 if linked else 0)
    # a stamp ahead of the stream: the difference is negative, so within burst_ns
    S, G = B.fresh(W, H), B.fresh(W, H)
    S[2][3], G[2][3] = T0 + 10 ** 9, 1
    v, S2, _, _, _, _ = both([(3, 2, T0, 1), (3, 2, T0 + 1, 1)], W, H, B.STC_CUT_TRAIL, NS, bstamp=S, bflags=G)
    assert v == [K, D] and S2[2][3] == T0 + 1
    # a planted stamp 0 is "none" whatever the flags say
    G[2][3], S[2][3] = 3, 0
    v, _, _, _, _, _ = both([(3, 2, T0, 1)], W, H, B.TRAIL, NS, bstamp=S, bflags=G)
    assert v == [K]


@pytest.mark.parametrize("seed", (5, 6))
def test_stage_off_is_esvo_event_filter_host(seed):
    ev, mask = R.random_stream(seed, 1500)
    rec = R.records(ev)
    gv, gk, gL, gc = lib.event_filter_host(rec, R.W, R.H, R.REFRACTORY_NS, R.SUPPORT_NS, mask)
    v, k, S, G, L, bc, fc = lib.event_burst_filter_host(rec, R.W, R.H, B.OFF, 0, R.REFRACTORY_NS, R.SUPPORT_NS, mask)
    assert v.tobytes() == gv.tobytes() and k.tobytes() == gk.tobytes() and L.tobytes() == gL.tobytes() and fc == gc
    assert bc == B.ZERO_BURST and not S.any() and not G.any()
    both(ev, R.W, R.H, B.OFF, 0, R.REFRACTORY_NS, R.SUPPORT_NS, mask)
    # b == NULL, and no state arrays at all
    so, f = lib.load(), abi.event_filter_struct(R.REFRACTORY_NS, R.SUPPORT_NS, mask, R.W, R.H)
    L2, v2 = np.zeros((R.H, R.W), np.uint64), np.zeros(len(ev), np.uint8)
    assert so.esvo_event_burst_filter_host(None, ctypes.addressof(f[0]), R.W, R.H, None, None, L2.ctypes.data, rec.ctypes.data, len(ev), v2.ctypes.data,
                                           None, 0, None, None, None) == 0
    assert v2.tobytes() == gv.tobytes() and L2.tobytes() == gL.tobytes()


def test_refusals_and_a_failed_call_leaves_the_state():
    ev = R.records(chain([10, 10, 5000, 10]))
    for kw in (dict(mode=4, burst_ns=NS), dict(mode=B.TRAIL, burst_ns=0), dict(mode=B.TRAIL, burst_ns=NS, reserved=(0, 1, 0)), dict(mode=B.OFF, burst_ns=0, reserved=(1, 0, 0))):
        with pytest.raises(lib.EsvoError) as e:
            lib.event_burst_filter_host(ev, 16, 12, **kw)
        assert e.value.code == abi.ERR_INVALID_ARG, kw
    so = lib.load()
    b, f = abi.event_burst_struct(B.TRAIL, NS), abi.EventFilterStruct()
    S, G, L = np.zeros((12, 16), np.uint64), np.zeros((12, 16), np.uint8), np.zeros((12, 16), np.uint64)
    S[5, 5], G[5, 5], L[5, 5] = 7, 3, 9
    keep = S.copy(), G.copy(), L.copy()
    out, n_out = np.zeros(2, abi.EVENT_DTYPE), ctypes.c_size_t(9)
    args = lambda s, g: (ctypes.addressof(b), ctypes.addressof(f), 16, 12, s, g, L.ctypes.data, ev.ctypes.data, len(ev), None)  # noqa: E731
    # the stage on needs both state arrays
    assert so.esvo_event_burst_filter_host(*args(None, G.ctypes.data), None, 0, None, None, None) == abi.ERR_INVALID_ARG
    assert so.esvo_event_burst_filter_host(*args(S.ctypes.data, None), None, 0, None, None, None) == abi.ERR_INVALID_ARG
    # TRAIL keeps #1 and #4: more than cap = 1, and all three images stay
    assert so.esvo_event_burst_filter_host(*args(S.ctypes.data, G.ctypes.data), out.ctypes.data, 1, ctypes.byref(n_out), None, None) == abi.ERR_CAPACITY
    assert all(np.array_equal(a, k) for a, k in zip((S, G, L), keep))
    # counts are added to
    bc, fc = abi.EventBurstCounts(), abi.EventFilterCounts()
    bc.dropped, fc.kept = 10, 100
    assert so.esvo_event_burst_filter_host(*args(S.ctypes.data, G.ctypes.data), out.ctypes.data, 2, ctypes.byref(n_out), ctypes.addressof(bc), ctypes.addressof(fc)) == 0
    assert n_out.value == 2 and bc.as_dict() == {"judged": 5, "passed": 2, "dropped": 13} and fc.kept == 102 and fc.events_in == 2
    assert S[5, 5] == T0 + 5030 and G[5, 5] == 3 and L[5, 5] == T0 + 5020


@pytest.mark.parametrize("seed", SEEDS)
def test_bursty_stream_and_its_floors(seed):
    ev, mask = B.bursty_stream(seed)
    assert 5000 <= len(ev) <= 5600 and sum(a[2] == b[2] for a, b in zip(ev, ev[1:])) >= 800
    so, rec = lib.load(), R.records(ev)
    f, _keep = abi.event_filter_struct(B.REFRACTORY_NS, B.SUPPORT_NS, mask, B.W, B.H)
    for mode in B.MODES:
        v, S, G, L, bc, fc = both(ev, B.W, B.H, mode, B.BURST_NS, B.REFRACTORY_NS, B.SUPPORT_NS, mask)
        share = B.shares(v)
        print(seed, mode, [round(100 * s, 1) for s in share])
        # every class holds at least 3 % of the packet; STC_CUT keeps one event per burst, which rarely falls into a refractory period
        floor = [s for k, s in enumerate(share) if not (mode == B.STC_CUT_TRAIL and k == B.REFRACTORY)]
        assert min(floor) >= 0.03, (mode, share)
        b = abi.event_burst_struct(mode, B.BURST_NS)
        for cut in (1, 7, 64, 1000):                    # the same stream in packets, the three images carried
            cS, cG, cL = np.zeros((B.H, B.W), np.uint64), np.zeros((B.H, B.W), np.uint8), np.zeros((B.H, B.W), np.uint64)
            got, cb = np.zeros(len(ev), np.uint8), abi.EventBurstCounts()
            for a in range(0, len(ev), cut):
                m = min(cut, len(ev) - a)
                assert so.esvo_event_burst_filter_host(ctypes.addressof(b), ctypes.addressof(f), B.W, B.H, cS.ctypes.data, cG.ctypes.data, cL.ctypes.data,
                                                       rec[a:].ctypes.data, m, got[a:].ctypes.data, None, 0, None, ctypes.addressof(cb), None) == 0
            assert got.tolist() == v and cb.as_dict() == bc
            assert cS.tobytes() == B.stamp_array(S).tobytes() and cG.tobytes() == B.flags_array(G).tobytes() and cL.tobytes() == R.last_array(L).tobytes()
