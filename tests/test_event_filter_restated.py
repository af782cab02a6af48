"""esvo_event_filter_host (include/esvo_hip.h) against the Python-int restatement of the rule (tests/event_filter_restated.py):
verdict for verdict, `last` byte for byte, count for count.  Host only."""
import ctypes

import numpy as np
import pytest

import event_filter_restated as R
from esvo_amd import abi, lib

T0 = R.T_BASE
SEEDS = (11, 12, 13)


def both(events, W, H, refractory_ns, support_ns, mask=None, last=None):
    """the rule by the restatement and by the library, compared; -> the restatement's (verdicts, last, counts)"""
    v, L, c = R.run(events, W, H, refractory_ns, support_ns, mask, last)
    gv, gk, gL, gc = lib.event_filter_host(R.records(events), W, H, refractory_ns, support_ns, mask, None if last is None else R.last_array(last))
    assert gv.tolist() == v
    assert gL.tobytes() == R.last_array(L).tobytes()
    assert gc == c and c["events_in"] == sum(c[k] for k in R.NAMES)
    assert gk.tobytes() == R.records(R.kept(events, v)).tobytes()
    return v, L, c


def test_sizes_and_bindings():
    assert lib.event_filter_sizes() == [ctypes.sizeof(abi.EventFilterStruct), ctypes.sizeof(abi.EventFilterCounts), 0, 0] == [40, 48, 0, 0]
    assert lib.abi_sizes()[7] == 8   # additive: the ABI number stays
    assert (abi.FILTER_KEPT, abi.FILTER_OUTSIDE, abi.FILTER_MASKED, abi.FILTER_REFRACTORY, abi.FILTER_UNSUPPORTED) == (
        R.KEPT, R.OUTSIDE, R.MASKED, R.REFRACTORY, R.UNSUPPORTED)
    assert {"esvo_ts_filter_configure", "esvo_ts_filter_stats", "esvo_ts_filter_state", "esvo_event_filter_host", "esvo_event_filter_sizes"} <= set(lib.SYMBOLS)


def test_refractory_boundary_is_strict():
    ref = 1000
    for gap, want in ((ref - 1, R.REFRACTORY), (ref, R.KEPT)):
        v, L, _ = both([(5, 5, T0, 1), (5, 5, T0 + gap, 0)], 16, 12, ref, 0)
        assert v == [R.KEPT, want]
        assert L[5][5] == (T0 + gap if want == R.KEPT else T0)   # a dropped event does not restart the period


def test_support_boundary_is_inclusive():
    sup = 700
    for gap, want in ((sup, R.KEPT), (sup + 1, R.UNSUPPORTED)):
        v, L, _ = both([(5, 5, T0, 1), (6, 6, T0 + gap, 0)], 16, 12, 0, sup)
        assert v == [R.UNSUPPORTED, want]
        assert L[6][6] == T0 + gap                               # an unsupported event updates `last` all the same


def test_equal_stamp_neighbour_supports_only_when_earlier():
    v, _, _ = both([(4, 4, T0, 1), (5, 4, T0, 1)], 16, 12, 0, 10)
    assert v == [R.UNSUPPORTED, R.KEPT]


def test_pixel_never_supports_itself():
    v, _, _ = both([(4, 4, T0, 1), (4, 4, T0 + 1, 1), (4, 4, T0 + 2, 1)], 16, 12, 0, 10)
    assert v == [R.UNSUPPORTED] * 3


def test_unsupported_event_supports_and_restarts_the_period():
    v, _, _ = both([(4, 4, T0, 1), (4, 4, T0 + 5, 1), (5, 5, T0 + 6, 0)], 16, 12, 10, 10)
    assert v == [R.UNSUPPORTED, R.REFRACTORY, R.KEPT]


def test_corners_and_an_edge():
    W, H = 16, 12
    for (x, y), (nx, ny) in (((0, 0), (1, 1)), ((W - 1, 0), (W - 2, 1)), ((0, H - 1), (1, H - 2)), ((W - 1, H - 1), (W - 2, H - 2)), ((7, 0), (8, 0))):
        v, _, _ = both([(nx, ny, T0, 1), (x, y, T0 + 3, 1), (x, y, T0 + 100, 1)], W, H, 0, 10)
        assert v == [R.UNSUPPORTED, R.KEPT, R.UNSUPPORTED]


def test_masked_neighbour_does_not_support():
    mask = [[0] * 16 for _ in range(12)]
    mask[4][4] = 7
    v, L, _ = both([(4, 4, T0, 1), (5, 4, T0 + 1, 1)], 16, 12, 0, 10, mask)
    assert v == [R.MASKED, R.UNSUPPORTED] and L[4][4] == 0


def test_refractory_dropped_neighbour_does_not_support():
    # (4,4) fires at T0 and, dropped, at T0 + 50: at T0 + 55 its `last` is still T0, 55 > support away
    v, _, _ = both([(4, 4, T0, 1), (4, 4, T0 + 50, 1), (5, 4, T0 + 55, 1)], 16, 12, 100, 10)
    assert v == [R.UNSUPPORTED, R.REFRACTORY, R.UNSUPPORTED]


def test_coordinates_at_width_and_height_are_outside():
    W, H = 16, 12
    v, L, c = both([(W, 3, T0, 1), (3, H, T0, 1), (W - 1, H - 1, T0, 1), (65535, 65535, T0, 0)], W, H, 5, 5)
    assert v == [R.OUTSIDE, R.OUTSIDE, R.UNSUPPORTED, R.OUTSIDE] and c["outside"] == 3


@pytest.mark.parametrize("with_mask", (False, True))
def test_both_periods_zero(with_mask):
    ev, mask = R.random_stream(5, 400)
    v, _, c = both(ev, R.W, R.H, 0, 0, mask if with_mask else None)
    assert c["refractory"] == c["unsupported"] == 0 and (c["masked"] > 0) == with_mask and c["kept"] > 0


def test_resumed_last_and_a_state_ahead_of_the_stream():
    last = R.fresh_last(16, 12)
    last[3][3] = T0 - 5          # supports (4, 4) at T0
    last[8][8] = T0 - 5          # (8, 8) is still refractory at T0
    last[2][10] = T0 + 50        # planted ahead of the stream: the differences are negative
    v, L, _ = both([(4, 4, T0, 1), (8, 8, T0, 1), (10, 2, T0, 1), (10, 3, T0 + 1, 1)], 16, 12, 10, 10, None, last)
    assert v == [R.KEPT, R.REFRACTORY, R.REFRACTORY, R.KEPT]
    assert L[2][10] == T0 + 50


def test_cap_too_small_and_null_arguments():
    ev = R.records([(1, 1, T0, 1), (2, 2, T0 + 1, 1), (3, 3, T0 + 2, 1)])
    with pytest.raises(lib.EsvoError) as e:
        lib.event_filter_host(ev, 16, 12, cap=2)
    assert e.value.code == abi.ERR_CAPACITY
    so = lib.load()
    f = abi.EventFilterStruct()
    L = np.zeros((12, 16), np.uint64)
    keep = L.copy()
    out, n_out = np.zeros(3, abi.EVENT_DTYPE), ctypes.c_size_t(9)
    # more kept than cap: `last` is left as it was
    assert so.esvo_event_filter_host(ctypes.addressof(f), 16, 12, L.ctypes.data, ev.ctypes.data, 3, None, out.ctypes.data, 2, ctypes.byref(n_out), None) == abi.ERR_CAPACITY
    assert np.array_equal(L, keep)
    # out == NULL counts; verdict, n_out and add may be NULL
    assert so.esvo_event_filter_host(ctypes.addressof(f), 16, 12, L.ctypes.data, ev.ctypes.data, 3, None, None, 0, ctypes.byref(n_out), None) == 0
    assert n_out.value == 3 and L[3, 3] == T0 + 2
    assert so.esvo_event_filter_host(ctypes.addressof(f), 16, 12, L.ctypes.data, ev.ctypes.data, 3, None, None, 0, None, None) == 0
    for bad in ((None, 16, 12, L.ctypes.data, ev.ctypes.data), (ctypes.addressof(f), 16, 12, None, ev.ctypes.data),
                (ctypes.addressof(f), 16, 12, L.ctypes.data, None), (ctypes.addressof(f), 0, 12, L.ctypes.data, ev.ctypes.data)):
        assert so.esvo_event_filter_host(*bad, 3, None, None, 0, None, None) == abi.ERR_INVALID_ARG
    f.reserved[2] = 1
    assert so.esvo_event_filter_host(ctypes.addressof(f), 16, 12, L.ctypes.data, ev.ctypes.data, 3, None, None, 0, None, None) == abi.ERR_INVALID_ARG
    # counts are added to
    f.reserved[2] = 0
    add = abi.EventFilterCounts()
    add.kept = 10
    assert so.esvo_event_filter_host(ctypes.addressof(f), 16, 12, L.ctypes.data, ev.ctypes.data, 3, None, None, 0, None, ctypes.addressof(add)) == 0
    assert add.kept == 13 and add.events_in == 3


@pytest.mark.parametrize("seed", SEEDS)
def test_random_stream(seed):
    ev, mask = R.random_stream(seed)
    v, L, c = R.run(ev, R.W, R.H, R.REFRACTORY_NS, R.SUPPORT_NS, mask)
    share = {k: c[k] / len(ev) for k in R.NAMES}
    print(seed, {k: round(100 * s, 1) for k, s in share.items()})
    assert min(share.values()) >= 0.03, share       # each of the five verdicts holds at least 3 % of the events
    both(ev, R.W, R.H, R.REFRACTORY_NS, R.SUPPORT_NS, mask)
    so, rec = lib.load(), R.records(ev)
    f, _keep = abi.event_filter_struct(R.REFRACTORY_NS, R.SUPPORT_NS, mask, R.W, R.H)
    for cut in (1, 7, 64, 1000):                    # the same stream in packets, `last` carried
        carried, got = np.zeros((R.H, R.W), np.uint64), np.zeros(len(ev), np.uint8)
        for a in range(0, len(ev), cut):
            m = min(cut, len(ev) - a)
            assert so.esvo_event_filter_host(ctypes.addressof(f), R.W, R.H, carried.ctypes.data, rec[a:].ctypes.data, m, got[a:].ctypes.data,
                                             None, 0, None, None) == 0
        assert got.tolist() == v and carried.tobytes() == R.last_array(L).tobytes()
