"""The column conversion of esvo_ts_push_event_columns on the host (include/esvo_hip.h): esvo_event_columns_to_events (C) and
abi.columns_to_events (numpy) against the Python-int restatement of tests/columns_restated.py, byte for byte, at the values where
an integer conversion can go wrong.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

from esvo_amd import abi, lib

import columns_restated as R

END = R.STAMP_END
I64_MIN, I64_MAX, U32_MAX = -2 ** 63, 2 ** 63 - 1, 2 ** 32 - 1


def convert_all(x, y, t, p, t_type, p_type, t_offset):
    """the three conversions of one packet -> the restatement's (records, first_bad); the C and numpy ones are asserted equal to it"""
    x, y = np.asarray(x, np.uint16), np.asarray(y, np.uint16)
    t = np.asarray(t, R.T_DTYPE[t_type])
    p = None if p is None else np.asarray(p, np.uint8).view(R.P_DTYPE[p_type])
    want, bad = R.columns_to_events(x, y, t, None if p is None else p.view(np.uint8), t_type, p_type, t_offset)
    unit = R.T_UNIT[t_type]
    # the C entry: the records before the first invalid element are written, *first_bad names it
    s, (n, _keep) = lib.event_columns_struct(x, y, t, p, unit, t_offset)
    out, fb = np.zeros(n, abi.EVENT_DTYPE), ctypes.c_size_t(12345)
    rc = lib.load().esvo_event_columns_to_events(ctypes.addressof(s), n, out.ctypes.data, ctypes.byref(fb))
    if bad is None:
        assert rc == 0 and fb.value == n
        assert out.tobytes() == want.tobytes()
        assert abi.columns_to_events(x, y, t, p, unit, t_offset).tobytes() == want.tobytes()
        assert lib.columns_to_events_c(x, y, t, p, unit, t_offset).tobytes() == want.tobytes()
    else:
        assert rc == abi.ERR_INVALID_ARG and fb.value == bad
        assert str(bad) in lib.load().esvo_last_error(None).decode()
        assert out[:bad].tobytes() == want.tobytes()
        with pytest.raises(abi.ColumnsError) as e:
            abi.columns_to_events(x, y, t, p, unit, t_offset)
        assert e.value.first_bad == bad
        with pytest.raises(abi.ColumnsError) as e:
            lib.columns_to_events_c(x, y, t, p, unit, t_offset)
        assert e.value.first_bad == bad
    return want, bad


def one(t, t_type, t_offset=0):
    """a single element: (valid, stamp) by all three conversions"""
    want, bad = convert_all([7], [9], [t], [1], t_type, abi.P_U8, t_offset)
    if bad is not None:
        return False, None
    return True, int(want["sec"][0]) * 10 ** 9 + int(want["nsec"][0])


def test_struct_size_and_abi_number():
    assert lib.event_columns_sizes() == [ctypes.sizeof(abi.EventColumnsStruct), 0, 0, 0]
    assert ctypes.sizeof(abi.EventColumnsStruct) == 56
    assert lib.abi_sizes()[7] == 8
    assert {"esvo_ts_push_event_columns", "esvo_event_columns_to_events", "esvo_event_columns_sizes"} <= set(lib.SYMBOLS)


@pytest.mark.parametrize("t_type", [abi.T_NS_I64, abi.T_US_I64, abi.T_US_U32])
def test_second_boundaries_zero_and_the_largest_stamp(t_type):
    k = R.UNIT[t_type]
    tmax = U32_MAX if t_type == abi.T_US_U32 else I64_MAX
    # a second boundary: ...999 999 999 ns and the stamp after it; with microseconds ...999 999 us and + 1
    b = 5 * 10 ** 9 // k
    for t, want in ((b - 1, (b - 1) * k), (b, b * k), (0, 0), (1, k)):
        assert one(t, t_type) == (True, want)
    ok, s = one(b - 1, t_type)
    assert (s // 10 ** 9, s % 10 ** 9) == ((4, 999_999_999) if k == 1 else (4, 999_999_000))
    # the largest valid stamp and the one above it (a u32 of microseconds cannot reach it: its own maximum is valid)
    last = (END - 1) // k
    if last <= tmax:
        assert one(last, t_type) == (True, last * k)
        assert one(last + 1, t_type) == (False, None)
    else:
        assert one(tmax, t_type) == (True, tmax * k)
    # ... reached through the offset as well
    assert one(min(tmax, 1000), t_type, last - min(tmax, 1000)) == (True, last * k)
    assert one(min(tmax, 1000), t_type, last - min(tmax, 1000) + 1) == (False, None)


@pytest.mark.parametrize("t_type", [abi.T_NS_I64, abi.T_US_I64, abi.T_US_U32])
def test_offsets_bring_a_value_to_zero_and_below(t_type):
    k = R.UNIT[t_type]
    assert one(123456, t_type, -123456) == (True, 0)
    assert one(123456, t_type, -123457) == (False, None)
    assert one(123456, t_type, -123455) == (True, k)
    assert one(0, t_type, 55) == (True, 55 * k)
    assert one(0, t_type, -1) == (False, None)
    if t_type != abi.T_US_U32:
        assert one(-55, t_type, 55) == (True, 0)
        assert one(-56, t_type, 55) == (False, None)
        assert one(-1, t_type, 0) == (False, None)


@pytest.mark.parametrize("t_type", [abi.T_NS_I64, abi.T_US_I64, abi.T_US_U32])
def test_extremes_whose_sum_or_scaling_overflows(t_type):
    k = R.UNIT[t_type]
    tmax = U32_MAX if t_type == abi.T_US_U32 else I64_MAX
    tmin = 0 if t_type == abi.T_US_U32 else I64_MIN
    # the sum leaves int64 (a wrapped sum would be a small number)
    assert one(tmax, t_type, I64_MAX) == (False, None)
    assert one(max(tmax, 1), t_type, I64_MAX - max(tmax, 1) + 1) == (False, None)
    assert one(tmin, t_type, I64_MIN) == (False, None)
    # the sum fits, its scaled value does not fit u64 / int64 (a wrapped product could land inside the valid range)
    assert one(0, t_type, I64_MAX) == (False, None)
    for wrap in (2 ** 64, 2 ** 63):
        s = -(-wrap // k)  # the smallest sum whose product reaches the wrap
        if s <= I64_MAX:
            assert one(0, t_type, s) == (False, None)
            assert one(min(tmax, 3), t_type, s) == (False, None)
    # extremes that cancel: a valid stamp
    if t_type != abi.T_US_U32:
        assert one(I64_MIN, t_type, I64_MAX) == (False, None)       # -1
        assert one(I64_MAX, t_type, -I64_MAX) == (True, 0)
        assert one(I64_MAX, t_type, I64_MIN) == (False, None)       # -1
        assert one(I64_MIN + 1, t_type, I64_MAX) == (True, 0)
    else:
        assert one(U32_MAX, t_type, -U32_MAX) == (True, 0)
        assert one(U32_MAX, t_type, 0) == (True, U32_MAX * 1000)
        assert one(U32_MAX, t_type, I64_MIN) == (False, None)


@pytest.mark.parametrize("p_type", [abi.P_U8, abi.P_I8])
def test_polarity_rules_and_coordinates(p_type):
    pv = [0, 1, 2, 128, 255]
    cv = [0, 345, 346, 32767, 32768, 65535]
    combos = list(itertools.product(cv, cv, pv))
    x, y, p = (np.array([c[k] for c in combos]) for k in range(3))
    t = np.arange(len(combos)) * 999_999_937 + 3
    want, bad = convert_all(x, y, t, p, abi.T_NS_I64, p_type, 0)
    assert bad is None
    assert np.array_equal(want["x"], x) and np.array_equal(want["y"], y)
    on = {abi.P_U8: {1, 2, 128, 255}, abi.P_I8: {1, 2}}[p_type]
    assert np.array_equal(want["polarity"], np.array([1 if v in on else 0 for v in p], np.uint8))
    assert not want["_pad"].any()
    # no p column: every event ON, what abi.make_events does
    want, bad = convert_all(x, y, t, None, abi.T_NS_I64, p_type, 0)
    assert bad is None and (want["polarity"] == 1).all()
    assert want.tobytes() == abi.make_events(x, y, t).tobytes()
    # int16 coordinates: their bits are copied
    ev = abi.columns_to_events(x.astype(np.uint16).view(np.int16), y.astype(np.uint16).view(np.int16), t.astype(np.int64))
    assert ev.tobytes() == want.tobytes()
    assert lib.columns_to_events_c(x.astype(np.uint16).view(np.int16), y.astype(np.uint16).view(np.int16), t.astype(np.int64)).tobytes() == want.tobytes()


def test_equals_make_events_where_it_applies():
    rng = np.random.default_rng(20251020)
    n = 4096
    x, y = rng.integers(0, 65536, n), rng.integers(0, 65536, n)
    t_ns = np.sort(rng.integers(0, END, n, dtype=np.int64))
    pol = rng.integers(0, 2, n).astype(np.uint8)
    ref = abi.make_events(x, y, t_ns, pol)
    want, bad = convert_all(x, y, t_ns, pol, abi.T_NS_I64, abi.P_U8, 0)
    assert bad is None and want.tobytes() == ref.tobytes()
    # the +-1 convention, microseconds with an offset (DSEC: u32 + t_offset)
    t_us = np.sort(rng.integers(0, 2 ** 32, n, dtype=np.int64))
    off = 1_600_000_000_000_000
    ref = abi.make_events(x, y, (t_us + off) * 1000, pol)
    for t_type in (abi.T_US_I64, abi.T_US_U32):
        want, bad = convert_all(x, y, t_us, np.where(pol, 1, 255), t_type, abi.P_I8, off)
        assert bad is None and want.tobytes() == ref.tobytes()


def test_first_bad_is_the_first():
    t = np.array([5, 6, -1, 7, -2, 8], np.int64)
    for lo in range(6):
        want, bad = convert_all(np.arange(6 - lo), np.arange(6 - lo), t[lo:], None, abi.T_NS_I64, abi.P_U8, 0)
        assert bad == ([2 - lo, 4 - lo][lo > 2] if lo <= 4 else None)
    # an empty packet converts to nothing
    want, bad = convert_all([], [], [], None, abi.T_US_U32, abi.P_U8, -5)
    assert bad is None and len(want) == 0


def test_unknown_types_and_device_memory_are_refused():
    so = lib.load()
    x = np.zeros(4, np.uint16)
    t = np.zeros(4, np.int64)
    out = np.zeros(4, abi.EVENT_DTYPE)
    for field, value in (("t_type", 3), ("t_type", -1), ("p_type", 2), ("memory", 2), ("memory", abi.MEM_DEVICE)):
        s, _ = lib.event_columns_struct(x, x, t)
        setattr(s, field, value)
        fb = ctypes.c_size_t(99)
        assert so.esvo_event_columns_to_events(ctypes.addressof(s), 4, out.ctypes.data, ctypes.byref(fb)) == abi.ERR_INVALID_ARG
        assert fb.value == 4   # no element is bad: the arguments are
    # the bindings refuse what the C-ABI has no type for
    for bad_t, unit in ((np.zeros(4, np.uint32), "ns"), (np.zeros(4, np.float64), "ns"), (np.zeros(4, np.int32), "us"), (t, "s")):
        with pytest.raises(ValueError, match="t must be"):
            lib.event_columns_struct(x, x, bad_t, unit=unit)
        with pytest.raises(ValueError, match="t must be"):
            abi.columns_to_events(x, x, bad_t, unit=unit)
    with pytest.raises(ValueError, match="p must be"):
        lib.event_columns_struct(x, x, t, np.zeros(4, np.int16))
    with pytest.raises(ValueError, match="uint16 or int16"):
        lib.event_columns_struct(x.astype(np.int32), x, t)
    with pytest.raises(ValueError, match="differ in length"):
        lib.event_columns_struct(x[:3], x, t)
    with pytest.raises(ValueError, match="fit int64"):
        lib.event_columns_struct(x, x, t, t_offset=2 ** 63)
