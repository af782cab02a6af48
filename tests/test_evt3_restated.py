"""The host EVT 3.0 decoder (esvo_evt3_to_events, include/esvo_hip.h) against the Python-int restatement of tests/evt3_restated.py:
record for record, state for state, count for count, at the words where the state machine switches.  esvo_evt3_raw_header on
small headers.  No GPU."""
import ctypes

import numpy as np
import pytest

from esvo_amd import abi, calib, lib, synth

import evt3_restated as R

TH, TL, AY, AX, VB, V12, V8, EXT = (R.TIME_HIGH << 12, R.TIME_LOW << 12, R.ADDR_Y << 12, R.ADDR_X << 12, R.VECT_BASE_X << 12, R.VECT_12 << 12,
                                     R.VECT_8 << 12, R.EXT_TRIGGER << 12)


def c_state(s):
    st = abi.Evt3State()
    st.flags, st.y, st.base_x, st.time_high, st.time_low, st.loops = R.state_tuple(s)
    return st


def both(words, state=None, t_offset_us=0):
    """the restatement's (events, state, counts) of the words; the C decoder is asserted equal to it, in record and in count-only mode"""
    words = np.asarray(words, np.uint16)
    want, s1, c1 = R.decode(words.tolist(), state, t_offset_us)
    st0 = c_state(state) if state is not None else None
    got, st, cnt = abi.evt3_to_events(words, st0, t_offset_us)
    assert got.tobytes() == R.records(want).tobytes()
    assert st.as_tuple() == R.state_tuple(s1) and st.reserved == 0
    assert cnt == c1
    none, st_c, cnt_c = abi.evt3_to_events(words, st0, t_offset_us, count_only=True)
    assert none is None and st_c.as_tuple() == st.as_tuple() and cnt_c == c1
    return want, s1, c1


def soup(rng, n):
    """words of every type, the reserved ones included, with enough state-setting words that events flow"""
    types = rng.choice(np.arange(16), n, p=np.array([3, 1, 6, 3, 4, 3, 3, 1, 2, 1, 1, 1, 1, 1, 1, 1]) / 33.0)
    return ((types << 12) | rng.integers(0, 4096, n)).astype(np.uint16)


@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 500, 2048, 5000])
def test_word_soups(n):
    rng = np.random.default_rng(n)
    for _ in range(4):
        w = soup(rng, n)
        both(w)
        both(w, R.loops_state(int(rng.integers(0, 2 ** 40))))


def _synth_events():
    rig = calib.dataset_rig("upenn")
    st = synth.make_stream(rig, 400, 0.02, 0.16, 1.0, seed=7)
    ev = st.ev_left[:6000]
    t_us = (abi.event_ns(ev) // np.uint64(1000)).astype(np.int64)
    return ev, t_us


@pytest.mark.parametrize("vect", [False, True])
def test_decode_of_encode_is_identity(vect):
    ev, t_us = _synth_events()
    base = int(t_us[0]) - 5
    # sorted by (t, y, polarity, x) inside a microsecond, so that the greedy encoder finds runs
    order = np.lexsort((ev["x"], ev["polarity"], ev["y"], t_us))
    E = [(int(ev["x"][i]), int(ev["y"][i]), int(t_us[i]) - base, int(ev["polarity"][i] != 0)) for i in order]
    # synthetic edges fire one pixel at a time: every tenth event gets neighbours in its row at the same microsecond (runs of 2..4)
    E = sorted(set(E + [(x + d, y, t, p) for k, (x, y, t, p) in enumerate(E) if k % 10 == 0 for d in (1, 3, 7, 11)[:1 + k // 10 % 4]]),
               key=lambda e: (e[2], e[1], e[3], e[0]))
    words = R.encode(E, vect=vect)
    want, s1, c1 = both(words, None, base)
    assert [(x, y, stamp // 1000 - base, p) for x, y, stamp, p in want] == E
    assert c1["dropped_events"] == 0 and c1["ignored_words"] == 0
    if vect:
        assert len(words) < len(R.encode(E, vect=False))
    # ... and from a stream that stands far beyond the first loop (the encoder steps TIME_HIGH by at most 1024 across the gap)
    far = 5 * 2 ** 24 + 4090 * 4096
    E2 = [(x, y, t + far + 3 * 2 ** 24, p) for x, y, t, p in E[:500]]
    words = R.encode(E2, vect=vect, start_t_us=far)
    want, s1, c1 = both(words, R.loops_state(far), 0)
    assert [(x, y, stamp // 1000, p) for x, y, stamp, p in want] == E2
    assert c1["time_loops"] == (E2[-1][2] >> 24) - (far >> 24) >= 3


def test_time_high_threshold():
    for step, loops in ((-2047, 0), (-2048, 1), (-4095, 1), (-1, 0), (0, 0), (5, 0)):
        first = 4095 if step < 0 else 10
        w = [TH | first, AY | 3, AX | 7, TH | (first + step), AX | 8]
        want, s, c = both(w)
        assert c["time_loops"] == loops and s["loops"] == loops and len(want) == 2
        assert want[1][2] == (loops << 24 | (first + step) << 12) * 1000
    # the first TIME_HIGH of a stream never loops; one carried in the state does
    assert both([TH | 0])[2]["time_loops"] == 0
    assert both([TH | 0], R.loops_state(4000 << 12))[2]["time_loops"] == 1
    s = R.loops_state(4000 << 12)
    s["have_th"] = 0
    assert both([TH | 0], s)[2]["time_loops"] == 0


def test_time_low_wrap_with_and_without_time_high():
    w = [TH | 5, AY | 1, TL | 0xFFF, AX | 1, TL | 0, AX | 2]           # no TIME_HIGH between: time steps BACK by 4095 us
    want, _, _ = both(w)
    assert [e[2] for e in want] == [(5 << 12 | 0xFFF) * 1000, (5 << 12) * 1000]
    w = [TH | 5, AY | 1, TL | 0xFFF, AX | 1, TH | 6, AX | 2, TL | 0, AX | 3]   # TIME_LOW is kept across the TIME_HIGH
    want, _, _ = both(w)
    assert [e[2] for e in want] == [(5 << 12 | 0xFFF) * 1000, (6 << 12 | 0xFFF) * 1000, (6 << 12) * 1000]


@pytest.mark.parametrize("mask", [0, 1, 0x800, 0xFFF, 0x80, 0xFF, 0x555])
def test_vector_masks(mask):
    w = [TH | 1, AY | 9, VB | 0x800 | 100, V12 | mask, V8 | (mask & 0xFF), V12 | mask]
    want, s, c = both(w)
    bits12, bits8 = [i for i in range(12) if mask >> i & 1], [i for i in range(8) if mask >> i & 1]
    assert [e[0] for e in want] == [100 + i for i in bits12] + [112 + i for i in bits8] + [120 + i for i in bits12]
    assert all(e[3] == 1 and e[1] == 9 for e in want) and s["base_x"] == 132


def test_base_x_wraps_past_0xffff():
    s = R.loops_state(0)
    s.update(have_y=1, have_base=1, base_x=0xFFF0, y=2)
    want, s1, _ = both([V12 | 0xFFF, V12 | 0xFFF, V8 | 0xFF], s)
    assert [e[0] for e in want] == [(0xFFF0 + i) & 0xFFFF for i in range(32)] and s1["base_x"] == 0x10
    # from a stream alone: VECT_12 words walk base_x from 2047 past 0xFFFF
    w = [TH | 1, AY | 1, VB | 2047] + [V12 | 0] * 5290 + [V12 | 0x801] * 4
    want, s1, _ = both(w)
    assert [e[0] for e in want] == [(2047 + 12 * (5290 + k) + i) & 0xFFFF for k in range(4) for i in (0, 11)]
    assert any(e[0] < 100 for e in want) and any(e[0] > 0xFF00 for e in want)


def test_events_before_the_state_is_complete_are_dropped_and_counted():
    w = [AX | 1, V12 | 0x7, V8 | 0x3,                       # nothing known: 1 + 3 + 2 dropped, base_x advances 20
         TH | 2, AX | 2, V12 | 0x1,                         # no y: 1 + 1
         AY | 4, AX | 3, V8 | 0xFF,                         # x emits; no base: 8 dropped, base_x 40
         VB | 7, V12 | 0x3, EXT | 5, 0x1000, 0xF123]
    want, s, c = both(w)
    assert [e[0] for e in want] == [3, 7, 8] and c["dropped_events"] == 16 and c["ext_triggers"] == 1 and c["ignored_words"] == 2
    # base_x advances while dropping: the carried base is 0 + 12 + 8 + 12 + 8 = 40 before VECT_BASE_X replaces it
    _, s_mid, _ = both(w[:9])
    assert s_mid["base_x"] == 40 and s_mid["have_base"] == 0
    want, _, _ = both([VB | 0] + [V8 | 0] * 3 + [V8 | 1], s_mid)
    assert [e[0] for e in want] == [24]


def test_cut_at_every_word_boundary():
    rng = np.random.default_rng(3)
    w = np.concatenate([np.array([TH | 4000, AY | 5, VB | 40], np.uint16), soup(rng, 300)])
    whole, s_whole, c_whole = both(w)
    for k in range(len(w) + 1):
        a, s_a, c_a = R.decode(w[:k].tolist())
        got_a, st_a, cnt_a = abi.evt3_to_events(w[:k])
        got_b, st_b, cnt_b = abi.evt3_to_events(w[k:], st_a)
        assert got_a.tobytes() + got_b.tobytes() == R.records(whole).tobytes(), k
        assert st_a.as_tuple() == R.state_tuple(s_a) and st_b.as_tuple() == R.state_tuple(s_whole), k
        assert {key: cnt_a[key] + cnt_b[key] for key in cnt_a} == c_whole, k


def test_cap_too_small_fails_and_leaves_the_state():
    w = np.array([TH | 1, AY | 2, AX | 3, VB | 9, V12 | 0xFFF, TH | 7], np.uint16)
    so = lib.load()
    for cap in (0, 1, 12):
        st, n_out, out = abi.Evt3State(), ctypes.c_size_t(99), np.zeros(16, abi.EVENT_DTYPE)
        st.loops = 77
        rc = so.esvo_evt3_to_events(ctypes.byref(st), w.ctypes.data, w.size, 0, out.ctypes.data, cap, ctypes.byref(n_out), None)
        assert rc == abi.ERR_CAPACITY and st.as_tuple() == (0, 0, 0, 0, 0, 77)
        with pytest.raises(lib.EsvoError) as e:
            abi.evt3_to_events(w, cap=cap)
        assert e.value.code == abi.ERR_CAPACITY
    got, st, cnt = abi.evt3_to_events(w, cap=13)
    assert len(got) == 13 and st.time_high == 7


def test_bad_stamp_names_the_event():
    w = [TH | 0, AY | 1, TL | 5, AX | 1, AX | 2, TL | 9, VB | 3, V12 | 0x5, TL | 10, AX | 4]
    # t_us: 5, 5, 9, 9, 10 -- an offset of -5 keeps every stamp at or above 0, -6 makes event 0 the first bad one
    for off, bad in ((-5, None), (-6, 0), (-10, 0), (0, None)):
        if bad is None:
            both(w, None, off)
            continue
        with pytest.raises(R.BadStamp) as want:
            R.decode(w, None, off)
        assert want.value.first_bad == bad
        with pytest.raises(abi.Evt3Error) as e:
            abi.evt3_to_events(np.array(w, np.uint16), None, off)
        assert e.value.first_bad == bad
    # a stream whose time FALLS below the offset later: events 0..1 are fine, event 2 is the first bad one
    w = [TH | 1, AY | 1, TL | 5, AX | 1, AX | 2, TH | 0, AX | 3, V12 | 1]
    off = -(1 << 12)
    with pytest.raises(R.BadStamp) as want:
        R.decode(w, None, off)
    assert want.value.first_bad == 2
    st = abi.Evt3State()
    n_out = ctypes.c_size_t(0)
    words = np.array(w, np.uint16)
    rc = lib.load().esvo_evt3_to_events(ctypes.byref(st), words.ctypes.data, words.size, off, None, 0, ctypes.byref(n_out), None)
    assert rc == abi.ERR_INVALID_ARG and n_out.value == 2 and st.as_tuple() == (0, 0, 0, 0, 0, 0)
    assert "event 2 " in lib.load().esvo_last_error(None).decode()
    # the upper end: 2^32 * 10^9 ns is the first stamp that does not fit
    top = R.STAMP_END // 1000
    both([TH | 0, AY | 0, AX | 0], None, top - 1)
    with pytest.raises(abi.Evt3Error):
        abi.evt3_to_events(np.array([TH | 0, AY | 0, AX | 0], np.uint16), None, top)


def test_sizes_and_arguments():
    assert lib.evt3_sizes() == [ctypes.sizeof(abi.Evt3State), ctypes.sizeof(abi.Evt3Counts), 0, 0] == [20, 48, 0, 0]
    so, st = lib.load(), abi.Evt3State()
    assert so.esvo_evt3_to_events(None, None, 0, 0, None, 0, None, None) == abi.ERR_INVALID_ARG
    assert so.esvo_evt3_to_events(ctypes.byref(st), None, 3, 0, None, 0, None, None) == abi.ERR_INVALID_ARG
    assert so.esvo_evt3_to_events(ctypes.byref(st), None, 0, 0, None, 0, None, None) == 0
    got, st1, cnt = abi.evt3_to_events(b"")
    assert len(got) == 0 and cnt["words"] == 0
    got, _, _ = abi.evt3_to_events(np.array([TH | 1, AY | 2, AX | 3], "<u2").tobytes())
    assert len(got) == 1 and got[0]["x"] == 3 and got[0]["y"] == 2
    with pytest.raises(ValueError):
        abi.evt3_to_events(b"\x00\x00\x00")


def test_raw_header():
    words = np.array([TH | 1, AY | 2, AX | 3], "<u2").tobytes()
    head = b"% camera_integrator_name Prophesee\n% date 2024-01-01 10:00:00\n% evt 3.0\n% format EVT3;height=720;width=1280\n% geometry 1280x720\n"
    assert abi.evt3_raw_header(head + b"% end\n" + words) == (len(head) + 6, 1280, 720)
    assert abi.evt3_raw_header(head + words) == (len(head), 1280, 720)            # ended by the first line that has no '%'
    assert abi.evt3_raw_header(b"% evt 3.0\r\n% end\r\n" + words) == (18, 0, 0)
    assert abi.evt3_raw_header(b"% format EVT3;height=480;width=640\n" + words) == (35, 640, 480)
    assert abi.evt3_raw_header(b"% geometry 640x480\n% end\n% not a header any more\n")[0] == 25
    assert abi.evt3_raw_header(words) == (0, 0, 0)                                 # words only (TIME_HIGH 1 is not '%')
    assert abi.evt3_raw_header(b"") == (0, 0, 0)
    for bad in (b"% evt 2.0\n", b"% evt 2.1\n% end\n", b"% format EVT2;height=480;width=640\n", b"% format EVT21\n"):
        with pytest.raises(lib.EsvoError) as e:
            abi.evt3_raw_header(bad + words)
        assert e.value.code == -5
    off, w, h = abi.evt3_raw_header(head + b"% end\n" + words)
    got, _, _ = abi.evt3_to_events((head + b"% end\n" + words)[off:])
    assert len(got) == 1
