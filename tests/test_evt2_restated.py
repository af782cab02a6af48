"""The host EVT 2.0 / 2.1 decoder (esvo_evt2_to_events, include/esvo_hip.h) against the Python-int restatement of
tests/evt2_restated.py: record for record, state for state, count for count, in record and count-only mode, for the three
formats.  esvo_raw_header on small headers, esvo_evt3_raw_header unchanged on the same bytes.  No GPU."""
import ctypes

import numpy as np
import pytest

from esvo_amd import abi, calib, lib, synth

import evt2_restated as R

F20, F21, F21L = R.FORMATS


def c_state(s):
    st = abi.Evt2State()
    st.flags, st.time_high, st.loops = R.state_tuple(s)
    return st


def both(u32, format, state=None, t_offset_us=0):
    """the restatement's (events, state, counts) of a memory image; the C decoder is asserted equal to it, in record and in
    count-only mode"""
    u32 = np.asarray(u32, np.uint32)
    want, s1, c1 = R.decode(u32.tolist(), format, state, t_offset_us)
    st0 = c_state(state) if state is not None else None
    got, st, cnt = abi.evt2_to_events(u32, format, st0, t_offset_us)
    assert got.tobytes() == R.records(want).tobytes()
    assert st.as_tuple() == R.state_tuple(s1) and st.reserved == 0
    assert cnt == c1
    none, st_c, cnt_c = abi.evt2_to_events(u32, format, st0, t_offset_us, count_only=True)
    assert none is None and st_c.as_tuple() == st.as_tuple() and cnt_c == c1
    return want, s1, c1


def soup(rng, n, format):
    """the memory image of n words of every type nibble, with enough TIME_HIGH words that events flow; TIME_HIGH mostly creeps up
    and sometimes jumps anywhere (loops)"""
    types = rng.choice(np.arange(16), n, p=np.array([8, 8, 1, 1, 1, 1, 1, 1, 4, 1, 2, 1, 1, 1, 1, 1]) / 34.0)
    out, th = [], int(rng.integers(0, 2 ** 28))
    for t in types.tolist():
        if t == R.TIME_HIGH:
            th = int(rng.integers(0, 2 ** 28)) if rng.random() < 0.3 else min(th + int(rng.integers(0, 3)), 2 ** 28 - 1)
            out += R.time_high_word(th, format)
        elif format == F20:
            out.append(t << 28 | int(rng.integers(0, 2 ** 28)))
        else:
            valid = int(rng.choice([0, 1, 0xFFFFFFFF, int(rng.integers(0, 2 ** 32))], p=[0.1, 0.2, 0.1, 0.6]))
            out += R.image([t << 60 | int(rng.integers(0, 2 ** 28)) << 32 | valid], format)
    return np.array(out, np.uint32)


def far_state(t_us):
    s = R.fresh_state()
    s["loops"], s["time_high"], s["have_th"] = t_us >> 34, (t_us >> 6) & 0x0FFFFFFF, 1
    return s


@pytest.mark.parametrize("format", R.FORMATS)
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 500, 2048, 5000])
def test_word_soups(n, format):
    rng = np.random.default_rng(1000 * format + n)
    for _ in range(2):
        w = soup(rng, n, format)
        assert len(w) == (n if format == F20 else 2 * n)
        _, _, c = both(w, format)
        assert c["words"] == n
        both(w, format, far_state(int(rng.integers(0, 2 ** 40))))


@pytest.mark.parametrize("format", R.FORMATS)
def test_decode_of_encode_is_identity(format):
    rig = calib.dataset_rig("upenn")
    st = synth.make_stream(rig, 400, 0.02, 0.16, 1.0, seed=7)
    ev = st.ev_left[:4000]
    t_us = (abi.event_ns(ev) // np.uint64(1000)).astype(np.int64)
    base = int(t_us[0]) - 5
    order = np.lexsort((ev["x"], ev["polarity"], ev["y"], t_us))
    E = [(int(ev["x"][i]), int(ev["y"][i]), int(t_us[i]) - base, int(ev["polarity"][i] != 0)) for i in order]
    # synthetic edges fire one pixel at a time: every tenth event gets neighbours in its row at the same microsecond
    E = sorted(set(E + [(x + d, y, t, p) for k, (x, y, t, p) in enumerate(E) if k % 10 == 0 for d in (1, 3, 31, 32)[:1 + k // 10 % 4]]),
               key=lambda e: (e[2], e[1], e[3], e[0]))
    u32 = R.encode(E, format)
    want, s1, c1 = both(u32, format, None, base)
    assert [(x, y, stamp // 1000 - base, p) for x, y, stamp, p in want] == E
    assert c1["dropped_events"] == 0 and c1["ignored_words"] == 0 and c1["time_loops"] == 0
    if format != F20:
        assert c1["words"] < len(R.encode(E, F20))     # groups: fewer words than events + TIME_HIGH words


@pytest.mark.parametrize("format", R.FORMATS)
def test_time_high_threshold(format):
    def cd(x):
        return [R.cd_word(1, 3, x, 4)] if format == F20 else R.image([R.vector_word(1, 3, x, 4, 1)], format)

    for step, loops in ((-(2 ** 27 - 1), 0), (-2 ** 27, 1), (-(2 ** 28 - 1), 1), (-1, 0), (0, 0), (5, 0)):
        first = 2 ** 28 - 1 if step < 0 else 10
        w = R.time_high_word(first, format) + cd(7) + R.time_high_word(first + step, format) + cd(8)
        want, s, c = both(w, format)
        assert c["time_loops"] == loops and s["loops"] == loops and len(want) == 2
        assert want[1][2] == (loops << 34 | (first + step) << 6 | 3) * 1000
    # the first TIME_HIGH of a stream never loops; one carried in the state does
    assert both(R.time_high_word(0, format), format)[2]["time_loops"] == 0
    assert both(R.time_high_word(0, format), format, far_state((2 ** 28 - 5) << 6))[2]["time_loops"] == 1
    s = far_state((2 ** 28 - 5) << 6)
    s["have_th"] = 0
    assert both(R.time_high_word(0, format), format, s)[2]["time_loops"] == 0


@pytest.mark.parametrize("format", [F21, F21L])
@pytest.mark.parametrize("x0", [0, 31, 2016, 2047])
@pytest.mark.parametrize("valid", [0, 1, 0x80000000, 0xFFFFFFFF, 0x55555555])
def test_validity_masks(valid, x0, format):
    w = R.time_high_word(9, format) + R.image([R.vector_word(0, 5, x0, 77, valid), R.vector_word(1, 6, x0, 78, valid)], format)
    want, s, c = both(w, format)
    bits = [i for i in range(32) if valid >> i & 1]
    assert [e[0] for e in want] == [x0 + i for i in bits] * 2
    assert [e[1:] for e in want] == [(77, (9 << 6 | 5) * 1000, 0)] * len(bits) + [(78, (9 << 6 | 6) * 1000, 1)] * len(bits)
    assert c["events"] == 2 * len(bits) and c["ignored_words"] == 0


@pytest.mark.parametrize("format", R.FORMATS)
def test_events_before_the_first_time_high_are_dropped_and_counted(format):
    if format == F20:
        w = [R.cd_word(1, 0, 1, 1), R.cd_word(0, 0, 2, 2), R.EXT_TRIGGER << 28 | 5, 0xE << 28, 0xF << 28 | 1] + R.time_high_word(3, format) + [R.cd_word(1, 1, 3, 3)]
        dropped = 2
    else:
        W = [R.vector_word(1, 0, 1, 1, 0x7), R.vector_word(0, 0, 2, 2, 0xFFFFFFFF), R.vector_word(0, 0, 2, 2, 0), R.EXT_TRIGGER << 60 | 5, 0xE << 60, 0xF << 60 | 1]
        w = R.image(W, format) + R.time_high_word(3, format) + R.image([R.vector_word(1, 1, 3, 3, 1)], format)
        dropped = 35
    want, s, c = both(w, format)
    assert want == [(3, 3, (3 << 6 | 1) * 1000, 1)]
    assert c["dropped_events"] == dropped and c["ext_triggers"] == 1 and c["ignored_words"] == 2 and c["words"] == (7 if format == F20 else 8)


def test_native_and_legacy_images_give_the_same_records():
    rng = np.random.default_rng(5)
    native = soup(rng, 700, F21)
    legacy = native.reshape(-1, 2)[:, ::-1].reshape(-1).copy()
    a, b = both(native, F21), both(legacy, F21L)
    assert a == b and len(a[0]) > 100
    # one image read the other way is another stream
    assert R.decode(native.tolist(), F21L)[2] != a[2]


@pytest.mark.parametrize("format", R.FORMATS)
def test_cut_at_every_word_boundary(format):
    rng = np.random.default_rng(3)
    w = np.concatenate([np.array(R.time_high_word(4000, format), np.uint32), soup(rng, 300, format)])
    per = 1 if format == F20 else 2
    whole, s_whole, c_whole = both(w, format)
    assert len(whole) > 50
    for k in range(0, len(w) + 1, per):
        a, s_a, c_a = R.decode(w[:k].tolist(), format)
        got_a, st_a, cnt_a = abi.evt2_to_events(w[:k], format)
        got_b, st_b, cnt_b = abi.evt2_to_events(w[k:], format, st_a)
        assert got_a.tobytes() + got_b.tobytes() == R.records(whole).tobytes(), k
        assert st_a.as_tuple() == R.state_tuple(s_a) and st_b.as_tuple() == R.state_tuple(s_whole), k
        assert {key: cnt_a[key] + cnt_b[key] for key in cnt_a} == c_whole, k


@pytest.mark.parametrize("format", R.FORMATS)
def test_cap_too_small_fails_and_leaves_the_state(format):
    if format == F20:
        w = R.time_high_word(1, format) + [R.cd_word(1, 0, x, 2) for x in range(13)] + R.time_high_word(7, format)
    else:
        w = R.time_high_word(1, format) + R.image([R.vector_word(1, 0, 3, 2, 1), R.vector_word(1, 0, 9, 2, 0xFFF)], format) + R.time_high_word(7, format)
    w = np.array(w, np.uint32)
    so = lib.load()
    for cap in (0, 1, 12):
        st, n_out, out = abi.Evt2State(), ctypes.c_size_t(99), np.zeros(16, abi.EVENT_DTYPE)
        st.loops = 77
        rc = so.esvo_evt2_to_events(ctypes.byref(st), w.ctypes.data, w.nbytes, format, 0, out.ctypes.data, cap, ctypes.byref(n_out), None)
        assert rc == abi.ERR_CAPACITY and st.as_tuple() == (0, 0, 77)
        with pytest.raises(lib.EsvoError) as e:
            abi.evt2_to_events(w, format, cap=cap)
        assert e.value.code == abi.ERR_CAPACITY
    got, st, cnt = abi.evt2_to_events(w, format, cap=13)
    assert len(got) == 13 and st.time_high == 7


@pytest.mark.parametrize("format", R.FORMATS)
def test_bad_stamp_names_the_event(format):
    def cd(ts6, x, n=1):
        return [R.cd_word(1, ts6, x + i, 1) for i in range(n)] if format == F20 else R.image([R.vector_word(1, ts6, x, 1, (1 << n) - 1)], format)

    w = R.time_high_word(0, format) + cd(5, 1, 2) + cd(9, 3, 2) + cd(10, 4)
    # t_us: 5, 5, 9, 9, 10 -- an offset of -5 keeps every stamp at or above 0, -6 makes event 0 the first bad one
    for off, bad in ((-5, None), (-6, 0), (-10, 0), (0, None)):
        if bad is None:
            both(w, format, None, off)
            continue
        with pytest.raises(R.BadStamp) as want:
            R.decode(w, format, None, off)
        assert want.value.first_bad == bad
        with pytest.raises(abi.Evt2Error) as e:
            abi.evt2_to_events(np.array(w, np.uint32), format, None, off)
        assert e.value.first_bad == bad
    # a stream whose time FALLS below the offset later: events 0..1 are fine, event 2 is the first bad one
    w = np.array(R.time_high_word(1, format) + cd(5, 1, 2) + R.time_high_word(0, format) + cd(5, 3, 2), np.uint32)
    off = -(1 << 6)
    with pytest.raises(R.BadStamp) as want:
        R.decode(w.tolist(), format, None, off)
    assert want.value.first_bad == 2
    st, n_out = abi.Evt2State(), ctypes.c_size_t(0)
    rc = lib.load().esvo_evt2_to_events(ctypes.byref(st), w.ctypes.data, w.nbytes, format, off, None, 0, ctypes.byref(n_out), None)
    assert rc == abi.ERR_INVALID_ARG and n_out.value == 2 and st.as_tuple() == (0, 0, 0)
    assert "event 2 " in lib.load().esvo_last_error(None).decode()
    # the upper end: 2^32 * 10^9 ns is the first stamp that does not fit
    top = R.STAMP_END // 1000
    one = R.time_high_word(0, format) + cd(0, 0)
    both(one, format, None, top - 1)
    with pytest.raises(abi.Evt2Error):
        abi.evt2_to_events(np.array(one, np.uint32), format, None, top)
    # loops = 2^18 is invalid whatever the offset; 2^18 - 1 with an offset that brings the stamp into the range is fine
    s = far_state(0)
    s["loops"] = 2 ** 18
    with pytest.raises(R.BadStamp):
        R.decode(cd(0, 0), format, s, -(2 ** 52))
    with pytest.raises(abi.Evt2Error) as e:
        abi.evt2_to_events(np.array(cd(0, 0), np.uint32), format, c_state(s), -(2 ** 52))
    assert e.value.first_bad == 0
    s["loops"] = 2 ** 18 - 1
    want, _, _ = both(cd(0, 0), format, s, -((2 ** 18 - 1) << 34))
    assert want[0][2] == 0


def test_sizes_and_arguments():
    assert lib.evt2_sizes() == [ctypes.sizeof(abi.Evt2State), ctypes.sizeof(abi.Evt2Counts), 0, 0] == [16, 48, 0, 0]
    so, st = lib.load(), abi.Evt2State()
    w = np.zeros(8, np.uint32)
    call = so.esvo_evt2_to_events
    assert call(None, None, 0, F20, 0, None, 0, None, None) == abi.ERR_INVALID_ARG
    assert call(ctypes.byref(st), None, 4, F20, 0, None, 0, None, None) == abi.ERR_INVALID_ARG
    assert call(ctypes.byref(st), None, 0, F20, 0, None, 0, None, None) == 0
    for fmt, n_bytes, ok in ((F20, 4, True), (F20, 6, False), (F20, 7, False), (F21, 8, True), (F21, 12, False), (F21L, 4, False), (F21L, 16, True)):
        assert (call(ctypes.byref(st), w.ctypes.data, n_bytes, fmt, 0, None, 0, None, None) == 0) == ok, (fmt, n_bytes)
    assert call(ctypes.byref(st), w.ctypes.data + 2, 8, F20, 0, None, 0, None, None) == abi.ERR_INVALID_ARG    # an address = 2 mod 4
    assert call(ctypes.byref(st), w.ctypes.data + 4, 8, F21, 0, None, 0, None, None) == 0                     # 4-byte alignment suffices for EVT 2.1
    for fmt in (0, 2, 22, 30, 120, -21):                                                                     # unknown formats; 30 is esvo_evt3_to_events'
        assert call(ctypes.byref(st), w.ctypes.data, 8, fmt, 0, None, 0, None, None) == abi.ERR_INVALID_ARG, fmt
    got, st1, cnt = abi.evt2_to_events(b"", F21)
    assert len(got) == 0 and cnt["words"] == 0
    img = np.array(R.time_high_word(1, F21) + R.image([R.vector_word(1, 0, 3, 2, 1)], F21), "<u4")
    got, _, _ = abi.evt2_to_events(img.tobytes(), F21)
    assert len(got) == 1 and got[0]["x"] == 3 and got[0]["y"] == 2
    got64, _, _ = abi.evt2_to_events(img.view("<u8"), F21)                                                     # 64-bit integers for EVT 2.1
    assert got64.tobytes() == got.tobytes()
    with pytest.raises(ValueError):
        abi.evt2_to_events(b"\x00" * 12, F21)
    with pytest.raises(ValueError):
        abi.evt2_to_events(b"\x00" * 6, F20)
    with pytest.raises(ValueError):
        abi.evt2_to_events(img, 30)


def test_raw_header():
    words = np.array([0x80000001, 0x10000000], "<u4").tobytes()      # (TIME_HIGH first: 0x01 is not '%')
    tail = b"% geometry 1280x720\n"
    for lines, fmt in ((b"% evt 2.0\n", abi.EVT_2_0), (b"% format EVT2;height=720;width=1280\n", abi.EVT_2_0),
                       (b"% evt 2.1\n", abi.EVT_2_1), (b"% format EVT21;height=720;width=1280\n", abi.EVT_2_1),
                       (b"% evt 2.1\n% format EVT21;endianness=legacy;height=720;width=1280\n", abi.EVT_2_1_LEGACY),
                       (b"% format EVT21;height=720;width=1280;endianness=legacy\n% evt 2.1\n", abi.EVT_2_1_LEGACY),
                       (b"% format EVT21;endianness=little;height=720;width=1280\n", abi.EVT_2_1),
                       (b"% evt 3.0\n", abi.EVT_3_0), (b"% format EVT3;height=720;width=1280\n", abi.EVT_3_0),
                       (b"% date 2024-01-01 10:00:00\n", 0)):
        head = b"% camera_integrator_name Prophesee\n" + lines + tail
        assert abi.raw_header(head + b"% end\n" + words) == (len(head) + 6, 1280, 720, fmt)
        assert abi.raw_header(head + words) == (len(head), 1280, 720, fmt)          # ended by the first line that has no '%'
        # esvo_evt3_raw_header on the same bytes: as before, EVT 3.0 (or no named format) only
        if fmt in (abi.EVT_3_0, 0):
            assert abi.evt3_raw_header(head + words) == (len(head), 1280, 720)
        else:
            with pytest.raises(lib.EsvoError) as e:
                abi.evt3_raw_header(head + words)
            assert e.value.code == -5
    crlf = b"% format EVT21;height=480;width=640\r\n% end\r\n"
    assert abi.raw_header(crlf + words) == (len(crlf), 640, 480, abi.EVT_2_1)
    assert abi.raw_header(words) == (0, 0, 0, 0) and abi.raw_header(b"") == (0, 0, 0, 0)
    for bad in (b"% evt 4.0\n", b"% evt 2\n", b"% format EVT4;height=1\n", b"% format EVT22\n", b"% format DAT\n"):
        with pytest.raises(lib.EsvoError) as e:
            abi.raw_header(bad + words)
        assert e.value.code == -5
    # the snippet of INTEGRATION.md: header, then the words by format
    data = b"% evt 2.0\n% end\n" + words
    off, w, h, fmt = abi.raw_header(data)
    got, _, _ = abi.evt2_to_events(data[off:], fmt)
    assert fmt == abi.EVT_2_0 and len(got) == 1 and got[0]["polarity"] == 1
