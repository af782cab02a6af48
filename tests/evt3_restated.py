"""Prophesee EVT 3.0 restated in Python ints from the table in include/esvo_hip.h (esvo_ts_push_evt3) and nothing else: a sequential
decoder, and an encoder for test streams.  No numpy arithmetic on values: words, states and stamps are Python ints.

State: dict(have_th, have_y, have_base, vect_pol, y, base_x, time_high, time_low, loops); `flags` packs the first four as the
C struct does (bit0 have_th, bit1 have_y, bit2 have_base, bit3 vect_pol)."""

STAMP_END = 2 ** 32 * 10 ** 9
ADDR_Y, ADDR_X, VECT_BASE_X, VECT_12, VECT_8, TIME_LOW, TIME_HIGH, EXT_TRIGGER = 0x0, 0x2, 0x3, 0x4, 0x5, 0x6, 0x8, 0xA
RESERVED = (0x1, 0x7, 0x9, 0xB, 0xC, 0xD, 0xE, 0xF)
COUNTS = ("words", "events", "dropped_events", "ignored_words", "ext_triggers", "time_loops")


def fresh_state():
    return dict(have_th=0, have_y=0, have_base=0, vect_pol=0, y=0, base_x=0, time_high=0, time_low=0, loops=0)


def state_tuple(s):
    """(flags, y, base_x, time_high, time_low, loops): what abi.Evt3State.as_tuple() gives"""
    return (s["have_th"] | s["have_y"] << 1 | s["have_base"] << 2 | s["vect_pol"] << 3, s["y"], s["base_x"], s["time_high"], s["time_low"], s["loops"])


class BadStamp(Exception):
    def __init__(self, first_bad):
        super().__init__(f"event {first_bad}")
        self.first_bad = first_bad


def decode(words, state=None, t_offset_us=0):
    """-> (events [(x, y, stamp_ns, polarity)], state behind the words, counts); the state passed in is not changed.
    BadStamp (index of the first bad event) where (t_us + t_offset_us) * 1000 lies outside [0, 2^32 * 10^9)."""
    s = dict(state) if state is not None else fresh_state()
    c = dict.fromkeys(COUNTS, 0)
    out = []

    def emit(x, pol):
        t_us = s["loops"] << 24 | s["time_high"] << 12 | s["time_low"]
        stamp = (t_us + t_offset_us) * 1000
        if not 0 <= stamp < STAMP_END:
            raise BadStamp(len(out))
        out.append((x, s["y"], stamp, pol))

    for w in words:
        w = int(w)
        assert 0 <= w < 65536
        c["words"] += 1
        typ = w >> 12
        if typ == ADDR_Y:
            s["y"], s["have_y"] = w & 0x7FF, 1
        elif typ == ADDR_X:
            if s["have_th"] and s["have_y"]:
                emit(w & 0x7FF, (w >> 11) & 1)
            else:
                c["dropped_events"] += 1
        elif typ == VECT_BASE_X:
            s["base_x"], s["vect_pol"], s["have_base"] = w & 0x7FF, (w >> 11) & 1, 1
        elif typ in (VECT_12, VECT_8):
            width = 12 if typ == VECT_12 else 8
            mask = w & ((1 << width) - 1)
            for i in range(width):
                if mask >> i & 1:
                    if s["have_th"] and s["have_y"] and s["have_base"]:
                        emit((s["base_x"] + i) & 0xFFFF, s["vect_pol"])
                    else:
                        c["dropped_events"] += 1
            s["base_x"] = (s["base_x"] + width) & 0xFFFF
        elif typ == TIME_LOW:
            s["time_low"] = w & 0xFFF
        elif typ == TIME_HIGH:
            v = w & 0xFFF
            if s["have_th"] and v < s["time_high"] and s["time_high"] - v >= 2048:
                s["loops"] = (s["loops"] + 1) & 0xFFFFFFFF
                c["time_loops"] += 1
            s["time_high"], s["have_th"] = v, 1
        elif typ == EXT_TRIGGER:
            c["ext_triggers"] += 1
        else:
            c["ignored_words"] += 1
    c["events"] = len(out)
    return out, s, c


def records(events):
    """the esvo_event_t array of decoded events (padding 0)"""
    import numpy as np
    from esvo_amd import abi
    ev = np.zeros(len(events), abi.EVENT_DTYPE)
    for i, (x, y, stamp, pol) in enumerate(events):
        ev[i]["x"], ev[i]["y"], ev[i]["sec"], ev[i]["nsec"], ev[i]["polarity"] = x, y, stamp // 10 ** 9, stamp % 10 ** 9, pol
    return ev


def encode(events, vect=False, start_t_us=None):
    """words for events [(x, y, t_us, polarity)] with x, y < 2048, t_us ascending and below 2^24 * 2^32.  vect: greedy VECT_12 / VECT_8
    over runs of equal (t, y, polarity) whose x fit one window behind the run's first x, else every event an ADDR_X word.
    TIME_HIGH is sent whenever it changes and at least every 1024 TIME_HIGH units across a gap, so loops stay unambiguous.  The
    stream starts at start_t_us: a TIME_HIGH word for it comes first (decode it from loops_state(start_t_us)); by default the
    first TIME_HIGH jumps straight to the first event's time, which a decoder in zero state reads right below 2^24 us."""
    words = []
    cur_hi = None     # the full upper time (t_us >> 12) the stream stands at
    cur_lo = cur_y = None
    if start_t_us is not None:
        cur_hi = start_t_us >> 12
        words.append(TIME_HIGH << 12 | (cur_hi & 0xFFF))

    def goto_hi(hi):
        nonlocal cur_hi
        if cur_hi is None:
            cur_hi = hi
            words.append(TIME_HIGH << 12 | (hi & 0xFFF))
        while cur_hi < hi:
            cur_hi = min(hi, cur_hi + 1024)
            words.append(TIME_HIGH << 12 | (cur_hi & 0xFFF))

    i, n = 0, len(events)
    while i < n:
        x, y, t, pol = (int(v) for v in events[i])
        assert 0 <= x < 2048 and 0 <= y < 2048 and pol in (0, 1)
        hi, lo = t >> 12, t & 0xFFF
        assert cur_hi is None or hi >= cur_hi
        if hi != cur_hi:
            goto_hi(hi)
        if lo != cur_lo:
            words.append(TIME_LOW << 12 | lo)
            cur_lo = lo
        if y != cur_y:
            words.append(ADDR_Y << 12 | y)
            cur_y = y
        j = i + 1
        if vect:
            while j < n and tuple(int(v) for v in events[j][1:]) == (y, t, pol) and x < int(events[j][0]) < x + 12 and int(events[j][0]) > int(events[j - 1][0]):
                j += 1
        if j - i >= 2:
            xs = [int(e[0]) - x for e in events[i:j]]
            mask = sum(1 << d for d in xs)
            words.append(VECT_BASE_X << 12 | pol << 11 | x)
            words.append((VECT_8 << 12 | mask) if max(xs) < 8 else (VECT_12 << 12 | mask))
        else:
            words.append(ADDR_X << 12 | pol << 11 | x)
            j = i + 1
        i = j
    return words


def loops_state(t_us):
    """the state of a stream that stands at time t_us (loops and TIME_HIGH known, nothing else): where encode(...,
    start_t_us=t_us) continues without a spurious loop, for streams whose time does not start near zero"""
    s = fresh_state()
    s["loops"], s["time_high"], s["time_low"], s["have_th"] = t_us >> 24, (t_us >> 12) & 0xFFF, t_us & 0xFFF, 1
    return s
