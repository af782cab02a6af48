"""Prophesee EVT 2.0 and EVT 2.1 restated in Python ints from the table in include/esvo_hip.h (esvo_ts_push_evt2) and nothing else: a
sequential decoder, and encoders for test streams.  No numpy arithmetic on values: words, states and stamps are Python ints.

A stream is the list of its little-endian uint32 as they lie in memory: one per EVT 2.0 word, two per EVT 2.1 word (image() lays
64-bit words W out in either half order).  State: dict(have_th, time_high, loops); `flags` is have_th as the C struct packs it."""

STAMP_END = 2 ** 32 * 10 ** 9
EVT_2_0, EVT_2_1, EVT_2_1_LEGACY = 20, 21, 121
FORMATS = (EVT_2_0, EVT_2_1, EVT_2_1_LEGACY)
CD_OFF, CD_ON, TIME_HIGH, EXT_TRIGGER = 0x0, 0x1, 0x8, 0xA
OTHER = (0x2, 0x3, 0x4, 0x5, 0x6, 0x7, 0x9, 0xB, 0xC, 0xD, 0xE, 0xF)
COUNTS = ("words", "events", "dropped_events", "ignored_words", "ext_triggers", "time_loops")


def fresh_state():
    return dict(have_th=0, time_high=0, loops=0)


def state_tuple(s):
    """(flags, time_high, loops): what abi.Evt2State.as_tuple() gives"""
    return (s["have_th"], s["time_high"], s["loops"])


class BadStamp(Exception):
    def __init__(self, first_bad):
        super().__init__(f"event {first_bad}")
        self.first_bad = first_bad


def image(W, format):
    """64-bit EVT 2.1 words as the uint32 of their memory image"""
    out = []
    for w in W:
        lo, hi = w & 0xFFFFFFFF, w >> 32
        out += [lo, hi] if format == EVT_2_1 else [hi, lo]
    return out


def words_of(u32, format):
    """the words of a memory image: (type, ts6, x0, y, valid mask, TIME_HIGH payload) each"""
    if format == EVT_2_0:
        for w in u32:
            assert 0 <= w < 2 ** 32
            yield w >> 28, (w >> 22) & 0x3F, (w >> 11) & 0x7FF, w & 0x7FF, 1, w & 0x0FFFFFFF
        return
    assert format in (EVT_2_1, EVT_2_1_LEGACY) and len(u32) % 2 == 0
    for first, second in zip(u32[0::2], u32[1::2]):
        W = (second << 32 | first) if format == EVT_2_1 else (first << 32 | second)
        yield W >> 60, (W >> 54) & 0x3F, (W >> 43) & 0x7FF, (W >> 32) & 0x7FF, W & 0xFFFFFFFF, (W >> 32) & 0x0FFFFFFF


def decode(u32, format, state=None, t_offset_us=0):
    """-> (events [(x, y, stamp_ns, polarity)], state behind the words, counts); the state passed in is not changed.
    BadStamp (index of the first bad event) where loops >= 2^18 or (t_us + t_offset_us) * 1000 lies outside [0, 2^32 * 10^9)."""
    s = dict(state) if state is not None else fresh_state()
    c = dict.fromkeys(COUNTS, 0)
    out = []
    for typ, ts6, x0, y, valid, v in words_of([int(w) for w in u32], format):
        c["words"] += 1
        if typ in (CD_OFF, CD_ON):
            for i in range(32):
                if valid >> i & 1:
                    if not s["have_th"]:
                        c["dropped_events"] += 1
                        continue
                    t_us = s["loops"] << 34 | s["time_high"] << 6 | ts6
                    stamp = (t_us + t_offset_us) * 1000
                    if s["loops"] >= 2 ** 18 or not 0 <= stamp < STAMP_END:
                        raise BadStamp(len(out))
                    assert x0 + i < 65536
                    out.append((x0 + i, y, stamp, typ))
        elif typ == TIME_HIGH:
            if s["have_th"] and v < s["time_high"] and s["time_high"] - v >= 2 ** 27:
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
    if events:   # (the values are split in Python ints; numpy only stores them)
        ev["x"], ev["y"] = [e[0] for e in events], [e[1] for e in events]
        ev["sec"], ev["nsec"] = [e[2] // 10 ** 9 for e in events], [e[2] % 10 ** 9 for e in events]
        ev["polarity"] = [e[3] for e in events]
    return ev


def time_high_word(v, format):
    """the memory image of one TIME_HIGH word"""
    return [TIME_HIGH << 28 | v] if format == EVT_2_0 else image([TIME_HIGH << 60 | v << 32], format)


def vector_word(pol, ts6, x0, y, valid):
    """one EVT 2.1 word W"""
    assert pol in (0, 1) and 0 <= ts6 < 64 and 0 <= x0 < 2048 and 0 <= y < 2048 and 0 <= valid < 2 ** 32
    return pol << 60 | ts6 << 54 | x0 << 43 | y << 32 | valid


def cd_word(pol, ts6, x, y):
    """one EVT 2.0 CD word"""
    assert pol in (0, 1) and 0 <= ts6 < 64 and 0 <= x < 2048 and 0 <= y < 2048
    return pol << 28 | ts6 << 22 | x << 11 | y


def encode(events, format):
    """the memory image for events [(x, y, t_us, polarity)] with x, y < 2048, t_us ascending and below 2^34: a TIME_HIGH word wherever
    t_us >> 6 changes (and in front of the first event); EVT 2.0: one word per event; EVT 2.1: one word per group, a group being a
    run of events of equal (t_us, y, polarity) whose x ascend and stay below the first one's + 32"""
    out, cur_hi = [], None
    i, n = 0, len(events)
    while i < n:
        x, y, t, pol = (int(v) for v in events[i])
        assert 0 <= t < 2 ** 34 and (cur_hi is None or t >> 6 >= cur_hi)
        if t >> 6 != cur_hi:
            cur_hi = t >> 6
            out += time_high_word(cur_hi, format)
        j = i + 1
        if format == EVT_2_0:
            out.append(cd_word(pol, t & 0x3F, x, y))
        else:
            valid = 1
            while j < n and tuple(int(v) for v in events[j][1:]) == (y, t, pol) and int(events[j - 1][0]) < int(events[j][0]) < x + 32:
                valid |= 1 << (int(events[j][0]) - x)
                j += 1
            out += image([vector_word(pol, t & 0x3F, x, y, valid)], format)
        i = j
    return out
