"""Which refusal wins where a push is wrong in two ways at once (esvo_amd/csrc/api_ingest.hip, api_words.hip, ingest.hpp).  The
test_refusals_* tests of the ingest suites pin every refusal alone; here each row of ROWS makes a call that two checks object to and
pins the (code, message) that comes out, and that the ring (esvo_debug_ts_ring), the counters and, where they are on, the filter's and
the survey's totals are as before.  One handle with the ring, width and height of tests/test_gpu_event_columns.py, packets of 1 to 4
events (RING + 1 where "larger than the ring" is one of the two).  Every row is refused on the host before anything is staged; the one
row with device columns launches the kernel that turns their `t` into stamps in the column staging first, as every such push does."""
import ctypes

import numpy as np
import pytest

from esvo_amd import abi, lib, params

pytestmark = pytest.mark.gpu

RING = 1024
W, H = 346, 260
T0_NS = 1_700_000_000 * 10 ** 9

RING_FULL = "event ring full: render (scatter) before staging more events"
TOO_LARGE = "event block larger than the event ring"
SURVEY_FULL = "event survey: the packet would take events_in + outside beyond 2^32 - 1 (take the mask, then esvo_ts_survey_end / _begin)"


def bad_element(i):
    return f"event columns: element {i} has no valid time stamp ((t + t_offset) * unit outside [0, 2^32 * 10^9))"


@pytest.fixture(scope="module")
def dev(upenn_rig):
    assert (upenn_rig.width, upenn_rig.height) == (W, H)
    p = params.make_params(params.PRESETS["mapping_upenn"], upenn_rig, max_events_per_tick=4096, event_ring_capacity=RING, regularization=0)[0]
    d = lib.Esvo(p, upenn_rig)
    yield d
    d.close()


def records(stamps_ns):
    ev = np.zeros(len(stamps_ns), abi.EVENT_DTYPE)
    ev["x"], ev["y"], ev["polarity"] = 7 + np.arange(len(ev)), 9, 1
    ev["sec"], ev["nsec"] = [t // 10 ** 9 for t in stamps_ns], [t % 10 ** 9 for t in stamps_ns]
    return ev


def columns(stamps, n=None):
    """host columns of len(stamps) events (or n events, all at T0_NS), stamps in ns as int64"""
    n = len(stamps) if n is None else n
    t = np.array(stamps, np.int64) if len(stamps) == n else np.full(n, T0_NS, np.int64)
    return np.full(n, 7, np.uint16), np.full(n, 9, np.uint16), t, np.ones(n, np.uint8)


def fill_ring(dev):
    """RING staged events, none scattered: not one more fits.  -> the newest staged stamp"""
    dev.ts_push_events(0, records([T0_NS + 1000 * i for i in range(RING)]))
    return T0_NS + 1000 * (RING - 1)


# ---- the rows: each sets the handle up and returns the call that is refused (its value: the C call's code) -----------------------------
def call_columns(dev, cols, n=None, memory=None, x_shift=0):
    s, (n_cols, _keep) = lib.event_columns_struct(*cols)
    if memory is not None:
        s.memory = memory
    s.x += x_shift
    return lib.load().esvo_ts_push_event_columns(dev.h, 0, ctypes.addressof(s), n_cols if n is None else n)


def call_records(dev, ev):
    return lib.load().esvo_ts_push_events(dev.h, 0, ev.ctypes.data, len(ev))


def larger_than_ring_and_unaligned(dev):
    return lambda: call_columns(dev, columns([], RING + 1), x_shift=1)


def evt3_unknown_memory_and_odd_bytes(dev):
    buf = np.zeros(2, np.uint16)
    return lambda: lib.load().esvo_ts_push_evt3(dev.h, 0, buf.ctypes.data, 3, 2, 0, None)


def evt2_unknown_memory_and_odd_bytes(dev):
    buf = np.zeros(2, np.uint32)
    return lambda: lib.load().esvo_ts_push_evt2(dev.h, 0, buf.ctypes.data, 6, abi.EVT_2_0, 2, 0, None)


def host_labelled_device_and_larger_than_ring(dev):
    return lambda: call_columns(dev, columns([], RING + 1), memory=abi.MEM_DEVICE)


def ring_full_and_unsorted_records(dev):
    newest = fill_ring(dev)
    return lambda: call_records(dev, records([newest + 10, newest + 5, newest + 20]))


def ring_full_and_older_than_staged_columns(dev):
    newest = fill_ring(dev)
    return lambda: call_columns(dev, columns([newest - 3000, newest - 2000]))


def filter_bad_stamp_and_ring_full_host(dev):
    newest = fill_ring(dev)
    dev.ts_filter_configure(0)
    return lambda: call_columns(dev, columns([newest + 1, newest + 2, -1, newest + 4]))


def filter_bad_stamp_and_ring_full_device(dev):
    """device columns under the filter: their stamps are judged by the filter's last kernel, which a full ring never lets run"""
    import torch
    newest = fill_ring(dev)
    dev.ts_filter_configure(0)
    x, y, t, p = columns([newest + 1, newest + 2, -1, newest + 4])
    d = tuple(torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda() for a in (x, y, t, p))
    torch.cuda.synchronize()
    return lambda: call_columns(dev, d)


def survey_overflow_and_ring_full(dev):
    newest = fill_ring(dev)
    dev.ts_filter_configure(0)
    dev.ts_survey_begin(0)
    dev.ts_survey_state(0, set=np.zeros((2, H, W), np.uint32), stats=dict(events_in=2 ** 32 - 2, outside=0, packets=1, t_first=T0_NS, t_last=newest))
    return lambda: call_records(dev, records([newest + 1, newest + 2]))


# (the row, then the code and the message: read off a build of the commit before ingest was split out of api_ts.hip)
ROWS = [
    (larger_than_ring_and_unaligned, abi.ERR_INVALID_ARG, "event columns: a column base is not aligned for its element type"),
    (evt3_unknown_memory_and_odd_bytes, abi.ERR_INVALID_ARG, "EVT3 words: unknown memory"),
    (evt2_unknown_memory_and_odd_bytes, abi.ERR_INVALID_ARG, "EVT2 words: unknown memory"),
    (host_labelled_device_and_larger_than_ring, abi.ERR_CAPACITY, TOO_LARGE),
    (ring_full_and_unsorted_records, abi.ERR_CAPACITY, RING_FULL),
    (ring_full_and_older_than_staged_columns, abi.ERR_CAPACITY, RING_FULL),
    (filter_bad_stamp_and_ring_full_host, abi.ERR_INVALID_ARG, bad_element(2)),
    (filter_bad_stamp_and_ring_full_device, abi.ERR_CAPACITY, RING_FULL),
    (survey_overflow_and_ring_full, abi.ERR_CAPACITY, SURVEY_FULL),
]


def state(dev, filter_on, survey_on):
    ev, st, b0, b1 = dev.debug_ts_ring(0)
    s = dev.stats()
    return dict(records=ev.tobytes(), stamps=st.tobytes(), bounds=(b0, b1), staged=list(s.events_staged), late=list(s.late_events),
                scattered=list(s.events_scattered), filter=dev.ts_filter_stats(0) if filter_on else None,
                survey=dev.ts_survey_stats(0) if survey_on else None)


@pytest.mark.parametrize("row,code,message", ROWS, ids=[r[0].__name__ for r in ROWS])
def test_which_refusal_wins(dev, row, code, message):
    filter_on, survey_on = "filter" in row.__name__ or "survey" in row.__name__, "survey" in row.__name__
    dev.reset()
    try:
        refused = row(dev)
        before = state(dev, filter_on, survey_on)
        got = (refused(), lib.load().esvo_last_error(dev.h).decode())
        assert got == (code, message)
        assert state(dev, filter_on, survey_on) == before
    finally:
        if survey_on:
            dev.ts_survey_end(0)
        if filter_on:
            dev.ts_filter_configure(0, off=True)
