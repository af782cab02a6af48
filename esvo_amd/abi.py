"""ctypes / numpy mirrors of the POD types declared in include/esvo_hip.h.

Shared by the product bindings (esvo_amd.lib) and by the test-only oracle bindings
(oracle/oracle.py).  Layouts are asserted against sizeof() exported by the libraries.
"""
import ctypes as C

import numpy as np

EVENT_DTYPE = np.dtype(
    [("x", "<u2"), ("y", "<u2"), ("sec", "<u4"), ("nsec", "<u4"), ("polarity", "u1"), ("_pad", "u1", (3,))]
)
assert EVENT_DTYPE.itemsize == 16

MATCH_DTYPE = np.dtype(
    [("x_left", "<f8", (2,)), ("inv_depth", "<f8"), ("cost", "<f8"), ("disp", "<f8"),
     ("event_idx", "<u4"), ("pose_idx", "<u4")]
)
assert MATCH_DTYPE.itemsize == 48

DEPTH_POINT_DTYPE = np.dtype(
    [("row", "<u4"), ("col", "<u4"), ("x", "<f8", (2,)), ("inv_depth", "<f8"), ("scale2", "<f8"),
     ("nu", "<f8"), ("variance", "<f8"), ("residual", "<f8"), ("age", "<u8"), ("p_cam", "<f8", (3,)),
     ("pose_idx", "<u4"), ("seq", "<u4")]
)
assert DEPTH_POINT_DTYPE.itemsize == 104

# esvo_status_t values the bindings and the tests name (include/esvo_hip.h)
ERR_INVALID_ARG, ERR_CAPACITY, ERR_STATE = -1, -4, -6

CAM_LEFT, CAM_RIGHT = 0, 1
FUSION_CONST_FRAMES, FUSION_CONST_POINTS = 0, 1
LSNORM_TDIST, LSNORM_L2 = 0, 1


class CalibStruct(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("P", C.c_double * 12),
        ("rect_lut", C.c_void_p), ("rect_mask", C.c_void_p),
        ("map_x", C.c_void_p), ("map_y", C.c_void_p),
    ]


class ParamsStruct(C.Structure):
    _fields_ = [
        ("decay_ms", C.c_double),
        ("median_blur_kernel_size", C.c_int32),
        ("ignore_polarity", C.c_int32),
        ("patch_size_x", C.c_int32),
        ("patch_size_y", C.c_int32),
        ("ls_norm", C.c_int32),
        ("td_nu", C.c_double),
        ("td_scale", C.c_double),
        ("lm_max_iteration", C.c_int32),
        ("reg_radius", C.c_int32),
        ("reg_min_neighbours", C.c_int32),
        ("reg_min_close_neighbours", C.c_int32),
        ("bm_min_disparity", C.c_int32),
        ("bm_max_disparity", C.c_int32),
        ("bm_step", C.c_int32),
        ("bm_zncc_threshold", C.c_double),
        ("bm_updown", C.c_int32),
        ("smooth_time_surface", C.c_int32),
        ("invdepth_min", C.c_double),
        ("invdepth_max", C.c_double),
        ("stdvar_vis_threshold", C.c_double),
        ("residual_vis_threshold", C.c_double),
        ("age_vis_threshold", C.c_double),
        ("fusion_radius", C.c_int32),
        ("fusion_strategy", C.c_int32),
        ("max_fusion_frames", C.c_int32),
        ("max_fusion_points", C.c_int32),
        ("clean_requires_full_window", C.c_int32),
        ("regularization", C.c_int32),
        ("denoising", C.c_int32),
        ("process_event_num", C.c_int32),
        ("bm_half_slice_thickness", C.c_double),
        ("num_threads", C.c_int32),
        ("max_events_per_tick", C.c_int32),
        ("max_window_points", C.c_int32),
        ("max_poses_per_tick", C.c_int32),
        ("event_ring_capacity", C.c_int64),
        ("max_event_queue_len", C.c_int32),   # ABI 5: 0 = one stamp per pixel (fast path), 1..32 = EventQueueMat semantics
        ("lm_scale_pass_limit", C.c_int32),   # 0: off; > 0: pass limit per evaluation; LM_SCALE_COUNT_ONLY: count only
    ]


class StatsStruct(C.Structure):
    _fields_ = [
        ("ticks", C.c_uint64),
        ("events_staged", C.c_uint64 * 2),
        ("events_scattered", C.c_uint64 * 2),
        ("ts_frames", C.c_uint64 * 2),
        ("last_events_in", C.c_uint32),
        ("last_matches", C.c_uint32),
        ("last_solved", C.c_uint32),
        ("last_points", C.c_uint32),
        ("last_window_frames", C.c_uint32),
        ("last_window_points", C.c_uint32),
        ("last_fusions", C.c_uint32),
        ("last_map_size", C.c_uint32),
        ("ms_ts_scatter", C.c_float), ("ms_ts_render", C.c_float),
        ("ms_bm", C.c_float), ("ms_refine", C.c_float), ("ms_fusion", C.c_float),
        ("ms_regularization", C.c_float), ("ms_tick_total", C.c_float),
        ("ms_kernel", C.c_float * 8),
        ("pad_", C.c_float),
        ("total_events_in", C.c_uint64), ("total_matches", C.c_uint64), ("total_points", C.c_uint64),
        ("sum_ms_kernel", C.c_double * 8),
        ("last_bm_info_noise_low", C.c_uint32), ("last_bm_coarse_fail", C.c_uint32), ("last_bm_fine_fail", C.c_uint32), ("pad2_", C.c_uint32),
        ("total_bm_info_noise_low", C.c_uint64), ("total_bm_coarse_fail", C.c_uint64), ("total_bm_fine_fail", C.c_uint64),
        # ABI 3: in-run shader-clock probe of the refinement kernel (include/esvo_hip.h)
        ("clk_cycles", C.c_uint64 * 8), ("clk_ref_ticks", C.c_uint64 * 8), ("clk_samples", C.c_uint64),
        ("clk_ref_khz", C.c_uint32), ("stage_timing_samples", C.c_uint32),
        # ABI 6: routed band mode
        ("halo_violations", C.c_uint64),
        ("late_events", C.c_uint64 * 2),
        ("pipeline_resyncs", C.c_uint64),
    ]

    def kernel_ms_mean(self, base=None):
        """mean HIP-event time per launch of the eight ms_kernel slots since `base` (an earlier StatsStruct) or since esvo_create:
        sum_ms_kernel[2..6] over the ticks that recorded their stage events (stage_timing_samples, ABI 8: stage timings are sampled),
        [0..1] over the sampled Time-Surface renders (two per pair sample, counted in [7])"""
        ks = [float(self.sum_ms_kernel[i]) - (float(base.sum_ms_kernel[i]) if base is not None else 0.0) for i in range(8)]
        n = int(self.stage_timing_samples) - (int(base.stage_timing_samples) if base is not None else 0)
        out = [k / n if n > 0 else 0.0 for k in ks]
        if ks[7] > 0:
            out[0], out[1] = 2 * ks[0] / ks[7], 2 * ks[1] / ks[7]
        out[7] = ks[7]
        return out

    def sclk_mhz(self, base=None):
        """(all XCDs, [per XCD]) shader clock in MHz the LM kernel ran at since `base` (an earlier StatsStruct) or since
        esvo_create: sum of s_memtime differences / sum of s_memrealtime differences x the reference rate; None without samples"""
        cyc = [int(self.clk_cycles[i]) - (int(base.clk_cycles[i]) if base is not None else 0) for i in range(8)]
        ref = [int(self.clk_ref_ticks[i]) - (int(base.clk_ref_ticks[i]) if base is not None else 0) for i in range(8)]
        khz = float(self.clk_ref_khz)
        per = [c / r * khz / 1e3 if r > 0 else None for c, r in zip(cyc, ref)]
        tot = sum(cyc) / sum(ref) * khz / 1e3 if sum(ref) > 0 else None
        return tot, per


class CommStatsStruct(C.Structure):
    """esvo_comm_stats_t (ABI 7): the tick-interleaved frame exchange of one rank"""
    _fields_ = [
        ("rounds", C.c_uint64), ("gathers", C.c_uint64), ("regrows", C.c_uint64), ("bytes_sent", C.c_uint64),
        ("points_gathered", C.c_uint64), ("host_wait_us", C.c_uint64), ("last_stride_points", C.c_uint32), ("stride_cap_points", C.c_uint32),
    ]


def make_events(x, y, t_ns, polarity=None):
    """Build an esvo_event_t array from coordinate / nanosecond-timestamp arrays."""
    t_ns = np.asarray(t_ns, dtype=np.uint64)
    ev = np.zeros(t_ns.shape[0], dtype=EVENT_DTYPE)
    ev["x"] = x
    ev["y"] = y
    ev["sec"] = (t_ns // np.uint64(1_000_000_000)).astype(np.uint32)
    ev["nsec"] = (t_ns % np.uint64(1_000_000_000)).astype(np.uint32)
    ev["polarity"] = 1 if polarity is None else polarity
    return ev


# ---- event columns (esvo_event_columns_t of include/esvo_hip.h): x / y / t / p arrays in host or device memory
T_NS_I64, T_US_I64, T_US_U32 = 0, 1, 2
P_U8, P_I8 = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
STAMP_END_NS = 2 ** 32 * 10 ** 9   # a valid stamp is below this: what sec (u32) can hold


class EventColumnsStruct(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("t", C.c_void_p), ("p", C.c_void_p),
        ("t_offset", C.c_int64),
        ("t_type", C.c_int32), ("p_type", C.c_int32), ("memory", C.c_int32), ("reserved", C.c_int32),
    ]


class ColumnsError(ValueError):
    """an element of the columns has no valid stamp; `first_bad` is its index"""

    def __init__(self, first_bad):
        super().__init__(f"event columns: element {first_bad} has no valid time stamp ((t + t_offset) * unit outside [0, 2^32 * 10^9))")
        self.first_bad = int(first_bad)


def column_t_type(dtype, unit):
    """t_type of a stamp column from its dtype and unit ("ns" | "us"); ValueError for a combination the C-ABI does not take"""
    dtype = np.dtype(dtype)
    if unit == "ns" and dtype == np.int64:
        return T_NS_I64
    if unit == "us" and dtype == np.int64:
        return T_US_I64
    if unit == "us" and dtype == np.uint32:
        return T_US_U32
    raise ValueError(f"event columns: t must be int64 (unit 'ns' or 'us') or uint32 (unit 'us'), not {dtype} with unit {unit!r}")


def column_p_type(dtype):
    dtype = np.dtype(dtype)
    if dtype in (np.dtype(np.uint8), np.dtype(np.bool_)):
        return P_U8
    if dtype == np.int8:
        return P_I8
    raise ValueError(f"event columns: p must be uint8 / bool (!= 0 is ON) or int8 (> 0 is ON), not {dtype}")


def check_t_offset(t_offset):
    t_offset = int(t_offset)
    if not -2 ** 63 <= t_offset < 2 ** 63:
        raise ValueError("event columns: t_offset must fit int64")
    return t_offset


def columns_to_events(x, y, t, p=None, unit="ns", t_offset=0):
    """esvo_event_columns_to_events in numpy: the esvo_event_t records of the columns x, y (16-bit), t (int64 ns / us or uint32 us)
    and p (uint8: != 0 is ON; int8: > 0 is ON; None: all ON), stamp = (t + t_offset) * unit.  Exact: no element is added or scaled
    before it is known to stay inside int64.  Raises ColumnsError (first_bad) where a stamp is not in [0, 2^32 * 10^9)."""
    t = np.asarray(t)
    t_type = column_t_type(t.dtype, unit)
    off, k = check_t_offset(t_offset), (1 if t_type == T_NS_I64 else 1000)
    n = t.shape[0]
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype.itemsize != 2 or y.dtype.itemsize != 2 or x.dtype.kind not in "iu" or y.dtype.kind not in "iu":
        raise ValueError("event columns: x and y must be 16-bit integers")
    if x.shape != (n,) or y.shape != (n,) or (p is not None and np.asarray(p).shape != (n,)):
        raise ValueError("event columns: one-dimensional columns of one length are expected")
    t64 = t.astype(np.int64)
    lo, hi = max(-off, -2 ** 63), min((STAMP_END_NS - 1) // k - off, 2 ** 63 - 1)   # 0 <= t + off <= hi + off, as bounds on t
    ok = (t64 >= np.int64(lo)) & (t64 <= np.int64(hi)) if lo <= hi else np.zeros(n, bool)
    if not ok.all():
        raise ColumnsError(int(np.argmin(ok)))
    s = (t64 + np.int64(off)).astype(np.uint64) * np.uint64(k)
    ev = np.zeros(n, dtype=EVENT_DTYPE)
    ev["x"], ev["y"] = x.view(np.uint16), y.view(np.uint16)
    ev["sec"] = (s // np.uint64(1_000_000_000)).astype(np.uint32)
    ev["nsec"] = (s % np.uint64(1_000_000_000)).astype(np.uint32)
    if p is None:
        ev["polarity"] = 1
    else:
        p = np.asarray(p)
        ev["polarity"] = (p > 0) if column_p_type(p.dtype) == P_I8 else (p != 0)
    return ev


# ---- Prophesee EVT 3.0 words (esvo_ts_push_evt3 of include/esvo_hip.h)
class Evt3State(C.Structure):
    """esvo_evt3_state_t: flags bit0 have_th, bit1 have_y, bit2 have_base, bit3 vect_pol"""
    _fields_ = [("flags", C.c_uint32), ("y", C.c_uint16), ("base_x", C.c_uint16), ("time_high", C.c_uint16), ("time_low", C.c_uint16),
                ("loops", C.c_uint32), ("reserved", C.c_uint32)]

    def as_tuple(self):
        return (self.flags, self.y, self.base_x, self.time_high, self.time_low, self.loops)

    def copy(self):
        return Evt3State.from_buffer_copy(self)


class Evt3Counts(C.Structure):
    """esvo_evt3_counts_t"""
    _fields_ = [(k, C.c_uint64) for k in ("words", "events", "dropped_events", "ignored_words", "ext_triggers", "time_loops")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class Evt3Error(ValueError):
    """an event of the words has no valid stamp; `first_bad` is its index among the events"""

    def __init__(self, first_bad):
        super().__init__(f"EVT3 words: event {first_bad} has no valid time stamp ((t_us + t_offset_us) * 1000 outside [0, 2^32 * 10^9))")
        self.first_bad = int(first_bad)


def evt3_words(words):
    """a contiguous uint16 host array over bytes / bytearray / memoryview (little-endian words) or anything numpy takes"""
    if isinstance(words, (bytes, bytearray, memoryview)):
        if len(words) % 2:
            raise ValueError("EVT3 words: an odd number of bytes")
        return np.frombuffer(words, "<u2")
    words = np.asarray(words)
    if words.dtype != np.uint16 or words.ndim != 1:
        raise ValueError(f"EVT3 words: a one-dimensional uint16 array is expected, not {words.dtype} with {words.ndim} dimensions")
    return np.ascontiguousarray(words)


def evt3_to_events(words, state=None, t_offset_us=0, count_only=False, cap=None):
    """esvo_evt3_to_events (the library's host decoder; no GPU): -> (events or None, the state behind the words, counts as a dict).
    state: an Evt3State (not changed) or None for a stream's start.  cap: room for that many records (default: as many as the words
    hold).  Raises Evt3Error (first_bad) for a bad stamp, lib.EsvoError (code -4, capacity) where cap is too small."""
    from . import lib
    words = evt3_words(words)
    st = state.copy() if state is not None else Evt3State()
    so, n_out, counts = lib.load(), C.c_size_t(0), Evt3Counts()
    off = check_t_offset(t_offset_us)
    out, room = None, 0
    if not count_only:
        if cap is None:  # count first (a bad stamp shows again below)
            so.esvo_evt3_to_events(C.byref(st.copy()), words.ctypes.data, words.size, off, None, 0, C.byref(n_out), None)
            cap = n_out.value
        room = int(cap)
        out = np.zeros(max(room, 1), EVENT_DTYPE)   # (never NULL: a NULL `out` counts)
    rc = so.esvo_evt3_to_events(C.byref(st), words.ctypes.data, words.size, off, None if out is None else out.ctypes.data, room,
                                C.byref(n_out), C.byref(counts))
    if rc == -1 and "no valid time stamp" in so.esvo_last_error(None).decode(errors="replace"):
        raise Evt3Error(n_out.value)
    if rc != 0:
        raise lib.EsvoError(f"esvo_evt3_to_events failed ({rc}): {so.esvo_last_error(None).decode(errors='replace')}", code=rc)
    return (None if count_only else out[:n_out.value]), st, counts.as_dict()


def evt3_raw_header(data):
    """esvo_evt3_raw_header on the first bytes of a Prophesee .raw file -> (data_offset, width, height); width / height 0 if absent.
    lib.EsvoError (code -5, unsupported) for a file that is not EVT 3.0."""
    from . import lib
    buf = np.frombuffer(bytes(data), np.uint8)
    off, w, h = C.c_size_t(0), C.c_int(0), C.c_int(0)
    so = lib.load()
    rc = so.esvo_evt3_raw_header(buf.ctypes.data if buf.size else None, buf.size, C.byref(off), C.byref(w), C.byref(h))
    if rc != 0:
        raise lib.EsvoError(f"esvo_evt3_raw_header failed ({rc}): {so.esvo_last_error(None).decode(errors='replace')}", code=rc)
    return int(off.value), int(w.value), int(h.value)


# ---- Prophesee EVT 2.0 / 2.1 words (esvo_ts_push_evt2 of include/esvo_hip.h)
EVT_2_0, EVT_2_1, EVT_2_1_LEGACY, EVT_3_0 = 20, 21, 121, 30
EVT2_FORMATS = (EVT_2_0, EVT_2_1, EVT_2_1_LEGACY)


class Evt2State(C.Structure):
    """esvo_evt2_state_t: flags bit0 have_th"""
    _fields_ = [("flags", C.c_uint32), ("time_high", C.c_uint32), ("loops", C.c_uint32), ("reserved", C.c_uint32)]

    def as_tuple(self):
        return (self.flags, self.time_high, self.loops)

    def copy(self):
        return Evt2State.from_buffer_copy(self)


Evt2Counts = Evt3Counts   # esvo_evt2_counts_t; `words` counts 32- or 64-bit words, by format


# esvo_event_filter_host / esvo_ts_filter_*: the verdicts of the event filter (include/esvo_hip.h)
FILTER_KEPT, FILTER_OUTSIDE, FILTER_MASKED, FILTER_REFRACTORY, FILTER_UNSUPPORTED = 0, 1, 2, 3, 4


class EventFilterStruct(C.Structure):
    """esvo_event_filter_t"""
    _fields_ = [("refractory_ns", C.c_uint64), ("support_ns", C.c_uint64), ("mask", C.c_void_p), ("reserved", C.c_uint32 * 4)]


class EventFilterCounts(C.Structure):
    """esvo_event_filter_counts_t"""
    _fields_ = [(k, C.c_uint64) for k in ("events_in", "kept", "outside", "masked", "refractory", "unsupported")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def event_filter_struct(refractory_ns, support_ns, mask, width, height):
    """(EventFilterStruct, the array its mask points into or None): mask is None or (height, width), non-zero = masked"""
    s = EventFilterStruct()
    s.refractory_ns, s.support_ns = int(refractory_ns), int(support_ns)
    keep = None
    if mask is not None:
        keep = np.ascontiguousarray((np.asarray(mask) != 0).astype(np.uint8))
        if keep.shape != (int(height), int(width)):
            raise ValueError(f"event filter mask: expected shape {(int(height), int(width))}, got {keep.shape}")
        s.mask = keep.ctypes.data
    return s, keep


# esvo_ts_burst_* / esvo_event_burst_filter_host: the burst stage of the event filter (include/esvo_hip.h)
BURST_OFF, BURST_TRAIL, BURST_STC_CUT_TRAIL, BURST_STC_KEEP_TRAIL = 0, 1, 2, 3
FILTER_BURST = 5


class EventBurstStruct(C.Structure):
    """esvo_event_burst_t"""
    _fields_ = [("burst_ns", C.c_uint64), ("mode", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class EventBurstCounts(C.Structure):
    """esvo_event_burst_counts_t"""
    _fields_ = [(k, C.c_uint64) for k in ("judged", "passed", "dropped")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def event_burst_struct(mode, burst_ns, reserved=(0, 0, 0)):
    s = EventBurstStruct()
    s.mode, s.burst_ns = int(mode), int(burst_ns)
    s.reserved[:] = [int(v) for v in reserved]
    return s


# esvo_ts_survey_* / esvo_event_survey_host / esvo_hot_pixel_mask_host: the event survey and its hot-pixel rule (include/esvo_hip.h)
SURVEY_COUNT_ONLY = 1
MASK_KEEP, MASK_REPLACE, MASK_UNION = 0, 1, 2


class _DictStruct(C.Structure):
    def as_dict(self):
        return {k: int(getattr(self, k)) for k, t in self._fields_ if not k.startswith("pad") and k != "reserved"}


class EventSurveyStruct(C.Structure):
    """esvo_event_survey_t"""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class EventSurveyStats(_DictStruct):
    """esvo_event_survey_stats_t"""
    _fields_ = [(k, C.c_uint64) for k in ("events_in", "outside", "packets", "t_first", "t_last")]


class HotPixelRule(_DictStruct):
    """esvo_hot_pixel_rule_t"""
    _fields_ = [("min_count", C.c_uint32), ("factor", C.c_uint32), ("rank_permille", C.c_uint32), ("max_rate_hz", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class HotPixelReport(_DictStruct):
    """esvo_hot_pixel_report_t"""
    _fields_ = [("baseline", C.c_uint32), ("rate_count", C.c_uint32), ("n_hot", C.c_uint32), ("max_count", C.c_uint32), ("max_pixel", C.c_uint32),
                ("pad_", C.c_uint32), ("events_hot", C.c_uint64)]


def event_survey_stats(stats):
    """an EventSurveyStats from a dict (missing keys: 0) or None"""
    s = EventSurveyStats()
    for k, v in (stats or {}).items():
        setattr(s, k, int(v))
    return s


def hot_pixel_rule(min_count=1, factor=0, rank_permille=500, max_rate_hz=0, reserved=(0, 0, 0, 0)):
    r = HotPixelRule()
    r.min_count, r.factor, r.rank_permille, r.max_rate_hz = int(min_count), int(factor), int(rank_permille), int(max_rate_hz)
    r.reserved[:] = [int(v) for v in reserved]
    return r


class Evt2Error(ValueError):
    """an event of the words has no valid stamp; `first_bad` is its index among the events"""

    def __init__(self, first_bad):
        super().__init__(f"EVT2 words: event {first_bad} has no valid time stamp ((t_us + t_offset_us) * 1000 outside [0, 2^32 * 10^9))")
        self.first_bad = int(first_bad)


def evt2_words(words, format):
    """a contiguous host array of 4- or 8-byte integers over bytes / bytearray / memoryview (the words as they lie in memory) or
    anything numpy takes: uint32 / int32 for every format (two per EVT 2.1 word), uint64 / int64 for EVT 2.1 as well"""
    if format not in EVT2_FORMATS:
        raise ValueError(f"EVT2 words: unknown format {format}")
    size = 4 if format == EVT_2_0 else 8
    if isinstance(words, (bytes, bytearray, memoryview)):
        if len(words) % size:
            raise ValueError(f"EVT2 words: the number of bytes is not a multiple of {size}")
        return np.frombuffer(words, "<u4")
    words = np.asarray(words)
    if words.dtype.kind not in "iu" or words.dtype.itemsize not in (4, size) or words.ndim != 1:
        raise ValueError(f"EVT2 words: a one-dimensional array of {size}-byte (or 4-byte) integers is expected, not {words.dtype} with {words.ndim} dimensions")
    return np.ascontiguousarray(words)


def evt2_to_events(words, format, state=None, t_offset_us=0, count_only=False, cap=None):
    """esvo_evt2_to_events (the library's host decoder; no GPU): -> (events or None, the state behind the words, counts as a dict).
    state: an Evt2State (not changed) or None for a stream's start.  cap: room for that many records (default: as many as the words
    hold).  Raises Evt2Error (first_bad) for a bad stamp, lib.EsvoError (code -4, capacity) where cap is too small."""
    from . import lib
    words = evt2_words(words, format)
    st = state.copy() if state is not None else Evt2State()
    so, n_out, counts = lib.load(), C.c_size_t(0), Evt2Counts()
    off = check_t_offset(t_offset_us)
    out, room = None, 0
    if not count_only:
        if cap is None:  # count first (a bad stamp shows again below)
            so.esvo_evt2_to_events(C.byref(st.copy()), words.ctypes.data, words.nbytes, int(format), off, None, 0, C.byref(n_out), None)
            cap = n_out.value
        room = int(cap)
        out = np.zeros(max(room, 1), EVENT_DTYPE)   # (never NULL: a NULL `out` counts)
    rc = so.esvo_evt2_to_events(C.byref(st), words.ctypes.data, words.nbytes, int(format), off, None if out is None else out.ctypes.data, room,
                                C.byref(n_out), C.byref(counts))
    if rc == -1 and "no valid time stamp" in so.esvo_last_error(None).decode(errors="replace"):
        raise Evt2Error(n_out.value)
    if rc != 0:
        raise lib.EsvoError(f"esvo_evt2_to_events failed ({rc}): {so.esvo_last_error(None).decode(errors='replace')}", code=rc)
    return (None if count_only else out[:n_out.value]), st, counts.as_dict()


def raw_header(data):
    """esvo_raw_header on the first bytes of a Prophesee .raw file -> (data_offset, width, height, format); width / height 0 if absent,
    format EVT_2_0 / EVT_2_1 / EVT_2_1_LEGACY / EVT_3_0, or 0 where no line names one.  lib.EsvoError (code -5, unsupported) for
    any other named format."""
    from . import lib
    buf = np.frombuffer(bytes(data), np.uint8)
    off, w, h, fmt = C.c_size_t(0), C.c_int(0), C.c_int(0), C.c_int(0)
    so = lib.load()
    rc = so.esvo_raw_header(buf.ctypes.data if buf.size else None, buf.size, C.byref(off), C.byref(w), C.byref(h), C.byref(fmt))
    if rc != 0:
        raise lib.EsvoError(f"esvo_raw_header failed ({rc}): {so.esvo_last_error(None).decode(errors='replace')}", code=rc)
    return int(off.value), int(w.value), int(h.value), int(fmt.value)


def event_ns(ev):
    return ev["sec"].astype(np.uint64) * np.uint64(1_000_000_000) + ev["nsec"].astype(np.uint64)


class Calib:
    """Host-side calibration products for one camera, kept alive for the C struct."""

    def __init__(self, width, height, P, rect_lut, rect_mask, map_x, map_y):
        self.width, self.height = int(width), int(height)
        self.P = np.ascontiguousarray(P, dtype=np.float64).reshape(12)
        self.rect_lut = np.ascontiguousarray(rect_lut, dtype=np.float32).reshape(height, width, 2)
        self.rect_mask = None if rect_mask is None else np.ascontiguousarray(rect_mask, dtype=np.uint8).reshape(height, width)
        self.map_x = np.ascontiguousarray(map_x, dtype=np.float32).reshape(height, width)
        self.map_y = np.ascontiguousarray(map_y, dtype=np.float32).reshape(height, width)

    def as_struct(self):
        s = CalibStruct()
        s.width, s.height = self.width, self.height
        for i in range(12):
            s.P[i] = float(self.P[i])
        s.rect_lut = self.rect_lut.ctypes.data
        s.rect_mask = 0 if self.rect_mask is None else self.rect_mask.ctypes.data
        s.map_x = self.map_x.ctypes.data
        s.map_y = self.map_y.ctypes.data
        return s


def serialize_event_array(ev, width, height, seq=0, stamp_ns=0, frame_id=""):
    """ROS1 wire format of a dvs_msgs/EventArray carrying `ev` (esvo_event_t array): std_msgs/Header (u32 seq, u32 sec,
    u32 nsec, u32 len + frame_id), u32 height, u32 width, u32 count, count x {u16 x, u16 y, u32 sec, u32 nsec, u8 polarity}."""
    import struct
    fid = frame_id.encode()
    head = struct.pack("<III", seq, stamp_ns // 1_000_000_000, stamp_ns % 1_000_000_000) + struct.pack("<I", len(fid)) + fid
    head += struct.pack("<III", height, width, len(ev))
    wire = np.zeros(len(ev), dtype=np.dtype([("x", "<u2"), ("y", "<u2"), ("sec", "<u4"), ("nsec", "<u4"), ("polarity", "u1")]))
    for f in ("x", "y", "sec", "nsec", "polarity"):
        wire[f] = ev[f]
    assert wire.dtype.itemsize == 13
    return head + wire.tobytes()


# ---- event-to-event matching (esvo_em_* of include/esvo_hip.h)
class EmParamsStruct(C.Structure):
    _fields_ = [
        ("slice_thickness", C.c_double), ("time_threshold", C.c_double), ("epipolar_threshold", C.c_double),
        ("ncc_threshold", C.c_double), ("num_event_matching", C.c_int32), ("patch_intensity_threshold", C.c_int32),
        ("patch_valid_ratio", C.c_double),
    ]


class EmSelectionStruct(C.Structure):
    _fields_ = [
        ("t_low_ns", C.c_uint64), ("t_up_ns", C.c_uint64), ("left_first", C.c_uint64), ("right_first", C.c_uint64),
        ("left_count", C.c_uint32), ("right_count", C.c_uint32), ("n_slices", C.c_uint32), ("pad_", C.c_uint32),
    ]


class EmStatsStruct(C.Structure):
    _fields_ = [
        ("events", C.c_uint64), ("right_events", C.c_uint64), ("time_polarity", C.c_uint64), ("epipolar", C.c_uint64),
        ("patch_ok", C.c_uint64), ("matches", C.c_uint64), ("slices", C.c_uint64), ("ms_match", C.c_float), ("pad_", C.c_float),
    ]


# ---- the scale-loop guard of the LM refinement (esvo_lm_stats_t of include/esvo_hip.h)
LM_SCALE_COUNT_ONLY = 2 ** 31 - 1   # ESVO_LM_SCALE_COUNT_ONLY: ParamsStruct.lm_scale_pass_limit that counts and never abandons


class LmStatsStruct(C.Structure):
    _fields_ = [
        ("enabled", C.c_uint32), ("last_max_passes_eval", C.c_uint32), ("last_max_passes_match", C.c_uint32), ("last_abandoned", C.c_uint32),
        ("last_passes", C.c_uint64), ("last_evals", C.c_uint64), ("last_shortcut_evals", C.c_uint64),
        ("total_passes", C.c_uint64), ("total_evals", C.c_uint64), ("total_shortcut_evals", C.c_uint64), ("total_abandoned", C.c_uint64),
    ]


# ---- semi-global matching per tick (esvo_sgm_* of include/esvo_hip.h)
class SgmStatsStruct(C.Structure):
    _fields_ = [
        ("events", C.c_uint64), ("on_image", C.c_uint64), ("matched_columns", C.c_uint64), ("disp_ok", C.c_uint64),
        ("points", C.c_uint64), ("zero_disp", C.c_uint64), ("ms_sgbm", C.c_float), ("ms_points", C.c_float),
        ("ms_propagate", C.c_float), ("pad_", C.c_float),
    ]


# ---- the global point cloud (esvo_map_gpc_* of include/esvo_hip.h)
class GpcParamsStruct(C.Structure):
    _fields_ = [
        ("visualize_range", C.c_double), ("interval_s", C.c_double), ("num_added_per_refresh", C.c_uint64),
        ("capacity_points", C.c_uint64), ("leaf", C.c_float), ("reserved", C.c_uint32),
    ]


class GpcStatsStruct(C.Structure):
    _fields_ = [
        ("updates", C.c_uint64), ("refreshes", C.c_uint64), ("total_points", C.c_uint64),
        ("last_near", C.c_uint32), ("last_voxels", C.c_uint32), ("last_added", C.c_uint32), ("last_refreshed", C.c_uint32),
        ("t_last_pub", C.c_double), ("ms_last", C.c_float), ("pad", C.c_uint32),
    ]


# ---- the tracker's registration loop (esvo_track_solve of include/esvo_hip.h)
TRACK_SOLVE_MAX_ITERATIONS = 64


class TrackSolveParamsStruct(C.Structure):
    _fields_ = [
        ("n_points", C.c_uint64), ("batch_size", C.c_uint64), ("ls_norm", C.c_int32), ("max_iterations", C.c_int32),
        ("on_device", C.c_int32), ("reserved", C.c_int32), ("huber_threshold", C.c_double), ("damping", C.c_double),
    ]


class TrackIterStruct(C.Structure):
    _fields_ = [
        ("cost", C.c_double), ("lambda_", C.c_double), ("step_norm", C.c_double), ("n", C.c_uint32), ("offset", C.c_uint32),
        ("pick", C.c_int32), ("trials", C.c_int32),
    ]


class TrackSolveInfoStruct(C.Structure):
    _fields_ = [("rms", C.c_double), ("iterations", C.c_int32), ("ok", C.c_int32), ("stop", C.c_int32), ("launches", C.c_int32)]


# esvo_track_iter_t as a record array: what Esvo.track_solve returns its trace in
TRACK_ITER_DTYPE = np.dtype([("cost", "<f8"), ("lambda", "<f8"), ("step_norm", "<f8"), ("n", "<u4"), ("offset", "<u4"),
                             ("pick", "<i4"), ("trials", "<i4")])
assert TRACK_ITER_DTYPE.itemsize == C.sizeof(TrackIterStruct) == 40


# the pose callback of esvo_map_tick_em: int (*)(void* user, uint64_t t_ns, double T_world_cam[16])
EM_POSE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_double))
