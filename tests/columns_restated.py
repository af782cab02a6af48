"""The column conversion of esvo_ts_push_event_columns (include/esvo_hip.h) restated in Python integers, one element at a time:
no numpy arithmetic, so nothing can wrap.  tests/test_event_columns.py holds the library's C conversion and the numpy one of
esvo_amd.abi to it byte for byte; tests/test_gpu_event_columns.py builds its expected records with it."""
import numpy as np

from esvo_amd import abi

STAMP_END = 2 ** 32 * 10 ** 9
UNIT = {abi.T_NS_I64: 1, abi.T_US_I64: 1000, abi.T_US_U32: 1000}
T_DTYPE = {abi.T_NS_I64: np.int64, abi.T_US_I64: np.int64, abi.T_US_U32: np.uint32}
T_UNIT = {abi.T_NS_I64: "ns", abi.T_US_I64: "us", abi.T_US_U32: "us"}
P_DTYPE = {abi.P_U8: np.uint8, abi.P_I8: np.int8}


def stamp_ns(t, t_offset, t_type):
    """(t + t_offset) * unit as a Python int, or None where it is not in [0, 2^32 * 10^9)"""
    s = (int(t) + int(t_offset)) * UNIT[t_type]
    return s if 0 <= s < STAMP_END else None


def polarity(p, p_type):
    """p: the column's BYTE (0..255), or None for a missing column"""
    if p is None:
        return 1
    p = int(p) & 0xff
    if p_type == abi.P_I8:
        return 1 if 0 < p < 128 else 0
    return 1 if p else 0


def columns_to_events(x, y, t, p, t_type, p_type, t_offset):
    """-> (records, first_bad): the esvo_event_t records of the elements before the first invalid one, and its index (None: all valid)"""
    out = np.zeros(len(t), abi.EVENT_DTYPE)
    raw = out.view(np.uint8).reshape(len(t), 16)
    for i in range(len(t)):
        s = stamp_ns(t[i], t_offset, t_type)
        if s is None:
            return out[:i], i
        words = [(int(x[i]) & 0xffff) | ((int(y[i]) & 0xffff) << 16), s // 10 ** 9, s % 10 ** 9, polarity(None if p is None else p[i], p_type)]
        raw[i] = np.frombuffer(b"".join(int(w).to_bytes(4, "little") for w in words), np.uint8)
    return out, None
