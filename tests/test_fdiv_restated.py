"""CPU tests of what tests/test_gpu_primitives.py leans on: the numpy restatement of fdiv.hpp's windows (tests/fdiv_restated.py) on
hand-computed cases, the argument checks of the esvo_debug_* bindings, and the host-side predicates of scan.hip.  No GPU needed:
every refusal here happens before the first device call."""
import ctypes as C
import math

import numpy as np
import pytest

import fdiv_restated as F
from esvo_amd import abi, lib

P2 = lambda k: math.ldexp(1.0, k)           # noqa: E731
BELOW = lambda x: np.nextafter(x, 0.0)      # noqa: E731
DENORMAL = 5e-324


def _f(*v):
    return np.array(v, np.float64)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_fields_of_hand_written_numbers():
    assert list(F.exponent(_f(1.0, 2.0, 0.5, 0.0, DENORMAL, np.inf, np.nan, P2(-332), P2(333)))) == [1023, 1024, 1022, 0, 0, 2047, 2047, 691, 1356]
    assert F.from_bits(0, 1023, 0)[()] == 1.0 and F.from_bits(1, 1024, 1 << 51)[()] == -3.0
    assert F.from_bits(0, 691, 0)[()] == P2(-332) and F.from_bits(0, 1355, (1 << 52) - 1)[()] == BELOW(P2(333))


def test_window_edges_by_hand():
    # biased exponent 690 = [2^-333, 2^-332): out.  691 = 2^-332: in.  1355 = up to just below 2^333: in.  1356 = 2^333: out.
    v = _f(P2(-333), BELOW(P2(-332)), P2(-332), -P2(-332), 1.0, BELOW(P2(333)), -BELOW(P2(333)), P2(333), -P2(333))
    assert list(F.in_window(v)) == [False, False, True, True, True, True, True, False, False]
    assert list(F.recip_fast(v)) == list(F.in_window(v))
    assert list(F.fdiv_ok(v)) == list(F.in_window(v))


def test_positive_zero_is_a_numerator_but_no_divisor():
    v = _f(0.0, -0.0, DENORMAL, -DENORMAL, np.inf, -np.inf, np.nan)
    assert list(F.fdiv_ok(v)) == [True, False, False, False, False, False, False]   # -0 / b keeps its sign only on the plain path
    assert not F.recip_fast(v).any()


def test_b4_by_hand():
    one = _f(1.0)

    def b4(b=1.0, a1=1.0, a2=1.0, a3=1.0, a4=1.0):
        return bool(F.fdiv_ok_b4(_f(b), _f(a1), _f(a2), _f(a3), _f(a4))[0])
    assert b4()
    assert b4(a2=0.0) and not b4(a2=-0.0)                   # the one numerator that may be zero: +0
    assert not b4(a1=0.0) and not b4(a3=0.0) and not b4(a4=-0.0) and not b4(b=0.0)
    assert not b4(a2=DENORMAL) and not b4(a2=np.nan) and not b4(a2=np.inf)
    for k in ("b", "a1", "a2", "a3", "a4"):
        assert b4(**{k: P2(-332)}) and b4(**{k: -BELOW(P2(333))}), k
        assert not b4(**{k: P2(-333)}) and not b4(**{k: BELOW(P2(-332))}) and not b4(**{k: P2(333)}), k
    assert F.fdiv_ok_b4(one, one, one, one, one).dtype == np.bool_


def test_b4_acceptance_implies_every_single_test():
    rng = np.random.default_rng(7)
    ops = [F.edge_operands(rng, F.DIV_EXPONENTS)[rng.integers(0, 1632, 20000)] for _ in range(5)]
    ok = F.fdiv_ok_b4(*ops)
    assert ok.any() and not ok.all()
    assert F.recip_fast(ops[0])[ok].all() and all(F.fdiv_ok(a)[ok].all() for a in ops[1:])


def test_same_bits_tells_zeros_apart_and_nans_not():
    assert list(F.same_bits(_f(0.0, np.nan, 1.0), _f(-0.0, -np.nan, 1.0))) == [False, True, True]


def test_operand_sets_have_the_stated_shape():
    rng = np.random.default_rng(1)
    ops = F.edge_operands(rng, F.DIV_EXPONENTS)
    assert len(ops) == 12 * 68 * 2 and set(F.exponent(ops)) == set(F.DIV_EXPONENTS)
    m = F.bits(ops) & F.MANT_MASK
    assert {0, (1 << 52) - 1, 1 << 51, 1} <= set(int(x) for x in m)
    assert np.signbit(ops).sum() == len(ops) // 2
    r = F.random_operands(rng, 4096, 600, 1450)
    assert F.exponent(r).min() == 600 and F.exponent(r).max() == 1450


# ---- scan.hip's host-side predicates (no device call) ------------------------------------------------------------------------
def test_scan_predicates_at_the_switch_points():
    P = lib.debug_scan_predicates
    assert [P(n)[1] for n in (0, 1, 10240, 10241)] == [False, True, True, False]          # scan_compact_is_small
    assert [P(n)[0] for n in (0, 1, 32767, 32768, 32769)] == [True, True, True, True, False]  # scan_is_small
    assert [P(n)[2] for n in (0, 1, 2048, 2049, 526336, 526341)] == [0, 1, 1, 2, 257, 258]  # scan_tiles: 2048 elements each
    assert all(P(n)[3] == P(n)[2] + 1 for n in (0, 1, 2048, 2049, 1050629))              # scan_scratch_elems


# ---- the bindings refuse what the kernels would trust ------------------------------------------------------------------------
def test_bindings_check_types_and_lengths():
    u32, f64 = np.zeros(4, np.uint32), np.zeros(4, np.float64)
    with pytest.raises(ValueError):
        lib.debug_scan_u32(np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        lib.debug_scan_u32(np.zeros((2, 2), np.uint32))
    with pytest.raises(ValueError):
        lib.debug_scan_code_bit0(u32)
    with pytest.raises(ValueError):
        lib.debug_scan_code_bit0(np.zeros(8, np.uint8), zero_words=7)
    with pytest.raises(ValueError, match="single-workgroup"):
        lib.debug_scan_code_bit0(np.zeros(32768, np.uint8), tile_sums=np.zeros(16, np.uint32))
    with pytest.raises(ValueError):
        lib.debug_scan_code_bit0(np.zeros(32769, np.uint8), tile_sums=np.zeros(16, np.uint32))   # 17 tiles
    with pytest.raises(ValueError):
        lib.debug_fdiv(f64, f64[:3])
    with pytest.raises(ValueError):
        lib.debug_fdiv(f64.astype(np.float32), f64)
    with pytest.raises(ValueError):
        lib.debug_fdiv_b4(f64, f64, f64, f64[:2], f64)
    with pytest.raises(ValueError):
        lib.debug_sqrt_moderate(u32)
    with pytest.raises(ValueError):
        lib.debug_upload_words(u32, zero_words=300, n_zero=257)
    with pytest.raises(ValueError):
        lib.debug_upload_words(u32, zero_words=None, n_zero=1)
    with pytest.raises(ValueError):
        lib.debug_back_prologue(u32, f64, np.zeros(2, np.uint64))
    with pytest.raises(ValueError):
        lib.debug_back_prologue(u32, np.zeros(2, np.uint64), np.zeros(2, np.uint64), a_prefix=u32)


def test_compaction_bindings_check_size_and_flag_contract():
    for dtype, fn in ((abi.MATCH_DTYPE, lib.debug_compact_matches), (abi.DEPTH_POINT_DTYPE, lib.debug_compact_points)):
        with pytest.raises(ValueError, match="SCAN_COMPACT_SMALL_MAX"):
            fn(np.zeros(0, np.uint32), np.zeros(0, dtype))
        with pytest.raises(ValueError, match="SCAN_COMPACT_SMALL_MAX"):
            fn(np.zeros(10241, np.uint32), np.zeros(10241, dtype))
        with pytest.raises(ValueError, match="0 or 1"):
            fn(np.array([0, 2], np.uint32), np.zeros(2, dtype))
        with pytest.raises(ValueError):
            fn(np.zeros(3, np.uint32), np.zeros(2, dtype))
    with pytest.raises(ValueError):
        lib.debug_compact_points(np.zeros(2, np.uint32), np.zeros(2, abi.MATCH_DTYPE))
    with pytest.raises(ValueError):
        lib.debug_compact_points(np.zeros(2, np.uint32), np.zeros(2, abi.DEPTH_POINT_DTYPE), pinned_row=True)
    with pytest.raises(ValueError):
        lib.debug_compact_points(np.zeros(2, np.uint32), np.zeros(2, abi.DEPTH_POINT_DTYPE), row=np.zeros(4, np.uint32), total_index=4)
    pts = np.zeros(3, abi.DEPTH_POINT_DTYPE)
    with pytest.raises(ValueError, match="outside"):
        lib.debug_back_prologue(np.zeros(0, np.uint32), pts, np.zeros(0, np.uint64), a_flags=np.ones(3, np.uint32),
                                a_prefix=np.array([0, 1, 3], np.uint32))


def test_c_entries_refuse_bad_arguments_before_any_device_call():
    so = lib.load()
    one = (C.c_uint32 * 1)()
    f = so.esvo_debug_compact_matches
    f.argtypes, f.restype = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5, C.c_int
    assert f(None, 1, None, None, None, None, None) == abi.ERR_INVALID_ARG
    assert f(one, 0, one, one, one, None, None) == abi.ERR_INVALID_ARG          # n = 0 and n = 10241 are the parallel path's
    assert f(one, 10241, one, one, one, None, None) == abi.ERR_INVALID_ARG
    g = so.esvo_debug_scan_code_bit0
    g.argtypes, g.restype = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t], C.c_int
    assert g(one, 4, one, one, None, None, 0) == abi.ERR_INVALID_ARG            # the down-sweep alone at a single-workgroup size
    assert g(one, 4, None, one, None, one, 3) == abi.ERR_INVALID_ARG            # a zero buffer shorter than n
    u = so.esvo_debug_upload_words
    u.argtypes, u.restype = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32], C.c_int
    assert u(one, 3, one, None, 0, 0) == abi.ERR_INVALID_ARG                    # not whole words
    assert u(one, 4, one, one, 300, 257) == abi.ERR_INVALID_ARG
    p = so.esvo_debug_scan_predicates
    p.argtypes, p.restype = [C.c_size_t, C.c_void_p], C.c_int
    assert p(1, None) == abi.ERR_INVALID_ARG
