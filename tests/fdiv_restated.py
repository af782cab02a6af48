"""The window tests of esvo_amd/csrc/fdiv.hpp restated in numpy from the exponent bits, exactly as that header's comments define
them, and the operand sets tests/test_gpu_primitives.py feeds the device with.  Plain numpy, no GPU.

    window        biased exponent in [691, 1355], i.e. |v| in [2^-332, 2^333)
    fdiv_ok(v)    v == +0, or v inside the window (a negative zero is refused: div_fast would lose its sign)
    Recip.fast    the divisor inside the window
    fdiv_ok_b4    b, a1, a3, a4 inside the window, a2 inside it or +0
"""
import numpy as np

WINDOW_LO, WINDOW_HI = 691, 1355     # biased exponents, both inside
MANT_MASK = np.uint64((1 << 52) - 1)


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def from_bits(sign, exponent, mantissa):
    """float64 from its three fields (arrays broadcast against each other)"""
    s, e, m = np.broadcast_arrays(np.asarray(sign, np.uint64), np.asarray(exponent, np.uint64), np.asarray(mantissa, np.uint64))
    assert int(e.max(initial=0)) <= 2047 and int(m.max(initial=0)) <= int(MANT_MASK) and int(s.max(initial=0)) <= 1
    return ((s << np.uint64(63)) | (e << np.uint64(52)) | m).view(np.float64)


def exponent(v):
    return ((bits(v) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)


def in_window(v):
    e = exponent(v)
    return (e >= WINDOW_LO) & (e <= WINDOW_HI)


def is_zero(v):
    """+0 alone: every bit clear"""
    return bits(v) == 0


def fdiv_ok(v):
    return in_window(v) | is_zero(v)


def recip_fast(b):
    return in_window(b)


def fdiv_ok_b4(b, a1, a2, a3, a4):
    return in_window(b) & in_window(a1) & (in_window(a2) | is_zero(a2)) & in_window(a3) & in_window(a4)


def same_bits(x, y):
    """bit for bit, two NaNs counting as equal whatever their payload"""
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    return (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))


# ---- operand sets ------------------------------------------------------------------------------------------------------------
DIV_EXPONENTS = (0, 1, 690, 691, 692, 1022, 1023, 1354, 1355, 1356, 2046, 2047)
SQRT_EXPONENTS = (323, 324, 1022, 1023, 1024, 1722, 1723)   # 2^-700 .. 2^700


def mantissas(rng, n_random=64):
    special = np.array([0, int(MANT_MASK), 0x8000000000000, 1], np.uint64)
    return np.concatenate([special, rng.integers(0, 1 << 52, n_random, dtype=np.uint64)])


def edge_operands(rng, exponents, signs=(0, 1)):
    """every exponent x every mantissa of mantissas() x every sign"""
    m = mantissas(rng)
    e = np.asarray(exponents, np.uint64)
    s = np.asarray(signs, np.uint64)
    return from_bits(s[:, None, None], e[None, :, None], m[None, None, :]).reshape(-1).copy()


def random_operands(rng, n, e_lo, e_hi, signed=True):
    """n operands with the biased exponent uniform in [e_lo, e_hi], random mantissa (and sign)"""
    return from_bits(rng.integers(0, 2, n, dtype=np.uint64) if signed else np.uint64(0),
                     rng.integers(e_lo, e_hi + 1, n, dtype=np.uint64), rng.integers(0, 1 << 52, n, dtype=np.uint64)).copy()
