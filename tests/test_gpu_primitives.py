"""The shared device primitives called by name, one launch at a time, through the esvo_debug_* entries (esvo_amd/csrc/api_dev.hip):
the exclusive scans of scan.hip in both forms, the down-sweep alone, the fused scan + stable compaction, upload_words_kernel,
back_prologue_kernel, and the shared-divisor division and square root of fdiv.hpp.

Every comparison is EXACT -- integers, copied bytes, IEEE-754 bits (two NaNs count as equal) -- and every call must report zero
disturbed guard words: each buffer a kernel may write has exactly the production size and sits between guard words on the device.
Output buffers start filled with lib.DEBUG_PREFILL_BYTE, so "not written" and "written as zero" differ.

References: numpy.cumsum in uint64 reduced mod 2^32 (scan), records[flags != 0] (compaction), numpy float64 / and sqrt (division).
The sizes are the switch points of scan.hip: SCAN_SMALL_MAX = 32768, SCAN_COMPACT_SMALL_MAX = 10240, the 8192-element tile of the
one-workgroup kernels, the 2048-element tile of the two-launch path, and more than 256 tiles (n > 524288), where the loop that adds
up the sums of the tiles in front takes a second pass.
"""
import numpy as np
import pytest

import fdiv_restated as F
from esvo_amd import abi, lib

pytestmark = pytest.mark.gpu

PRE = lib.DEBUG_PREFILL_U32
TILE = 2048
SCAN_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 32767, 32768, 32769, 34816, 34817, 526336, 526341,
              1050629)
SCAN_DOWN_SIZES = tuple(n for n in SCAN_SIZES if n > 32768)   # launch_scan_down_code_bit0's contract
COMPACT_SIZES = (1, 2, 8191, 8192, 8193, 10239, 10240)


def _exclusive(x):
    """(exclusive prefix sums mod 2^32, total mod 2^32) of an integer array, summed in uint64"""
    cs = np.cumsum(x.astype(np.uint64), dtype=np.uint64)
    ex = np.empty(len(x), np.uint64)
    if len(x):
        ex[0] = 0
        ex[1:] = cs[:-1]
    return ex.astype(np.uint32), int(cs[-1]) & 0xffffffff if len(x) else 0


def _single_one_positions(n):
    """index 0, n - 1, and the first and last element of every 2048-tile"""
    if n == 0:
        return []
    first = np.arange(0, n, TILE)
    return sorted(set([0, n - 1]) | set(first.tolist()) | set(np.minimum(first + TILE - 1, n - 1).tolist()))


def _scan_inputs(n, seed):
    """name -> uint32 input: all zero, all one, random 0 / 1 at densities 0.01 and 0.5, random full-range words (the sums wrap)"""
    rng = np.random.default_rng(seed)
    return {
        "zeros": np.zeros(n, np.uint32),
        "ones": np.ones(n, np.uint32),
        "density_0.01": (rng.random(n) < 0.01).astype(np.uint32),
        "density_0.5": (rng.random(n) < 0.5).astype(np.uint32),
        "full_range": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
    }


def _check_scan_u32(x, what):
    ref, ref_total = _exclusive(x)
    out, total, g = lib.debug_scan_u32(x)
    assert g == 0, (what, g)
    assert total == ref_total, (what, total, ref_total)
    assert np.array_equal(out, ref), (what, int(np.flatnonzero(out != ref)[0]))
    out_ip, total_ip, g = lib.debug_scan_u32(x, in_place=True)           # d_out == d_in (api_em.hip)
    assert g == 0 and total_ip == ref_total and np.array_equal(out_ip, out), what
    out_nt, none, g = lib.debug_scan_u32(x, want_total=False)             # total == nullptr: nothing else changes
    assert g == 0 and none is None and np.array_equal(out_nt, out), what
    out_nt, none, g = lib.debug_scan_u32(x, in_place=True, want_total=False)
    assert g == 0 and np.array_equal(out_nt, out), what


def _check_scan_code(codes, what, tile_sums=None):
    """the code-bit0 form (or, with tile_sums, its down-sweep alone): out, total, the cleared words, and each argument left out"""
    n = len(codes)
    ref, ref_total = _exclusive(codes & 1)
    out, total, zero, g = lib.debug_scan_code_bit0(codes, tile_sums=tile_sums, zero_words=n + 37)
    assert g == 0, (what, g)
    assert total == ref_total, (what, total, ref_total)
    assert np.array_equal(out, ref), (what, int(np.flatnonzero(out != ref)[0]))
    assert not zero[:n].any() and (zero[n:] == PRE).all(), what          # zero[0:n] cleared, zero[n:] untouched
    out2, total2, zero2, g = lib.debug_scan_code_bit0(codes, tile_sums=tile_sums)   # zero == nullptr
    assert g == 0 and zero2 is None and total2 == ref_total and np.array_equal(out2, out), what
    out3, none, zero3, g = lib.debug_scan_code_bit0(codes, tile_sums=tile_sums, want_total=False, zero_words=n)
    assert g == 0 and none is None and np.array_equal(out3, out) and not zero3.any(), what


def _junk_high_bits(flags, rng):
    """one byte per element: bit 0 is the flag, bits 1..7 random (the scan must ignore them)"""
    return (flags.astype(np.uint8) | (rng.integers(0, 128, len(flags), dtype=np.uint8) << 1)).astype(np.uint8)


# ---- the exclusive scan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan_u32(n):
    for name, x in _scan_inputs(n, 1000 + n).items():
        _check_scan_u32(x, (n, name))


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan_code_bit0(n):
    rng = np.random.default_rng(2000 + n)
    for name, x in _scan_inputs(n, 3000 + n).items():
        bit = (x & 1).astype(np.uint8)
        _check_scan_code(bit, (n, name, "clean"))
        _check_scan_code(_junk_high_bits(bit, rng), (n, name, "bits 1..7 set"))


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan_of_a_single_one(n):
    """a single 1 at index 0, at n - 1, and at the first and last element of every 2048-tile: a carry dropped at any seam shows"""
    x = np.zeros(n, np.uint32)
    codes = np.full(n, 0xfe, np.uint8)
    positions = _single_one_positions(n)
    for p in positions:
        x[p] = 1
        out, total, g = lib.debug_scan_u32(x)
        x[p] = 0
        assert g == 0 and total == 1, (n, p, total, g)
        assert not out[:p + 1].any() and (out[p + 1:] == 1).all(), (n, p)
        codes[p] = 0xff
        out, total, _, g = lib.debug_scan_code_bit0(codes)
        codes[p] = 0xfe
        assert g == 0 and total == 1, (n, p, total, g)
        assert not out[:p + 1].any() and (out[p + 1:] == 1).all(), (n, p)


def test_scan_of_nothing_writes_the_total_only():
    out, total, g = lib.debug_scan_u32(np.zeros(0, np.uint32))
    assert (len(out), total, g) == (0, 0, 0)
    out, total, g = lib.debug_scan_u32(np.zeros(0, np.uint32), want_total=False)
    assert (len(out), total, g) == (0, None, 0)
    out, total, zero, g = lib.debug_scan_code_bit0(np.zeros(0, np.uint8), zero_words=37)
    assert (len(out), total, g) == (0, 0, 0) and (zero == PRE).all()


@pytest.mark.parametrize("n", SCAN_DOWN_SIZES)
def test_scan_down_alone_on_the_callers_tile_sums(n):
    """launch_scan_down_code_bit0 (the band mode's frame order): the tile sums come from another kernel -- here from numpy, at
    exact multiples of the tile and at ragged n.  Called only above the single-workgroup bound, which is its contract."""
    assert not lib.debug_scan_predicates(n)[0] and lib.debug_scan_predicates(n)[2] == -(-n // TILE)
    rng = np.random.default_rng(4000 + n)
    for name, x in _scan_inputs(n, 5000 + n).items():
        codes = _junk_high_bits(x & 1, rng)
        padded = np.zeros(-(-n // TILE) * TILE, np.uint32)
        padded[:n] = codes & 1
        sums = padded.reshape(-1, TILE).sum(axis=1, dtype=np.uint64).astype(np.uint32)
        _check_scan_code(codes, (n, name, "down-sweep alone"), tile_sums=sums)
    codes = np.full(n, 0xfe, np.uint8)
    for p in _single_one_positions(n):     # one flag alone: index 0, n - 1, the first and last element of every tile
        codes[p] = 0xff
        sums = np.zeros(-(-n // TILE), np.uint32)
        sums[p // TILE] = 1
        out, total, _, g = lib.debug_scan_code_bit0(codes, tile_sums=sums)
        codes[p] = 0xfe
        assert g == 0 and total == 1 and not out[:p + 1].any() and (out[p + 1:] == 1).all(), (n, p)


def test_scan_predicates():
    P = lib.debug_scan_predicates
    assert [P(n)[1] for n in (0, 1, 10240, 10241)] == [False, True, True, False]
    assert [P(n)[0] for n in (32767, 32768, 32769)] == [True, True, False]
    for n in SCAN_SIZES:
        assert P(n)[2] == -(-n // TILE) and P(n)[3] == -(-n // TILE) + 1, n


# ---- scan + stable compaction in one workgroup --------------------------------------------------------------------------------
# The contract of these kernels is flags in {0, 1} (what block matching and the refinement write); the bindings refuse others.
def _records(n, dtype, rng):
    """records of random bytes, every byte of every field included (the dtypes have no padding: asserted below)"""
    return rng.integers(0, 256, n * dtype.itemsize, dtype=np.uint8).view(dtype)


def _bytes(rec):
    return np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), rec.dtype.itemsize)


def _flag_sets(n, rng):
    last = np.zeros(n, np.uint32)
    last[-1] = 1
    return {"none": np.zeros(n, np.uint32), "all": np.ones(n, np.uint32), "random": (rng.random(n) < 0.4).astype(np.uint32),
            "last only": last}


def test_record_layouts_match_the_library():
    s = lib.abi_sizes()
    assert s[3] == abi.MATCH_DTYPE.itemsize == 48 and s[4] == abi.DEPTH_POINT_DTYPE.itemsize == 104
    for dt in (abi.MATCH_DTYPE, abi.DEPTH_POINT_DTYPE):   # no padding: random bytes reach every byte of a record
        assert sum(dt.fields[k][0].itemsize for k in dt.names) == dt.itemsize
    assert abi.DEPTH_POINT_DTYPE.fields["seq"][1] == 100


@pytest.mark.parametrize("n", COMPACT_SIZES)
def test_compact_matches(n):
    rng = np.random.default_rng(6000 + n)
    slots = _records(n, abi.MATCH_DTYPE, rng)
    for name, flags in _flag_sets(n, rng).items():
        ref_prefix, ref_total = _exclusive(flags)
        src = np.flatnonzero(flags).astype(np.uint32)
        kept = _bytes(slots[flags != 0])
        for want_out, want_slot_of in ((True, True), (True, False), (False, True)):   # out + slot_of, out only, indices only
            r = lib.debug_compact_matches(flags, slots, want_out=want_out, want_slot_of=want_slot_of)
            what = (n, name, want_out, want_slot_of)
            assert r["guards"] == 0, (what, r["guards"])
            assert r["total"] == ref_total == len(src), what
            assert np.array_equal(r["prefix"], ref_prefix), what
            if want_out:
                assert np.array_equal(_bytes(r["out"][:ref_total]), kept), what          # byte-identical, in order
                assert (_bytes(r["out"][ref_total:]) == lib.DEBUG_PREFILL_BYTE).all(), what   # beyond total: untouched
            else:
                assert r["out"] is None
            if want_slot_of:
                assert np.array_equal(r["slot_of"][:ref_total], src), what
                assert (r["slot_of"][ref_total:] == PRE).all(), what
            else:
                assert r["slot_of"] is None


def _expected_points(slots, flags):
    kept = slots[flags != 0].copy()
    kept["seq"] = np.arange(len(kept), dtype=np.uint32)    # `seq` = the output position; every other byte unchanged
    return kept


@pytest.mark.parametrize("n", COMPACT_SIZES)
def test_compact_points(n):
    rng = np.random.default_rng(7000 + n)
    slots = _records(n, abi.DEPTH_POINT_DTYPE, rng)
    row_src = rng.integers(1, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)   # a tick's counter row: 64 words, n_points = word 1
    for name, flags in _flag_sets(n, rng).items():
        ref_prefix, ref_total = _exclusive(flags)
        expected = _bytes(_expected_points(slots, flags))
        row_after = row_src.copy()
        row_after[1] = ref_total
        for mode in ("alone", "row", "row + pinned row", "no out"):
            kw = {}
            if mode != "alone":
                kw.update(row=row_src, total_index=1, pinned_row=(mode != "row"))
            r = lib.debug_compact_points(flags, slots, want_out=(mode != "no out"), **kw)
            what = (n, name, mode)
            assert r["guards"] == 0, (what, r["guards"])
            assert r["total"] == ref_total, (what, r["total"], ref_total)
            assert np.array_equal(r["prefix"], ref_prefix), what
            if mode != "no out":
                assert np.array_equal(_bytes(r["out"][:ref_total]), expected), what
                assert (_bytes(r["out"][ref_total:]) == lib.DEBUG_PREFILL_BYTE).all(), what
            if mode != "alone":
                assert np.array_equal(r["row"], row_after), what                     # the device row: only the total changed
            if kw.get("pinned_row"):
                assert np.array_equal(r["row_host"], row_after), what                # the pinned row: row_src with the count in
            else:
                assert r["row_host"] is None


# ---- upload_words_kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", (0, 1, 65539))      # 65539 words: past the 256 x 256 grid, so the stride loop runs
@pytest.mark.parametrize("n_zero", (None, 0, 1, 256))
def test_upload_words(words, n_zero):
    rng = np.random.default_rng(8000 + words)
    src = rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
    dst, zero, g = lib.debug_upload_words(src, zero_words=None if n_zero is None else n_zero + 5, n_zero=n_zero or 0)
    assert g == 0
    assert np.array_equal(dst, src)
    if n_zero is None:
        assert zero is None
    else:
        assert not zero[:n_zero].any() and (zero[n_zero:] == PRE).all()


# ---- back_prologue_kernel -----------------------------------------------------------------------------------------------------
def _check_plain_prologue(n_src, n_a, n_b, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 1 << 32, n_src, dtype=np.uint64).astype(np.uint32)
    a, b = rng.integers(0, 1 << 63, n_a, dtype=np.uint64), rng.integers(0, 1 << 63, n_b, dtype=np.uint64)
    dst, a_dst, b_dst, g = lib.debug_back_prologue(src, a, b)
    assert g == 0, (n_src, n_a, n_b, g)
    assert np.array_equal(dst, src) and np.array_equal(a_dst, a) and np.array_equal(b_dst, b), (n_src, n_a, n_b)


@pytest.mark.parametrize("mask", range(8))
def test_back_prologue_plain_copies_each_empty_or_not(mask):
    _check_plain_prologue(7 if mask & 1 else 0, 13 * 5 if mask & 2 else 0, 257 if mask & 4 else 0, 9000 + mask)


@pytest.mark.parametrize("largest", range(3))
def test_back_prologue_grid_stride_loops(largest):
    """the largest copy exceeds 512 x 256 words: the grid is capped there and every loop strides"""
    sizes = [300, 11, 1029]
    sizes[largest] = 512 * 256 * 2 + 3
    _check_plain_prologue(*sizes, 9100 + largest)


@pytest.mark.parametrize("n", (8193, 2000))
def test_back_prologue_gather_equals_the_compaction(n):
    """gather mode: the stable compaction of the refinement's slots over the grid -- byte for byte what
    launch_scan_compact_points_small leaves from the same flags, and what numpy says"""
    rng = np.random.default_rng(9200 + n)
    slots = _records(n, abi.DEPTH_POINT_DTYPE, rng)
    flags = (rng.random(n) < 0.6).astype(np.uint32)
    comp = lib.debug_compact_points(flags, slots)
    ref_prefix, ref_total = _exclusive(flags)
    assert comp["guards"] == 0 and comp["total"] == ref_total and np.array_equal(comp["prefix"], ref_prefix)
    src = rng.integers(0, 1 << 32, 3 * 10 + 1, dtype=np.uint64).astype(np.uint32)      # the frame table: 3 nf + 1 words
    b = rng.integers(0, 1 << 63, 17 * 16, dtype=np.uint64)
    dst, a_dst, b_dst, g = lib.debug_back_prologue(src, slots, b, a_flags=flags, a_prefix=comp["prefix"])
    assert g == 0
    assert np.array_equal(dst, src) and np.array_equal(b_dst, b)
    assert np.array_equal(_bytes(a_dst[:ref_total]), _bytes(comp["out"][:ref_total]))
    assert np.array_equal(_bytes(a_dst[:ref_total]), _bytes(_expected_points(slots, flags)))
    assert (_bytes(a_dst[ref_total:]) == lib.DEBUG_PREFILL_BYTE).all()
    # the tick's other call (api_window.hip, flush_deferred_copies): the gather alone, nothing else to copy
    _, a_only, _, g = lib.debug_back_prologue(np.zeros(0, np.uint32), slots, np.zeros(0, np.uint64), a_flags=flags, a_prefix=comp["prefix"])
    assert g == 0 and np.array_equal(_bytes(a_only), _bytes(a_dst))


# ---- fdiv.hpp -----------------------------------------------------------------------------------------------------------------
def _quotient(a, b):
    with np.errstate(all="ignore"):
        return a / b


def _check_division(a, b, what):
    r = lib.debug_fdiv(a, b)
    assert r["guards"] == 0, what
    ok_a, fast = F.fdiv_ok(a), F.recip_fast(b)
    assert np.array_equal(r["ok_a"] != 0, ok_a), (what, "fdiv_ok")               # the device's decisions, on every operand
    assert np.array_equal(r["fast"] != 0, fast), (what, "make_recip().fast")
    ref = _quotient(a, b)
    bad = ~F.same_bits(r["div_by"], ref)
    assert not bad.any(), (what, "div_by", int(bad.sum()), a[bad][:4], b[bad][:4])
    pre = ok_a & fast                                                            # div_fast's precondition, restated
    for key in ("div_fast", "div_refined"):
        bad = pre & ~F.same_bits(r[key], ref)
        assert not bad.any(), (what, key, int(bad.sum()), a[bad][:4], b[bad][:4])
    return int(pre.sum())


def test_division_on_the_edge_operands():
    """biased exponents 0 (zero, denormals), 1, 690 | 691, 692, 1022, 1023, 1354, 1355 | 1356, 2046, 2047 (inf, NaN) x mantissas
    all-zeros, all-ones, 0x8000000000000, 1 and 64 random ones x both signs: every operand against every operand"""
    ops = F.edge_operands(np.random.default_rng(11), F.DIV_EXPONENTS)
    a, b = np.repeat(ops, len(ops)), np.tile(ops, len(ops))
    n_fast = _check_division(a, b, "edge x edge")
    assert n_fast == (6 * 68 * 2 + 1) * (6 * 68 * 2)      # numerators: six exponents inside the window, and +0


def test_division_on_random_pairs():
    rng = np.random.default_rng(12)
    n = 1 << 20
    a, b = F.random_operands(rng, n, 600, 1450), F.random_operands(rng, n, 600, 1450)
    n_fast = _check_division(a, b, "random pairs")
    assert 0.55 * n < n_fast < 0.67 * n       # (665 / 851)^2 = 0.61 of the pairs lie inside both windows


def test_refined_reciprocals_by_themselves():
    """recip_refined(b) and make_recip(b).y are the same three operations: bit-equal on every divisor inside the window.  And both
    are what two Newton steps leave: with y1 the value after the first step and e = 1 - b y1 (the inner fma, exact to 2^-53 e),
    the second step is the rounding of y1 (1 + e), whose error against 1 / b is e^2 -- below 2^-90, since v_rcp_f64 starts within
    2^-23 -- plus one rounding, 2^-53 relative: |b y - 1| < 2^-52.  One step alone leaves 2^-46.  Checked in exact rational
    arithmetic.  (Through a quotient this cannot be seen: div_fast's own correction hides a missing step on all but one pair in 2^40.)"""
    from fractions import Fraction
    rng = np.random.default_rng(17)
    edge = F.edge_operands(rng, F.DIV_EXPONENTS)
    b = np.concatenate([edge, F.random_operands(rng, 1 << 20, 600, 1450)])
    y_make, y_ref, g = lib.debug_recip(b)
    assert g == 0
    fast = F.recip_fast(b)
    assert fast.sum() > 800_000
    bad = fast & ~F.same_bits(y_make, y_ref)
    assert not bad.any(), (int(bad.sum()), b[bad][:4], y_make[bad][:4], y_ref[bad][:4])
    idx = np.flatnonzero(fast)
    idx = np.concatenate([idx[idx < len(edge)], idx[idx >= len(edge)][:2048]])     # every edge divisor inside the window + 2048 random
    bound = Fraction(1, 1 << 52)
    for name, y in (("make_recip", y_make), ("recip_refined", y_ref)):
        worst = max(abs(Fraction(float(b[i])) * Fraction(float(y[i])) - 1) for i in idx)
        assert worst < bound, (name, float(worst * (1 << 52)), "units of 2^-52")


def _check_b4(ops, what):
    b, a1, a2, a3, a4 = ops
    ok, q, g = lib.debug_fdiv_b4(b, a1, a2, a3, a4)
    assert g == 0, what
    ref_ok = F.fdiv_ok_b4(b, a1, a2, a3, a4)
    bad = (ok != 0) != ref_ok
    assert not bad.any(), (what, "fdiv_ok_b4", int(bad.sum()), [x[bad][:3] for x in ops])
    acc = ok != 0
    assert F.recip_fast(b)[acc].all() and all(F.fdiv_ok(x)[acc].all() for x in (a1, a2, a3, a4)), what   # acceptance implies each test
    for k, x in enumerate((a1, a2, a3, a4)):
        bad = acc & ~F.same_bits(q[:, k], _quotient(x, b))
        assert not bad.any(), (what, f"quotient {k + 1}", int(bad.sum()), x[bad][:4], b[bad][:4])
    return int(acc.sum())


def test_b4_with_one_operand_at_a_time_on_the_edges():
    """four operands well inside the window and the fifth walking the edge set, for each of the five positions: each bound of the
    window is decided by one operand alone"""
    rng = np.random.default_rng(13)
    edge = F.edge_operands(rng, F.DIV_EXPONENTS)
    accepted = 0
    for k in range(5):
        ops = [F.random_operands(rng, len(edge), 900, 1100) for _ in range(5)]
        ops[k] = edge
        n_acc = _check_b4(ops, f"operand {k} on the edges")
        assert n_acc == 6 * 68 * 2 + (1 if k == 2 else 0), (k, n_acc)     # a2 alone may be zero: +0
        accepted += n_acc
    assert accepted > 0


def test_b4_on_random_tuples():
    rng = np.random.default_rng(14)
    n = 1 << 20
    edge = F.edge_operands(rng, F.DIV_EXPONENTS)
    n_acc = _check_b4([edge[rng.integers(0, len(edge), n)] for _ in range(5)], "edge operands drawn at random")
    assert n_acc > n // 64                    # (1/2)^5 of the tuples, a little more with a2 = 0
    n_acc = _check_b4([F.random_operands(rng, n, 600, 1450) for _ in range(5)], "exponents uniform in [600, 1450]")
    assert n_acc > n // 8                     # (665 / 851)^5 = 0.29


def _check_sqrt(x, what):
    out, g = lib.debug_sqrt_moderate(x)
    assert g == 0, what
    bad = ~F.same_bits(out, np.sqrt(x))
    assert not bad.any(), (what, int(bad.sum()), x[bad][:4], out[bad][:4])


def test_sqrt_moderate_on_the_edge_operands():
    """biased exponents 323, 324 (2^-700), 1022, 1023, 1024, 1722, 1723 (2^700) x the mantissa set, positive"""
    _check_sqrt(F.edge_operands(np.random.default_rng(15), F.SQRT_EXPONENTS, signs=(0,)), "edges")


def test_sqrt_moderate_on_random_operands():
    rng = np.random.default_rng(16)
    x = F.random_operands(rng, 1 << 20, 323, 1722, signed=False)     # [2^-700, 2^700)
    x[:2] = (np.ldexp(1.0, -700), np.ldexp(1.0, 700))                # and the two ends themselves
    _check_sqrt(x, "random in [2^-700, 2^700]")
