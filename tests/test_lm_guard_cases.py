"""The scale-loop guard of the LM refinement on the CPU: the crafted cases of tests/lm_cases.py really have the pass counts the GPU
tests (tests/test_gpu_lm_guard.py) rely on -- per evaluation from the restated evaluator, per match over the evaluations the
restated solver visits (tests/lm_guard.py) -- and the bindings carry the new parameter, struct and calls.

Every limit used on the GPU stays at least MARGIN passes away from the per-match maxima that decide whether a match is abandoned,
except on solver_noise.  Where a limit meets a count on the way (solver_noise; the evaluations of the sparse cases that take 30 to
32 and 16 passes under the limits 32 and 16) the loop in question ends on the 5 % test, and none of any case ends within
test_lm_cases.STOP_MARGIN of it (test_no_scale_loop_is_decided_on_its_threshold): such a count does not depend on the order a
patch sum is taken in, and `passes == limit` on a loop that is done is not over the limit."""
import ctypes as C

import pytest

import lm_cases as LC
import lm_guard as G
from esvo_amd import abi, lib

MARGIN = 8


def test_solver_noise_counts():
    assert G.maxima("solver_noise") == [5, 6, 8, 7, 7, 7, 0, 0, 0]
    assert all(not sc for ev in G.evaluations("solver_noise")[:6] for p, sc, _ in ev if p)
    assert G.abandoned("solver_noise", 8) == set()
    assert G.abandoned("solver_noise", 7) == {2}
    assert G.abandoned("solver_noise", 6) == {2, 3, 4, 5}
    # the loops that decide end on the 5 % test, not on sum == 0: `passes == limit` is then a loop that is done
    assert not any(on_zero for ev in G.evaluations("solver_noise") for _, _, on_zero in ev)


@pytest.mark.parametrize("name,about", [("blob1", 500), ("blob8", 1960), ("blob100", 2550)])
def test_blob_counts(name, about):
    mx = G.maxima(name)
    assert all(abs(m - about) <= 0.02 * about for m in mx[:2]) and mx[2:] == [0, 0, 0], mx
    assert G.abandoned(name, 64) == {0, 1}


def test_sparse_counts():
    above, at = LC.observe("sparse_above")[0], LC.observe("sparse_at")[0]
    assert G.maxima("sparse_above") == [48, 0, 0, 0]
    assert max(e["iters"] for _, _, e in above["evals"] if e["shortcut"]) == 7395   # literal passes of what the device takes for granted
    assert G.abandoned("sparse_above", 64) == set() and G.abandoned("sparse_above", 32) == {0}
    assert all(e["shortcut"] or not e["ok"] for _, _, e in at["evals"])
    assert G.maxima("sparse_at") == [0, 0, 0, 0] and G.abandoned("sparse_at", 1) == set()


def test_general_patch_counts():
    mx = G.maxima("any5x5_blob")
    assert mx[0] == 0 and abs(mx[1] - 1016) <= 20 and mx[2:] == [0, 0, 0], mx
    assert any(sc for _, sc, _ in G.evaluations("any5x5_blob")[0])
    mx = G.maxima("any25x25_blob")
    assert all(abs(m - 346) <= 7 for m in mx[:2]) and mx[2:] == [0, 0, 0], mx
    assert G.maxima("any5x5_sparse_above") == [40, 0, 0, 0]


@pytest.mark.parametrize("name,limit,gone", G.WIDE_LIMITS + G.ANY_LIMITS)
def test_limits_abandon_what_the_gpu_tests_expect_and_keep_their_distance(name, limit, gone):
    assert G.abandoned(name, limit) == gone
    assert G.counters(name, limit)["last_abandoned"] == len(gone)
    if name != "solver_noise":   # (a maximum of 0 is a match no loop of which ever runs -- sparse_at under the limit 1 -- not a count)
        assert all(abs(m - limit) >= MARGIN for m in G.maxima(name) if m), (name, limit, G.maxima(name))
    # a count that meets the limit belongs to a loop the 5 % test ended: not over, whatever order the sums are taken in
    assert not any(p == limit and on_zero for ev in G.evaluations(name) for p, _, on_zero in ev)


def test_count_only_abandons_nothing_and_counts_everything():
    for name in ("solver_noise", "blob1", "sparse_above"):
        pm = G.per_match(name, G.COUNT_ONLY)
        assert not any(d["abandoned"] for d in pm)
        assert [d["evals"] for d in pm] == [len(ev) for ev in G.evaluations(name)]
        assert [d["passes"] for d in pm] == [sum(p for p, _, _ in ev) for ev in G.evaluations(name)]


# ---- the bindings ------------------------------------------------------------------------------------------------------------------
def test_params_struct_keeps_its_size_and_the_limit_sits_where_the_pad_was():
    assert C.sizeof(abi.ParamsStruct) == lib.abi_sizes()[2]
    f = abi.ParamsStruct.lm_scale_pass_limit
    assert f.size == 4 and f.offset == abi.ParamsStruct.max_event_queue_len.offset + 4
    assert abi.ParamsStruct._fields_[-1][0] == "lm_scale_pass_limit" and not hasattr(abi.ParamsStruct, "pad_params_")
    assert C.sizeof(abi.ParamsStruct) == f.offset + 4   # the last four bytes of the struct, as the pad was


def test_lm_sizes_and_abi_version():
    assert lib.lm_sizes() == [C.sizeof(abi.LmStatsStruct), abi.LM_SCALE_COUNT_ONLY, 0, 0]
    assert abi.LM_SCALE_COUNT_ONLY == 2 ** 31 - 1
    assert lib.abi_sizes()[7] == 8
    assert {"esvo_map_lm_stats", "esvo_lm_sizes"} <= set(lib.SYMBOLS)


def test_default_params_leave_the_guard_off():
    p = abi.ParamsStruct()
    p.lm_scale_pass_limit = 5
    lib.load().esvo_default_params(C.byref(p))
    assert p.lm_scale_pass_limit == 0
    assert LC.case_params(LC.case("zero")).lm_scale_pass_limit == 0


@pytest.mark.parametrize("limit", [-1, -(2 ** 31)])
def test_negative_limits_are_refused(limit):
    """validate_params runs before esvo_create touches a device: the refusal needs no GPU"""
    with pytest.raises(lib.EsvoError) as e:
        lib.Esvo(LC.case_params(LC.case("zero"), lm_scale_pass_limit=limit), LC.rig()).close()
    assert "lm_scale_pass_limit" in str(e.value)
