"""What the scale-loop guard of the LM refinement (ParamsStruct.lm_scale_pass_limit, include/esvo_hip.h) must count and abandon
on the crafted cases of tests/lm_cases.py, derived on the CPU from lm_cases.observe -- the canonical oracle's residual function
driven through the restated solver, every evaluation point classified by the restated evaluator.

A pass is one completed update s2 = sum / N with a non-zero sum: the restated evaluator's `iters` (the oracle's own counter,
oracle/esvo_oracle.cpp:778).  An evaluation whose collapse the device takes for granted (`shortcut`) has 0 passes there, whatever
the literal loop needs; so has one that takes the failure fill.  The device does not compute NumericalDiff's second F(x) -- it
holds that vector -- so the evaluations counted are the trace's without its 'base' entries; a 'base' point repeats an earlier
point of the same match, so it can never be the first one over a limit."""
import functools

import numpy as np

import lm_cases as LC
from esvo_amd.abi import LM_SCALE_COUNT_ONLY

COUNT_ONLY = LM_SCALE_COUNT_ONLY
FIELDS = ("last_max_passes_eval", "last_max_passes_match", "last_passes", "last_evals", "last_shortcut_evals", "last_abandoned")


@functools.lru_cache(maxsize=None)
def evaluations(name):
    """per match of a case, per evaluation the device computes: (passes, shortcut, ended on sum == 0)"""
    out = []
    for o in LC.observe(name):
        out.append(tuple((0 if e["shortcut"] else int(e["iters"]), bool(e["shortcut"]), bool(e["on_zero"]) and not e["shortcut"])
                         for kind, _, e in o["evals"] if kind != "base"))
    return tuple(out)


def maxima(name):
    """per match the most passes of one evaluation"""
    return [max((p for p, _, _ in ev), default=0) for ev in evaluations(name)]


def _over(passes, on_zero, limit):
    """the evaluation completed `limit` passes and its loop test asked for another: it went on to a further pass, or to the
    sum == 0 that ends the loop without one"""
    return passes > limit or (passes == limit and on_zero)


@functools.lru_cache(maxsize=None)
def per_match(name, limit):
    """per match: dict(abandoned, evals, passes, max_eval, shortcut) under a limit (COUNT_ONLY: nothing is abandoned).  The
    evaluation that abandons a match is its last one and counts `limit` passes."""
    out = []
    for ev in evaluations(name):
        d = dict(abandoned=False, evals=0, passes=0, max_eval=0, shortcut=0)
        for p, sc, on_zero in ev:
            d["evals"] += 1
            d["shortcut"] += int(sc)
            if limit != COUNT_ONLY and _over(p, on_zero, limit):
                p, d["abandoned"] = limit, True
            d["passes"] += p
            d["max_eval"] = max(d["max_eval"], p)
            if d["abandoned"]:
                break
        out.append(d)
    return tuple(out)


def abandoned(name, limit):
    return {i for i, d in enumerate(per_match(name, limit)) if d["abandoned"]}


def counters(name, limit, plan=None):
    """the fields of esvo_lm_stats_t a launch over plan (match indices per solver slot; None: the case's own list) leaves"""
    pm = per_match(name, limit)
    plan = range(len(pm)) if plan is None else plan
    n = np.bincount(np.asarray(plan, np.int64), minlength=len(pm))
    used = [i for i in range(len(pm)) if n[i]]
    return dict(last_max_passes_eval=max(pm[i]["max_eval"] for i in used), last_max_passes_match=max(pm[i]["passes"] for i in used),
                last_passes=int(sum(n[i] * pm[i]["passes"] for i in used)), last_evals=int(sum(n[i] * pm[i]["evals"] for i in used)),
                last_shortcut_evals=int(sum(n[i] * pm[i]["shortcut"] for i in used)), last_abandoned=int(sum(n[i] for i in used if pm[i]["abandoned"])))


def reduced(per_match_results, gone):
    """the oracle's per-match results ([(0- or 1-element point array, solved)]) with the abandoned matches left out: no point, not solved"""
    return [(r[0][:0], False) if i in gone else r for i, r in enumerate(per_match_results)]


# (case, limit) pairs of the wide layout and what each must abandon (asserted on the CPU in tests/test_lm_guard_cases.py)
WIDE_LIMITS = (("solver_noise", 8, set()), ("solver_noise", 7, {2}), ("solver_noise", 6, {2, 3, 4, 5}),
               ("blob1", 64, {0, 1}), ("blob8", 64, {0, 1}), ("blob100", 64, {0, 1}),
               ("sparse_above", 64, set()), ("sparse_above", 32, {0}), ("sparse_at", 1, set()))
ANY_LIMITS = (("any5x5_blob", 64, {1}), ("any25x25_blob", 64, {0, 1}), ("any5x5_sparse_above", 64, set()), ("any5x5_sparse_above", 16, {0}))
