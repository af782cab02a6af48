"""The event survey's host twins (esvo_event_survey_host, esvo_hot_pixel_mask_host) against the Python-int restatement
(tests/event_survey_restated.py): equality everywhere, no GPU."""
import ctypes

import numpy as np
import pytest

import event_filter_restated as F
import event_survey_restated as S
from esvo_amd import abi, lib

W, H = F.W, F.H


def test_sizes_and_bindings():
    sizes = [ctypes.sizeof(t) for t in (abi.EventSurveyStruct, abi.EventSurveyStats, abi.HotPixelRule, abi.HotPixelReport)]
    assert lib.event_survey_sizes() == sizes == [16, 40, 32, 32]
    assert lib.abi_sizes()[7] == 8   # additive: the ABI number stays
    assert (abi.SURVEY_COUNT_ONLY, abi.MASK_KEEP, abi.MASK_REPLACE, abi.MASK_UNION) == (1, 0, 1, 2)
    assert {"esvo_ts_survey_begin", "esvo_ts_survey_end", "esvo_ts_survey_stats", "esvo_ts_survey_state", "esvo_ts_survey_mask",
            "esvo_event_survey_host", "esvo_hot_pixel_mask_host", "esvo_event_survey_sizes"} <= set(lib.SYMBOLS)
    assert {"api_survey.hip", "kernels_survey.hip"} <= set(lib._SOURCES)


@pytest.mark.parametrize("seed", (21, 22))
def test_counts_of_random_streams_in_packets(seed):
    ev, _ = F.random_stream(seed)
    counts, stats, got, gstats = None, None, None, None
    for a, b in ((0, 1), (1, 700), (700, 700), (700, 4000), (4000, len(ev))):
        counts, stats = S.count(ev[a:b], W, H, counts, stats)
        got, gstats = lib.event_survey_host(F.records(ev[a:b]), W, H, got, gstats)
        assert gstats == stats and np.array_equal(got, S.counts_array(counts))
    assert stats["packets"] == 4 and stats["outside"] > 100 and stats["events_in"] == int(got.sum()) == len(ev) - stats["outside"]
    assert got[0].sum() > 1000 and got[1].sum() > 1000


def test_counts_normalise_polarity_and_take_unsorted_streams():
    ev = F.records([(0, 0, 5000, 1), (W - 1, H - 1, 3000, 0), (0, 0, 9000, 1), (W, 0, 1, 1), (0, H, 10 ** 12, 0)])
    ev["polarity"][0] = 200
    got, st = lib.event_survey_host(ev, W, H)
    assert got[1][0][0] == 2 and got[0][H - 1][W - 1] == 1 and int(got.sum()) == 3
    assert st == dict(events_in=3, outside=2, packets=1, t_first=3000, t_last=9000)


def test_the_bound_of_the_counters():
    ev = F.records([(1, 1, 10, 1), (2, 2, 20, 0)])
    near = dict(S.STATS0, events_in=S.U32_MAX - 3, outside=2, t_first=1, t_last=2)
    with pytest.raises(lib.EsvoError) as e:
        lib.event_survey_host(ev, W, H, stats=near)
    assert e.value.code == abi.ERR_CAPACITY
    _, st = lib.event_survey_host(ev[:1], W, H, stats=near)
    assert st["events_in"] + st["outside"] == S.U32_MAX


@pytest.mark.parametrize("w,h", ((37, 29), (W, H)))
def test_the_rule_on_crafted_count_images(w, h):
    for name, c, stats, rule in S.crafted_images(w, h):
        counts = S.split_planes(c, w, h)
        want_mask, want = S.hot_pixels(counts, stats, w, h, **rule)
        mask, rep = lib.hot_pixel_mask_host(S.counts_array(counts), stats, w, h, **rule)
        assert rep == want, name
        assert mask.tolist() == want_mask, name


def test_the_crafted_images_exercise_what_they_name():
    by_name = {name: S.hot_pixels(S.split_planes(c, 37, 29), st, 37, 29, **rule) for name, c, st, rule in S.crafted_images(37, 29)}
    rep = {k: v[1] for k, v in by_name.items()}
    assert rep["all_equal"]["n_hot"] == 0 and rep["all_equal"]["max_pixel"] == 0
    assert rep["dark_b0"]["baseline"] == 0 and rep["dark_b0"]["n_hot"] == 3 and rep["dark_b0_min_count"]["n_hot"] == 1
    assert rep["factor_times_b_beyond_u32"]["n_hot"] == 2 and rep["factor_times_b_beyond_u32_none"]["n_hot"] == 0
    assert rep["at_and_above_factor_b"]["n_hot"] == 2 and rep["at_and_above_factor_b"]["max_pixel"] == 18 and rep["at_and_above_factor_b"]["events_hot"] == 62
    assert rep["rate_alone"]["rate_count"] == 30 and rep["rate_alone"]["n_hot"] == 2
    assert rep["rate_and_baseline"]["rate_count"] == 10 and rep["rate_and_baseline"]["n_hot"] == 3
    assert rep["rate_duration_0"]["n_hot"] == 0 and rep["rate_duration_0"]["rate_count"] == 0 and rep["rate_duration_0_with_baseline"]["n_hot"] == 2
    assert rep["rate_clamped"]["rate_count"] == S.U32_MAX and rep["rate_clamped"]["n_hot"] == 0
    assert rep["digit_edges_rank0"]["baseline"] == 0 and rep["digit_edges_rank1000"]["baseline"] == S.U32_MAX
    assert 0 < rep["digit_edges_rank500"]["baseline"] < rep["digit_edges_rank999"]["baseline"]


def test_argument_errors_of_the_rule():
    counts, stats = np.zeros((2, 4, 4), np.uint32), dict(S.STATS0)
    for bad in (dict(), dict(factor=1, min_count=0), dict(factor=1, rank_permille=1001), dict(factor=1, reserved=(0, 0, 1, 0))):
        with pytest.raises(lib.EsvoError) as e:
            lib.hot_pixel_mask_host(counts, stats, 4, 4, **bad)
        assert e.value.code == abi.ERR_INVALID_ARG, bad
    counts[:, 1, 1] = 2 ** 31      # the planes of one pixel add up beyond 2^32 - 1
    with pytest.raises(lib.EsvoError) as e:
        lib.hot_pixel_mask_host(counts, stats, 4, 4, factor=1)
    assert e.value.code == abi.ERR_INVALID_ARG
