"""Host-side pieces of bench.py that run without a GPU: the committed-profile reader behind `roofline.traffic` / `roofline.valu`,
the algorithmic byte counts of the roofline rows, the synthetic workloads' shape."""
import json
import os

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_profile_is_the_newest_round_of_the_workload():
    for wl in ("dsec640x480", "upenn346x260"):
        prof = bench.committed_profile(wl)
        assert prof is not None, wl
        meta = json.load(open(os.path.join(ROOT, "profiles", prof["tag"] + "_meta.json")))
        assert meta["workload"] == wl
        assert all(os.path.exists(os.path.join(ROOT, f)) for f in prof["files"])
        lm = [k for k in prof["sq"] if "lm_refine_kernel" in k]
        assert lm and prof["sq"][lm[0]]["SQ_INSTS_VALU"] > 1e6
        # FETCH / WRITE come from separate counter passes: both present for the dominant kernel
        hb = [v for k, v in prof["hbm"].items() if "lm_refine_kernel" in k]
        assert hb and {"FETCH_SIZE", "WRITE_SIZE"} <= set(hb[0])


def test_profile_figures_and_the_whole_tick_rate():
    prof = bench.committed_profile("dsec640x480")
    traffic, valu = bench.profile_figures(prof, "lm_refine", 1.27)
    assert traffic > 1e6 and 0.2 < valu["frac"] < 1.0
    assert valu["peak"] == bench.VALU_PEAK_INST_S
    whole = bench.whole_tick_valu(prof, 1.37)
    # every kernel of a tick: more instructions than the LM kernel alone, and below the chip's issue peak
    assert whole["wave_insts_per_tick"] > valu["wave_insts_per_launch"]
    assert valu["frac"] < whole["frac"] < 1.0
    assert bench.whole_tick_valu(None, 1.0) is None and bench.profile_figures(None, "lm_refine", 1.0) == (None, None)


def test_workloads_have_the_stated_shape():
    rig, stream, p, ticks = bench.make_workload("upenn346x260", 3)
    assert (rig.width, rig.height) == (346, 260) and len(ticks) == 3
    t, stamps, poses, T = ticks[0]
    assert len(stamps) == len(poses) and np.asarray(T).shape == (4, 4)
    assert np.all(np.diff(stream.ns_left.astype(np.int64)) >= 0)
    # the reference-faithful variant cuts the per-tick selection to the yaml's PROCESS_EVENT_NUM
    _, _, p_small, _ = bench.make_workload("upenn346x260", 3, events_cap=1000)
    assert p_small.process_event_num == 1000 < p.process_event_num


def test_looped_stream_of_the_sustained_point_is_sorted_and_continuous():
    from esvo_amd.abi import event_ns
    rig, stream, p, ticks = bench.make_workload("upenn346x260", 3)
    a = stream.slice(0, stream.t0_ns, stream.t0_ns + 20_000_000)
    b = bench.shift_events(a, 3_000_000_123)
    assert np.array_equal(event_ns(b), event_ns(a) + np.uint64(3_000_000_123))
    assert np.array_equal(b["x"], a["x"]) and np.array_equal(b["y"], a["y"]) and np.array_equal(b["polarity"], a["polarity"])
    assert np.all(b["nsec"] < 1_000_000_000)


def test_looped_staging_advances_in_place_as_shift_events():
    """the looped stream's staging (benchlib/points.py) advances one buffer pass by pass: byte for byte shift_events"""
    from benchlib.workload import advance_events
    rig, stream, p, ticks = bench.make_workload("upenn346x260", 3)
    a = np.ascontiguousarray(stream.slice(1, stream.t0_ns, stream.t0_ns + 20_000_000))
    buf = a.copy()
    for k in range(1, 6):
        advance_events(buf, 400_000_000)
        assert buf.tobytes() == bench.shift_events(a, k * 400_000_000).tobytes(), k
    advance_events(buf, 3_000_000_123)
    assert buf.tobytes() == bench.shift_events(a, 5 * 400_000_000 + 3_000_000_123).tobytes()


def test_dump_outputs_writes_float64_fields_within_the_size_cap(tmp_path):
    from esvo_amd.abi import DEPTH_POINT_DTYPE
    from benchlib.workload import DUMP_LIMIT_BYTES, dump_outputs
    small = np.zeros(1000, DEPTH_POINT_DTYPE)
    small["inv_depth"] = np.linspace(0.1, 1.0, 1000)
    small["x"][:, 1] = 7.0
    dump_outputs(str(tmp_path / "a"), {"depth_map": small})
    got = np.load(tmp_path / "a" / "depth_map_inv_depth.npy")
    assert got.dtype == np.float64 and np.array_equal(got, small["inv_depth"])
    assert np.load(tmp_path / "a" / "depth_map_x.npy").shape == (1000, 2)
    assert {f.name for f in (tmp_path / "a").iterdir()} == {f"depth_map_{n}.npy" for n in DEPTH_POINT_DTYPE.names}
    # over the cap: the same seeded sample of rows in every field, run after run
    big = np.zeros(700_000, DEPTH_POINT_DTYPE)
    big["inv_depth"] = np.arange(len(big))
    big["row"] = np.arange(len(big)) % 480
    for d in ("b", "c"):
        dump_outputs(str(tmp_path / d), {"depth_map": big, "last_frame": small})
    total = sum(f.stat().st_size for f in (tmp_path / "b").iterdir())
    assert total <= DUMP_LIMIT_BYTES + 64 * 1024   # (+ the .npy headers)
    idx = np.load(tmp_path / "b" / "depth_map_inv_depth.npy").astype(np.int64)
    assert 0 < len(idx) < len(big) and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "b" / "depth_map_row.npy"), big["row"][idx].astype(np.float64))
    for f in (tmp_path / "b").iterdir():
        assert np.array_equal(np.load(f), np.load(tmp_path / "c" / f.name)), f.name
