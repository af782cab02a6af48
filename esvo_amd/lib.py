"""ctypes bindings of libesvo_hip.so (the C-ABI of include/esvo_hip.h) and a thin Python host
mirror of the reference's call sequence (TimeSurface node + mapper node) for tests/bench.

There is NO fallback: if the HIP extension is missing or no MI355X is visible, loading /
creating a handle raises.  Nothing in this module touches oracle/.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from .abi import (MEM_DEVICE, MEM_HOST, P_U8, ColumnsError, EventColumnsStruct, EventFilterCounts, EventFilterStruct, event_filter_struct, EventBurstCounts, event_burst_struct, EventSurveyStats, EventSurveyStruct, HotPixelReport, event_survey_stats, hot_pixel_rule, Evt2Counts, Evt2State, Evt3Counts, Evt3State, evt2_words, evt3_words, check_t_offset, column_p_type, column_t_type,
                  DEPTH_POINT_DTYPE, EM_POSE_FN, ERR_CAPACITY, ERR_INVALID_ARG, ERR_STATE, EVENT_DTYPE, MATCH_DTYPE, CalibStruct, EmSelectionStruct,
                  EmStatsStruct, GpcParamsStruct, GpcStatsStruct, LmStatsStruct, ParamsStruct, SgmStatsStruct, StatsStruct, TRACK_ITER_DTYPE, TRACK_SOLVE_MAX_ITERATIONS,
                  TrackSolveInfoStruct, TrackSolveParamsStruct)

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# ESVO_HIP_LIB: another build of the same library (A/B measurements of kernel variants, tools/ab_build.py); never a fallback
_LIB_PATH = os.environ.get("ESVO_HIP_LIB") or os.path.join(_CSRC, "libesvo_hip.so")
_SOURCES = ["api_core.hip", "api_ts.hip", "api_ingest.hip", "api_words.hip", "api_map.hip", "api_window.hip", "api_modes.hip", "api_shard.hip", "api_out.hip", "api_comm.hip", "api_bag.hip", "api_track.hip", "scan.hip", "kernels_ts.hip", "kernels_bm.hip", "kernels_lm.hip", "kernels_lm_any.hip", "kernels_fuse.hip", "kernels_shard.hip", "kernels_track.hip", "kernels_track_viz.hip", "kernels_viz.hip", "kernels_sgm.hip", "api_em.hip", "kernels_em.hip", "kernels_cloud.hip", "api_dev.hip", "api_gpc.hip", "kernels_voxel.hip", "api_history.hip", "api_filter.hip", "kernels_filter.hip", "api_survey.hip", "kernels_survey.hip"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
               "-Wno-unused-value", "-Wno-unused-result", "-ldl"]

SYMBOLS = [
    "esvo_default_params", "esvo_create", "esvo_destroy", "esvo_reset", "esvo_set_params", "esvo_last_error",
    "esvo_set_stream", "esvo_synchronize", "esvo_ts_push_events", "esvo_ts_push_events_async", "esvo_ts_push_wait", "esvo_host_alloc", "esvo_host_free", "esvo_ts_push_event_array", "esvo_ts_push_event_columns", "esvo_event_columns_to_events", "esvo_event_columns_sizes", "esvo_raw_header", "esvo_ts_render", "esvo_ts_render_forward", "esvo_map_set_observation",
    "esvo_map_match", "esvo_map_set_poses", "esvo_map_refine", "esvo_map_push_frame", "esvo_map_fuse",
    "esvo_map_tick", "esvo_map_tick_bm_only", "esvo_map_fuse_matches_naive", "esvo_map_tick_resident", "esvo_map_get_depth_points", "esvo_map_get_committed", "esvo_map_get_pointcloud_xyz", "esvo_map_get_last_frame",
    "esvo_get_stats", "esvo_shard_set_band", "esvo_shard_set_routing", "esvo_shard_get_rows", "esvo_shard_exchange", "esvo_shard_tick_phase", "esvo_abi_sizes",
    "esvo_map_front", "esvo_map_front_frame", "esvo_map_push_frame_device", "esvo_map_fuse_async",
    "esvo_track_set_current", "esvo_track_get_images", "esvo_track_set_reference", "esvo_track_residuals", "esvo_track_jacobian",
    "esvo_track_normal_equations", "esvo_track_normal_equations_batch", "esvo_track_register", "esvo_track_solve", "esvo_track_sizes",
    "esvo_map_init_sgm",
    "esvo_bag_open", "esvo_bag_close", "esvo_bag_last_error", "esvo_bag_next_event_array", "esvo_ts_push_bag",
    "esvo_map_get_debug_images", "esvo_map_get_pointcloud_near_xyz", "esvo_voxel_filter_xyz", "esvo_map_save_depth_map",
    "esvo_comm_unique_id", "esvo_comm_rccl_info", "esvo_comm_init", "esvo_comm_init_callbacks", "esvo_comm_destroy", "esvo_comm_owns_next_tick",
    "esvo_comm_tick", "esvo_comm_tick_resident", "esvo_comm_get_stats", "esvo_comm_flush", "esvo_comm_newest_map", "esvo_comm_shard_tick", "esvo_comm_gather_map", "esvo_comm_gather_pointcloud_xyz", "esvo_comm_gather_ts",
    "esvo_map_match_em", "esvo_map_tick_em", "esvo_map_em_get_selection", "esvo_map_em_stats", "esvo_em_sizes",
    "esvo_map_lm_stats", "esvo_lm_sizes",
    "esvo_map_tick_sgm", "esvo_map_push_disparity_frame", "esvo_map_sgm_stats", "esvo_sgm_sizes",
    "esvo_map_cloud_build", "esvo_map_cloud_get", "esvo_map_cloud_device", "esvo_track_set_reference_from_cloud", "esvo_track_stochastic_order",
    "esvo_map_cloud_near", "esvo_map_voxel_filter", "esvo_map_gpc_configure", "esvo_map_gpc_update", "esvo_map_gpc_get", "esvo_map_gpc_device",
    "esvo_map_gpc_stats", "esvo_gpc_sizes",
    "esvo_track_reprojection_map", "esvo_track_reprojection_map_device",
    "esvo_ts_history_configure", "esvo_ts_history_list", "esvo_ts_history_get", "esvo_ts_history_put", "esvo_map_set_observation_at",
    "esvo_track_set_current_at", "esvo_ts_history_select", "esvo_ts_history_select_observation",
    "esvo_ts_filter_configure", "esvo_ts_filter_stats", "esvo_ts_filter_state", "esvo_event_filter_host", "esvo_event_filter_sizes",
    "esvo_ts_burst_configure", "esvo_ts_burst_stats", "esvo_ts_burst_state", "esvo_event_burst_filter_host", "esvo_event_burst_sizes",
    "esvo_ts_survey_begin", "esvo_ts_survey_end", "esvo_ts_survey_stats", "esvo_ts_survey_state", "esvo_ts_survey_mask",
    "esvo_event_survey_host", "esvo_hot_pixel_mask_host", "esvo_event_survey_sizes",
]
# the EVT 3.0 entry points, listed apart: their names carry a digit (SYMBOLS is compared with a scan of the header for [a-z_] names)
SYMBOLS_EVT3 = ["esvo_ts_push_evt3", "esvo_ts_evt3_state", "esvo_ts_evt3_stats", "esvo_evt3_to_events", "esvo_evt3_raw_header", "esvo_evt3_sizes",
                # EVT 2.0 / 2.1 (esvo_raw_header has no digit and stands in SYMBOLS)
                "esvo_ts_push_evt2", "esvo_ts_evt2_state", "esvo_ts_evt2_stats", "esvo_evt2_to_events", "esvo_evt2_sizes"]

ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class EsvoError(RuntimeError):
    """a failed C call; `code` is its esvo_status_t (None for errors raised on the Python side)"""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


ERR_HALO = -7   # ESVO_ERR_HALO (include/esvo_hip.h)
ESVO_AGAIN = 1  # esvo_shard_tick_phase: exchange, then the same phase once more


_PERTURBED_PATH = os.path.join(_CSRC, "libesvo_hip_perturbed.so")


def build(force=False, verbose=False, perturbed=False):
    """hipcc cross-compiles the extension for gfx950 in-tree (works without a GPU): one object per source file (in parallel,
    only the files that changed), then one link.
    perturbed=True additionally links libesvo_hip_perturbed.so: the same library with -DESVO_PERTURB_ONE_ULP, i.e. the depth
    of every eighth solver slot's point off by one unit in the last place (lm_common.hpp, both refinement kernels) -- never loaded by the product; tests/test_gpu_bench_parity.py
    points ESVO_HIP_LIB at it to show that bench.py's `parity.oracle_equal` notices a single flipped bit."""
    from concurrent.futures import ThreadPoolExecutor
    inc = os.path.join(_CSRC, "..", "..", "include")
    headers = [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith(".hpp")] + [
        os.path.join(inc, "esvo_hip.h"), os.path.join(inc, "esvo_hip.hpp")]
    hdr_time = max(os.path.getmtime(h) for h in headers)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("ESVO_EXTRA_HIPCC_FLAGS", "").split()  # A/B experiments only
    lib_path = os.path.join(_CSRC, "libesvo_hip.so")  # always: ESVO_HIP_LIB names a library to LOAD (an A/B build), never one to write
    objdir = os.path.join(_CSRC, "build" + ("_" + str(abs(hash(" ".join(extra))) % 100000) if extra else ""))
    os.makedirs(objdir, exist_ok=True)
    cflags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-ldl")] + extra + ["-I", inc, "-c"]

    def compile_one(job):
        src, obj, defs = job
        if not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(src), hdr_time):
            return False
        cmd = [hipcc] + cflags + defs + ["-o", obj, src]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        return True

    jobs = [(os.path.join(_CSRC, s), os.path.join(objdir, s[:-4] + ".o"), []) for s in _SOURCES]
    twins = ("kernels_lm", "kernels_lm_any") if perturbed else ()   # the files whose kernels end in lm_common.hpp's lm_store_point
    jobs += [(os.path.join(_CSRC, t + ".hip"), os.path.join(objdir, t + "_perturbed.o"), ["-DESVO_PERTURB_ONE_ULP"]) for t in twins]
    with ThreadPoolExecutor(max_workers=min(len(jobs), 16, os.cpu_count() or 4)) as ex:
        rebuilt = list(ex.map(compile_one, jobs))
    objs = [j[1] for j in jobs[:len(_SOURCES)]]

    def link(out, obj_list, changed):
        if not changed and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(o) for o in obj_list):
            return
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + obj_list + ["-ldl"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)

    link(lib_path, objs, any(rebuilt[:len(_SOURCES)]))
    if perturbed:
        pobjs = [o[:-2] + "_perturbed.o" if os.path.basename(o)[:-2] in twins else o for o in objs]
        link(_PERTURBED_PATH, pobjs, any(rebuilt))
    return lib_path


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise EsvoError(f"{_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(the ESVO hot path has no CPU fallback)")
    lib = C.CDLL(_LIB_PATH)
    if os.environ.get("ESVO_HIP_LIB"):  # an A/B build of an older revision may lack the newest entry points: stub them
        class _Missing:
            argtypes = restype = None

            def __call__(self, *a):
                raise EsvoError("entry point missing in the ESVO_HIP_LIB build")
        for s in SYMBOLS + SYMBOLS_EVT3:
            if not hasattr(lib, s):
                setattr(lib, s, _Missing())
    vp, u64, sz, i32 = C.c_void_p, C.c_uint64, C.c_size_t, C.c_int
    psz = C.POINTER(C.c_size_t)
    lib.esvo_default_params.argtypes = [vp]
    lib.esvo_default_params.restype = None
    lib.esvo_create.argtypes = [vp, vp, vp, i32, C.POINTER(vp)]
    lib.esvo_destroy.argtypes = [vp]
    lib.esvo_reset.argtypes = [vp]
    lib.esvo_set_params.argtypes = [vp, vp]
    lib.esvo_last_error.argtypes = [vp]
    lib.esvo_last_error.restype = C.c_char_p
    lib.esvo_set_stream.argtypes = [vp, vp]
    lib.esvo_synchronize.argtypes = [vp]
    lib.esvo_ts_push_events.argtypes = [vp, i32, vp, sz]
    lib.esvo_ts_push_events_async.argtypes = [vp, i32, vp, sz]
    lib.esvo_ts_push_wait.argtypes = [vp, i32]
    lib.esvo_host_alloc.argtypes = [sz, C.POINTER(vp)]
    lib.esvo_host_free.argtypes = [vp]
    lib.esvo_ts_push_event_array.argtypes = [vp, i32, vp, sz, psz]
    lib.esvo_ts_push_event_columns.argtypes = [vp, i32, vp, sz]
    lib.esvo_event_columns_to_events.argtypes = [vp, sz, vp, psz]
    lib.esvo_event_columns_sizes.argtypes = [vp]
    lib.esvo_event_columns_sizes.restype = None
    lib.esvo_ts_push_evt3.argtypes = [vp, i32, vp, sz, i32, C.c_int64, psz]
    lib.esvo_ts_evt3_state.argtypes = [vp, i32, vp, vp]
    lib.esvo_ts_evt3_stats.argtypes = [vp, i32, vp]
    lib.esvo_evt3_to_events.argtypes = [vp, vp, sz, C.c_int64, vp, sz, psz, vp]
    lib.esvo_evt3_raw_header.argtypes = [vp, sz, psz, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.esvo_evt3_sizes.argtypes = [vp]
    lib.esvo_evt3_sizes.restype = None
    lib.esvo_ts_push_evt2.argtypes = [vp, i32, vp, sz, i32, i32, C.c_int64, psz]
    lib.esvo_ts_evt2_state.argtypes = [vp, i32, vp, vp]
    lib.esvo_ts_evt2_stats.argtypes = [vp, i32, vp]
    lib.esvo_evt2_to_events.argtypes = [vp, vp, sz, i32, C.c_int64, vp, sz, psz, vp]
    lib.esvo_raw_header.argtypes = [vp, sz, psz, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.esvo_evt2_sizes.argtypes = [vp]
    lib.esvo_evt2_sizes.restype = None
    lib.esvo_ts_render.argtypes = [vp, i32, u64, vp]
    lib.esvo_ts_render_forward.argtypes = [vp, i32, u64, vp]
    lib.esvo_map_set_observation.argtypes = [vp, u64, vp, vp, vp]
    lib.esvo_map_match.argtypes = [vp, vp, sz, vp, vp, sz, vp, sz, psz]
    lib.esvo_map_set_poses.argtypes = [vp, vp, vp, sz]
    lib.esvo_map_refine.argtypes = [vp, vp, sz, i32, vp, sz, psz]
    lib.esvo_map_push_frame.argtypes = [vp, vp, sz, vp, sz]
    lib.esvo_map_fuse.argtypes = [vp, psz]
    lib.esvo_map_tick.argtypes = [vp, u64, vp, vp, sz]
    lib.esvo_map_tick_resident.argtypes = [vp, u64, vp, vp, vp, sz]
    lib.esvo_map_tick_bm_only.argtypes = [vp, u64, vp, vp, sz]
    lib.esvo_map_fuse_matches_naive.argtypes = [vp, vp, sz, vp, sz]
    lib.esvo_map_get_depth_points.argtypes = [vp, vp, sz, psz]
    lib.esvo_map_get_committed.argtypes = [vp, vp, sz, psz, C.POINTER(C.c_uint64)]
    lib.esvo_map_get_pointcloud_xyz.argtypes = [vp, vp, sz, psz]
    lib.esvo_map_get_last_frame.argtypes = [vp, vp, sz, psz]
    lib.esvo_get_stats.argtypes = [vp, vp]
    lib.esvo_shard_set_band.argtypes = [vp, i32, i32, i32, i32]
    lib.esvo_shard_set_routing.argtypes = [vp, i32, i32]
    lib.esvo_shard_get_rows.argtypes = [vp, vp, vp, vp, vp]
    lib.esvo_shard_exchange.argtypes = [vp, vp, vp, vp]
    lib.esvo_shard_tick_phase.argtypes = [vp, i32, u64, vp, vp, sz]
    lib.esvo_map_front.argtypes = [vp, u64, vp, vp, sz, psz]
    lib.esvo_map_front_frame.argtypes = [vp, vp]
    lib.esvo_map_push_frame_device.argtypes = [vp, vp, sz, vp, sz]
    lib.esvo_map_fuse_async.argtypes = [vp]
    lib.esvo_track_set_current.argtypes = [vp, vp, i32]
    lib.esvo_track_get_images.argtypes = [vp, vp, vp, vp]
    lib.esvo_track_set_reference.argtypes = [vp, vp, sz, vp]
    lib.esvo_track_residuals.argtypes = [vp, vp, sz, sz, i32, C.c_double, vp, psz]
    lib.esvo_track_jacobian.argtypes = [vp, vp, vp, sz, sz, vp, psz]
    lib.esvo_track_normal_equations.argtypes = [vp, vp, vp, sz, sz, i32, C.c_double, vp, vp, C.POINTER(C.c_double), psz]
    lib.esvo_track_normal_equations_batch.argtypes = [vp, i32, vp, vp, sz, sz, i32, C.c_double, vp, vp, vp, psz]
    lib.esvo_track_register.argtypes = [vp, sz, vp, vp, i32, C.c_double, i32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.esvo_track_solve.argtypes = [vp, vp, vp, vp, vp, vp, sz]
    lib.esvo_track_sizes.argtypes = [vp]
    lib.esvo_track_sizes.restype = None
    lib.esvo_map_init_sgm.argtypes = [vp, vp, vp, sz, psz, vp]
    lib.esvo_bag_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.esvo_bag_close.argtypes = [vp]
    lib.esvo_bag_last_error.argtypes = [vp]
    lib.esvo_bag_next_event_array.argtypes = [vp, C.c_char_p, C.POINTER(vp), psz, C.POINTER(C.c_uint64), C.POINTER(C.c_char_p)]
    lib.esvo_ts_push_bag.argtypes = [vp, i32, vp, C.c_char_p, u64, psz]
    lib.esvo_map_get_debug_images.argtypes = [vp, C.c_double, vp, vp, vp, vp]
    lib.esvo_map_get_pointcloud_near_xyz.argtypes = [vp, C.c_double, vp, sz, psz]
    lib.esvo_voxel_filter_xyz.argtypes = [vp, sz, C.c_float, vp, sz, psz]
    lib.esvo_map_save_depth_map.argtypes = [vp, C.c_char_p, u64, psz]
    lib.esvo_comm_unique_id.argtypes = [vp]
    lib.esvo_comm_init.argtypes = [vp, vp, i32, i32]
    lib.esvo_comm_rccl_info.argtypes = [C.POINTER(C.c_int), C.c_char_p, sz]
    lib.esvo_comm_init_callbacks.argtypes = [vp, i32, i32, ALL_GATHER_FN, vp]
    lib.esvo_comm_destroy.argtypes = [vp]
    lib.esvo_comm_owns_next_tick.argtypes = [vp]
    lib.esvo_comm_tick.argtypes = [vp, u64, vp, vp, vp, sz]
    lib.esvo_comm_tick_resident.argtypes = [vp, u64, vp, vp, vp, sz]
    lib.esvo_comm_get_stats.argtypes = [vp, vp]
    lib.esvo_comm_flush.argtypes = [vp]
    lib.esvo_comm_newest_map.argtypes = [vp, vp, sz, psz, C.POINTER(C.c_longlong)]
    lib.esvo_comm_shard_tick.argtypes = [vp, u64, vp, vp, sz]
    lib.esvo_comm_gather_map.argtypes = [vp, vp, sz, psz]
    lib.esvo_comm_gather_pointcloud_xyz.argtypes = [vp, vp, sz, psz]
    lib.esvo_comm_gather_ts.argtypes = [vp, i32]
    lib.esvo_map_match_em.argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, vp, sz, vp, sz, psz]
    lib.esvo_map_tick_em.argtypes = [vp, vp, i32, u64, u64, EM_POSE_FN, vp]
    lib.esvo_map_em_get_selection.argtypes = [vp, vp, vp, vp, vp, vp, sz]
    lib.esvo_map_em_stats.argtypes = [vp, vp]
    lib.esvo_em_sizes.argtypes = [vp]
    lib.esvo_em_sizes.restype = None
    lib.esvo_map_lm_stats.argtypes = [vp, vp]
    lib.esvo_lm_sizes.argtypes = [vp]
    lib.esvo_lm_sizes.restype = None
    lib.esvo_map_tick_sgm.argtypes = [vp, vp, vp, psz, vp]
    lib.esvo_map_push_disparity_frame.argtypes = [vp, vp, vp, sz, psz]
    lib.esvo_map_sgm_stats.argtypes = [vp, vp]
    lib.esvo_sgm_sizes.argtypes = [vp]
    lib.esvo_sgm_sizes.restype = None
    lib.esvo_map_cloud_build.argtypes = [vp, psz]
    lib.esvo_map_cloud_get.argtypes = [vp, vp, sz, psz]
    lib.esvo_map_cloud_device.argtypes = [vp, C.POINTER(vp), psz, C.POINTER(C.c_uint64)]
    lib.esvo_track_set_reference_from_cloud.argtypes = [vp, vp, sz, vp]
    lib.esvo_track_stochastic_order.argtypes = [sz, sz, vp, vp]
    lib.esvo_map_cloud_near.argtypes = [vp, C.c_double, vp, sz, psz]
    lib.esvo_map_voxel_filter.argtypes = [vp, vp, sz, C.c_float, vp, sz, psz]
    lib.esvo_map_gpc_configure.argtypes = [vp, vp]
    lib.esvo_map_gpc_update.argtypes = [vp, u64, C.POINTER(C.c_int)]
    lib.esvo_map_gpc_get.argtypes = [vp, vp, sz, psz]
    lib.esvo_map_gpc_device.argtypes = [vp, C.POINTER(vp), psz]
    lib.esvo_map_gpc_stats.argtypes = [vp, vp]
    lib.esvo_gpc_sizes.argtypes = [vp]
    lib.esvo_gpc_sizes.restype = None
    lib.esvo_track_reprojection_map.argtypes = [vp, vp, vp, sz, C.c_double, C.c_double, vp, psz]
    lib.esvo_track_reprojection_map_device.argtypes = [vp, C.POINTER(vp)]
    lib.esvo_ts_history_configure.argtypes = [vp, sz]
    lib.esvo_ts_history_list.argtypes = [vp, vp, vp, sz, psz]
    lib.esvo_ts_history_get.argtypes = [vp, u64, i32, vp]
    lib.esvo_ts_history_put.argtypes = [vp, u64, i32, vp]
    lib.esvo_map_set_observation_at.argtypes = [vp, u64, vp]
    lib.esvo_track_set_current_at.argtypes = [vp, u64, i32]
    lib.esvo_ts_history_select.argtypes = [vp, sz, i32, EM_POSE_FN, vp, psz, vp]
    lib.esvo_ts_history_select_observation.argtypes = [vp, i32, EM_POSE_FN, vp, C.POINTER(C.c_uint64), vp]
    lib.esvo_ts_filter_configure.argtypes = [vp, i32, vp]
    lib.esvo_ts_filter_stats.argtypes = [vp, i32, vp]
    lib.esvo_ts_filter_state.argtypes = [vp, i32, vp, vp]
    lib.esvo_event_filter_host.argtypes = [vp, i32, i32, vp, vp, sz, vp, vp, sz, psz, vp]
    lib.esvo_event_filter_sizes.argtypes = [vp]
    lib.esvo_event_filter_sizes.restype = None
    lib.esvo_ts_burst_configure.argtypes = [vp, i32, vp]
    lib.esvo_ts_burst_stats.argtypes = [vp, i32, vp]
    lib.esvo_ts_burst_state.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.esvo_event_burst_filter_host.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, sz, vp, vp, sz, psz, vp, vp]
    lib.esvo_event_burst_sizes.argtypes = [vp]
    lib.esvo_event_burst_sizes.restype = None
    lib.esvo_ts_survey_begin.argtypes = [vp, i32, vp]
    lib.esvo_ts_survey_end.argtypes = [vp, i32]
    lib.esvo_ts_survey_stats.argtypes = [vp, i32, vp]
    lib.esvo_ts_survey_state.argtypes = [vp, i32, vp, vp, vp]
    lib.esvo_ts_survey_mask.argtypes = [vp, i32, vp, vp, i32, vp]
    lib.esvo_event_survey_host.argtypes = [i32, i32, vp, vp, vp, sz]
    lib.esvo_hot_pixel_mask_host.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.esvo_event_survey_sizes.argtypes = [vp]
    lib.esvo_event_survey_sizes.restype = None
    for s in SYMBOLS + SYMBOLS_EVT3:
        if s not in ("esvo_default_params", "esvo_last_error", "esvo_abi_sizes", "esvo_bag_last_error", "esvo_em_sizes", "esvo_lm_sizes", "esvo_sgm_sizes",
                     "esvo_track_sizes", "esvo_gpc_sizes", "esvo_event_columns_sizes", "esvo_evt3_sizes", "esvo_evt2_sizes", "esvo_event_filter_sizes", "esvo_event_burst_sizes", "esvo_event_survey_sizes"):
            getattr(lib, s).restype = C.c_int
    lib.esvo_abi_sizes.argtypes = [vp]
    lib.esvo_abi_sizes.restype = None
    lib.esvo_bag_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def _pose_trampoline(pose_fn):
    """pose_fn(t_ns) -> 4x4 T_world_cam or None, as an esvo_em_pose_fn.  An exception must not unwind through the C frames: it is
    kept (the second value, a list) and the stamp counts as one without a pose."""
    raised = []

    def trampoline(user, t_ns, out):
        try:
            T = None if pose_fn is None else pose_fn(int(t_ns))
            if T is None:
                return 0
            T = np.asarray(T, np.float64).reshape(16)
            for k in range(16):
                out[k] = float(T[k])
            return 1
        except BaseException as e:  # noqa: BLE001
            raised.append(e)
            return 0
    return EM_POSE_FN(trampoline), raised


def ts_history_select(stamps, pose_fn=None, initialization=False):
    """dataTransferring's choice among the stamps of complete pairs, ascending (esvo_ts_history_select; host code, no GPU):
    (index, 4x4 T_world_cam), or None where the node would return false.  pose_fn(t_ns) -> 4x4 pose, or None where no pose is
    known; it is not consulted while the system initialises."""
    lib = load()
    st = np.ascontiguousarray(stamps, np.uint64)
    cb, raised = _pose_trampoline(pose_fn)
    idx, T = C.c_size_t(0), np.zeros(16, np.float64)
    rc = lib.esvo_ts_history_select(st.ctypes.data if len(st) else None, len(st), 1 if initialization else 0, cb, None, C.byref(idx),
                                    T.ctypes.data)
    if raised:
        raise raised[0]
    if rc == ESVO_AGAIN:
        return None
    if rc != 0:
        raise EsvoError(f"esvo_ts_history_select failed ({rc}): {lib.esvo_last_error(None).decode(errors='replace')}", code=rc)
    return int(idx.value), T.reshape(4, 4)


def stochastic_order(n_cloud, n_take, draws):
    """The order RegProblemLM::setProblem's swaps (RegProblemLM.cpp:45-49) leave, from the cloud's size and the draws alone:
    for i < min(n_take, n_cloud), positions i and i + draws[i] % (n_cloud - i) of the identity over n_cloud are swapped;
    returns what ends up at the positions [0, n_take) as uint32.  O(n_take) through a sparse map -- include/esvo_hip.hpp's
    esvo_hip::stochastic_order (and the library's esvo_track_stochastic_order) in Python."""
    n_cloud, n_take = int(n_cloud), min(int(n_take), int(n_cloud))
    draws = np.asarray(draws, np.uint32)
    assert len(draws) >= n_take, "one draw per taken point"
    moved, order = {}, np.empty(n_take, np.uint32)
    for i in range(n_take):
        j = i + int(draws[i]) % (n_cloud - i)
        vi, vj = moved.get(i, i), moved.get(j, j)
        order[i] = vj
        moved[j] = vi
        moved.pop(i, None)
    return order


def stochastic_order_c(n_cloud, n_take, draws):
    """the same through the library's C entry esvo_track_stochastic_order (which calls the C++ inline)"""
    lib = load()
    n_cloud, n_take = int(n_cloud), min(int(n_take), int(n_cloud))
    draws = np.ascontiguousarray(draws, np.uint32)
    assert len(draws) >= n_take, "one draw per taken point"
    order = np.empty(n_take, np.uint32)
    rc = lib.esvo_track_stochastic_order(n_cloud, n_take, draws.ctypes.data if n_take else None, order.ctypes.data if n_take else None)
    if rc != 0:
        raise EsvoError(f"esvo_track_stochastic_order failed ({rc}): {lib.esvo_last_error(None).decode(errors='replace')}", code=rc)
    return order


def selftest_division(n=1 << 28, seed=1):
    """device self-test of fdiv.hpp: returns the number of (a, b) pairs where the shared-divisor
    quotient differs from a / b (must be 0)"""
    lib = load()
    bad = C.c_ulonglong(0)
    lib.esvo_selftest_division.argtypes = [C.c_ulonglong, C.c_ulonglong, C.POINTER(C.c_ulonglong)]
    lib.esvo_selftest_division.restype = C.c_int
    rc = lib.esvo_selftest_division(int(n), int(seed), C.byref(bad))
    if rc != 0:
        raise EsvoError(f"selftest failed ({rc}): {lib.esvo_last_error(None).decode(errors='replace')}")
    return bad.value


# ---- esvo_debug_* (api_dev.hip): the shared device primitives one launch at a time; tests/test_gpu_primitives.py -----------------
# Not part of the documented ABI.  Every buffer the kernel may write sits between guard words on the device; the buffers start
# filled with DEBUG_PREFILL_BYTE, so "never written" and "written as zero" differ.  Each call returns its results and, last,
# the number of disturbed guard words (must be 0).
DEBUG_PREFILL_BYTE = 0xC7
DEBUG_PREFILL_U32 = 0xC7C7C7C7


def _prefilled(n, dtype):
    a = np.empty(int(n), dtype)
    a.view(np.uint8)[...] = DEBUG_PREFILL_BYTE
    return a


def _dbg_fn(name, argtypes):
    fn = getattr(load(), name)
    fn.argtypes, fn.restype = argtypes, C.c_int
    return fn


def _dbg_rc(rc, name):
    if rc < 0:
        raise EsvoError(f"{name} failed ({rc}): {load().esvo_last_error(None).decode(errors='replace')}", code=rc)
    return int(rc)


def _dbg_array(a, dtype, name, n=None):
    a = np.asarray(a)
    if a.dtype != dtype or a.ndim != 1:
        raise ValueError(f"{name}: a one-dimensional {np.dtype(dtype)} array is expected, not {a.dtype} with {a.ndim} axes")
    if n is not None and len(a) != n:
        raise ValueError(f"{name}: {n} elements expected, not {len(a)}")
    return np.ascontiguousarray(a)


def debug_scan_predicates(n):
    """(scan_is_small(n), scan_compact_is_small(n), scan_tiles(n), scan_scratch_elems(n))"""
    out = (C.c_size_t * 4)()
    _dbg_rc(_dbg_fn("esvo_debug_scan_predicates", [C.c_size_t, C.c_void_p])(int(n), out), "esvo_debug_scan_predicates")
    return bool(out[0]), bool(out[1]), int(out[2]), int(out[3])


def debug_scan_u32(x, in_place=False, want_total=True):
    """launch_exclusive_scan_u32 -> (out, total or None, disturbed guard words); in_place: d_out == d_in"""
    x = _dbg_array(x, np.uint32, "x")
    out = _prefilled(len(x), np.uint32)
    total = _prefilled(1, np.uint32) if want_total else None
    fn = _dbg_fn("esvo_debug_scan_u32", [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p])
    g = _dbg_rc(fn(x.ctypes.data, len(x), out.ctypes.data, 1 if in_place else 0, _p(total)), "esvo_debug_scan_u32")
    return out, (int(total[0]) if want_total else None), g


def debug_scan_code_bit0(codes, tile_sums=None, want_total=True, zero_words=None):
    """launch_exclusive_scan_code_bit0, or with tile_sums (scan_tiles(n) words) launch_scan_down_code_bit0 alone
    -> (out, total or None, zero or None, disturbed guard words); zero_words (>= n): the size of the buffer cleared on the way"""
    codes = _dbg_array(codes, np.uint8, "codes")
    n = len(codes)
    if tile_sums is not None:
        if debug_scan_predicates(n)[0]:
            raise ValueError("the down-sweep alone is for n above the single-workgroup bound")
        tile_sums = _dbg_array(tile_sums, np.uint32, "tile_sums", debug_scan_predicates(n)[2])
    if zero_words is not None and zero_words < n:
        raise ValueError(f"zero_words: at least n = {n} words are cleared")
    out = _prefilled(n, np.uint32)
    total = _prefilled(1, np.uint32) if want_total else None
    zero = None if zero_words is None else _prefilled(zero_words, np.uint32)
    fn = _dbg_fn("esvo_debug_scan_code_bit0", [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t])
    g = _dbg_rc(fn(codes.ctypes.data, n, _p(tile_sums), out.ctypes.data, _p(total), _p(zero), 0 if zero is None else len(zero)),
                "esvo_debug_scan_code_bit0")
    return out, (int(total[0]) if want_total else None), zero, g


def _check_compact_args(flags, slots, dtype):
    flags = _dbg_array(flags, np.uint32, "flags")
    slots = _dbg_array(slots, dtype, "slots", len(flags))
    if not debug_scan_predicates(len(flags))[1]:   # scan_compact_is_small: the library's own bound
        raise ValueError("the single-workgroup compaction takes 1 .. SCAN_COMPACT_SMALL_MAX flags")
    if flags.max() > 1:
        raise ValueError("flags are 0 or 1")
    return flags, slots


def debug_compact_matches(flags, slots, want_out=True, want_slot_of=True):
    """launch_scan_compact_matches_small -> dict(prefix, total, out, slot_of, guards); out / slot_of None where not asked for"""
    flags, slots = _check_compact_args(flags, slots, MATCH_DTYPE)
    n = len(flags)
    prefix, total = _prefilled(n, np.uint32), _prefilled(1, np.uint32)
    out = _prefilled(n, MATCH_DTYPE) if want_out else None
    slot_of = _prefilled(n, np.uint32) if want_slot_of else None
    fn = _dbg_fn("esvo_debug_compact_matches", [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5)
    g = _dbg_rc(fn(flags.ctypes.data, n, slots.ctypes.data, prefix.ctypes.data, total.ctypes.data, _p(out), _p(slot_of)),
                "esvo_debug_compact_matches")
    return dict(prefix=prefix, total=int(total[0]), out=out, slot_of=slot_of, guards=g)


def debug_lm_order(matches, max_matches, width, height, left, right, num_threads=1, updown=False):
    """launch_lm_pixel_order on a compacted list of match records and a launch bound -> dict(order, variant, guards): the
    processing order of the narrow LM launch (max_matches words, prefilled), which sort key the library was built with
    (0: the pixel; 1: the patch-SSD octave above it) and the disturbed guard words"""
    matches = _dbg_array(matches, MATCH_DTYPE, "matches")
    left = _dbg_array(np.asarray(left).reshape(-1), np.uint8, "left", width * height)
    right = _dbg_array(np.asarray(right).reshape(-1), np.uint8, "right", width * height)
    order = _prefilled(max_matches, np.uint32)
    variant = C.c_int(-1)
    fn = _dbg_fn("esvo_debug_lm_order", [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p])
    g = _dbg_rc(fn(matches.ctypes.data if len(matches) else None, len(matches), int(max_matches), int(width), int(height), int(num_threads),
                   1 if updown else 0, left.ctypes.data, right.ctypes.data, order.ctypes.data, C.addressof(variant)), "esvo_debug_lm_order")
    return dict(order=order, variant=int(variant.value), guards=g)


def debug_compact_points(flags, slots, want_out=True, row=None, total_index=0, pinned_row=False):
    """launch_scan_compact_points_small -> dict(prefix, total, out, row, row_host, guards).  row (uint32 words): the device counter
    row whose word total_index is the total (returned as it is afterwards); pinned_row: the kernel also writes the finished row
    to pinned host memory (row_host, prefilled)"""
    flags, slots = _check_compact_args(flags, slots, DEPTH_POINT_DTYPE)
    n = len(flags)
    if row is None and pinned_row:
        raise ValueError("pinned_row needs the device row it mirrors")
    if row is not None:
        row = _dbg_array(row, np.uint32, "row").copy()
        if not 0 <= total_index < len(row) <= 1024:
            raise ValueError("total_index must lie inside the row (at most 1024 words)")
    prefix, total = _prefilled(n, np.uint32), _prefilled(1, np.uint32)
    out = _prefilled(n, DEPTH_POINT_DTYPE) if want_out else None
    row_host = _prefilled(len(row), np.uint32) if pinned_row else None
    fn = _dbg_fn("esvo_debug_compact_points", [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5 + [C.c_uint32, C.c_uint32, C.c_void_p])
    g = _dbg_rc(fn(flags.ctypes.data, n, slots.ctypes.data, prefix.ctypes.data, None if row is not None else total.ctypes.data, _p(out),
                   _p(row), 0 if row is None else len(row), int(total_index), _p(row_host)), "esvo_debug_compact_points")
    return dict(prefix=prefix, total=int(total[0]) if row is None else int(row[total_index]), out=out, row=row, row_host=row_host,
                guards=g)


def debug_upload_words(src, zero_words=None, n_zero=0):
    """launch_upload_words from a pinned copy of src (uint32) -> (dst, zero or None, disturbed guard words)"""
    src = _dbg_array(src, np.uint32, "src")
    if not 0 <= n_zero <= 256 or n_zero > (zero_words or 0):
        raise ValueError("n_zero: at most 256 words, inside the zero buffer")
    dst = _prefilled(len(src), np.uint32)
    zero = None if zero_words is None else _prefilled(zero_words, np.uint32)
    fn = _dbg_fn("esvo_debug_upload_words", [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32])
    g = _dbg_rc(fn(src.ctypes.data if len(src) else None, src.nbytes, dst.ctypes.data if len(src) else None, _p(zero),
                   0 if zero is None else len(zero), int(n_zero)), "esvo_debug_upload_words")
    return dst, zero, g


def debug_back_prologue(src, a, b, a_flags=None, a_prefix=None):
    """launch_back_prologue -> (dst, a_dst, b_dst, disturbed guard words).  src: uint32 words (through pinned memory), b: uint64
    words; a: uint64 words (plain copy), or with a_flags / a_prefix the depth-point slot records that are gathered into a_dst
    (as many records as slots, prefilled)"""
    src, b = _dbg_array(src, np.uint32, "src"), _dbg_array(b, np.uint64, "b")
    gather = a_flags is not None
    if gather:
        a_flags = _dbg_array(a_flags, np.uint32, "a_flags")
        a = _dbg_array(a, DEPTH_POINT_DTYPE, "a", len(a_flags))
        a_prefix = _dbg_array(a_prefix, np.uint32, "a_prefix", len(a_flags))
        if len(a_flags) and int(a_prefix[a_flags != 0].max(initial=0)) >= len(a_flags):
            raise ValueError("a_prefix points outside a_dst")
        a_dst = _prefilled(len(a), DEPTH_POINT_DTYPE)
    else:
        if a_prefix is not None:
            raise ValueError("a_prefix without a_flags")
        a = _dbg_array(a, np.uint64, "a")
        a_dst = _prefilled(len(a), np.uint64)
    dst, b_dst = _prefilled(len(src), np.uint32), _prefilled(len(b), np.uint64)

    def ptr(x):
        return x.ctypes.data if x.nbytes else None
    fn = _dbg_fn("esvo_debug_back_prologue", [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32])
    if gather and len(a_flags) == 0:
        raise ValueError("gather mode needs at least one slot")
    g = _dbg_rc(fn(ptr(src), src.nbytes, ptr(dst), ptr(a), a.nbytes, ptr(a_dst), a_dst.nbytes, ptr(b), b.nbytes, ptr(b_dst),
                   _p(a_flags), _p(a_prefix), len(a_flags) if gather else 0), "esvo_debug_back_prologue")
    return dst, a_dst, b_dst, g


def debug_fdiv(a, b):
    """fdiv.hpp on pairs -> dict(div_by, div_fast, div_refined, fast, ok_a, guards): div_by(a, make_recip(b)); div_fast(a,
    make_recip(b)) and div_fast(a, {b, recip_refined(b)}) (computed on every pair; meaningful where fast & ok_a);
    make_recip(b).fast; fdiv_ok(a)"""
    a = _dbg_array(a, np.float64, "a")
    b = _dbg_array(b, np.float64, "b", len(a))
    n = len(a)
    q_by, q_fast, q_ref = _prefilled(n, np.float64), _prefilled(n, np.float64), _prefilled(n, np.float64)
    fast, ok_a = _prefilled(n, np.uint32), _prefilled(n, np.uint32)
    fn = _dbg_fn("esvo_debug_fdiv", [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5)
    g = _dbg_rc(fn(a.ctypes.data, b.ctypes.data, n, q_by.ctypes.data, q_fast.ctypes.data, q_ref.ctypes.data, fast.ctypes.data,
                   ok_a.ctypes.data), "esvo_debug_fdiv")
    return dict(div_by=q_by, div_fast=q_fast, div_refined=q_ref, fast=fast, ok_a=ok_a, guards=g)


def debug_fdiv_b4(b, a1, a2, a3, a4):
    """fdiv_ok_b4(b, a1, a2, a3, a4) -> (ok uint32 per tuple, the four div_fast quotients (n, 4), disturbed guard words)"""
    b = _dbg_array(b, np.float64, "b")
    n = len(b)
    a1, a2, a3, a4 = (_dbg_array(x, np.float64, f"a{k + 1}", n) for k, x in enumerate((a1, a2, a3, a4)))
    ok, q = _prefilled(n, np.uint32), _prefilled(4 * n, np.float64)
    fn = _dbg_fn("esvo_debug_fdiv_b4", [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p, C.c_void_p])
    g = _dbg_rc(fn(b.ctypes.data, a1.ctypes.data, a2.ctypes.data, a3.ctypes.data, a4.ctypes.data, n, ok.ctypes.data, q.ctypes.data),
                "esvo_debug_fdiv_b4")
    return ok, q.reshape(n, 4), g


def debug_recip(b):
    """(make_recip(b).y, recip_refined(b), disturbed guard words): the refined reciprocals themselves"""
    b = _dbg_array(b, np.float64, "b")
    y_make, y_ref = _prefilled(len(b), np.float64), _prefilled(len(b), np.float64)
    fn = _dbg_fn("esvo_debug_recip", [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p])
    g = _dbg_rc(fn(b.ctypes.data, len(b), y_make.ctypes.data, y_ref.ctypes.data), "esvo_debug_recip")
    return y_make, y_ref, g


def debug_sqrt_moderate(x):
    """sqrt_moderate(x) -> (values, disturbed guard words)"""
    x = _dbg_array(x, np.float64, "x")
    out = _prefilled(len(x), np.float64)
    fn = _dbg_fn("esvo_debug_sqrt_moderate", [C.c_void_p, C.c_size_t, C.c_void_p])
    g = _dbg_rc(fn(x.ctypes.data, len(x), out.ctypes.data), "esvo_debug_sqrt_moderate")
    return out, g


def debug_live_allocations():
    """(live allocations, live bytes) of the process: every device / pinned buffer a handle owns (devmem.hpp)"""
    out = (C.c_size_t * 2)()
    fn = getattr(load(), "esvo_debug_live_allocations")
    fn.argtypes, fn.restype = [C.c_void_p], None
    fn(out)
    return int(out[0]), int(out[1])


def debug_devmem_selftest(pinned=False):
    """the owning buffer type step by step against its ledger: 0, or the number of the first step that failed"""
    return _dbg_rc(_dbg_fn("esvo_debug_devmem_selftest", [C.c_int])(1 if pinned else 0), "esvo_debug_devmem_selftest")


class BagReader:
    """rosbag format 2.0 reader of the C-ABI (esvo_bag_*): iterates (topic, bag stamp ns, serialised EventArray bytes)"""

    def __init__(self, path):
        self.lib = load()
        b = C.c_void_p()
        rc = self.lib.esvo_bag_open(path.encode(), C.byref(b))
        if rc != 0:
            raise EsvoError(f"esvo_bag_open failed ({rc}): {self.lib.esvo_last_error(None).decode(errors='replace')}")
        self.b = b

    def close(self):
        if getattr(self, "b", None):
            self.lib.esvo_bag_close(self.b)
            self.b = None

    def __del__(self):
        self.close()

    def messages(self, topic=None):
        while True:
            msg, nb, st, tp = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_char_p()
            rc = self.lib.esvo_bag_next_event_array(self.b, topic.encode() if topic else None, C.byref(msg), C.byref(nb), C.byref(st), C.byref(tp))
            if rc == 1:
                return
            if rc != 0:
                raise EsvoError(f"bag read failed ({rc}): {self.lib.esvo_bag_last_error(self.b).decode(errors='replace')}")
            yield tp.value.decode(errors='replace'), int(st.value), C.string_at(msg.value, nb.value)


def voxel_filter(xyz, leaf):
    """pcl::VoxelGrid with a cubic leaf (host helper of the C-ABI)"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = np.empty((max(len(xyz), 1), 3), np.float32)
    n = C.c_size_t()
    rc = load().esvo_voxel_filter_xyz(xyz.ctypes.data, xyz.shape[0], float(leaf), out.ctypes.data, out.shape[0], C.byref(n))
    if rc != 0:
        raise EsvoError(f"esvo_voxel_filter_xyz failed ({rc})")
    return out[: n.value].copy()


def comm_unique_id():
    """ncclGetUniqueId through the C-ABI (128 bytes; create on one rank, hand to the others)"""
    buf = (C.c_uint8 * 128)()
    rc = load().esvo_comm_unique_id(buf)
    if rc != 0:
        raise EsvoError(f"esvo_comm_unique_id failed ({rc}): {load().esvo_last_error(None).decode(errors='replace')}")
    return bytes(buf)


def comm_rccl_info():
    """(ncclGetVersion code, path of the RCCL shared object the C library resolved)"""
    v, buf = C.c_int(), C.create_string_buffer(512)
    rc = load().esvo_comm_rccl_info(C.byref(v), buf, 512)
    if rc != 0:
        raise EsvoError(f"esvo_comm_rccl_info failed ({rc}): {load().esvo_last_error(None).decode(errors='replace')}")
    return int(v.value), buf.value.decode(errors="replace")


class PinnedEvents:
    """an esvo_event_t array in pinned host memory (esvo_host_alloc): what a node's message pool would be"""

    def __init__(self, n):
        self.lib = load()
        self.ptr = C.c_void_p()
        rc = self.lib.esvo_host_alloc(max(int(n), 1) * EVENT_DTYPE.itemsize, C.byref(self.ptr))
        if rc:
            raise EsvoError(f"esvo_host_alloc: {rc}")
        buf = (C.c_char * (max(int(n), 1) * EVENT_DTYPE.itemsize)).from_address(self.ptr.value)
        self.array = np.frombuffer(buf, dtype=EVENT_DTYPE, count=int(n))

    def free(self):
        if self.ptr:
            self.array = None
            self.lib.esvo_host_free(self.ptr)
            self.ptr = None


def _column(a, name):
    """(address, numpy dtype, length, on_device, what to keep alive) of one column: a numpy array (or anything numpy takes as one),
    or device / host memory behind data_ptr() + is_cuda (torch) or __cuda_array_interface__; one-dimensional and contiguous"""
    if hasattr(a, "data_ptr") and hasattr(a, "is_cuda"):
        if a.dim() != 1 or not a.is_contiguous():
            raise ValueError(f"event columns: {name} must be one-dimensional and contiguous")
        return int(a.data_ptr()), np.dtype(str(a.dtype).replace("torch.", "")), int(a.numel()), bool(a.is_cuda), a
    cai = getattr(a, "__cuda_array_interface__", None)
    if cai is not None:
        shape, dt = tuple(cai["shape"]), np.dtype(cai["typestr"])
        if len(shape) != 1 or cai.get("strides") not in (None, (dt.itemsize,)):
            raise ValueError(f"event columns: {name} must be one-dimensional and contiguous")
        return int(cai["data"][0]), dt, int(shape[0]), True, a
    arr = np.asarray(a)
    if arr.ndim != 1:
        raise ValueError(f"event columns: {name} must be one-dimensional")
    arr = np.ascontiguousarray(arr)
    return arr.ctypes.data, arr.dtype, len(arr), False, arr


def event_columns_struct(x, y, t, p=None, unit="ns", t_offset=0):
    """an esvo_event_columns_t over the given columns -> (struct, (n, what the struct's pointers need alive)); the types come from
    the dtypes (abi.column_t_type / column_p_type), anything else is refused with a ValueError"""
    cols = {"x": _column(x, "x"), "y": _column(y, "y"), "t": _column(t, "t")}
    if p is not None:
        cols["p"] = _column(p, "p")
    n = cols["t"][2]
    if any(c[2] != n for c in cols.values()):
        raise ValueError("event columns: the columns differ in length: " + ", ".join(f"{k} {c[2]}" for k, c in cols.items()))
    if len({c[3] for c in cols.values()}) != 1:
        raise ValueError("event columns: all columns must be in host memory or all in device memory")
    for k in ("x", "y"):
        if cols[k][1].itemsize != 2 or cols[k][1].kind not in "iu":
            raise ValueError(f"event columns: {k} must be uint16 or int16, not {cols[k][1]}")
    s = EventColumnsStruct()
    s.x, s.y, s.t, s.p = cols["x"][0] or None, cols["y"][0] or None, cols["t"][0] or None, (cols["p"][0] or None) if p is not None else None
    s.t_type = column_t_type(cols["t"][1], unit)
    s.p_type = column_p_type(cols["p"][1]) if p is not None else P_U8
    s.t_offset = check_t_offset(t_offset)
    s.memory = MEM_DEVICE if cols["t"][3] else MEM_HOST
    return s, (n, [c[4] for c in cols.values()])


def columns_to_events_c(x, y, t, p=None, unit="ns", t_offset=0):
    """esvo_event_columns_to_events on host columns -> the esvo_event_t records; abi.ColumnsError (first_bad) for an invalid element"""
    s, (n, _keep) = event_columns_struct(x, y, t, p, unit, t_offset)
    out, bad = np.zeros(n, EVENT_DTYPE), C.c_size_t(0)
    rc = load().esvo_event_columns_to_events(C.addressof(s), n, out.ctypes.data if n else None, C.byref(bad))
    if rc == ERR_INVALID_ARG and bad.value < n:
        raise ColumnsError(bad.value)
    if rc != 0:
        raise EsvoError(f"esvo_event_columns_to_events failed ({rc}): {load().esvo_last_error(None).decode(errors='replace')}", code=rc)
    return out


def event_columns_sizes():
    """sizeof(esvo_event_columns_t), 0, 0, 0 (esvo_event_columns_sizes)"""
    out = (C.c_size_t * 4)()
    load().esvo_event_columns_sizes(out)
    return list(out)


def evt3_sizes():
    """sizeof(esvo_evt3_state_t), sizeof(esvo_evt3_counts_t), 0, 0 (esvo_evt3_sizes)"""
    out = (C.c_size_t * 4)()
    load().esvo_evt3_sizes(out)
    return list(out)


def evt2_sizes():
    """sizeof(esvo_evt2_state_t), sizeof(esvo_evt2_counts_t), 0, 0 (esvo_evt2_sizes)"""
    out = (C.c_size_t * 4)()
    load().esvo_evt2_sizes(out)
    return list(out)


def event_filter_sizes():
    """sizeof(esvo_event_filter_t), sizeof(esvo_event_filter_counts_t), 0, 0 (esvo_event_filter_sizes)"""
    out = (C.c_size_t * 4)()
    load().esvo_event_filter_sizes(out)
    return list(out)


def event_filter_host(events, width, height, refractory_ns=0, support_ns=0, mask=None, last=None, cap=None, want_verdicts=True):
    """esvo_event_filter_host: the filter's rule on the host -> (verdicts uint8 [n], kept records, last (height, width) uint64, counts
    dict).  last: the state to resume from (None: all zero), not modified -- the returned image is the advanced copy.  cap: room of
    the output (None: n; 0 with no output: count only)."""
    ev = np.ascontiguousarray(events, EVENT_DTYPE)
    n = len(ev)
    f, _keep = event_filter_struct(refractory_ns, support_ns, mask, width, height)
    L = np.zeros((int(height), int(width)), np.uint64) if last is None else np.array(last, np.uint64).reshape(int(height), int(width)).copy()
    verdict = np.zeros(n, np.uint8)
    room = n if cap is None else int(cap)
    out = np.zeros(max(room, 1), EVENT_DTYPE)
    n_out, cnt = C.c_size_t(0), EventFilterCounts()
    rc = load().esvo_event_filter_host(C.addressof(f), int(width), int(height), L.ctypes.data, ev.ctypes.data if n else None, n,
                                       verdict.ctypes.data if want_verdicts and n else None, out.ctypes.data, room, C.byref(n_out), C.addressof(cnt))
    if rc != 0:
        raise EsvoError(f"esvo_event_filter_host failed ({rc}): {load().esvo_last_error(None).decode(errors='replace')}", code=rc)
    return verdict, out[:n_out.value].copy(), L, cnt.as_dict()


def event_burst_sizes():
    """sizeof(esvo_event_burst_t), sizeof(esvo_event_burst_counts_t), 0, 0 (esvo_event_burst_sizes)"""
    out = (C.c_size_t * 4)()
    load().esvo_event_burst_sizes(out)
    return list(out)


def event_burst_filter_host(events, width, height, mode=0, burst_ns=0, refractory_ns=0, support_ns=0, mask=None, bstamp=None, bflags=None, last=None,
                            cap=None, reserved=(0, 0, 0)):
    """esvo_event_burst_filter_host: the filter's rule with its burst stage on the host -> (verdicts uint8 [n], kept records, bstamp
    (height, width) uint64, bflags (height, width) uint8, last (height, width) uint64, burst counts dict, filter counts dict).
    bstamp / bflags / last: the state to resume from (None: all zero), not modified -- the returned images are the advanced copies."""
    ev = np.ascontiguousarray(events, EVENT_DTYPE)
    n, shape = len(ev), (int(height), int(width))
    b = event_burst_struct(mode, burst_ns, reserved)
    f, _keep = event_filter_struct(refractory_ns, support_ns, mask, width, height)
    S = np.zeros(shape, np.uint64) if bstamp is None else np.array(bstamp, np.uint64).reshape(shape).copy()
    G = np.zeros(shape, np.uint8) if bflags is None else np.array(bflags, np.uint8).reshape(shape).copy()
    L = np.zeros(shape, np.uint64) if last is None else np.array(last, np.uint64).reshape(shape).copy()
    verdict = np.zeros(n, np.uint8)
    room = n if cap is None else int(cap)
    out = np.zeros(max(room, 1), EVENT_DTYPE)
    n_out, bc, fc = C.c_size_t(0), EventBurstCounts(), EventFilterCounts()
    rc = load().esvo_event_burst_filter_host(C.addressof(b), C.addressof(f), shape[1], shape[0], S.ctypes.data, G.ctypes.data, L.ctypes.data,
                                             ev.ctypes.data if n else None, n, verdict.ctypes.data if n else None, out.ctypes.data, room,
                                             C.byref(n_out), C.addressof(bc), C.addressof(fc))
    if rc != 0:
        raise EsvoError(f"esvo_event_burst_filter_host failed ({rc}): {load().esvo_last_error(None).decode(errors='replace')}", code=rc)
    return verdict, out[:n_out.value].copy(), S, G, L, bc.as_dict(), fc.as_dict()


def event_survey_sizes():
    """sizeof() of esvo_event_survey_t, esvo_event_survey_stats_t, esvo_hot_pixel_rule_t, esvo_hot_pixel_report_t (esvo_event_survey_sizes)"""
    out = (C.c_size_t * 4)()
    load().esvo_event_survey_sizes(out)
    return list(out)


def event_survey_host(events, width, height, counts=None, stats=None):
    """esvo_event_survey_host: the survey's counting on the host -> (counts (2, height, width) uint32, stats dict).  counts / stats:
    what to resume from (None: zero), not modified -- the returned ones are the advanced copies."""
    ev = np.ascontiguousarray(events, EVENT_DTYPE)
    shape = (2, int(height), int(width))
    cnt = np.zeros(shape, np.uint32) if counts is None else np.array(counts, np.uint32).reshape(shape).copy()
    st = event_survey_stats(stats)
    rc = load().esvo_event_survey_host(int(width), int(height), cnt.ctypes.data, C.addressof(st), ev.ctypes.data if len(ev) else None, len(ev))
    if rc != 0:
        raise EsvoError(f"esvo_event_survey_host failed ({rc}): {load().esvo_last_error(None).decode(errors='replace')}", code=rc)
    return cnt, st.as_dict()


def hot_pixel_mask_host(counts, stats, width, height, **rule):
    """esvo_hot_pixel_mask_host: the hot-pixel rule on the host -> (mask (height, width) uint8, report dict).  counts: (2, height, width);
    stats: a dict with t_first / t_last / events_in (the rate test's duration); rule: the fields of esvo_hot_pixel_rule_t."""
    shape = (2, int(height), int(width))
    cnt = np.ascontiguousarray(np.asarray(counts, np.uint32).reshape(shape))
    st, r, rep = event_survey_stats(stats), hot_pixel_rule(**rule), HotPixelReport()
    mask = np.zeros(shape[1:], np.uint8)
    rc = load().esvo_hot_pixel_mask_host(C.addressof(r), int(width), int(height), cnt.ctypes.data, C.addressof(st), mask.ctypes.data, C.addressof(rep))
    if rc != 0:
        raise EsvoError(f"esvo_hot_pixel_mask_host failed ({rc}): {load().esvo_last_error(None).decode(errors='replace')}", code=rc)
    return mask, rep.as_dict()


def abi_sizes():
    out = (C.c_size_t * 8)()
    load().esvo_abi_sizes(out)
    return list(out)


def em_sizes():
    """sizeof() of esvo_em_params_t, esvo_em_selection_t, esvo_em_stats_t (esvo_em_sizes)"""
    out = (C.c_size_t * 4)()
    load().esvo_em_sizes(out)
    return list(out)


def lm_sizes():
    """sizeof(esvo_lm_stats_t), ESVO_LM_SCALE_COUNT_ONLY, 0, 0 (esvo_lm_sizes)"""
    out = (C.c_size_t * 4)()
    load().esvo_lm_sizes(out)
    return list(out)


def sgm_sizes():
    """sizeof(esvo_sgm_stats_t), numDisparities, 0, 0 (esvo_sgm_sizes)"""
    out = (C.c_size_t * 4)()
    load().esvo_sgm_sizes(out)
    return list(out)


def gpc_sizes():
    """sizeof(esvo_gpc_params_t), sizeof(esvo_gpc_stats_t), the default capacity_points, 0 (esvo_gpc_sizes)"""
    out = (C.c_size_t * 4)()
    load().esvo_gpc_sizes(out)
    return list(out)


def track_sizes():
    """sizeof() of esvo_track_solve_params_t, esvo_track_iter_t, esvo_track_solve_info_t, and the iteration limit (esvo_track_sizes)"""
    out = (C.c_size_t * 4)()
    load().esvo_track_sizes(out)
    return list(out)


def _p(a):
    return None if a is None else a.ctypes.data


class Esvo:
    """One handle = one GPU: TS-left, TS-right and the mapper behind the same device state."""

    def __init__(self, params: ParamsStruct, rig, device=0):
        self.lib = load()
        self.rig, self.params = rig, params
        self.W, self.H = rig.width, rig.height
        self._cl, self._cr = rig.left.as_struct(), rig.right.as_struct()
        h = C.c_void_p()
        rc = self.lib.esvo_create(C.addressof(params), C.addressof(self._cl), C.addressof(self._cr), int(device), C.byref(h))
        if rc != 0:
            raise EsvoError(f"esvo_create failed ({rc}): {self.lib.esvo_last_error(None).decode(errors='replace')}")
        self.h = h
        self._poses = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.esvo_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _ck(self, rc):
        if rc != 0:
            raise EsvoError(f"esvo call failed ({rc}): {self.lib.esvo_last_error(self.h).decode(errors='replace')}", code=rc)

    # ---- lifecycle
    def reset(self):
        self._ck(self.lib.esvo_reset(self.h))

    def set_params(self, params):
        self._ck(self.lib.esvo_set_params(self.h, C.addressof(params)))
        self.params = params

    def set_stream(self, stream_ptr):
        self._ck(self.lib.esvo_set_stream(self.h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._ck(self.lib.esvo_synchronize(self.h))

    # ---- Time Surface (esvo_time_surface node: eventsCallback / createTimeSurfaceAtTime)
    def ts_push_events(self, cam, ev):
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        self._ck(self.lib.esvo_ts_push_events(self.h, int(cam), ev.ctypes.data, ev.shape[0]))

    def ts_push_events_async(self, cam, ev):
        """enqueue the copy and return; `ev` (ideally pinned: pinned_events) is kept alive here until ts_push_wait(cam)"""
        assert ev.dtype == EVENT_DTYPE and ev.flags["C_CONTIGUOUS"]
        self._async_keep = getattr(self, "_async_keep", {0: [], 1: []})
        self._async_keep[int(cam)].append(ev)
        self._ck(self.lib.esvo_ts_push_events_async(self.h, int(cam), ev.ctypes.data, ev.shape[0]))

    def ts_push_wait(self, cam):
        self._ck(self.lib.esvo_ts_push_wait(self.h, int(cam)))
        if hasattr(self, "_async_keep"):
            self._async_keep[int(cam)].clear()

    def ts_push_event_array(self, cam, msg):
        """stage one serialised dvs_msgs/EventArray (bytes / uint8 array, ROS1 wire format); returns its event count"""
        buf = np.frombuffer(msg, np.uint8) if isinstance(msg, (bytes, bytearray, memoryview)) else np.ascontiguousarray(msg, np.uint8)
        n = C.c_size_t()
        self._ck(self.lib.esvo_ts_push_event_array(self.h, int(cam), buf.ctypes.data, buf.size, C.byref(n)))
        return int(n.value)

    def ts_push_columns(self, cam, x, y, t, p=None, unit="ns", t_offset=0):
        """stage events from columns (esvo_ts_push_event_columns): x, y 16-bit; t int64 with unit "ns" / "us" or uint32 with unit
        "us", stamp = (t + t_offset) * unit; p uint8 / bool (!= 0 is ON), int8 (> 0 is ON) or None (all ON).  The columns are numpy
        arrays, or anything with data_ptr() / is_cuda (torch tensors) or __cuda_array_interface__: all in host memory or all in
        device memory of the handle's GPU.  Device columns must be complete: torch's current stream is synchronised here, a producer
        on any other stream is the caller's to wait for.  Synchronous: the columns may be reused when the call returns."""
        s, keep = event_columns_struct(x, y, t, p, unit, t_offset)
        if s.memory == MEM_DEVICE:
            import sys
            torch = sys.modules.get("torch")
            if torch is not None and torch.cuda.is_available():
                torch.cuda.current_stream().synchronize()
        self._ck(self.lib.esvo_ts_push_event_columns(self.h, int(cam), C.addressof(s), keep[0]))

    def ts_push_evt3(self, cam, words, t_offset_us=0):
        """stage events from Prophesee EVT 3.0 words (esvo_ts_push_evt3): `words` is bytes / bytearray / memoryview, a numpy uint16
        array, or uint16 / int16 device memory behind data_ptr() / is_cuda (a torch tensor) or __cuda_array_interface__, one-dimensional
        and contiguous.  The camera's decoder state carries over from call to call (evt3_state / reset).  Device words must be
        complete: torch's current stream is synchronised here.  Synchronous.  Returns the number of events the words emitted."""
        if isinstance(words, (bytes, bytearray, memoryview)):
            words = evt3_words(words)
        addr, dt, n, on_device, _keep = _column(words, "words")
        if dt.itemsize != 2 or dt.kind not in "iu":
            raise ValueError(f"EVT3 words: uint16 is expected, not {dt}")
        if on_device:
            import sys
            torch = sys.modules.get("torch")
            if torch is not None and torch.cuda.is_available():
                torch.cuda.current_stream().synchronize()
        n_ev = C.c_size_t(0)
        self._ck(self.lib.esvo_ts_push_evt3(self.h, int(cam), addr or None, 2 * n, MEM_DEVICE if on_device else MEM_HOST,
                                            check_t_offset(t_offset_us), C.byref(n_ev)))
        return int(n_ev.value)

    def evt3_state(self, cam, set=None):
        """the camera's EVT 3.0 decoder state (an abi.Evt3State); set: an Evt3State that replaces it (a reader seeks or resumes)"""
        got = Evt3State()
        self._ck(self.lib.esvo_ts_evt3_state(self.h, int(cam), C.addressof(got), None if set is None else C.addressof(set)))
        return got

    def evt3_stats(self, cam):
        """running totals of the camera's ts_push_evt3 calls as a dict (esvo_ts_evt3_stats); cleared by reset"""
        tot = Evt3Counts()
        self._ck(self.lib.esvo_ts_evt3_stats(self.h, int(cam), C.addressof(tot)))
        return tot.as_dict()

    def debug_evt3_device_min(self, n_words):
        """packets of fewer words are decoded on the host (esvo_debug_evt3_device_min; not part of the ABI) -> the previous bound"""
        fn = _dbg_fn("esvo_debug_evt3_device_min", [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)])
        prev = C.c_size_t(0)
        self._ck(fn(self.h, int(n_words), C.byref(prev)))
        return int(prev.value)

    def ts_push_evt2(self, cam, words, format, t_offset_us=0):
        """stage events from Prophesee EVT 2.0 / 2.1 words (esvo_ts_push_evt2; format: abi.EVT_2_0, EVT_2_1 or EVT_2_1_LEGACY): `words`
        is bytes / bytearray / memoryview, a numpy array of 4-byte integers (two per EVT 2.1 word; 8-byte integers for EVT 2.1 as
        well), or such device memory behind data_ptr() / is_cuda (a torch tensor) or __cuda_array_interface__, one-dimensional and
        contiguous; a 4-byte aligned base suffices.  The camera's decoder state carries over from call to call (evt2_state / reset).
        Device words must be complete: torch's current stream is synchronised here.  Synchronous.  Returns the number of events."""
        if isinstance(words, (bytes, bytearray, memoryview)):
            words = evt2_words(words, format)
        addr, dt, n, on_device, _keep = _column(words, "words")
        if dt.kind not in "iu" or dt.itemsize not in ((4,) if format == 20 else (4, 8)):
            raise ValueError(f"EVT2 words: 4-byte integers (or 8-byte ones for EVT 2.1) are expected, not {dt}")
        if on_device:
            import sys
            torch = sys.modules.get("torch")
            if torch is not None and torch.cuda.is_available():
                torch.cuda.current_stream().synchronize()
        n_ev = C.c_size_t(0)
        self._ck(self.lib.esvo_ts_push_evt2(self.h, int(cam), addr or None, dt.itemsize * n, int(format), MEM_DEVICE if on_device else MEM_HOST,
                                            check_t_offset(t_offset_us), C.byref(n_ev)))
        return int(n_ev.value)

    def ts_filter_configure(self, cam, refractory_ns=0, support_ns=0, mask=None, off=False):
        """the camera's event filter (esvo_ts_filter_configure): hot-pixel mask ((H, W), non-zero = masked, copied), refractory period
        and neighbour support in ns (0: that test is off); zeroes the camera's `last` image, keeps the totals.  off=True switches the
        filter off and frees its memory.  From then on every ts_push_* call of the camera stages only the events the filter keeps."""
        if off:
            self._ck(self.lib.esvo_ts_filter_configure(self.h, int(cam), None))
            return
        f, _keep = event_filter_struct(refractory_ns, support_ns, mask, self.rig.width, self.rig.height)
        self._ck(self.lib.esvo_ts_filter_configure(self.h, int(cam), C.addressof(f)))

    def ts_filter_stats(self, cam):
        """totals of the camera's filter since create / reset as a dict: events_in = kept + outside + masked + refractory + unsupported"""
        tot = EventFilterCounts()
        self._ck(self.lib.esvo_ts_filter_stats(self.h, int(cam), C.addressof(tot)))
        return tot.as_dict()

    def ts_filter_state(self, cam, set=None):
        """the camera's `last` image, (H, W) uint64 ns stamps (esvo_ts_filter_state); set: an image that replaces it afterwards"""
        H, W = self.rig.height, self.rig.width
        got = np.zeros((H, W), np.uint64)
        new = None if set is None else np.ascontiguousarray(np.asarray(set, np.uint64).reshape(H, W))
        self._ck(self.lib.esvo_ts_filter_state(self.h, int(cam), got.ctypes.data, None if new is None else new.ctypes.data))
        return got

    def ts_burst_configure(self, cam, mode=0, burst_ns=0, reserved=(0, 0, 0)):
        """the burst stage of the camera's filter (esvo_ts_burst_configure): abi.BURST_TRAIL keeps the first event of every same-polarity
        burst of a pixel, BURST_STC_CUT_TRAIL the second, BURST_STC_KEEP_TRAIL all but the first; burst_ns: the largest gap inside a
        burst.  Zeroes the stage's state, keeps its totals; abi.BURST_OFF switches it off and frees its memory.  The camera's filter
        must be configured (ts_filter_configure(cam) with no arguments passes everything)."""
        b = event_burst_struct(mode, burst_ns, reserved)
        self._ck(self.lib.esvo_ts_burst_configure(self.h, int(cam), C.addressof(b)))

    def ts_burst_stats(self, cam):
        """totals of the camera's burst stage since create / reset as a dict: judged = passed + dropped"""
        tot = EventBurstCounts()
        self._ck(self.lib.esvo_ts_burst_stats(self.h, int(cam), C.addressof(tot)))
        return tot.as_dict()

    def ts_burst_state(self, cam, set=None):
        """the stage's state (esvo_ts_burst_state) -> (bstamp (H, W) uint64, bflags (H, W) uint8); set: a (bstamp, bflags) pair that
        replaces it afterwards"""
        H, W = self.rig.height, self.rig.width
        st, fl = np.zeros((H, W), np.uint64), np.zeros((H, W), np.uint8)
        new = None if set is None else (np.ascontiguousarray(np.asarray(set[0], np.uint64).reshape(H, W)), np.ascontiguousarray(np.asarray(set[1], np.uint8).reshape(H, W)))
        self._ck(self.lib.esvo_ts_burst_state(self.h, int(cam), st.ctypes.data, fl.ctypes.data, None if new is None else new[0].ctypes.data,
                                              None if new is None else new[1].ctypes.data))
        return st, fl

    def ts_survey_begin(self, cam, count_only=False, flags=None, reserved=(0, 0, 0)):
        """opens the camera's event survey (esvo_ts_survey_begin): per-pixel counts of every packet its push calls accept, kept on the
        device.  The camera's filter must be configured.  count_only: packets are decoded and counted and nothing is staged."""
        s = EventSurveyStruct()
        s.flags = int(flags) if flags is not None else (1 if count_only else 0)
        s.reserved[:] = [int(v) for v in reserved]
        self._ck(self.lib.esvo_ts_survey_begin(self.h, int(cam), C.addressof(s)))

    def ts_survey_end(self, cam):
        self._ck(self.lib.esvo_ts_survey_end(self.h, int(cam)))

    def ts_survey_stats(self, cam):
        """the survey's stats as a dict: events_in, outside, packets, t_first, t_last"""
        st = EventSurveyStats()
        self._ck(self.lib.esvo_ts_survey_stats(self.h, int(cam), C.addressof(st)))
        return st.as_dict()

    def ts_survey_state(self, cam, set=None, stats=None):
        """the survey's counts, (2, H, W) uint32, plane = polarity (esvo_ts_survey_state); set: counts that replace them afterwards,
        stats: a dict that replaces the stats with them"""
        shape = (2, self.rig.height, self.rig.width)
        got = np.zeros(shape, np.uint32)
        new = None if set is None else np.ascontiguousarray(np.asarray(set, np.uint32).reshape(shape))
        st = None if stats is None else event_survey_stats(stats)
        self._ck(self.lib.esvo_ts_survey_state(self.h, int(cam), got.ctypes.data, None if new is None else new.ctypes.data,
                                               None if st is None else C.addressof(st)))
        return got

    def ts_survey_mask(self, cam, install=0, want_mask=True, **rule):
        """esvo_ts_survey_mask: the hot-pixel rule on the survey's counts, on the device -> (mask (H, W) uint8 or None, report dict).
        install: abi.MASK_KEEP / MASK_REPLACE / MASK_UNION puts the mask into the camera's filter, device to device."""
        r, rep = hot_pixel_rule(**rule), HotPixelReport()
        mask = np.zeros((self.rig.height, self.rig.width), np.uint8) if want_mask else None
        self._ck(self.lib.esvo_ts_survey_mask(self.h, int(cam), C.addressof(r), None if mask is None else mask.ctypes.data, int(install), C.addressof(rep)))
        return mask, rep.as_dict()

    def evt2_state(self, cam, set=None):
        """the camera's EVT 2.x decoder state (an abi.Evt2State); set: an Evt2State that replaces it (a reader seeks or resumes)"""
        got = Evt2State()
        self._ck(self.lib.esvo_ts_evt2_state(self.h, int(cam), C.addressof(got), None if set is None else C.addressof(set)))
        return got

    def evt2_stats(self, cam):
        """running totals of the camera's ts_push_evt2 calls as a dict (esvo_ts_evt2_stats); cleared by reset"""
        tot = Evt2Counts()
        self._ck(self.lib.esvo_ts_evt2_stats(self.h, int(cam), C.addressof(tot)))
        return tot.as_dict()

    def debug_evt2_device_min(self, n_bytes):
        """packets of fewer bytes are decoded on the host, for every EVT 2.x format (esvo_debug_evt2_device_min; not part of the ABI)
        -> the previous bound of EVT 2.0"""
        fn = _dbg_fn("esvo_debug_evt2_device_min", [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)])
        prev = C.c_size_t(0)
        self._ck(fn(self.h, int(n_bytes), C.byref(prev)))
        return int(prev.value)

    def debug_ts_ring(self, cam, first_abs=None, n=None):
        """(records, stamps, ring_base, ring_next) of a camera's event ring (esvo_debug_ts_ring; not part of the ABI): the records and
        the host's stamp mirror of the absolute indices [first_abs, first_abs + n), by default everything the ring still holds"""
        fn = _dbg_fn("esvo_debug_ts_ring", [C.c_void_p, C.c_int, C.c_uint64, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p])
        bounds = np.zeros(2, np.uint64)
        self._ck(fn(self.h, int(cam), 0, 0, None, None, bounds.ctypes.data))
        first_abs = int(bounds[0]) if first_abs is None else int(first_abs)
        n = int(bounds[1]) - first_abs if n is None else int(n)
        ev, stamps = np.zeros(max(n, 0), EVENT_DTYPE), np.zeros(max(n, 0), np.uint64)
        self._ck(fn(self.h, int(cam), first_abs, max(n, 0), ev.ctypes.data if n > 0 else None, stamps.ctypes.data if n > 0 else None,
                    bounds.ctypes.data))
        return ev, stamps, int(bounds[0]), int(bounds[1])

    def ts_push_bag(self, cam, bag, topic, until_ns=0):
        """stage the dvs_msgs/EventArray messages of `topic` (bag time < until_ns; 0: all) from a BagReader; returns the event count"""
        n = C.c_size_t()
        self._ck(self.lib.esvo_ts_push_bag(self.h, int(cam), bag.b, topic.encode() if topic else None, int(until_ns), C.byref(n)))
        return int(n.value)

    def ts_render(self, cam, t_ns, download=True):
        out = np.empty((self.H, self.W), np.uint8) if download else None
        self._ck(self.lib.esvo_ts_render(self.h, int(cam), int(t_ns), _p(out)))
        return out

    # ---- Time-Surface history (the nodes' TS_history_ on the device)
    def ts_history_configure(self, length):
        """retain `length` pairs by stamp (TS_HISTORY_LENGTH: 100); 0 switches the history off.  Empties it."""
        self._ck(self.lib.esvo_ts_history_configure(self.h, int(length)))

    def ts_history(self):
        """(stamps uint64 ascending, cams uint8: bit 0 left present, bit 1 right present)"""
        n = C.c_size_t(0)
        self._ck(self.lib.esvo_ts_history_list(self.h, None, None, 0, C.byref(n)))
        t, cams = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.uint8)
        self._ck(self.lib.esvo_ts_history_list(self.h, t.ctypes.data, cams.ctypes.data, len(t), C.byref(n)))
        return t[: n.value].copy(), cams[: n.value].copy()

    def ts_history_get(self, t_ns, cam):
        out = np.empty((self.H, self.W), np.uint8)
        self._ck(self.lib.esvo_ts_history_get(self.h, int(t_ns), int(cam), out.ctypes.data))
        return out

    def ts_history_put(self, t_ns, cam, img):
        img = np.ascontiguousarray(img, np.uint8)
        if img.size != self.W * self.H:
            raise ValueError(f"a {self.W} x {self.H} mono8 image is expected, not {img.shape}")
        self._ck(self.lib.esvo_ts_history_put(self.h, int(t_ns), int(cam), img.ctypes.data))

    def set_observation_at(self, t_ns, T_world_cam):
        """set_observation(t_ns, left, right, T) on the retained pair of that stamp"""
        T = np.ascontiguousarray(T_world_cam, np.float64).reshape(16)
        self._ck(self.lib.esvo_map_set_observation_at(self.h, int(t_ns), T.ctypes.data))

    def track_set_current_at(self, t_ns, kernel_size=5):
        """track_set_current(left, kernel_size) on the retained left frame of that stamp"""
        self._ck(self.lib.esvo_track_set_current_at(self.h, int(t_ns), int(kernel_size)))

    def ts_history_select_observation(self, pose_fn=None, initialization=False):
        """dataTransferring's choice among the retained complete pairs: (t_ns, 4x4 T_world_cam), or None where the node would
        return false.  pose_fn as for ts_history_select."""
        cb, raised = _pose_trampoline(pose_fn)
        t, T = C.c_uint64(0), np.zeros(16, np.float64)
        rc = self.lib.esvo_ts_history_select_observation(self.h, 1 if initialization else 0, cb, None, C.byref(t), T.ctypes.data)
        if raised:
            raise raised[0]
        if rc == ESVO_AGAIN:
            return None
        self._ck(rc)
        return int(t.value), T.reshape(4, 4)

    # ---- mapper, stage-wise (EventBM / DepthProblemSolver / DepthFusion seams)
    def ts_render_forward(self, cam, t_ns, download=True):
        """esvo_ts_render_forward: the camera's Time Surface in the reference's FORWARD mode"""
        out = np.empty((self.H, self.W), np.uint8) if download else None
        self._ck(self.lib.esvo_ts_render_forward(self.h, int(cam), int(t_ns), _p(out)))
        return out

    def set_observation(self, t_ns, ts_left, ts_right, T_world_cam):
        l = None if ts_left is None else np.ascontiguousarray(ts_left, np.uint8)
        r = None if ts_right is None else np.ascontiguousarray(ts_right, np.uint8)
        T = np.ascontiguousarray(T_world_cam, np.float64).reshape(16)
        self._ck(self.lib.esvo_map_set_observation(self.h, int(t_ns), _p(l), _p(r), T.ctypes.data))

    def set_poses(self, stamps, poses):
        st = np.ascontiguousarray(stamps, np.uint64)
        T = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        self._poses = T
        self._ck(self.lib.esvo_map_set_poses(self.h, st.ctypes.data, T.ctypes.data, st.shape[0]))

    def match(self, ev, stamps=None, poses=None):
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        if stamps is not None:
            self.set_poses(stamps, poses)
        out = np.zeros(max(ev.shape[0], 1), MATCH_DTYPE)
        n = C.c_size_t(0)
        self._ck(self.lib.esvo_map_match(self.h, ev.ctypes.data, ev.shape[0], None, None, 0, out.ctypes.data,
                                         out.shape[0], C.byref(n)))
        return out[: n.value]

    def refine(self, matches, cull=True):
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        out = np.zeros(max(m.shape[0], 1), DEPTH_POINT_DTYPE)
        n = C.c_size_t(0)
        self._ck(self.lib.esvo_map_refine(self.h, m.ctypes.data, m.shape[0], int(cull), out.ctypes.data, out.shape[0],
                                          C.byref(n)))
        return out[: n.value]

    def push_frame(self, pts, poses=None):
        pts = np.ascontiguousarray(pts, dtype=DEPTH_POINT_DTYPE)
        T = self._poses if poses is None else np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        self._ck(self.lib.esvo_map_push_frame(self.h, pts.ctypes.data, pts.shape[0], T.ctypes.data, T.shape[0]))

    def fuse(self):
        n = C.c_size_t(0)
        self._ck(self.lib.esvo_map_fuse(self.h, C.byref(n)))
        return n.value

    def init_sgm(self, ts_left=None, ts_right=None, min_points=500, want_disp=True):
        """InitializationAtTime (SGM bootstrap) on the observation set last; returns (#points, disparity*16 image or None)"""
        l = None if ts_left is None else np.ascontiguousarray(ts_left, np.uint8)
        r = None if ts_right is None else np.ascontiguousarray(ts_right, np.uint8)
        disp = np.empty((self.H, self.W), np.int16) if want_disp else None
        n = C.c_size_t()
        self._ck(self.lib.esvo_map_init_sgm(self.h, _p(l), _p(r), int(min_points), C.byref(n), _p(disp)))
        return int(n.value), disp

    # ---- mapper, fused tick (MappingAtTime on device-resident data)
    def tick(self, t_ns, stamps, poses):
        st = np.ascontiguousarray(stamps, np.uint64)
        T = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        self._ck(self.lib.esvo_map_tick(self.h, int(t_ns), st.ctypes.data, T.ctypes.data, st.shape[0]))

    def tick_bm_only(self, t_ns, stamps, poses):
        """esvo_MVStereo's PURE_BLOCK_MATCHING mode: block matching, vEMP2vDP, naive propagation of the window"""
        st = np.ascontiguousarray(stamps, np.uint64)
        T = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        self._ck(self.lib.esvo_map_tick_bm_only(self.h, int(t_ns), st.ctypes.data, T.ctypes.data, st.shape[0]))

    def fuse_matches_naive(self, matches, poses=None):
        """vEMP2vDP + window of maxNumFusionFrames + naive propagation on the given matches (stage-wise PURE_BLOCK_MATCHING)"""
        mt = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        T = self._poses if poses is None else np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        self._ck(self.lib.esvo_map_fuse_matches_naive(self.h, mt.ctypes.data, mt.shape[0], T.ctypes.data, T.shape[0]))

    # ---- event-to-event matching: esvo_MVStereo modes 0 / 2 (EventMatcher)
    def match_em(self, em, left, slice_begin, slice_count, slice_T, right):
        """EventMatcher::createMatchProblem + match_all_HyperThread on host arrays (esvo_map_match_em): the matches in the
        reference's stride-N order.  em: abi.EmParamsStruct; slice_T: (n_slices, 4, 4) T_world of each slice."""
        l = np.ascontiguousarray(left, dtype=EVENT_DTYPE)
        r = np.ascontiguousarray(right, dtype=EVENT_DTYPE)
        b = np.ascontiguousarray(slice_begin, np.uint32)
        c = np.ascontiguousarray(slice_count, np.uint32)
        T = np.ascontiguousarray(slice_T, np.float64).reshape(-1, 16)
        assert len(b) == len(c) == len(T)
        out = np.zeros(max(int(c.sum()), 1), MATCH_DTYPE)
        n = C.c_size_t(0)
        self._ck(self.lib.esvo_map_match_em(self.h, C.addressof(em), l.ctypes.data, l.shape[0], b.ctypes.data, c.ctypes.data,
                                            T.ctypes.data, len(b), r.ctypes.data, r.shape[0], out.ctypes.data, out.shape[0],
                                            C.byref(n)))
        return out[: n.value].copy()

    def tick_em(self, em, mode, t_low_ns, t_up_ns, pose_fn=None):
        """esvo_MVStereo::MappingAtTime in MVStereoMode 0 (PURE_EVENT_MATCHING) or 2 (EM_PLUS_ESTIMATION) on the staged events
        (esvo_map_tick_em).  pose_fn(t_ns) -> 4x4 T_world_cam, or None where no pose is known (the slice keeps the identity)."""
        def trampoline(user, t_ns, out):  # an exception must not unwind through the C frames: report it, use no pose
            try:
                T = None if pose_fn is None else pose_fn(int(t_ns))
                if T is None:
                    return 0
                T = np.asarray(T, np.float64).reshape(16)
                for k in range(16):
                    out[k] = float(T[k])
                return 1
            except BaseException:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 0
        cb = EM_POSE_FN(trampoline)
        self._ck(self.lib.esvo_map_tick_em(self.h, C.addressof(em), int(mode), int(t_low_ns), int(t_up_ns), cb, None))

    def em_selection(self):
        """the last tick_em's selection: dict of the esvo_em_selection_t fields + slice table (begin, count, t_ns, T)"""
        sel = EmSelectionStruct()
        self._ck(self.lib.esvo_map_em_get_selection(self.h, C.byref(sel), None, None, None, None, 0))
        ns = int(sel.n_slices)
        b, c = np.zeros(max(ns, 1), np.uint32), np.zeros(max(ns, 1), np.uint32)
        t, T = np.zeros(max(ns, 1), np.uint64), np.zeros((max(ns, 1), 16), np.float64)
        self._ck(self.lib.esvo_map_em_get_selection(self.h, C.byref(sel), b.ctypes.data, c.ctypes.data, t.ctypes.data,
                                                    T.ctypes.data, max(ns, 1)))
        d = {k: int(getattr(sel, k)) for k, _ in EmSelectionStruct._fields_ if k != "pad_"}
        d.update(slice_begin=b[:ns], slice_count=c[:ns], slice_t_ns=t[:ns], slice_T=T[:ns].reshape(-1, 4, 4))
        return d

    def em_stats(self):
        s = EmStatsStruct()
        self._ck(self.lib.esvo_map_em_stats(self.h, C.byref(s)))
        return s

    def lm_stats(self):
        """the scale-loop guard's counts (esvo_map_lm_stats; ParamsStruct.lm_scale_pass_limit): all zero while the limit is 0"""
        s = LmStatsStruct()
        self._ck(self.lib.esvo_map_lm_stats(self.h, C.byref(s)))
        return s

    # ---- semi-global matching per tick: esvo_MVStereo mode 4
    def tick_sgm(self, ts_left=None, ts_right=None, want_disp=True):
        """esvo_MVStereo::MappingAtTime in MVStereoMode 4 (PURE_SEMI_GLOBAL_MATCHING) on the staged events and the observation set
        last (esvo_map_tick_sgm); None = the device-resident Time Surfaces.  Returns (#points, disparity*16 image or None)"""
        l = None if ts_left is None else np.ascontiguousarray(ts_left, np.uint8)
        r = None if ts_right is None else np.ascontiguousarray(ts_right, np.uint8)
        disp = np.empty((self.H, self.W), np.int16) if want_disp else None
        n = C.c_size_t()
        self._ck(self.lib.esvo_map_tick_sgm(self.h, _p(l), _p(r), C.byref(n), _p(disp)))
        return int(n.value), disp

    def push_disparity_frame(self, disp16, ev):
        """the mode-4 seam behind a node's own StereoSGBM (esvo_map_push_disparity_frame): disp16 (H, W) int16 or None for the
        device's last SGM result, ev = vEventsPtr_left_SGM_ in the node's order.  Returns the number of points of the frame"""
        d = None if disp16 is None else np.ascontiguousarray(disp16, np.int16)
        assert d is None or d.shape == (self.H, self.W)
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        n = C.c_size_t()
        self._ck(self.lib.esvo_map_push_disparity_frame(self.h, _p(d), ev.ctypes.data if len(ev) else None, ev.shape[0], C.byref(n)))
        return int(n.value)

    def sgm_stats(self):
        s = SgmStatsStruct()
        self._ck(self.lib.esvo_map_sgm_stats(self.h, C.byref(s)))
        return s

    def tick_resident(self, t_ns, T_world_cam, stamps, poses):
        """render both Time Surfaces at t_ns, take them as the observation, tick: one call"""
        st = np.ascontiguousarray(stamps, np.uint64)
        T = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        Tw = np.ascontiguousarray(T_world_cam, np.float64).reshape(16)
        self._ck(self.lib.esvo_map_tick_resident(self.h, int(t_ns), Tw.ctypes.data, st.ctypes.data, T.ctypes.data, st.shape[0]))

    # ---- outputs
    def get_map(self):
        n = C.c_size_t(0)
        out = np.zeros(self.W * self.H, DEPTH_POINT_DTYPE)
        self._ck(self.lib.esvo_map_get_depth_points(self.h, out.ctypes.data, out.shape[0], C.byref(n)))
        return out[: n.value].copy()

    def debug_fuse_cell_counts(self):
        """esvo_debug_fuse_cell_counts (api_dev.hip, not part of the ABI): the (H, W) record counts the tile kernel of the last
        fusion wrote per cell; a copy, nothing is launched.  Cells outside the handle's band hold stale values."""
        out = np.zeros((self.H, self.W), np.uint32)
        fn = _dbg_fn("esvo_debug_fuse_cell_counts", [C.c_void_p, C.c_void_p, C.c_size_t])
        self._ck(fn(self.h, out.ctypes.data, out.size))
        return out

    def debug_bm_owner_count(self):
        """esvo_debug_bm_owner_count (api_dev.hip, not part of the ABI): the searches of the newest block-matching launch that ran
        once per distinct raw pixel (its owner count), or None for a handle that has no such path."""
        n, shared = C.c_uint32(0), C.c_int(0)
        fn = _dbg_fn("esvo_debug_bm_owner_count", [C.c_void_p, C.c_void_p, C.c_void_p])
        self._ck(fn(self.h, C.byref(n), C.byref(shared)))
        return int(n.value) if shared.value else None

    def get_committed_map(self):
        """(DepthMap of the newest committed tick, its stamp) without completing a pending tick"""
        out = np.zeros(self.W * self.H, DEPTH_POINT_DTYPE)
        n, t = C.c_size_t(), C.c_uint64()
        self._ck(self.lib.esvo_map_get_committed(self.h, out.ctypes.data, out.shape[0], C.byref(n), C.byref(t)))
        return out[:n.value].copy(), int(t.value)

    def get_pointcloud(self):
        n = C.c_size_t(0)
        out = np.zeros((self.W * self.H, 3), np.float32)
        self._ck(self.lib.esvo_map_get_pointcloud_xyz(self.h, out.ctypes.data, out.shape[0], C.byref(n)))
        return out[: n.value].copy()

    def map_cloud_build(self):
        """esvo_map_cloud_build: the cloud of get_pointcloud() built and kept on the device (a snapshot); returns its point count"""
        n = C.c_size_t(0)
        self._ck(self.lib.esvo_map_cloud_build(self.h, C.byref(n)))
        return int(n.value)

    def map_cloud(self):
        """the snapshot of the last map_cloud_build() as (n, 3) float32 (12 B per point cross the bus); empty before a build"""
        n = C.c_size_t(0)
        self._ck(self.lib.esvo_map_cloud_get(self.h, None, 0, C.byref(n)))
        out = np.zeros((int(n.value), 3), np.float32)
        if n.value:
            self._ck(self.lib.esvo_map_cloud_get(self.h, out.ctypes.data, out.shape[0], C.byref(n)))
        return out

    def map_cloud_device(self):
        """(device pointer, point count, stamp of the tick it was built from) of the snapshot: valid until the next build / reset"""
        ptr, n, t = C.c_void_p(), C.c_size_t(), C.c_uint64()
        self._ck(self.lib.esvo_map_cloud_device(self.h, C.byref(ptr), C.byref(n), C.byref(t)))
        return (ptr.value or 0), int(n.value), int(t.value)

    def get_debug_images(self, age_max_range=10.0):
        """(inverse depth, standard deviation, age, cost) images of publishMappingResults, BGR8"""
        imgs = [np.empty((self.H, self.W, 3), np.uint8) for _ in range(4)]
        self._ck(self.lib.esvo_map_get_debug_images(self.h, float(age_max_range), *[i.ctypes.data for i in imgs]))
        return imgs

    def get_pointcloud_near(self, visualize_range):
        n = C.c_size_t(0)
        out = np.zeros((self.W * self.H, 3), np.float32)
        self._ck(self.lib.esvo_map_get_pointcloud_near_xyz(self.h, float(visualize_range), out.ctypes.data, out.shape[0], C.byref(n)))
        return out[: n.value].copy()

    def map_cloud_near(self, visualize_range):
        """esvo_map_cloud_near: get_pointcloud_near() built on the device -- same points, order and bits; only the points come back"""
        n = C.c_size_t(0)
        out = np.zeros((self.W * self.H, 3), np.float32)
        self._ck(self.lib.esvo_map_cloud_near(self.h, float(visualize_range), out.ctypes.data, out.shape[0], C.byref(n)))
        return out[: n.value].copy()

    def map_voxel_filter(self, xyz, leaf, cap_points=None, out=None):
        """esvo_map_voxel_filter: lib.voxel_filter() with all arithmetic on the device, the same bytes.  cap_points / out: the
        capacity handed to the C call and the array it writes (tests); default: room for one centroid per row"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        if out is None:
            out = np.empty((max(len(xyz), 1) if cap_points is None else max(int(cap_points), 1), 3), np.float32)
        n = C.c_size_t()
        self._ck(self.lib.esvo_map_voxel_filter(self.h, xyz.ctypes.data if len(xyz) else None, xyz.shape[0], float(leaf), out.ctypes.data,
                                                out.shape[0] if cap_points is None else int(cap_points), C.byref(n)))
        return out[: n.value].copy()

    def gpc_configure(self, visualize_range=2.5, interval_s=3.0, num_added_per_refresh=1000, capacity_points=0, leaf=0.3):
        """esvo_map_gpc_configure: allocates the global cloud (capacity_points 0: 5 000 000), empties it, t_last_pub = 0"""
        p = GpcParamsStruct(visualize_range=float(visualize_range), interval_s=float(interval_s),
                            num_added_per_refresh=int(num_added_per_refresh), capacity_points=int(capacity_points), leaf=float(leaf),
                            reserved=0)
        self._ck(self.lib.esvo_map_gpc_configure(self.h, C.byref(p)))

    def gpc_update(self, t_ns):
        """esvo_map_gpc_update: publishPointCloud's global-cloud branch on the current map; True when the interval let it through"""
        r = C.c_int(0)
        self._ck(self.lib.esvo_map_gpc_update(self.h, int(t_ns), C.byref(r)))
        return bool(r.value)

    def gpc_cloud(self):
        """the global cloud as (n, 3) float32; empty before gpc_configure"""
        n = C.c_size_t(0)
        self._ck(self.lib.esvo_map_gpc_get(self.h, None, 0, C.byref(n)))
        out = np.zeros((int(n.value), 3), np.float32)
        if n.value:
            self._ck(self.lib.esvo_map_gpc_get(self.h, out.ctypes.data, out.shape[0], C.byref(n)))
        return out

    def gpc_device(self):
        """(device pointer, point count) of the global cloud: valid until the next refreshing gpc_update / gpc_configure / reset"""
        ptr, n = C.c_void_p(), C.c_size_t()
        self._ck(self.lib.esvo_map_gpc_device(self.h, C.byref(ptr), C.byref(n)))
        return (ptr.value or 0), int(n.value)

    def gpc_stats(self):
        st = GpcStatsStruct()
        self._ck(self.lib.esvo_map_gpc_stats(self.h, C.byref(st)))
        return st

    def save_depth_map(self, save_dir, t_ns):
        """esvo_MVStereo::saveDepthMap: writes <save_dir><t_ns>.txt ("x y depth" per valid element); returns the line count"""
        n = C.c_size_t()
        self._ck(self.lib.esvo_map_save_depth_map(self.h, str(save_dir).encode(), int(t_ns), C.byref(n)))
        return int(n.value)

    def get_last_frame(self):
        n = C.c_size_t(0)
        cap = max(int(self.params.max_events_per_tick), int(self.params.process_event_num), 1)
        out = np.zeros(cap, DEPTH_POINT_DTYPE)
        self._ck(self.lib.esvo_map_get_last_frame(self.h, out.ctypes.data, cap, C.byref(n)))
        return out[: n.value].copy()

    def stats(self):
        s = StatsStruct()
        self._ck(self.lib.esvo_get_stats(self.h, C.addressof(s)))
        return s

    # ---- device-resident stage calls (tick-interleaved multi-GPU operation, dist.TickShardedEsvo) ----
    def front(self, t_ns, stamps, poses):
        """front stage of a tick on the staged events; returns (device pointer of the frame, number of points)"""
        st = np.ascontiguousarray(stamps, np.uint64)
        T = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        n = C.c_size_t()
        self._ck(self.lib.esvo_map_front(self.h, int(t_ns), st.ctypes.data, T.ctypes.data, st.shape[0], C.byref(n)))
        ptr = C.c_void_p()
        self._ck(self.lib.esvo_map_front_frame(self.h, C.byref(ptr)))
        return (ptr.value or 0), int(n.value)

    def push_frame_device(self, d_ptr, n, poses):
        T = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        self._ck(self.lib.esvo_map_push_frame_device(self.h, C.c_void_p(int(d_ptr)), int(n), T.ctypes.data, T.shape[0]))

    def fuse_async(self):
        self._ck(self.lib.esvo_map_fuse_async(self.h))

    # ---- tracker residual / Jacobian evaluation (RegProblemLM.cpp), SURVEY.md section 8(f).1 ----
    def track_set_current(self, ts_left=None, kernel_size=5):
        img = None if ts_left is None else np.ascontiguousarray(ts_left, np.uint8)
        self._ck(self.lib.esvo_track_set_current(self.h, None if img is None else img.ctypes.data, int(kernel_size)))

    def track_images(self):
        neg = np.empty((self.H, self.W), np.uint8)
        du = np.empty((self.H, self.W), np.int16)
        dv = np.empty((self.H, self.W), np.int16)
        self._ck(self.lib.esvo_track_get_images(self.h, neg.ctypes.data, du.ctypes.data, dv.ctypes.data))
        return neg, du, dv

    def track_set_reference(self, xyz_world, T_world_ref):
        xyz = np.ascontiguousarray(xyz_world, np.float32).reshape(-1, 3)
        T = np.ascontiguousarray(T_world_ref, np.float64).reshape(16)
        self._ck(self.lib.esvo_track_set_reference(self.h, xyz.ctypes.data, xyz.shape[0], T.ctypes.data))

    def track_set_reference_from_cloud(self, order, T_world_ref, n=None):
        """esvo_track_set_reference_from_cloud: position i of the reference = point order[i] of the map_cloud_build() snapshot
        (stochastic_order); order None: the first n points in list order.  Same bits as track_set_reference(cloud[order], T)"""
        T = np.ascontiguousarray(T_world_ref, np.float64).reshape(16)
        if order is None:
            assert n is not None, "order=None needs n"
            self._ck(self.lib.esvo_track_set_reference_from_cloud(self.h, None, int(n), T.ctypes.data))
            return
        o = np.ascontiguousarray(order, np.uint32).reshape(-1)
        self._ck(self.lib.esvo_track_set_reference_from_cloud(self.h, o.ctypes.data if len(o) else None, len(o), T.ctypes.data))

    def track_residuals(self, T_left_ref, offset, count, huber=True, huber_threshold=50.0):
        T = np.ascontiguousarray(T_left_ref, np.float64).reshape(16)
        out = np.empty(max(count, 1), np.float64)
        n = C.c_size_t()
        self._ck(self.lib.esvo_track_residuals(self.h, T.ctypes.data, int(offset), int(count), 1 if huber else 0,
                                               float(huber_threshold), out.ctypes.data, C.byref(n)))
        return out[:n.value]

    def track_jacobian(self, R, t, offset, count):
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        out = np.empty(6 * max(count, 1), np.float64)
        n = C.c_size_t()
        self._ck(self.lib.esvo_track_jacobian(self.h, R.ctypes.data, t.ctypes.data, int(offset), int(count), out.ctypes.data, C.byref(n)))
        return out[:6 * n.value].reshape(6, n.value).T  # (n, 6); column-major like Eigen's fjac

    def track_normal_equations(self, R, t, offset, count, huber=True, huber_threshold=50.0):
        """(H = J^T J 6x6, b = J^T f, |f|^2, n) at (R, t): residuals, Jacobian and their products in one device call"""
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        H, b = np.zeros((6, 6), np.float64), np.zeros(6, np.float64)
        cost, n = C.c_double(), C.c_size_t()
        self._ck(self.lib.esvo_track_normal_equations(self.h, R.ctypes.data, t.ctypes.data, int(offset), int(count), 1 if huber else 0,
                                                      float(huber_threshold), H.ctypes.data, b.ctypes.data, C.byref(cost), C.byref(n)))
        return H, b, cost.value, n.value

    def track_normal_equations_batch(self, Rs, ts, offset, count, huber=True, huber_threshold=50.0):
        """the same at k poses (Rs: k x 3 x 3, ts: k x 3) in one launch -> (H k x 6 x 6, b k x 6, cost k, n)"""
        Rs = np.ascontiguousarray(Rs, np.float64).reshape(-1, 9)
        ts = np.ascontiguousarray(ts, np.float64).reshape(-1, 3)
        k = len(Rs)
        H, b, cost = np.zeros((k, 6, 6), np.float64), np.zeros((k, 6), np.float64), np.zeros(k, np.float64)
        n = C.c_size_t()
        self._ck(self.lib.esvo_track_normal_equations_batch(self.h, k, Rs.ctypes.data, ts.ctypes.data, int(offset), int(count),
                                                            1 if huber else 0, float(huber_threshold), H.ctypes.data, b.ctypes.data,
                                                            cost.ctypes.data, C.byref(n)))
        return H, b, cost, n.value

    def track_register(self, n_points, R, t, huber=True, huber_threshold=50.0, max_iterations=12, damping=1e-3):
        """the registration loop inside the library (esvo_hip::gauss_newton_register over the normal equations):
        -> (R 3x3, t, rms, iterations)"""
        R = np.ascontiguousarray(R, np.float64).reshape(9).copy()
        t = np.ascontiguousarray(t, np.float64).reshape(3).copy()
        rms, it = C.c_double(), C.c_int()
        self._ck(self.lib.esvo_track_register(self.h, int(n_points), R.ctypes.data, t.ctypes.data, 1 if huber else 0, float(huber_threshold),
                                              int(max_iterations), float(damping), C.byref(rms), C.byref(it)))
        return R.reshape(3, 3), t, rms.value, it.value

    def track_solve(self, n_points, R, t, batch_size=0, huber=True, huber_threshold=50.0, max_iterations=12, damping=1e-3,
                    on_device=True):
        """esvo_track_solve: the registration with the shipped configs' batch schedule (batch_size 0: all points in every
        iteration, what track_register does) and a record of what it did.  on_device: the whole loop in one kernel launch,
        bit for bit what the host loop (on_device=False: one launch per evaluation) returns.
        -> (R 3x3, t, info: abi.TrackSolveInfoStruct, trace: one abi.TRACK_ITER_DTYPE record per iteration)"""
        R = np.ascontiguousarray(R, np.float64).reshape(9).copy()
        t = np.ascontiguousarray(t, np.float64).reshape(3).copy()
        prm = TrackSolveParamsStruct(int(n_points), int(batch_size), 1 if huber else 0, int(max_iterations), 1 if on_device else 0, 0,
                                     float(huber_threshold), float(damping))
        info = TrackSolveInfoStruct()
        trace = np.zeros(TRACK_SOLVE_MAX_ITERATIONS, TRACK_ITER_DTYPE)
        self._ck(self.lib.esvo_track_solve(self.h, C.addressof(prm), R.ctypes.data, t.ctypes.data, C.addressof(info), trace.ctypes.data,
                                           len(trace)))
        return R.reshape(3, 3), t, info, trace[:info.iterations].copy()

    def track_reprojection_map(self, R, t, n_points=2000, inv_depth_min=None, inv_depth_max=None, download=True):
        """esvo_track_reprojection_map: RegProblemSolverLM's Reproj_Map_Left for the motion (R, t) -- the grey TS_negative_left_
        with the first n_points reference points painted in the jet colour of 1/z between inv_depth_min and inv_depth_max
        (the tracker's invDepth_min_range / invDepth_max_range; no default: they are the node's parameters).
        -> ((H, W, 3) uint8 BGR, n_inside); download=False leaves the image on the device (track_reprojection_map_device) and
        returns (None, n_inside)"""
        assert inv_depth_min is not None and inv_depth_max is not None, "inv_depth_min / inv_depth_max are the tracker's ranges"
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        img = np.empty((self.H, self.W, 3), np.uint8) if download else None
        n = C.c_size_t()
        self._ck(self.lib.esvo_track_reprojection_map(self.h, R.ctypes.data, t.ctypes.data, int(n_points), float(inv_depth_min),
                                                      float(inv_depth_max), None if img is None else img.ctypes.data, C.byref(n)))
        return img, int(n.value)

    def track_reprojection_map_device(self):
        """device pointer of the last track_reprojection_map()'s H x W x 3 image: valid until the next such call / destroy"""
        ptr = C.c_void_p()
        self._ck(self.lib.esvo_track_reprojection_map_device(self.h, C.byref(ptr)))
        return ptr.value or 0

    # ---- multi-GPU exchange behind the C-ABI (api_comm.hip): RCCL, or the two collectives as callbacks ----
    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._ck(self.lib.esvo_comm_init(self.h, buf, int(rank), int(world)))

    def comm_init_callbacks(self, rank, world, all_gather):
        """all_gather(d_send, d_recv, bytes_per_rank, stream) -> 0 on success: the one collective the library issues"""
        def trampoline(user, s, r, n, st):   # an exception must not unwind through the C frames: report it, fail the collective
            try:
                return int(all_gather(s, r, n, st) or 0)
            except BaseException:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1
        self._cb = ALL_GATHER_FN(trampoline)  # kept alive with the handle
        self._ck(self.lib.esvo_comm_init_callbacks(self.h, int(rank), int(world), self._cb, None))

    def comm_destroy(self):
        self._ck(self.lib.esvo_comm_destroy(self.h))

    def comm_owns_next_tick(self):
        return bool(self.lib.esvo_comm_owns_next_tick(self.h))

    def comm_tick(self, t_ns, T_world_cam, stamps, poses):
        st = np.ascontiguousarray(stamps, np.uint64)
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        T = np.ascontiguousarray(T_world_cam, np.float64).reshape(16)
        self._ck(self.lib.esvo_comm_tick(self.h, int(t_ns), T.ctypes.data, st.ctypes.data, P.ctypes.data, st.shape[0]))

    def comm_tick_resident(self, t_ns, T_world_cam, stamps, poses):
        """esvo_comm_tick with the owner's Time Surfaces rendered inside the call"""
        st = np.ascontiguousarray(stamps, np.uint64)
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        T = np.ascontiguousarray(T_world_cam, np.float64).reshape(16)
        self._ck(self.lib.esvo_comm_tick_resident(self.h, int(t_ns), T.ctypes.data, st.ctypes.data, P.ctypes.data, st.shape[0]))

    def comm_stats(self):
        from .abi import CommStatsStruct
        st = CommStatsStruct()
        self._ck(self.lib.esvo_comm_get_stats(self.h, C.byref(st)))
        return st

    def comm_flush(self):
        self._ck(self.lib.esvo_comm_flush(self.h))

    def comm_newest_map(self):
        out = np.zeros(self.W * self.H, DEPTH_POINT_DTYPE)
        n, k = C.c_size_t(), C.c_longlong()
        self._ck(self.lib.esvo_comm_newest_map(self.h, out.ctypes.data, out.shape[0], C.byref(n), C.byref(k)))
        return out[: n.value].copy(), int(k.value)

    def comm_shard_tick(self, t_ns, stamps, poses):
        st = np.ascontiguousarray(stamps, np.uint64)
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        self._ck(self.lib.esvo_comm_shard_tick(self.h, int(t_ns), st.ctypes.data, P.ctypes.data, st.shape[0]))

    def comm_gather_pointcloud(self):
        """the whole map's publishPointCloud cloud on every rank (collective): (n, 3) float32, world frame"""
        out = np.zeros((self.W * self.H, 3), np.float32)
        n = C.c_size_t()
        self._ck(self.lib.esvo_comm_gather_pointcloud_xyz(self.h, out.ctypes.data, out.shape[0], C.byref(n)))
        return out[: n.value].copy()

    def comm_gather_ts(self, cam):
        """routed band mode: the other ranks' rows of camera `cam`'s resident Time Surface (collective)"""
        self._ck(self.lib.esvo_comm_gather_ts(self.h, int(cam)))

    def comm_gather_map(self):
        out = np.zeros(self.W * self.H, DEPTH_POINT_DTYPE)
        n = C.c_size_t()
        self._ck(self.lib.esvo_comm_gather_map(self.h, out.ctypes.data, out.shape[0], C.byref(n)))
        return out[: n.value].copy()

    def set_band(self, y0, y1, shard=0, n_shards=1, routing=None, ts_halo_rows=-1):
        """row band + shard of this handle; routing: None / "broadcast" (every rank stages all events and renders the full Time
        Surfaces, per-event work dealt by slot) or "y_rect" (events routed by image row, banded raster)"""
        self._ck(self.lib.esvo_shard_set_band(self.h, int(y0), int(y1), int(shard), int(n_shards)))
        if routing not in (None, "broadcast"):
            assert routing == "y_rect", routing
            self._ck(self.lib.esvo_shard_set_routing(self.h, 1, int(ts_halo_rows)))

    def shard_rows(self):
        """dict of (begin, end) rows: render, observation, source_left, source_right (esvo_shard_get_rows)"""
        r = [(C.c_int * 2)() for _ in range(4)]
        self._ck(self.lib.esvo_shard_get_rows(self.h, *r))
        return dict(zip(("render", "observation", "source_left", "source_right"), [(int(a[0]), int(a[1])) for a in r]))

    def shard_exchange(self):
        """(send pointer, receive pointer, block bytes) of the all-gather due before the next phase (device pointers; block
        bytes == 0: nothing to do; one shard: receive aliases send)"""
        snd, rcv, nb = C.c_void_p(), C.c_void_p(), C.c_size_t()
        self._ck(self.lib.esvo_shard_exchange(self.h, C.byref(snd), C.byref(rcv), C.byref(nb)))
        return (snd.value or 0), (rcv.value or 0), int(nb.value)

    def shard_phase(self, phase, t_ns=0, stamps=None, poses=None):
        """one phase of esvo_shard_tick_phase; returns True when the phase must be called AGAIN behind the exchange that is now due
        (ESVO_AGAIN: phase 0 of a routed handle with Denoising -- the second call takes no arguments)"""
        if phase == 0 and stamps is not None:
            st = np.ascontiguousarray(stamps, np.uint64)
            T = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
            rc = self.lib.esvo_shard_tick_phase(self.h, 0, int(t_ns), st.ctypes.data, T.ctypes.data, st.shape[0])
        else:
            rc = self.lib.esvo_shard_tick_phase(self.h, int(phase), 0, None, None, 0)
        if rc == ESVO_AGAIN:
            return True
        self._ck(rc)
        return False
