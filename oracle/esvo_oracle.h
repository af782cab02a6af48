/*
 * esvo_oracle.h — C API of the CPU oracle (TEST INFRASTRUCTURE, NOT PRODUCT).
 *
 * The oracle is a dependency-free C++17 restatement of the ESVO reference's hot
 * path (Time-Surface raster + stereo mapper).  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load it.  The product library
 * (esvo_amd/csrc -> libesvo_hip.so) never links, loads or calls anything in here.
 *
 * PARITY: pinned to REFERENCE SOURCE for the mapper.  oracle/_ref/libesvo_ref.so (make -C oracle ref) is the
 * reference's own EventBM / DepthProblem / DepthProblemSolver / DepthFusion / DepthRegularization / DepthPoint /
 * SmartGrid / CameraSystem sources and the tracker's RegProblemLM / cayley / ResidualItem sources compiled unmodified
 * against the stand-in headers of oracle/ref_shim/ (libesvo_ref_ts.so: the Time-Surface node class TimeSurface.cpp;
 * libesvo_ref_node.so / libesvo_ref_mvstereo.so: the mapper NODE objects esvo_Mapping.cpp / esvo_MVStereo.cpp driven through
 * their own callbacks -- event selection, denoising, pose-table stamps, window policy, tick glue, SGM bootstrap glue);
 * tests/golden/ref_*.npz are its outputs and tests/test_ref_pin.py checks this oracle against them stage by stage
 * (block matching, fusion/clean/regularise, the tracker functor's residuals + Jacobian and the Time-Surface raster before
 * its OpenCV stages bit-identical, the mapper's
 * residual functor to 1e-9, the LM end result statistically: DESIGN.md section 2).
 * PARITY UNPINNED for the third-party pieces that are absent from /root/reference and from this image: OpenCV
 * (convertTo's rounding / medianBlur / remap / GaussianBlur of the Time-Surface raster, initUndistortRectifyMap, StereoSGBM), Eigen's
 * LevenbergMarquardt + NumericalDiff driver (restated twice, independently: here for n = 1 and in ref_shim for
 * general n), PCL VoxelGrid.  Those are
 * restated from the published algorithms and checked by known-answer and independent-
 * formulation tests (tests/test_oracle*.py, tests/test_sgm.py, tests/test_viz.py).
 *
 * POD types (events, params, matches, depth points) are shared with the boundary
 * header include/esvo_hip.h so that tests compare like with like.
 */
#ifndef ESVO_ORACLE_H
#define ESVO_ORACLE_H

#include "../include/esvo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------- Time Surface (esvo_time_surface/) ---------- */
typedef struct orc_ts* orc_ts_handle;
orc_ts_handle orc_ts_create(int width, int height, int queue_len);
void orc_ts_destroy(orc_ts_handle h);
void orc_ts_clear(orc_ts_handle h);
/* EventQueueMat::insertEvent, TimeSurface.h:39-50 (events must be time sorted) */
void orc_ts_push(orc_ts_handle h, const esvo_event_t* ev, size_t n);
/* TimeSurface::createTimeSurfaceAtTime, TimeSurface.cpp:52-152 (BACKWARD mode).
 * map_x/map_y may be NULL -> out is the un-rectified (median-filtered) image.
 * out_prefilter (nullable) receives the u8 image before the median filter. */
void orc_ts_render(orc_ts_handle h, uint64_t t_ns, double decay_ms, int ignore_polarity,
                   int median_blur_kernel_size, const float* map_x, const float* map_y,
                   uint8_t* out, uint8_t* out_prefilter);
/* FORWARD mode of the same function (TimeSurface.cpp:85-116): rect_lut = (u, v) of every raw pixel; out_f64 (nullable) =
 * the image handed to convertTo(CV_8U) */
void orc_ts_render_forward(orc_ts_handle h, uint64_t t_ns, double decay_ms, int ignore_polarity, int median_blur_kernel_size,
                           const float* rect_lut, uint8_t* out, double* out_f64);

/* OpenCV-style image primitives restated in Appendix B.2 (exposed for unit tests) */
void orc_median3_u8(const uint8_t* src, uint8_t* dst, int w, int h);
void orc_remap_bilinear_u8(const uint8_t* src, uint8_t* dst, int w, int h, const float* map_x,
                           const float* map_y);
void orc_gaussian5_u8(const uint8_t* src, uint8_t* dst, int w, int h);

/* ---------- Mapper (esvo_core/) ---------- */
typedef struct orc_mapper* orc_mapper_handle;
orc_mapper_handle orc_mapper_create(const esvo_params_t* p, const esvo_calib_t* left,
                                    const esvo_calib_t* right);
void orc_mapper_destroy(orc_mapper_handle h);
void orc_mapper_reset(orc_mapper_handle h);
void orc_mapper_set_params(orc_mapper_handle h, const esvo_params_t* p);
void orc_mapper_set_threads(orc_mapper_handle h, int real_threads); /* >1: run BM / LM on
        real std::threads (same outputs; used only for the timed CPU baseline) */
double orc_mapper_baseline(orc_mapper_handle h);
/* bm_exact_int=1: ZNCC cost from exact integer moments; lm_canonical=1: canonical reduction
 * order in the LM sums.  (0,0) = literal restatement (default).  (1,1) = bit-comparable with the
 * GPU; tests bound the difference between the two. */
void orc_mapper_set_mode(orc_mapper_handle h, int bm_exact_int, int lm_canonical);

/* TS_obs_ : mono8 left/right + T_world_cam (row-major 4x4) */
void orc_mapper_set_observation(orc_mapper_handle h, uint64_t t_ns, const uint8_t* ts_left,
                                const uint8_t* ts_right, const double T_world_cam[16]);
void orc_mapper_set_poses(orc_mapper_handle h, const uint64_t* pose_t_ns, const double* pose_T,
                          size_t m);
/* dataTransferring's event selection, esvo_Mapping.cpp:555-575; returns count; out_idx gets
 * indices into ev (newest first). */
size_t orc_select_events(const esvo_event_t* ev, size_t n, uint64_t t_ns, double half_slice,
                         size_t max_num, uint32_t* out_idx, size_t cap);
/* createDenoisingMask + extractDenoisedEvents, esvo_Mapping.cpp:1046-1072 */
size_t orc_denoise_events(const esvo_event_t* ev, const uint32_t* idx, size_t n, int w, int h,
                          size_t max_num, uint32_t* out_idx);

/* EventBM::match_all_HyperThread, EventBM.cpp:269-315 (output in the reference's
 * thread-stride order).  Uses the current observation + pose table. */
size_t orc_mapper_match(orc_mapper_handle h, const esvo_event_t* ev, size_t n, esvo_match_t* out,
                        size_t cap);
/* the reference's failure counters (EventBM.h:89) over the last orc_mapper_match: infoNoiseRatioLowNum_,
 * coarseSearchingFailNum_, fineSearchingFailNum_ */
void orc_mapper_bm_fail_counts(orc_mapper_handle h, uint64_t out[3]);
/* per-event diagnostic: all candidate costs of one event (for near-tie analysis).
 * costs[d - dmin]; returns 0 if the event is rejected before the search. */
int orc_mapper_match_costs(orc_mapper_handle h, const esvo_event_t* ev, double* costs,
                           int exact_int);
/* DepthProblemSolver::solve (+pointCulling if cull), DepthProblemSolver.cpp:28-136,216-244.
 * lm_info (nullable, 4 doubles per input match): iterations, nfev, last status, solved flag */
size_t orc_mapper_refine(orc_mapper_handle h, const esvo_match_t* matches, size_t n, int cull,
                         esvo_depth_point_t* out, size_t cap, double* lm_info);
/* window policy, esvo_Mapping.cpp:341-368 */
void orc_mapper_push_frame(orc_mapper_handle h, const esvo_depth_point_t* pts, size_t n,
                           const double* pose_T, size_t m);
/* fusion loop + clean + regularisation, esvo_Mapping.cpp:370-395; returns numFusionCount */
size_t orc_mapper_fuse(orc_mapper_handle h);
/* whole MappingAtTime on already-selected events (esvo_Mapping.cpp:261-431) */
size_t orc_mapper_tick(orc_mapper_handle h, const esvo_event_t* ev, size_t n);
/* esvo_MVStereo's PURE_BLOCK_MATCHING mode (esvo_MVStereo.cpp:383-432): BM, vEMP2vDP, CONST_FRAMES window, naive_propagation */
size_t orc_mapper_tick_bm_only(orc_mapper_handle h, const esvo_event_t* ev, size_t n);

size_t orc_mapper_map_size(orc_mapper_handle h);
size_t orc_mapper_get_map(orc_mapper_handle h, esvo_depth_point_t* out, size_t cap);
/* true grid cell of every returned element (row*W+col), same order as get_map; -1 if the
 * element is orphaned (Appendix A-7) */
size_t orc_mapper_get_map_cells(orc_mapper_handle h, int32_t* out, size_t cap);
size_t orc_mapper_get_last_frame(orc_mapper_handle h, esvo_depth_point_t* out, size_t cap);
size_t orc_mapper_get_pointcloud_xyz(orc_mapper_handle h, float* out_xyz, size_t cap_points);
/* counters: [0] window frames [1] window points [2] replace-branch hits [3] replace hits with
 * a displaced cell (row/col differ) [4] max t-scale loop iterations seen [5] LM evaluations */
void orc_mapper_counters(orc_mapper_handle h, uint64_t out[8]);
/* SGM initialisation (esvo_Mapping.cpp:102-108,433-492,537-552): cv::StereoSGBM restated ("parity unpinned"),
 * the SGM event selection, InitializationAtTime + DepthFusion::naive_propagation */
void orc_sgbm_compute(const uint8_t* left, const uint8_t* right, int W, int H, int num_disp, int block, int P1, int P2,
                      int uniqueness, int16_t* disp);
long orc_decode_event_array(const uint8_t* msg, size_t n_bytes, esvo_event_t* out, size_t cap, uint32_t* height, uint32_t* width);
size_t orc_select_events_sgm(const esvo_event_t* ev, size_t n, uint64_t t_ns, double half_slice, size_t max_num, uint32_t* out_idx,
                             size_t cap);
size_t orc_mapper_init_sgm(orc_mapper_handle h, const uint8_t* ts_left, const uint8_t* ts_right, const esvo_event_t* ev, size_t n,
                           size_t min_points, int16_t* disp_out);
/* debug images + global-cloud helpers: Visualization::plot_map / DrawPoint (Visualization.cpp:13-94) with
 * publishMappingResults' arguments (esvo_Mapping.cpp:868-884); type 0 InvDepth, 1 StdVar, 2 Cost, 3 Age; bgr = H*W*3 */
void orc_jet_bgr(uint8_t out[768]);
void orc_mapper_debug_image(orc_mapper_handle h, int type, double age_max_range, uint8_t* bgr);
size_t orc_mapper_get_pointcloud_near_xyz(orc_mapper_handle h, double visualize_range, float* out_xyz, size_t cap_points);
size_t orc_voxel_filter(const float* xyz, size_t n, float leaf, float* out); /* pcl::VoxelGrid, esvo_Mapping.cpp:960-964 */
/* unit-test hooks */
int orc_mapper_eval_residual(orc_mapper_handle h, const double x_left[2], uint32_t pose_idx, double rho, double* fvec);
double orc_zncc_cost(const double* l, const double* r, int wx, int wy, int exact_int);
void orc_abi_sizes(size_t out[8]);

/* ---------- Tracker residual / Jacobian evaluation (esvo_core/src/core/RegProblemLM.cpp) ---------- */
typedef struct orc_tracker* orc_tracker_handle;
orc_tracker_handle orc_tracker_create(const esvo_calib_t* left);
void orc_tracker_destroy(orc_tracker_handle h);
/* getTimeSurfaceNegative(kernelSize in {0,5}) + computeTsNegativeGrad; returns -1 for another kernel size */
int orc_tracker_set_current(orc_tracker_handle h, const uint8_t* ts_left, int kernel_size);
void orc_tracker_get_images(orc_tracker_handle h, uint8_t* neg, int16_t* du, int16_t* dv);
void orc_tracker_set_reference(orc_tracker_handle h, const float* xyz_world, size_t n, const double T_world_ref[16]);
size_t orc_tracker_residuals(orc_tracker_handle h, const double T_left_ref[16], size_t offset, size_t count, int huber,
                             double huber_threshold, double* fvec);
size_t orc_tracker_jacobian(orc_tracker_handle h, const double R[9], const double t[3], size_t offset, size_t count,
                            double* fjac);
/* H = J^T J (upper triangle, 21), b = J^T f (6), |f|^2 of one tracker iteration in the device's summation order */
size_t orc_tracker_normal_equations(orc_tracker_handle h, const double R[9], const double t[3], size_t offset, size_t count,
                                    int huber, double huber_threshold, double out[28]);

#ifdef __cplusplus
}
#endif
#endif
