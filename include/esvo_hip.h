/*
 * esvo_hip.h — C-ABI of the MI355X-native ESVO hot path (Time-Surface raster +
 * semi-dense stereo mapper).
 *
 * This header is the drop-in boundary.  The reference (ESVO) has
 * no FFI/plugin interface: its algorithms are C++ classes called directly by the
 * ROS nodes.  Every entry point below therefore names the reference *seam* it
 * stands behind (file:line relative to the ESVO repository) — the call a
 * maintainer replaces in esvo_time_surface/src/TimeSurface.cpp and
 * esvo_core/src/esvo_Mapping.cpp / esvo_MVStereo.cpp.
 *
 * Conventions
 *   - plain C, opaque handle, no exceptions, no exit(): every call returns
 *     ESVO_OK (0) or a negative esvo_status_t; esvo_last_error() gives text.
 *   - all input buffers are borrowed for the duration of the call only.
 *   - outputs go to caller-allocated arrays (capacity + returned count).
 *   - Threads.  Distinct handles are independent.  On ONE handle the calls form three groups that may run
 *     concurrently, one thread per group -- the threading of the reference's nodes (esvo_Mapping.cpp:160,179-247: the
 *     MappingLoop worker thread; :669-703 and TimeSurface.cpp:403-425: eventsCallback on the ROS spinner under
 *     data_mutex_; esvo_Tracking's own loop):
 *       INGEST   esvo_ts_push_events(_async), esvo_ts_push_wait, esvo_ts_push_event_array, esvo_ts_push_event_columns, esvo_ts_push_evt3, esvo_ts_push_evt2, esvo_ts_push_bag (one thread per camera is fine)
 *       TRACKER  esvo_track_*
 *       MAPPER   every other call that takes the handle (renders, observation, ticks, stage-wise calls, outputs,
 *                parameters, esvo_comm_*, esvo_reset -- which excludes the other two groups while it runs)
 *       (esvo_ts_history_list and esvo_ts_history_select_observation belong to no group: any thread may call them)
 *     Calls of the same group are serialised by the library (safe from several threads, never concurrent).  The node's
 *     data_mutex_ is therefore NOT needed around these calls.  What the caller still owns is causality: a render or
 *     tick at time t sees the events staged when it is called, exactly like the reference's TS_history_/events_left_
 *     snapshot (dataTransferring) -- stage the events up to t before asking for t.  An ingest call never waits for a
 *     running tick (own HIP stream; the ring bookkeeping is locked for microseconds); the tracker calls run on a HIP
 *     stream of their own and wait only for the render that produced the Time Surface they read.
 *     esvo_last_error returns the message of the calling thread's last failed call.
 *   - every call is synchronous w.r.t. its host-visible outputs; calls without
 *     host outputs only enqueue work on the handle's HIP stream.
 *   - pointers named d_* are DEVICE pointers (HBM), everything else is host.
 *   - there is no CPU fallback: esvo_create() fails with ESVO_ERR_NO_DEVICE
 *     when no gfx950 device is visible.
 *   - Scheduling is the library's business and never changes a result: how many HIP queues a tick's stages use, which
 *     layout the refinement kernel runs in, whether two refinement launches are in flight -- the handle decides from the
 *     sizes of the launches and from its own stage timings (HIP events).  The ESVO_* environment variables read at
 *     esvo_create (tools/README.md lists them) pin those choices for measurements; none of them alters an output bit.
 *     ABI 8: the handle tells a tick that runs ALONE (its predecessor was completed and read before it was handed in -- the ROS
 *     node's pattern, esvo_Mapping.cpp:261-431 once per MappingLoop turn) from ticks that OVERLAP (a throughput loop that hands in
 *     tick k + 1 while tick k is in flight).  The first kind takes the latency path: one queue for the front stage and the LM
 *     launch, no stage-timing event between dependent kernels except on sampled ticks (esvo_stats_t.stage_timing_samples), the
 *     tick's frame compacted straight into the fusion window, polled host waits (the calling thread spins for up to 3 ms instead
 *     of sleeping on the completion interrupt) -- 0.54 instead of 0.68 ms for a DSEC tick of 10 000 events, same bits.
 */
#ifndef ESVO_HIP_H
#define ESVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESVO_HIP_ABI_VERSION 8

typedef enum esvo_status_t {
  ESVO_OK = 0,
  ESVO_ERR_INVALID_ARG = -1,
  ESVO_ERR_NO_DEVICE = -2,
  ESVO_ERR_HIP = -3,
  ESVO_ERR_CAPACITY = -4,
  ESVO_ERR_UNSUPPORTED = -5,
  ESVO_ERR_STATE = -6,
  ESVO_ERR_HALO = -7,  /* routed band mode: a refinement read outside the rank's Time-Surface rows (esvo_shard_set_routing) */
  ESVO_AGAIN = 1       /* not an error -- esvo_shard_tick_phase(h, 0, ...) on a routed handle with Denoising: all-gather the block of
                          esvo_shard_exchange (one bit per selected event: the rank's share of the denoising mask's verdicts), then call
                          phase 0 again (its arguments are ignored the second time) */
} esvo_status_t;

typedef struct esvo_context* esvo_handle;

enum { ESVO_CAM_LEFT = 0, ESVO_CAM_RIGHT = 1 };
enum { ESVO_FUSION_CONST_FRAMES = 0, ESVO_FUSION_CONST_POINTS = 1 };
enum { ESVO_LSNORM_TDIST = 0, ESVO_LSNORM_L2 = 1 /* Gaussian model; no shipped config uses it */ };

/* Layout-identical to the in-memory dvs_msgs::Event (uint16 x, uint16 y,
 * ros::Time{uint32 sec, uint32 nsec}, bool polarity; sizeof == 16), so ROS glue
 * passes msg->events.data() without a copy. */
typedef struct esvo_event_t {
  uint16_t x, y;
  uint32_t sec, nsec;
  uint8_t polarity;
  uint8_t _pad[3];
} esvo_event_t;

/* Per-camera calibration products.  They are what the reference's
 * PerspectiveCamera::preComputeRectifiedCoordinate (CameraSystem.cpp:36-111) and
 * TimeSurface::cameraInfoCallback (TimeSurface.cpp:313-401) compute once with
 * OpenCV; the caller passes them in (ROS glue: straight from its CameraSystem;
 * ROS-free harness: esvo_amd/calib.py). */
typedef struct esvo_calib_t {
  int32_t width, height;
  double P[12];              /* rectified 3x4 projection matrix, row-major (CameraSystem.cpp:31) */
  const float* rect_lut;     /* [H*W*2] raw pixel -> rectified (x,y), float32 as returned by
                                cv::undistortPoints (CameraSystem.cpp:62,106-110) */
  const uint8_t* rect_mask;  /* [H*W] 0/255 UndistortRectify_mask_ (CameraSystem.cpp:67-72);
                                may be NULL for the right camera */
  const float* map_x;        /* [H*W] undistort_map1_ CV_32FC1 (TimeSurface.cpp:341-351) */
  const float* map_y;        /* [H*W] undistort_map2_ */
} esvo_calib_t;

/* One POD carrying every yaml key the hot path reads. */
typedef struct esvo_params_t {
  /* esvo_time_surface (cfg/time_surface/ts_parameters.yaml; TimeSurface.cpp:23-30) */
  double decay_ms;                 /* 30 */
  int32_t median_blur_kernel_size; /* k: medianBlur(2k + 1); 1 -> 3x3 (every shipped config); 0 disables; 0..3 */
  int32_t ignore_polarity;         /* 1 */
  /* DepthProblemConfig (DepthProblem.h:15-51) */
  int32_t patch_size_x;            /* 15 in every shipped config (register-layout kernels); any 1..64 otherwise */
  int32_t patch_size_y;            /* 7 in every shipped config; any 1..40 otherwise */
  int32_t ls_norm;                 /* ESVO_LSNORM_TDIST */
  double td_nu;                    /* Tdist_nu */
  double td_scale;                 /* Tdist_scale */
  int32_t lm_max_iteration;        /* ITERATION_OPTIMIZATION (10); maxfev = 3x */
  int32_t reg_radius;              /* RegularizationRadius */
  int32_t reg_min_neighbours;      /* RegularizationMinNeighbours */
  int32_t reg_min_close_neighbours;/* RegularizationMinCloseNeighbours */
  /* EventBM (EventBM.cpp:34-54).  min/max are the EFFECTIVE range after the
   * depth-range clamp of esvo_Mapping.cpp:110-116 (esvo_amd/params.py does it). */
  int32_t bm_min_disparity;
  int32_t bm_max_disparity;
  int32_t bm_step;                 /* 1 in every shipped config; > 1: coarse-to-fine search (EventBM.cpp:118-138) */
  double bm_zncc_threshold;        /* 0.1 */
  int32_t bm_updown;               /* BM_bUpDownConfiguration: vertical epipolar search (EventBM.cpp:178-186) */
  int32_t smooth_time_surface;     /* SmoothTimeSurface: 5x5 Gaussian before BM (DSEC) */
  /* mapping node (esvo_Mapping.cpp:63-99) */
  double invdepth_min, invdepth_max;
  double stdvar_vis_threshold;     /* sigma; culling/clean compare against its square */
  double residual_vis_threshold;   /* cost threshold = thr^2 * patch area */
  double age_vis_threshold;
  int32_t fusion_radius;           /* 0 -> 2x2, !=0 -> 3x3 (DepthFusion.cpp:98-117) */
  int32_t fusion_strategy;         /* ESVO_FUSION_CONST_FRAMES / _CONST_POINTS */
  int32_t max_fusion_frames;
  int32_t max_fusion_points;
  int32_t clean_requires_full_window; /* 1: esvo_Mapping.cpp:385; 0: esvo_MVStereo.cpp:496 */
  int32_t regularization;          /* Regularization */
  int32_t denoising;               /* Denoising: event-map median mask on the selected events
                                      (esvo_Mapping.cpp:282-296,1046-1072); applied by esvo_map_tick */
  int32_t process_event_num;       /* PROCESS_EVENT_NUM (events block-matched per tick) */
  double bm_half_slice_thickness;  /* 0.001 s; event window = 10x (esvo_Mapping.cpp:563) */
  int32_t num_threads;             /* NUM_THREAD_MAPPING (4): reproduces the stride-N output
                                      permutation of EventBM.cpp:289-308 and
                                      DepthProblemSolver.cpp:75-90 */
  /* capacities (device allocations; 288 GB of HBM makes generous defaults cheap) */
  int32_t max_events_per_tick;     /* >= process_event_num */
  int32_t max_window_points;       /* total DepthPoints the fusion window may hold */
  int32_t max_poses_per_tick;      /* >= 201 */
  int64_t event_ring_capacity;     /* staged events per camera */
  /* esvo_time_surface: max_event_queue_len (TimeSurface.cpp:30, default 20).  0 (default here): ONE stamp per pixel -- the
   * fast path; render times must not decrease and the queue's eviction artefact (a render older than max_event_queue_len
   * newer events of a pixel reads that pixel empty, TimeSurface.h:39-75) is not reproduced.  1..32: EventQueueMat semantics
   * exactly -- every staged event enters its pixel's queue at the next render, renders at any time in any order. */
  int32_t max_event_queue_len;
  /* Scale-loop guard of the LM refinement (esvo_map_lm_stats below).  The reference's Student-t scale loop
   * (DepthProblem.cpp:96-124) has no iteration cap.  0 (default): off -- nothing is counted or bounded.  > 0: a match is abandoned
   * by its first evaluation that has completed this many passes while the loop test asks for another; it yields no point.
   * ESVO_LM_SCALE_COUNT_ONLY: passes are counted, no match is abandoned.  Negative: refused. */
  int32_t lm_scale_pass_limit;
} esvo_params_t;
#define ESVO_LM_SCALE_COUNT_ONLY INT32_MAX

/* What flows EventBM -> DepthProblemSolver.  The reference's EventMatchPair
 * (EventMatchPair.h:16-38) carries a full pose; consumers read only x_left_,
 * trans_, invDepth_ (DepthProblemSolver.cpp:92-94) and cost_/disp_ in BM-only mode. */
typedef struct esvo_match_t {
  double x_left[2];   /* rectified left coordinate */
  double inv_depth;   /* disparity / (baseline * P(0,0)) */
  double cost;        /* ZNCC cost of the best candidate */
  double disp;
  uint32_t event_idx; /* index into the events passed to the call */
  uint32_t pose_idx;  /* index into the tick's pose table (first stamp >= event ts) */
} esvo_match_t;

/* Every field of DepthPoint (DepthPoint.h:70-88); the 4x4 T_world_cam_ is
 * carried as an index into the pose table of the frame the point came from. */
typedef struct esvo_depth_point_t {
  uint32_t row, col;
  double x[2];
  double inv_depth;
  double scale2;
  double nu;
  double variance;
  double residual;
  uint64_t age;
  double p_cam[3];
  uint32_t pose_idx;
  uint32_t seq;       /* DepthMap outputs: creation order in the reference's element list */
} esvo_depth_point_t;

/* Stage timings use the reference's own stage boundaries (esvo_Mapping.cpp:405-430). */
typedef struct esvo_stats_t {
  uint64_t ticks;
  uint64_t events_staged[2];
  uint64_t events_scattered[2];
  uint64_t ts_frames[2];
  uint32_t last_events_in;      /* events handed to block matching in the last tick */
  uint32_t last_matches;        /* BM successes */
  uint32_t last_solved;         /* LM problems solved */
  uint32_t last_points;         /* after pointCulling */
  uint32_t last_window_frames;
  uint32_t last_window_points;
  uint32_t last_fusions;        /* DepthFusion::update return, summed over the window */
  uint32_t last_map_size;       /* DepthMap::size() after clean/regularisation */
  float ms_ts_scatter, ms_ts_render;
  float ms_bm, ms_refine, ms_fusion, ms_regularization, ms_tick_total;
  /* HIP-event time of single kernels / stages of the last tick (for roofline accounting):
   * [0] ts_scatter [1] ts_decay+median_remap [2] bm_match [3] lm_refine
   * [4] propagate+bucket+fuse_cells [5] clean [6] regularize [7] reserved.
   * The matching stage ([0]-[2]), the LM stage ([3]) and the fusion stage ([4]-[6]) of consecutive ticks run on three
   * streams at the same time, so the values are not additive and each includes the slowdown from the other streams'
   * kernels. */
  float ms_kernel[8];
  float pad_;
  /* Running totals over all ticks since esvo_create / esvo_reset.  A throughput loop reads them once at its
   * end: esvo_get_stats drains the streams, so calling it after every tick serialises the overlap of one
   * tick's LM and fusion stages with the next tick's matching stage. */
  uint64_t total_events_in;
  uint64_t total_matches;
  uint64_t total_points;
  double sum_ms_kernel[8];      /* same slots as ms_kernel; [7] = launches of ts kernels summed in [0],[1] */
  /* EventBM's failure counters by reason (EventBM.h:89; incremented at EventBM.cpp:107, :124, :135), of the last block
   * matching and summed over the ticks: left patch with > 95 % of its pixels below 1, coarse search without a match
   * (with BM_step 1: no candidate below the ZNCC threshold), fine search without a match. */
  uint32_t last_bm_info_noise_low, last_bm_coarse_fail, last_bm_fine_fail, pad2_;
  uint64_t total_bm_info_noise_low, total_bm_coarse_fail, total_bm_fine_fail;
  /* ABI 3 -- the shader clock the refinement kernel really ran at, measured inside the run (no profiler): lane 0 of every
   * 65th workgroup of the kernel reads s_memtime (shader cycles) and s_memrealtime (constant reference clock, clk_ref_khz)
   * when it starts and when it ends; the differences are summed per XCD since esvo_create / esvo_reset.
   * clock [MHz] of XCD x = clk_cycles[x] / clk_ref_ticks[x] * clk_ref_khz / 1000; all XCDs: the ratio of the sums. */
  uint64_t clk_cycles[8];
  uint64_t clk_ref_ticks[8];
  uint64_t clk_samples;
  uint32_t clk_ref_khz;
  /* ABI 8 -- how many ticks contributed to ms_bm .. ms_regularization, ms_kernel[2..6] and sum_ms_kernel[2..6].  Stage timings come
   * from HIP events recorded between the stages, and every such record costs the queue about 5 us (the next dispatch waits for
   * the marker; kernels with no event between them follow each other without a gap).  So stage timings are SAMPLED where those
   * gaps are on the path somebody waits for: a tick that runs ALONE -- the caller read the previous tick's result before handing it
   * in, as the ROS node does -- records its events on the handle's first 8 such ticks and on one in 31 afterwards; small ticks that
   * overlap (at most 40 000 events: the host's enqueueing is their pace) on one tick in four.  Large overlapping ticks (the
   * throughput path, paced by the LM kernel) and the own ticks of a tick-interleaved multi-GPU rank record every tick.  ms_* hold the latest sample, sum_ms_kernel[2..6] the sum
   * over the samples, the mean per tick is sum / stage_timing_samples.  ms_ts_* / sum_ms_kernel[0..1] are sampled the same way with
   * their own count in [7]. */
  uint32_t stage_timing_samples;
  /* ABI 6 -- routed band mode (esvo_shard_set_routing): matches, summed over ALL ranks and the ticks since esvo_create /
   * esvo_reset, whose refinement read rows of the Time Surfaces this rank does not render.  Non-zero: the handle refuses
   * further ticks with ESVO_ERR_HALO. */
  uint64_t halo_violations;
  /* Events that arrived out of order (stamp below the newest stamp staged before them), per camera: sorted into the ring for
   * the mapper, withheld from the Time Surface as the reference's eventsCallback withholds them (esvo_ts_push_events). */
  uint64_t late_events[2];
  /* How often the tick pipeline let its back stream drain to get out of its slow operating point (api_map.hip, pipeline_resync):
   * 0 in an undisturbed run. */
  uint64_t pipeline_resyncs;
} esvo_stats_t;

/* ---- lifecycle -------------------------------------------------------------------- */

/* Fill *p with the reference's code defaults (esvo_Mapping.cpp:37-99, TimeSurface.cpp:23-30). */
void esvo_default_params(esvo_params_t* p);

/* Replaces: TimeSurface ctor + cameraInfoCallback (TimeSurface.cpp:12-50,313-401) and the
 * esvo_Mapping ctor's CameraSystem/EventBM/DepthProblemSolver/DepthFusion setup
 * (esvo_Mapping.cpp:26-128).  `device` is the HIP device ordinal. */
int esvo_create(const esvo_params_t* params, const esvo_calib_t* left, const esvo_calib_t* right,
                int device, esvo_handle* out);
int esvo_destroy(esvo_handle h);
/* Replaces esvo_Mapping::reset (esvo_Mapping.cpp:764-804): clears SAE, event rings, window, map. */
int esvo_reset(esvo_handle h);
/* Replaces EventBM::resetParameters (EventBM.cpp:34-54) + onlineParameterChangeCallback
 * (esvo_Mapping.cpp:806-866).  Capacities and image size cannot change. */
int esvo_set_params(esvo_handle h, const esvo_params_t* params);
const char* esvo_last_error(esvo_handle h); /* h may be NULL for create-time errors */
/* Run the handle's kernels on an external HIP stream (e.g. torch's current stream). */
int esvo_set_stream(esvo_handle h, void* hip_stream);
int esvo_synchronize(esvo_handle h);

/* ---- Time Surface ------------------------------------------------------------------ */

/* Replaces TimeSurface::eventsCallback + EventQueueMat::insertEvent (TimeSurface.cpp:403-425,
 * TimeSurface.h:39-50) and, for the left camera, esvo_Mapping::eventsCallback
 * (esvo_Mapping.cpp:669-703).  Events must be time-sorted (Appendix A-1). */
int esvo_ts_push_events(esvo_handle h, int cam, const esvo_event_t* ev, size_t n);
/* The same without waiting for the copy: the call returns once the host-to-device copy of `ev` is ENQUEUED on the ingest stream
 * (time stamps and order are checked during the call).  `ev` must stay valid and unchanged until esvo_ts_push_wait(h, cam) has
 * returned.  Meant for PINNED buffers (esvo_host_alloc below, or the node's own hipHostRegister'ed message pool): from pinned
 * memory the copy is a DMA that overlaps the running tick, so a node that stages every tick's events pays no PCIe time on
 * its mapping thread; from pageable memory the runtime stages the copy itself and the call is as synchronous as
 * esvo_ts_push_events.  Renders and ticks that read the events are ordered behind the copy on the device (an event wait on the
 * handle's front stream), never by a host wait. */
int esvo_ts_push_events_async(esvo_handle h, int cam, const esvo_event_t* ev, size_t n);
int esvo_ts_push_wait(esvo_handle h, int cam);
/* Pinned host memory for such buffers (hipHostMalloc / hipHostFree behind the C-ABI; no handle needed). */
int esvo_host_alloc(size_t bytes, void** out);
int esvo_host_free(void* p);
/* The same, straight from the ROS1 wire format: `msg` is one serialised
 * dvs_msgs/EventArray (Header, u32 height, u32 width, u32 count, count x 13-byte dvs_msgs/Event: u16 x, u16 y,
 * u32 sec, u32 nsec, u8 polarity) as a rosbag chunk or a TCPROS connection delivers it.  The packed records are copied to
 * the device as they are (13 instead of 16 B/event over PCIe) and widened into the ring by a kernel; no
 * std::vector<dvs_msgs::Event> is materialised (rosbag::MessageInstance::instantiate does that at
 * events_repacking_helper/src/EventMessageEditor.cpp:111).  *n_events (nullable) receives the message's event count. */
int esvo_ts_push_event_array(esvo_handle h, int cam, const uint8_t* msg, size_t n_bytes, size_t* n_events);
/* The same from COLUMNS: four arrays x / y / t / p of n elements each, in host or in device memory -- what DSEC's files hold
 * (x u16, y u16, p u8, t u32 microseconds + t_offset), what MVSEC-derived and simulator streams are, and what a GPU producer (a torch
 * loader, a simulator) has in device memory already.  No esvo_event_t is interleaved on the host and no stamp is split there.
 *   Conversion (exact, the same on every path): stamp_ns = (t[i] + t_offset) * (1 for ESVO_T_NS_I64, 1000 for the two US types), in
 *   integers without wrap-around.  An element is INVALID if an intermediate does not fit or the result lies outside
 *   0 <= stamp_ns < 2^32 * 10^9 (what sec can hold).  sec = stamp_ns / 10^9, nsec = stamp_ns % 10^9; the bits of x and y are copied;
 *   polarity is 1 where p[i] != 0 (ESVO_P_U8) or (int8_t)p[i] > 0 (ESVO_P_I8, the +-1 convention), else 0; p == NULL: every event
 *   ON; _pad is 0.  Any invalid element: ESVO_ERR_INVALID_ARG, esvo_last_error names the first bad index, nothing is staged and no
 *   handle state changes.
 *   Behaviour: exactly that of esvo_ts_push_events handed those records, in everything a later call can observe -- the in-order fast
 *   path; the out-of-order merge with its late marks, stats.late_events and the queue mode's second copies; the routed band path;
 *   the same capacity and state errors (out-of-order on a routed handle included); n == 0 is a no-op.  Synchronous: when the call
 *   returns it has finished reading the columns, they may be reused at once.
 *   memory = ESVO_MEM_DEVICE: the columns must be COMPLETE before the call (the caller synchronises its producing stream) and plain
 *   device memory of the handle's GPU; the library checks that with hipPointerGetAttributes before any launch or copy: host, managed
 *   or foreign-device pointers labelled DEVICE return ESVO_ERR_INVALID_ARG, and so does a device pointer labelled HOST.  Column
 *   bases need only the alignment of their element type (a caller passes slices).
 *   In-order packets on an unrouted handle are packed into the ring by a kernel: host columns go up as they are beside their u64
 *   stamps (13 B/event), device columns are read where they lie (8 B/event of stamps come down for the order check and the host's
 *   stamp index).  The other packets -- out of order inside themselves, reaching back behind the newest staged stamp, or any packet
 *   on a routed handle -- are materialised as esvo_event_t on the host and take the paths of esvo_ts_push_events. */
enum { ESVO_T_NS_I64 = 0, ESVO_T_US_I64 = 1, ESVO_T_US_U32 = 2 };   /* element type and unit of t */
enum { ESVO_P_U8 = 0 /* != 0 is ON */, ESVO_P_I8 = 1 /* > 0 is ON: the +-1 convention */ };
enum { ESVO_MEM_HOST = 0, ESVO_MEM_DEVICE = 1 };
typedef struct esvo_event_columns_t {
  const void* x; const void* y;   /* 16-bit each, read as unsigned (an int16 tensor's bits are fine) */
  const void* t;                  /* t_type */
  const void* p;                  /* p_type; NULL: every event ON */
  int64_t t_offset;               /* in t's unit, added BEFORE the unit is scaled (DSEC's t_offset) */
  int32_t t_type, p_type, memory, reserved;
} esvo_event_columns_t;
int esvo_ts_push_event_columns(esvo_handle h, int cam, const esvo_event_columns_t* c, size_t n);
/* The conversion alone: host memory only (memory must be ESVO_MEM_HOST), no handle, no GPU.  *first_bad (nullable) receives the
 * index of the first invalid element (then ESVO_ERR_INVALID_ARG is returned and `out` holds the records before it), else n. */
int esvo_event_columns_to_events(const esvo_event_columns_t* c, size_t n, esvo_event_t* out, size_t* first_bad);
/* sizeof(esvo_event_columns_t), 0, 0, 0 */
void esvo_event_columns_sizes(size_t out[4]);
/* The same from Prophesee EVT 3.0 words (Metavision SDK callbacks, the data of .raw files), decoded on the device: a stateful stream
 * of little-endian uint16 words, 2-4 bytes per event, in host or in device memory.  No esvo_event_t exists on the host for an
 * in-order packet on an unrouted handle.  type = w >> 12:
 *   0x0 ADDR_Y       y_cur = w & 0x7FF (bit 11 ignored); have_y
 *   0x2 ADDR_X       one event (w & 0x7FF, y_cur, t_cur, (w >> 11) & 1)
 *   0x3 VECT_BASE_X  base_x = w & 0x7FF; vect_pol = (w >> 11) & 1; have_base
 *   0x4 VECT_12      for i = 0..11 ascending with bit i of w & 0xFFF set: event ((base_x + i) & 0xFFFF, y_cur, t_cur, vect_pol); then
 *                    base_x = (base_x + 12) & 0xFFFF
 *   0x5 VECT_8       the same with w & 0xFF, i = 0..7 and base_x + 8
 *   0x6 TIME_LOW     time_low = w & 0xFFF
 *   0x8 TIME_HIGH    v = w & 0xFFF; if have_th && v < time_high && time_high - v >= 2048: loops += 1.  time_high = v; have_th.
 *                    time_low is KEPT.
 *   0xA EXT_TRIGGER  ignored, counted in ext_triggers;   every other type: ignored, counted in ignored_words
 *   t_us = loops << 24 | time_high << 12 | time_low;  stamp_ns = (t_us + t_offset_us) * 1000, by the conversion of ESVO_T_US_I64 columns
 *   above: a stamp outside [0, 2^32 * 10^9) makes the call fail.  An ADDR_X word emits iff have_th && have_y, a VECT word iff
 *   have_base as well; the events a word would have emitted otherwise are counted in dropped_events.  base_x advances on every VECT
 *   word whether it emits or not.  x and y are not checked against the sensor: the scatter skips events outside the image, as for
 *   every other source.  A stream starts with all state zero.
 *   PARITY UNPINNED in two points, which follow no third-party decoder: the time-loop threshold (a TIME_HIGH step back of 2048 units
 *   or more is a loop, a smaller one is not) and TIME_LOW being kept across a TIME_HIGH word.  Cameras send monotone TIME_HIGH words
 *   many times per millisecond, so every sane rule agrees on their streams.  Out of scope: delivery of EXT_TRIGGER events, AEDAT4,
 *   the Prophesee DAT format.  (EVT 2.0 / 2.1: esvo_ts_push_evt2 below.)
 *   The decoder state is kept per camera and carried from one call to the next: a stream may be cut at any word boundary.
 *   esvo_reset clears the state and the totals of both cameras; esvo_ts_evt3_state(set) lets a reader seek or resume.
 *   Behaviour: exactly that of esvo_ts_push_events handed the decoded records, in everything a later call can observe -- the in-order
 *   fast path; the out-of-order merge with its late marks, stats.late_events and the queue mode's second copies; the routed band
 *   path and its refusals; the same capacity and state errors.  ALL OR NOTHING: any failure (arguments, a bad stamp, ring capacity,
 *   a refusal) stages nothing and leaves the decoder state and the totals as they were; for a bad stamp esvo_last_error names the
 *   first bad EVENT index.  A packet that emits no event still advances the state and the totals and returns ESVO_OK with
 *   *n_events = 0.  n_bytes odd, words not 2-byte aligned, more than 2^31 - 1 words: ESVO_ERR_INVALID_ARG; a decoded count above
 *   the ring's capacity: ESVO_ERR_CAPACITY (the caller cuts the chunk).  Synchronous: words may be reused when the call returns.
 *   memory = ESVO_MEM_DEVICE: the words must be COMPLETE before the call and plain device memory of the handle's GPU; the library
 *   checks first and last byte with hipPointerGetAttributes before any launch or copy, as for columns.
 *   In-order packets on an unrouted handle are decoded by three dependent launches (a last-writer / sum scan over the words, the
 *   time-loop and event counts, the expansion into the column staging) and packed into the ring like device columns; one small
 *   read-back (event count, end state, counts, first bad stamp) decides before anything touches the ring.  The other packets -- out
 *   of order inside themselves, reaching back behind the newest staged stamp, any packet on a routed handle -- and packets too small
 *   to pay for the launches are decoded on the host by esvo_evt3_to_events and take the paths of esvo_ts_push_events. */
typedef struct esvo_evt3_state_t {
  uint32_t flags;   /* bit0 have_th, bit1 have_y, bit2 have_base, bit3 vect_pol */
  uint16_t y, base_x, time_high, time_low;
  uint32_t loops;
  uint32_t reserved;
} esvo_evt3_state_t;
typedef struct esvo_evt3_counts_t { uint64_t words, events, dropped_events, ignored_words, ext_triggers, time_loops; } esvo_evt3_counts_t;
int esvo_ts_push_evt3(esvo_handle h, int cam, const void* words, size_t n_bytes, int memory /* ESVO_MEM_HOST | ESVO_MEM_DEVICE */,
                      int64_t t_offset_us, size_t* n_events /* nullable */);
/* get (nullable) receives the camera's decoder state, then set (nullable) replaces it */
int esvo_ts_evt3_state(esvo_handle h, int cam, esvo_evt3_state_t* get, const esvo_evt3_state_t* set);
/* running totals of the camera's successful esvo_ts_push_evt3 calls; cleared by esvo_reset */
int esvo_ts_evt3_stats(esvo_handle h, int cam, esvo_evt3_counts_t* totals);
/* The decoder alone: host only, no handle, no GPU.  out == NULL counts (cap is ignored).  *n_out (nullable) receives the number of
 * events; *counts (nullable) what this call decoded.  More events than cap: ESVO_ERR_CAPACITY.  A bad stamp: ESVO_ERR_INVALID_ARG,
 * *n_out is the index of the first bad event (esvo_last_error(NULL) names it).  *st is advanced only on ESVO_OK. */
int esvo_evt3_to_events(esvo_evt3_state_t* st, const uint16_t* words, size_t n_words, int64_t t_offset_us,
                        esvo_event_t* out, size_t cap, size_t* n_out, esvo_evt3_counts_t* counts);
/* Prophesee .raw: ASCII header lines each starting with '%', ended by the first line that does not (or by "% end\n").
 * *data_offset = first byte of the word data; *width / *height (nullable) from a "% geometry WxH" line, or width= / height= fields
 * of a "% format" line, 0 if absent.  A "% evt" / "% format" line naming anything but 3.0 / EVT3: ESVO_ERR_UNSUPPORTED. */
int esvo_evt3_raw_header(const uint8_t* file, size_t n_bytes, size_t* data_offset, int* width, int* height);
/* sizeof(esvo_evt3_state_t), sizeof(esvo_evt3_counts_t), 0, 0 */
void esvo_evt3_sizes(size_t out[4]);
/* The same from Prophesee EVT 2.0 words (Gen3.1 / Gen4 kits, most archived .raw recordings) and EVT 2.1 words (the vectorised format of
 * the high-rate sensors), decoded on the device.
 *   EVT 2.0: little-endian uint32 words w; type = w >> 28:
 *     0x0 CD_OFF, 0x1 CD_ON  one event: x = (w >> 11) & 0x7FF, y = w & 0x7FF, ts6 = (w >> 22) & 0x3F, polarity = type.  The word emits
 *                            iff have_th; otherwise dropped_events += 1.
 *     0x8 EVT_TIME_HIGH      v = w & 0x0FFFFFFF; if have_th && v < time_high && time_high - v >= 2^27: loops += 1.  Then time_high = v;
 *                            have_th = 1.
 *     0xA EXT_TRIGGER        ignored, counted in ext_triggers
 *     every other type (0xE OTHERS, 0xF CONTINUED included): ignored, counted in ignored_words
 *   EVT 2.1: 64-bit words W; type = W >> 60, ts6 = (W >> 54) & 0x3F, x0 = (W >> 43) & 0x7FF, y = (W >> 32) & 0x7FF,
 *   valid = W & 0xFFFFFFFF:
 *     0x0 EVT_NEG, 0x1 EVT_POS  for i = 0..31 ascending with bit i of valid set: event (x0 + i, y, t, type).  x0 need not be a multiple
 *                            of 32; x0 + i fits 16 bits.  The word emits iff have_th; otherwise dropped_events += popcount(valid).
 *     0x8 EVT_TIME_HIGH      v = (W >> 32) & 0x0FFFFFFF, the rule of EVT 2.0
 *     0xA / every other type: as in EVT 2.0
 *     In memory a word is two little-endian uint32: ESVO_EVT_2_1: W = (u64)second << 32 | first, a plain little-endian uint64;
 *     ESVO_EVT_2_1_LEGACY: W = (u64)first << 32 | second, the upper half stored first.
 *   t_us = loops << 34 | time_high << 6 | ts6; loops >= 2^18 makes the stamp invalid (it would lie outside the range anyway, and the
 *   arithmetic stays inside 64 bits).  stamp_ns = (t_us + t_offset_us) * 1000, by the conversion of ESVO_T_US_I64 columns above: a stamp
 *   outside [0, 2^32 * 10^9) makes the call fail and esvo_last_error names the first bad EVENT index.  x and y are not checked against
 *   the sensor: the scatter skips events outside the image, as for every other source.  A stream starts with all state zero.
 *   PARITY UNPINNED: no Prophesee decoder or document was at hand; the tables follow the published description as recalled, and
 *   nothing third-party pins them.  Three points in particular: the time-loop threshold (a TIME_HIGH step back of 2^27 units or more
 *   is a loop, a smaller one is not); the half order of EVT 2.1 (ESVO_EVT_2_1 reads a word as one little-endian uint64,
 *   ESVO_EVT_2_1_LEGACY with the upper half first); and a "% evt 2.1" header without an endianness field, which esvo_raw_header takes
 *   for ESVO_EVT_2_1 (only "endianness=legacy" on the format line selects the legacy order).  Out of scope: delivery of EXT_TRIGGER
 *   events, AEDAT4, the Prophesee DAT format.
 *   esvo_ts_push_evt2 behaves sentence for sentence as esvo_ts_push_evt3 above: exactly as esvo_ts_push_events handed the decoded
 *   records, in everything a later call can observe (the in-order fast path; the out-of-order merge with its late marks and
 *   stats.late_events; the queue mode's second copies; the routed band path and its refusals; the same capacity and state errors);
 *   ALL OR NOTHING: any failure stages nothing and leaves the decoder state and the totals as they were; a packet that emits no event
 *   still advances the state and the totals; synchronous; for ESVO_MEM_DEVICE the first and last byte are checked with
 *   hipPointerGetAttributes before any launch or copy.  The state is per camera, carried across calls, cleared by esvo_reset; ONE state
 *   serves the three formats.  ESVO_ERR_INVALID_ARG: an unknown format (ESVO_EVT_3_0 included: that is esvo_ts_push_evt3's), n_bytes
 *   not a multiple of 4 (EVT 2.0) or 8 (EVT 2.1), a base that is not 4-byte aligned (4 bytes suffice for EVT 2.1 as well: a slice of an
 *   int32 tensor is a legal argument), more than 2^31 - 1 words.
 *   In-order packets on an unrouted handle are decoded by three dependent launches over tiles of 2048 words (the newest TIME_HIGH in
 *   front of every word by a max scan; the event and time-loop counts; the expansion into the column staging, where a wave writes two
 *   EVT 2.1 words per step, lane = bit index, so that stamps / x / y / p go out coalesced) and one 64-byte read-back decides before
 *   anything touches the ring.  Packets on a routed handle, out-of-order packets, packets below the host / device bound and packets
 *   above the tile limit are decoded on the host by esvo_evt2_to_events. */
enum { ESVO_EVT_2_0 = 20, ESVO_EVT_2_1 = 21, ESVO_EVT_2_1_LEGACY = 121, ESVO_EVT_3_0 = 30 };
typedef struct esvo_evt2_state_t { uint32_t flags /* bit0 have_th */, time_high, loops, reserved; } esvo_evt2_state_t;
typedef esvo_evt3_counts_t esvo_evt2_counts_t;   /* words (32- or 64-bit, by format), events, dropped_events, ignored_words, ext_triggers, time_loops */
int esvo_ts_push_evt2(esvo_handle h, int cam, const void* words, size_t n_bytes, int format /* ESVO_EVT_2_0 | ESVO_EVT_2_1 | ESVO_EVT_2_1_LEGACY */,
                      int memory /* ESVO_MEM_HOST | ESVO_MEM_DEVICE */, int64_t t_offset_us, size_t* n_events /* nullable */);
/* get (nullable) receives the camera's decoder state, then set (nullable) replaces it (flags masked to bit 0, time_high to 28 bits) */
int esvo_ts_evt2_state(esvo_handle h, int cam, esvo_evt2_state_t* get, const esvo_evt2_state_t* set);
/* running totals of the camera's successful esvo_ts_push_evt2 calls; cleared by esvo_reset */
int esvo_ts_evt2_stats(esvo_handle h, int cam, esvo_evt2_counts_t* totals);
/* The decoder alone: host only, no handle, no GPU; the contract of esvo_evt3_to_events (out == NULL counts; *st advances only on
 * ESVO_OK; a bad stamp: ESVO_ERR_INVALID_ARG with *n_out the index of the first bad event; more events than cap: ESVO_ERR_CAPACITY) */
int esvo_evt2_to_events(esvo_evt2_state_t* st, const void* words, size_t n_bytes, int format, int64_t t_offset_us,
                        esvo_event_t* out, size_t cap, size_t* n_out, esvo_evt2_counts_t* counts);
/* The general form of esvo_evt3_raw_header: *format (nullable) receives ESVO_EVT_2_0 for "% evt 2.0" / "% format EVT2;...",
 * ESVO_EVT_2_1 for "% evt 2.1" / "% format EVT21;...", ESVO_EVT_2_1_LEGACY where the format line carries "endianness=legacy",
 * ESVO_EVT_3_0 for 3.0 / EVT3, 0 if no line names a format.  Any other named format: ESVO_ERR_UNSUPPORTED. */
int esvo_raw_header(const uint8_t* file, size_t n_bytes, size_t* data_offset, int* width, int* height, int* format);
/* sizeof(esvo_evt2_state_t), sizeof(esvo_evt2_counts_t), 0, 0 */
void esvo_evt2_sizes(size_t out[4]);
/* Event filter on the device: hot-pixel mask, per-pixel refractory period and nearest-neighbour background-activity filter, applied
 * to a raw sensor stream between decode and the event ring.  Off unless configured; a handle without it takes the paths above
 * unchanged.  Each camera has its own state: one uint64 per RAW pixel, last[y][x], the ns stamp of the newest event at that pixel
 * that passed the mask and the refractory test (0: none; an event stamped 0 never counts).  Events are judged one by one in stream
 * order (t: the event's stamp in ns; the stream is time-sorted; differences are taken as integers, so a planted `last` ahead of
 * the stream gives a negative one):
 *   verdict(e):
 *     if e.x >= W or e.y >= H:            ESVO_FILTER_OUTSIDE      (1)  touches nothing
 *     if mask[e.y][e.x] != 0:             ESVO_FILTER_MASKED       (2)  touches nothing
 *     L = last[e.y][e.x]
 *     if refractory_ns > 0 and L != 0 and t - L < refractory_ns:
 *                                         ESVO_FILTER_REFRACTORY   (3)  touches nothing
 *     sup = any(last[n] != 0 and t - last[n] <= support_ns
 *               for n in the up-to-8 neighbours of (x, y) inside the image)    -- read BEFORE the next line
 *     last[e.y][e.x] = t
 *     if support_ns > 0 and not sup:      ESVO_FILTER_UNSUPPORTED  (4)
 *     else:                               ESVO_FILTER_KEPT         (0)
 *   So a refractory-dropped or masked event neither supports a neighbour nor restarts the refractory period; an unsupported event does
 *   both; an earlier event of the same packet with the same stamp supports, a later one does not; the pixel never supports itself.
 *   Polarity plays no part.  PINNED TO NOTHING THIRD-PARTY: the whole rule is this library's own, in particular `<` for the refractory
 *   test, `<=` for support, and unsupported events updating `last`.
 * Only KEPT events are staged: the ring, the stamp mirror, stats.events_staged, the Time Surface and the mapper's selection are those
 * of esvo_ts_push_events given just the kept events, in the same order.  With a filter configured EVERY push call of the camera goes
 * through it: esvo_ts_push_events, _async (then synchronous, as in routed mode), _event_array, _bag, _event_columns, _evt3, _evt2.
 * What those calls report about their INPUT is unchanged (*n_events and the EVT decoder totals count decoded events); how many were
 * staged is the `kept` delta of esvo_ts_filter_stats.  A packet of which nothing is kept returns ESVO_OK, stages nothing and still
 * advances `last`.  An out-of-order packet -- not sorted in itself, or starting before the newest staged stamp -- is refused with
 * ESVO_ERR_UNSUPPORTED: a raw sensor stream is monotone, the late-event rules of the unfiltered path are not extended.  Every refusal
 * (bad arguments, a bad stamp, ESVO_ERR_CAPACITY, ESVO_ERR_UNSUPPORTED) leaves ring, mirror, `last` and totals as they were; RING ROOM
 * IS THEREFORE JUDGED ON THE UNFILTERED COUNT, before the filter runs: a packet whose decoded events would not fit is refused even
 * if its kept events would.  esvo_reset zeroes `last` and the totals and keeps the configuration; esvo_destroy frees everything.
 * Every source reaches the ring through the column form (u64 stamp, u16 x, u16 y, polarity): a record handed in with nsec >= 10^9 or
 * a polarity byte above 1 is staged as sec * 10^9 + nsec re-split and polarity 0 / 1, padding 0.
 * The filter runs on the camera's column staging on the ingest stream: the packet's events are binned by 8x8-pixel tile (each also
 * into the neighbouring tiles whose one-pixel halo holds it), one wave per tile sorts its list into stream order and applies the
 * rule with the tile's 10x10 patch of `last` and of the mask in LDS -- the chains of the halo pixels are recomputed there, which
 * makes the tiles independent -- a scan over the verdicts compacts the columns, and the existing column pack writes the ring.  A
 * tile whose list overflows reads the packet itself instead: same answers, bounded cost.  A device-resident packet (device columns,
 * decoded words) is judged for order and stamp validity by the compaction kernel: its unfiltered stamps never come down, the one
 * read-back of the push carries the verdict counts and the kept stamps. */
enum { ESVO_FILTER_KEPT = 0, ESVO_FILTER_OUTSIDE = 1, ESVO_FILTER_MASKED = 2, ESVO_FILTER_REFRACTORY = 3, ESVO_FILTER_UNSUPPORTED = 4 };
typedef struct esvo_event_filter_t {
  uint64_t refractory_ns, support_ns;   /* 0: that test is off */
  const uint8_t* mask;                  /* [H * W], non-zero = masked; NULL: none.  Copied by esvo_ts_filter_configure. */
  uint32_t reserved[4];                 /* 0 */
} esvo_event_filter_t;
typedef struct esvo_event_filter_counts_t { uint64_t events_in, kept, outside, masked, refractory, unsupported; } esvo_event_filter_counts_t;  /* events_in: the sum of the other five */
/* f == NULL switches the camera's filter off and frees its memory; otherwise the mask is copied, the camera's `last` image is zeroed
 * and the totals stay.  ESVO_ERR_UNSUPPORTED on a row-routed band handle (esvo_shard_set_routing with ESVO_ROUTE_Y_RECT filters
 * packets on the host), and esvo_shard_set_routing to such a routing is refused on a handle with a filter on; broadcast band mode
 * and tick-interleaved handles are fine (every rank sees the whole stream and reaches the same verdicts).  ESVO_ERR_INVALID_ARG: a
 * non-zero reserved word.  Ingest group: not while another thread pushes to the same camera. */
int esvo_ts_filter_configure(esvo_handle h, int cam, const esvo_event_filter_t* f);
/* totals of the camera's successful push calls since esvo_create / esvo_reset (all zero while no filter has run) */
int esvo_ts_filter_stats(esvo_handle h, int cam, esvo_event_filter_counts_t* totals);
/* get_last (nullable, [H * W]) receives the camera's `last` image, then set_last (nullable, [H * W]) replaces it: a stream can be
 * resumed, a test can plant a state.  ESVO_ERR_STATE while no filter is configured. */
int esvo_ts_filter_state(esvo_handle h, int cam, uint64_t* get_last, const uint64_t* set_last);
/* The rule alone: host only, no handle, no GPU.  last: [height * width], in / out (it advances only on ESVO_OK).  verdict (nullable,
 * [n]) receives ESVO_FILTER_*; the kept events go to out[0 .. *n_out) in order (out == NULL counts; more kept than cap:
 * ESVO_ERR_CAPACITY); *add (nullable) is INCREMENTED by this call's counts.  The events are taken as sorted; f->reserved must be 0. */
int esvo_event_filter_host(const esvo_event_filter_t* f, int width, int height, uint64_t* last, const esvo_event_t* ev, size_t n,
                           uint8_t* verdict, esvo_event_t* out, size_t cap, size_t* n_out, esvo_event_filter_counts_t* add);
/* sizeof(esvo_event_filter_t), sizeof(esvo_event_filter_counts_t), 0, 0 */
void esvo_event_filter_sizes(size_t out[4]);
/* Burst stage of the event filter: trail and STC (spatio-temporal-contrast) filtering with polarity, on the device.  A Gen4 / IMX636
 * pixel answers one contrast edge with a burst of same-polarity events; the trailing ones keep the pixel bright in the Time Surface
 * after the edge has moved on and spend the mapper's event budget on one pixel.  The refractory test cannot remove them: it ignores
 * polarity and so swallows the opposite-polarity event of an object's other edge as well.  The stage is a SECOND STAGE of a camera's
 * filter, after the mask test and before the refractory test, with its own configuration, state and totals.  Off unless configured;
 * a handle that never configures it takes the paths above unchanged.  State per camera and RAW pixel:
 *   bstamp[y][x]  uint64: the ns stamp of the newest event the stage judged at that pixel (0: none)
 *   bflags[y][x]  uint8:  bit 0 that event's polarity, normalised to 0 / 1 as the ring holds it; bit 1 `linked`: that event continued a
 *                         burst; the other bits 0
 * The filter's rule with the stage in it (p: the event's polarity 0 / 1; the lines marked + are the stage):
 *   verdict(e):
 *     if e.x >= W or e.y >= H:            ESVO_FILTER_OUTSIDE      (1)  touches nothing
 *     if mask[e.y][e.x] != 0:             ESVO_FILTER_MASKED       (2)  touches nothing (no burst state either)
 *   + if mode != ESVO_BURST_OFF:
 *   +   T = bstamp[px]; P = bflags[px] & 1; K = bflags[px] >> 1 & 1
 *   +   linked = T != 0 and p == P and t - T <= burst_ns      -- integer difference: a planted T ahead of the stream gives a negative one
 *   +   pass   = ESVO_BURST_TRAIL:          not linked         -- the first event of every burst
 *   +            ESVO_BURST_STC_CUT_TRAIL:  linked and not K   -- the second event of every burst, and only that one
 *   +            ESVO_BURST_STC_KEEP_TRAIL: linked             -- every event of a burst but its first
 *   +   bstamp[px] = t; bflags[px] = p | linked << 1           -- ALWAYS, whatever the verdict
 *   +   if not pass:                      ESVO_FILTER_BURST        (5)  touches nothing else
 *     L = last[px] ... refractory test, support test, last[px] = t: as above
 *   So a burst-dropped event neither updates `last`, nor supports a neighbour, nor restarts the refractory period; equal stamps at one
 *   pixel link (difference 0); a polarity change always ends a burst; an isolated event passes TRAIL and is dropped by both STC modes;
 *   stamp 0 means "none", as for `last`.  PINNED TO NOTHING THIRD-PARTY, as the filter's rule: the three modes follow the published
 *   description of Metavision's trail / STC algorithms as recalled; `<=`, the state updating on every judged event and the stage's
 *   place between mask and refractory test are this library's choices.
 * The camera's filter must be configured (ESVO_ERR_STATE otherwise; a filter with both periods 0 and no mask passes everything: the
 * way to run the stage alone).  esvo_ts_filter_configure(h, cam, NULL) while the stage is on: ESVO_ERR_STATE; a non-NULL
 * reconfiguration keeps the stage, its state and its totals.  Row-routed band handles cannot have a filter, so they cannot have the
 * stage.  Transactional as the filter is: bstamp, bflags and the totals advance only behind a push that returned ESVO_OK; ring room is
 * still judged on the unfiltered count.  Burst-dropped events appear in NONE of esvo_event_filter_counts_t's fields (its events_in
 * stays the sum of its other five): packet size = the filter's events_in delta + the stage's `dropped` delta.  *n_events, the EVT decoder
 * totals, the survey (it counts the raw packet) and stats.events_staged (the kept events) keep their meaning.  A packet of which the
 * stage drops everything returns ESVO_OK, stages nothing and advances the state.
 * On the device the stage is one kernel between the filter's binning and its walk: one wave per 8x8 tile takes the tile's own-pixel
 * entries (the rule needs no halo), sorts them by (pixel, packet index) in LDS and judges them all at once -- an event's verdict
 * depends on the previous two raw events of its own pixel and on nothing else, which after the sort are its two left neighbours or
 * the planted state.  The walk then skips every entry the stage dropped, own pixels and halo alike.  A tile whose list overflows
 * reads the packet, collects its own events in LDS and judges them in batches by the same code, the state carried in LDS. */
enum { ESVO_BURST_OFF = 0, ESVO_BURST_TRAIL = 1, ESVO_BURST_STC_CUT_TRAIL = 2, ESVO_BURST_STC_KEEP_TRAIL = 3 };
enum { ESVO_FILTER_BURST = 5 };
typedef struct esvo_event_burst_t {
  uint64_t burst_ns;      /* > 0 with a mode other than ESVO_BURST_OFF */
  uint32_t mode;          /* ESVO_BURST_* */
  uint32_t reserved[3];   /* 0 */
} esvo_event_burst_t;
typedef struct esvo_event_burst_counts_t { uint64_t judged, passed, dropped; } esvo_event_burst_counts_t;  /* judged = passed + dropped */
/* b == NULL or mode ESVO_BURST_OFF switches the stage off and frees its memory; a mode zeroes bstamp / bflags and keeps the totals.
 * ESVO_ERR_STATE: the camera has no filter.  ESVO_ERR_INVALID_ARG: an unknown mode, burst_ns == 0 with a mode other than OFF, a
 * non-zero reserved word.  Ingest group: not while another thread pushes to the same camera. */
int esvo_ts_burst_configure(esvo_handle h, int cam, const esvo_event_burst_t* b);
/* totals of the camera's successful push calls since esvo_create / esvo_reset (esvo_reset zeroes state and totals and keeps the configuration) */
int esvo_ts_burst_stats(esvo_handle h, int cam, esvo_event_burst_counts_t* totals);
/* get_stamp / get_flags (nullable, [H * W]) receive the state, then set_stamp / set_flags ([H * W], both or neither) replace it.
 * ESVO_ERR_STATE while the stage is off; ESVO_ERR_INVALID_ARG: only one of the two set arrays, or a flag byte above 3. */
int esvo_ts_burst_state(esvo_handle h, int cam, uint64_t* get_stamp, uint8_t* get_flags, const uint64_t* set_stamp, const uint8_t* set_flags);
/* The whole two-stage rule on the host: esvo_event_filter_host with the stage in it.  bstamp, bflags: [height * width], in / out
 * like `last` (all three advance only on ESVO_OK; required unless the stage is off); verdict receives ESVO_FILTER_* including
 * ESVO_FILTER_BURST; *add_burst and *add_filter (nullable) are INCREMENTED.  With b == NULL or mode ESVO_BURST_OFF it is
 * esvo_event_filter_host, bit for bit. */
int esvo_event_burst_filter_host(const esvo_event_burst_t* b, const esvo_event_filter_t* f, int width, int height,
                                 uint64_t* bstamp, uint8_t* bflags, uint64_t* last, const esvo_event_t* ev, size_t n,
                                 uint8_t* verdict, esvo_event_t* out, size_t cap, size_t* n_out,
                                 esvo_event_burst_counts_t* add_burst, esvo_event_filter_counts_t* add_filter);
/* sizeof(esvo_event_burst_t), sizeof(esvo_event_burst_counts_t), 0, 0 */
void esvo_event_burst_sizes(size_t out[4]);
/* Event survey on the device: per-pixel event counts kept while a stream is pushed, and a hot-pixel mask learnt from them -- the
 * filter's mask without a host loop over events the host may never see (device columns, device-resident words).  Off unless begun;
 * a handle that never opens a survey takes the paths above unchanged.  Each camera has its own survey: counts[2][H][W] uint32, plane
 * 0 = polarity 0 (off), plane 1 = polarity 1 (on), and the stats below.
 * WHAT IS COUNTED: while a survey is open every packet that a push call of the camera ACCEPTS (esvo_ts_push_events, _async,
 * _event_array, _bag, _event_columns, _evt3, _evt2): each decoded event with x < W and y < H adds 1 to counts[polarity][y][x], polarity
 * normalised to 0 / 1 as the ring holds it; every other event adds 1 to stats.outside.  The RAW packet is counted, before the mask,
 * refractory and support tests: a masked pixel keeps being counted, so a refreshed mask does not forget it.  The camera's filter must
 * be configured (ESVO_ERR_STATE otherwise): with it every source reaches one place as a device-resident column packet, and the
 * survey reads that packet and nothing else.  A filter with both periods 0 and no mask passes every in-sensor event: the way to
 * survey a stream that is to stay unfiltered.  (Row-routed band handles cannot have a filter, so they cannot have a survey.)
 * flags == 0: ring, stamp mirror, esvo_get_stats, the filter's `last` and totals, rendered Time Surfaces and every return value are
 * those of the same pushes without a survey.  The survey is transactional as the filter is: counts and stats advance only behind a
 * push that returned ESVO_OK; bad arguments, a bad stamp, ESVO_ERR_CAPACITY and the filter's ESVO_ERR_UNSUPPORTED leave them as they
 * were.  An open survey adds no read-back to a push and no wait, except to a packet of which the filter keeps nothing (that push
 * waits for nothing else, and the packet may lie in the caller's memory); counts and stats come down only in the calls below.
 * ESVO_SURVEY_COUNT_ONLY (a dark recording): the packet is decoded and counted and NOTHING ELSE happens -- nothing is staged, no ring
 * room is needed, the filter's `last` and totals stay, no order is demanded (counting is order-free).  A packet with an invalid
 * stamp is still refused with ESVO_ERR_INVALID_ARG and nothing of it is counted; the EVT decoder states and totals advance as by a
 * normal push and *n_events reports the decoded count.
 * No counter may wrap: a push that would take events_in + outside beyond 2^32 - 1 is refused with ESVO_ERR_CAPACITY before anything
 * runs, judged on the host from the packet's unfiltered size.  esvo_reset zeroes counts and stats and keeps the survey open;
 * esvo_destroy frees everything; esvo_ts_filter_configure(h, cam, NULL) while a survey is open: ESVO_ERR_STATE (end it first), a
 * non-NULL reconfiguration keeps the survey and its counts.  Ingest group: not while another thread pushes to the same camera.
 * The counting kernel combines on chip first: a workgroup sorts the keys pixel << 1 | polarity of 1024 consecutive events in LDS and
 * issues one atomic add per run of equal keys, so a stuck pixel costs global memory one update per chunk, not one per event. */
enum { ESVO_SURVEY_COUNT_ONLY = 1 };
typedef struct esvo_event_survey_t { uint32_t flags; uint32_t reserved[3]; /* 0 */ } esvo_event_survey_t;
typedef struct esvo_event_survey_stats_t {
  uint64_t events_in;        /* events of accepted packets with x < W and y < H: the sum of all counters */
  uint64_t outside;          /* events of accepted packets with x >= W or y >= H (counted nowhere else) */
  uint64_t packets;          /* accepted packets */
  uint64_t t_first, t_last;  /* smallest / largest ns stamp among the counted events; 0, 0 while events_in == 0 */
} esvo_event_survey_stats_t;
/* counts and stats start at zero.  ESVO_ERR_STATE: no filter configured, or a survey is open already; ESVO_ERR_INVALID_ARG: an unknown
 * flag or a non-zero reserved word. */
int esvo_ts_survey_begin(esvo_handle h, int cam, const esvo_event_survey_t* s);
/* frees the survey's memory (ESVO_ERR_STATE: none is open; so for the three calls below) */
int esvo_ts_survey_end(esvo_handle h, int cam);
int esvo_ts_survey_stats(esvo_handle h, int cam, esvo_event_survey_stats_t* out);
/* counts: [2][H][W] uint32.  get (nullable) receives them, then set (nullable) replaces them; stats_set (nullable, only with set)
 * replaces the stats: a survey can be resumed, a test can plant one.  The two planes of a pixel must not add up beyond 2^32 - 1, nor
 * stats_set's events_in + outside (ESVO_ERR_INVALID_ARG). */
int esvo_ts_survey_state(esvo_handle h, int cam, uint32_t* get, const uint32_t* set, const esvo_event_survey_stats_t* stats_set);
/* The hot-pixel rule, all of it in integers on the survey's counts:
 *   c[px] = counts[0][px] + counts[1][px]
 *   k     = floor(rank_permille * (W * H - 1) / 1000)
 *   B     = the k-th smallest (0-based) of the W * H values c, zeros included
 *   R     = min(2^32 - 1, floor(max_rate_hz * (t_last - t_first) / 10^9)), computed once on the host in 128-bit arithmetic; with
 *           t_last == t_first the rate test contributes nothing
 *   hot(px) = c >= min_count and ((factor > 0 and c > factor * B) or (rate test on and c > R))      -- both strict, factor * B in 64 bits
 * PINNED TO NOTHING THIRD-PARTY: the whole rule is this library's own, as the filter's is; nothing in the reference corresponds to it.
 * ESVO_ERR_INVALID_ARG: both tests off (factor == 0 and max_rate_hz == 0), min_count == 0, rank_permille > 1000, a non-zero
 * reserved word, an unknown `install`.  The report: baseline = B; rate_count = R (0 with the rate test off or contributing nothing);
 * n_hot; events_hot = the sum of c over the hot pixels; max_count and max_pixel = the largest c and the smallest y * W + x holding it.
 * Everything runs on the device from the resident counts: B from an exact radix select (four histogram passes over the 32-bit values,
 * LDS histograms merged per workgroup), no sort and no download of the count image; only mask_out and the report come down (and,
 * first, the 32 bytes of device stats that R is computed from).
 * install: ESVO_MASK_KEEP leaves the filter alone; ESVO_MASK_REPLACE makes the mask the camera's filter mask, ESVO_MASK_UNION ORs it
 * into the one in force -- device to device, from the next push on, the filter's `last` image, periods and totals untouched (which
 * esvo_ts_filter_configure cannot do: it zeroes `last`).  The survey stays open and keeps its counts.  The calibration flow: begin
 * count-only, push the dark recording, take the mask with install, end, push the real stream. */
typedef struct esvo_hot_pixel_rule_t {
  uint32_t min_count;      /* >= 1: a pixel with fewer events is never hot (so a pixel with none never is) */
  uint32_t factor;         /* baseline test: c > factor * B.  0: test off */
  uint32_t rank_permille;  /* 0..1000: which order statistic of the counts is the baseline B; 500 = the median */
  uint32_t max_rate_hz;    /* rate test: c > R.  0: test off */
  uint32_t reserved[4];    /* 0 */
} esvo_hot_pixel_rule_t;
typedef struct esvo_hot_pixel_report_t {
  uint32_t baseline, rate_count, n_hot, max_count, max_pixel, pad_;
  uint64_t events_hot;
} esvo_hot_pixel_report_t;
enum { ESVO_MASK_KEEP = 0, ESVO_MASK_REPLACE = 1, ESVO_MASK_UNION = 2 };
/* mask_out: nullable, [H * W], 0 / 1; report: nullable */
int esvo_ts_survey_mask(esvo_handle h, int cam, const esvo_hot_pixel_rule_t* rule, uint8_t* mask_out, int install, esvo_hot_pixel_report_t* report);
/* The same rules on the host: no handle, no GPU.  counts: [2][height][width], in / out; *stats in / out (a call with n > 0 is one
 * packet).  ESVO_ERR_CAPACITY, and nothing changes, where the call would take events_in + outside beyond 2^32 - 1. */
int esvo_event_survey_host(int width, int height, uint32_t* counts, esvo_event_survey_stats_t* stats, const esvo_event_t* ev, size_t n);
/* mask (nullable, [height * width]) and report (nullable) of `rule` on counts and stats (its t_first / t_last) */
int esvo_hot_pixel_mask_host(const esvo_hot_pixel_rule_t* rule, int width, int height, const uint32_t* counts, const esvo_event_survey_stats_t* stats,
                             uint8_t* mask, esvo_hot_pixel_report_t* report);
/* sizeof(esvo_event_survey_t), sizeof(esvo_event_survey_stats_t), sizeof(esvo_hot_pixel_rule_t), sizeof(esvo_hot_pixel_report_t) */
void esvo_event_survey_sizes(size_t out[4]);
/* Still out of scope: polarity-aware support, event-rate control, reading decoded events back to the caller. */
/* rosbag (format 2.0) ingest, SURVEY.md §8(f).2: the reading side of events_repacking_helper
 * (events_repacking_helper/src/EventMessageEditor.cpp:66-119: rosbag::Bag::open, rosbag::View over an event topic,
 * MessageInstance::instantiate<dvs_msgs::EventArray>).  Chunks (compression none / bz2 / lz4) are walked in file order;
 * each serialised dvs_msgs/EventArray of the topic is returned as a byte range of the reader's buffer (valid until the next
 * call) -- the input of esvo_ts_push_event_array.  Returns ESVO_OK, 1 at the end of the bag, or a negative status
 * (esvo_bag_last_error).  topic == NULL: every topic of type dvs_msgs/EventArray.  Host code, no GPU needed. */
typedef struct esvo_bag* esvo_bag_handle;
int esvo_bag_open(const char* path, esvo_bag_handle* out);
int esvo_bag_close(esvo_bag_handle b);
const char* esvo_bag_last_error(esvo_bag_handle b);
int esvo_bag_next_event_array(esvo_bag_handle b, const char* topic, const uint8_t** msg, size_t* n_bytes, uint64_t* stamp_ns,
                              const char** topic_out);
/* Stage the messages of `topic` with a bag time stamp below until_ns (0: all that are left) for camera `cam`.  *n_events
 * (nullable) receives the events staged by this call, also when it fails.  A message the handle refuses (typically
 * ESVO_ERR_CAPACITY "event ring full: render before staging more") is NOT consumed: render and call again. */
int esvo_ts_push_bag(esvo_handle h, int cam, esvo_bag_handle b, const char* topic, uint64_t until_ns, size_t* n_events);
/* Replaces TimeSurface::createTimeSurfaceAtTime (TimeSurface.cpp:52-152), BACKWARD mode.
 * Uses every staged event with ts < t_ns.  out_mono8 (W*H) may be NULL: the rectified TS
 * also stays device-resident as the camera's latest frame.
 * Deviation from the reference, by construction: the device keeps ONE time stamp per pixel (the newest event with
 * ts < t_ns at render time) where the reference keeps a queue of the last 20 events per pixel and scans it backwards
 * (EventQueueMat, TimeSurface.h:28-96).  The two agree whenever renders are requested in non-decreasing time order --
 * what the sync topic of the ROS graph delivers.  (a) A render at a t_ns EARLIER than events of a previous render is
 * refused with ESVO_ERR_STATE (the queue would still find the older event, the single stamp cannot); esvo_reset and
 * re-stage to replay.  (b) The reference's corner case "more than 20 events newer than t_ns are already queued at a
 * pixel, so it reads as empty" (TimeSurface.h:52-75) cannot occur here: events with ts >= t_ns are never scattered
 * before the render at t_ns. */
int esvo_ts_render(esvo_handle h, int cam, uint64_t t_ns, uint8_t* out_mono8);
/* The same in FORWARD mode (time_surface_mode: 1, TimeSurface.cpp:85-116): every raw pixel's decayed value is splatted
 * bilinearly at the pixel's rectified position (the camera's rect_lut, which must have been given to esvo_create) with a
 * clamp to 1 after every add, in raster order of the source pixels -- reproduced by a gather over per-pixel contribution
 * lists sorted by source index (built on first use).  x255, round to u8, 3x3 median; the image is rectified by
 * construction (no remap).  Same staging / monotonic-time rules as esvo_ts_render; the result is the camera's resident
 * frame as well.  No shipped configuration selects this mode. */
int esvo_ts_render_forward(esvo_handle h, int cam, uint64_t t_ns, uint8_t* out_mono8);

/* ---- Mapper: stage-wise seams ------------------------------------------------------ */

/* Replaces the TS_obs_ selection of dataTransferring (esvo_Mapping.cpp:501-534) +
 * DepthFrame setup (esvo_Mapping.cpp:268-272).  ts_left/ts_right: host mono8 W*H, or NULL
 * to use the device-resident frames rendered last by esvo_ts_render. */
int esvo_map_set_observation(esvo_handle h, uint64_t t_ns, const uint8_t* ts_left,
                             const uint8_t* ts_right, const double T_world_cam[16]);
/* Replaces EventBM::createMatchProblem + match_all_HyperThread (EventBM.cpp:56-78,269-315).
 * pose_t_ns/pose_T: the st_map_ of esvo_Mapping.cpp:585-599 (m stamps, m row-major 4x4). */
int esvo_map_match(esvo_handle h, const esvo_event_t* ev, size_t n, const uint64_t* pose_t_ns,
                   const double* pose_T, size_t m, esvo_match_t* out, size_t cap, size_t* n_out);
/* Replaces DepthProblemSolver::solve (+ pointCulling when cull != 0)
 * (DepthProblemSolver.cpp:28-136,216-244).  Uses the pose table of the last esvo_map_match
 * or esvo_map_set_poses call. */
int esvo_map_set_poses(esvo_handle h, const uint64_t* pose_t_ns, const double* pose_T, size_t m);
int esvo_map_refine(esvo_handle h, const esvo_match_t* matches, size_t n, int cull,
                    esvo_depth_point_t* out, size_t cap, size_t* n_out);
/* Replaces dqvDepthPoints_.push_back(vdp) + window policy (esvo_Mapping.cpp:341-368). */
int esvo_map_push_frame(esvo_handle h, const esvo_depth_point_t* pts, size_t n,
                        const double* pose_T, size_t m);
/* Replaces the fusion loop + clean + regularisation (esvo_Mapping.cpp:370-395;
 * DepthFusion.cpp:71-192; SmartGrid.h:222-243; DepthRegularization.cpp:19-110). */
int esvo_map_fuse(esvo_handle h, size_t* n_fusions);

/* ---- Mapper: SGM bootstrap ---------------------------------------------- */

/* Replaces esvo_Mapping::InitializationAtTime (esvo_Mapping.cpp:433-492) and the SGM branch of dataTransferring (:537-552):
 * cv::StereoSGBM (0, 48, 11, P1 = 8*11*11, P2 = 32*11*11, -1, 0, 11; MODE_SGBM; :102-108) on the UN-smoothed Time-Surface
 * pair -- ts_left / ts_right: host mono8 W*H, or NULL for the device-resident frames of esvo_ts_render -- masked by the
 * rectified pixels of the newest <= PROCESS_EVENT_NUM + 1 staged left events of the last 2 * BM_half_slice_thickness
 * (createEdgeMask, :1000-1044), one Gaussian DepthPoint (variance 1e-6, age = age_vis_threshold) per masked event whose
 * disparity lies inside the inverse-depth range.  With at least min_points (INIT_SGM_DP_NUM_THRESHOLD, 500) of them the
 * points open the fusion window and DepthFusion::naive_propagation (DepthFusion.cpp:234-288) fills the DepthFrame of the
 * observation set last (esvo_map_set_observation gives its stamp and pose); otherwise *n_points is 0 and nothing
 * changes.  disp_out (nullable): the W*H int16 disparity image (x16, -16 = none).  StereoSGBM is third-party code that
 * is restated here from its published algorithm ("parity unpinned"). */
int esvo_map_init_sgm(esvo_handle h, const uint8_t* ts_left, const uint8_t* ts_right, size_t min_points, size_t* n_points,
                      int16_t* disp_out);

/* ---- Mapper: fused tick (everything stays in HBM) ---------------------------------- */

/* Replaces dataTransferring's event selection (esvo_Mapping.cpp:555-575) + MappingAtTime
 * (esvo_Mapping.cpp:261-431) on the staged left events and the current observation. */
int esvo_map_tick(esvo_handle h, uint64_t t_ns, const uint64_t* pose_t_ns, const double* pose_T,
                  size_t m);
/* Replaces esvo_MVStereo::MappingAtTime in MVStereoMode 1, PURE_BLOCK_MATCHING (esvo_MVStereo.cpp:383-432): the same event
 * selection (+ Denoising) and block matching, then vEMP2vDP (:1072-1094: one Gaussian DepthPoint per match, variance at the
 * 1e-6 bound, residual = ZNCC cost, age = age_vis_threshold), a window of max_fusion_frames frames and
 * DepthFusion::naive_propagation (DepthFusion.cpp:234-288) of every frame, newest first, into a new DepthFrame.  The map is
 * read with the usual output calls; nothing is culled, cleaned or regularised.  Synchronous. */
int esvo_map_tick_bm_only(esvo_handle h, uint64_t t_ns, const uint64_t* pose_t_ns, const double* pose_T, size_t m);
/* The stage-wise seam of that mode: what follows match_all_HyperThread (esvo_MVStereo.cpp:411-423) on the matches of
 * esvo_map_match -- vEMP2vDP, dqvDepthPoints_.push_back(vdp_em) + pop to maxNumFusionFrames_, naive_propagation of the window.
 * pose_T: the m virtual views the matches' pose_idx refer to (the st_map_ handed to esvo_map_match). */
int esvo_map_fuse_matches_naive(esvo_handle h, const esvo_match_t* matches, size_t n, const double* pose_T, size_t m);
/* One call for a node that hosts the Time Surfaces and the mapper on the same handle: esvo_ts_render of both cameras at
 * t_ns (device-resident, no download), esvo_map_set_observation on them with the pose T_world_cam, esvo_map_tick.  Same
 * results as the four calls; a reference-faithful tick is short enough for their host overhead to show. */
int esvo_map_tick_resident(esvo_handle h, uint64_t t_ns, const double T_world_cam[16], const uint64_t* pose_t_ns,
                           const double* pose_T, size_t m);

/* Device-resident variants of the stage-wise calls (no host copies of points): the front stage of a tick on the
 * events staged by esvo_ts_push_events (selection + match + refine + cull; the frame stays on the device,
 * esvo_map_front_frame), a frame pushed from device memory, and the fusion stage enqueued without waiting for it.
 * esvo_map_tick == front + push_frame_device(front_frame) + fuse_async, minus the point-count read-back stall.
 * They exist for tick-interleaved multi-GPU operation (esvo_amd/dist.py: TickShardedEsvo): a tick depends on the
 * previous ticks only through the frames in its window (the DepthFrame is rebuilt every tick,
 * esvo_Mapping.cpp:266-272), so rank r maps the ticks k = r (mod N) and the ranks all-gather their frames. */
int esvo_map_front(esvo_handle h, uint64_t t_ns, const uint64_t* pose_t_ns, const double* pose_T, size_t m,
                   size_t* n_points);
int esvo_map_front_frame(esvo_handle h, const esvo_depth_point_t** d_frame);
int esvo_map_push_frame_device(esvo_handle h, const esvo_depth_point_t* d_pts, size_t n, const double* pose_T,
                               size_t m);
int esvo_map_fuse_async(esvo_handle h);

/* ---- Mapper: event-to-event matching, esvo_MVStereo modes 0 and 2 ------------------------------------------------
 *
 * EventMatcher (EventMatcher.cpp), the generalised-time-surface stereo method of [26] (Ieng et al. 2018) that esvo_MVStereo runs
 * in MVStereoMode 0 (PURE_EVENT_MATCHING) and 2 (EM_PLUS_ESTIMATION).  For every left event: the right events within
 * +-EM_Time_THRESHOLD / 2 (two std::lower_bound over the right selection, ros::Time roundings included) with the same polarity,
 * rectified rows within EM_EPIPOLAR_THRESHOLD and x_right < x_left; per survivor depth = b f / (x_left - x_right), warping2 into the
 * observation pair with T_left_rv = T_obs^-1 T_slice, patchInterpolation2 of a patch_size_X x patch_size_Y patch on each UN-smoothed
 * Time Surface and zncc_cost; the first candidate with the smallest cost below 1.0 wins; costs above EM_TS_NCC_THRESHOLD are
 * rejected.  Output order: match_all_HyperThread's NUM_THREAD_MAPPING threads (esvo_params_t.num_threads), event i to thread
 * i % N, per-thread lists concatenated.  Results are restated in tests/em_restated.py and pinned to it bit for bit; they are not
 * pinned to the compiled reference.
 * esvo_match_t of a match: x_left, inv_depth = 1.0 / best_depth (the reference's two roundings), cost = the ZNCC cost, disp =
 * x_left - x_right of the chosen candidate, event_idx = position in the left array handed in, pose_idx = slice index.
 * Edge case kept from the reference: with ncc_threshold >= 1 and no candidate below cost 1, candidate 0 is emitted with cost 1.0 and
 * inv_depth = +inf.
 * Events off the sensor (x >= width or y >= height) have no rectified coordinate: as in block matching they are skipped -- a left
 * one keeps its position (event_idx) but gets no candidate, a right one is never a candidate and is not counted in the stats.
 * More than 2^32 - 1 (event, candidate) pairs past the epipolar test in one call: ESVO_ERR_CAPACITY.
 * The Time Surfaces are the observation's (esvo_map_set_observation); with SmoothTimeSurface set the handle holds only the smoothed
 * pair, so these calls return ESVO_ERR_UNSUPPORTED (the reference's EventMatcher reads TS_left_ / TS_right_ un-smoothed). */
typedef struct esvo_em_params_t {
  double slice_thickness;             /* EM_Slice_Thickness [s] (code default 1e-3) */
  double time_threshold;              /* EM_Time_THRESHOLD [s] (5e-5; shipped yaml 5e-4) */
  double epipolar_threshold;          /* EM_EPIPOLAR_THRESHOLD [px] (0.5; shipped yaml 1.0) */
  double ncc_threshold;               /* EM_TS_NCC_THRESHOLD (0.1) */
  int32_t num_event_matching;         /* EM_NUM_EVENT_MATCHING (3000): at most this + 1 events per camera and tick */
  int32_t patch_intensity_threshold;  /* EM_PATCH_INTENSITY_THRESHOLD: stored by the reference, never read; ignored */
  double patch_valid_ratio;           /* EM_PATCH_VALID_RATIO: stored by the reference, never read; ignored */
} esvo_em_params_t;

/* The selection and the slice table of the last esvo_map_tick_em (esvo_map_em_get_selection). */
typedef struct esvo_em_selection_t {
  uint64_t t_low_ns, t_up_ns;         /* the bounds handed in */
  uint64_t left_first, right_first;   /* absolute index of the first selected event in the camera's staged stream */
  uint32_t left_count, right_count;   /* selected events per camera (0: no tick) */
  uint32_t n_slices;
  uint32_t pad_;
} esvo_em_selection_t;

/* Counts of the last esvo_map_match_em / esvo_map_tick_em at each filter stage (pairs = (left event, right candidate)). */
typedef struct esvo_em_stats_t {
  uint64_t events;          /* left events matched (those of the slices) */
  uint64_t right_events;    /* length of the candidate queue */
  uint64_t time_polarity;   /* pairs inside the time window with equal polarity */
  uint64_t epipolar;        /* ... that pass the epipolar test: the pairs whose warp + ZNCC is evaluated */
  uint64_t patch_ok;        /* ... whose two projections and patches lie inside the images */
  uint64_t matches;         /* events with a match */
  uint64_t slices;
  float ms_match;           /* HIP-event time from the first matching kernel to the last (candidates, scans, pair costs, argmin,
                               compaction); it includes the host read-back of the pair count between the two candidate passes */
  float pad_;
} esvo_em_stats_t;

/* Replaces EventMatcher::createMatchProblem + match_all_HyperThread (EventMatcher.cpp:49-58,184-246) -- the host-array seam a ROS
 * node calls after its own dataTransferring (esvo_MVStereo.cpp:579-609) and eventSlicingForEM (:1096-1125).
 * left_ev[n_left]: vEventsPtr_left_; slice s covers slice_count[s] events from slice_begin[s] with the pose slice_T[16 s] (row-major
 * T_world, the slice's transf_).  As match_all_HyperThread does, the events matched are the sum of the slice counts taken
 * contiguously from slice_begin[0] (slices of eventSlicingForEM are contiguous).  right_ev[n_right]: vEventsPtr_right_, time-sorted.
 * The observation (pose and Time Surfaces) is the one set by esvo_map_set_observation; em->time_threshold,
 * epipolar_threshold, ncc_threshold are read, patch size and num_threads come from esvo_params_t. */
int esvo_map_match_em(esvo_handle h, const esvo_em_params_t* em, const esvo_event_t* left_ev, size_t n_left,
                      const uint32_t* slice_begin, const uint32_t* slice_count, const double* slice_T, size_t n_slices,
                      const esvo_event_t* right_ev, size_t n_right, esvo_match_t* out, size_t cap, size_t* n_out);
/* The pose of a slice: return 1 and fill T_world_cam (row-major) when a pose is known at t_ns, 0 otherwise (identity is used:
 * the reference's getPoseAt failure leaves EventSlice::transf_ at its default). */
typedef int (*esvo_em_pose_fn)(void* user, uint64_t t_ns, double T_world_cam[16]);
/* Replaces esvo_MVStereo::MappingAtTime in MVStereoMode 0 / 2 on the events staged by esvo_ts_push_events and the current
 * observation.  Synchronous.
 *   selection (dataTransferring, esvo_MVStereo.cpp:579-609): t_low_ns / t_up_ns are the oldest / newest stamps of the TS
 *     history.  Per camera lo = lower_bound(t_low), up = lower_bound(t_up) - 1; events from lo while it != up and fewer than
 *     num_event_matching + 1 are taken, oldest first (the last event before t_up is never taken).  A camera with no such event
 *     (up <= lo) means no tick: ESVO_OK, nothing changes.
 *   slicing (eventSlicingForEM, :1096-1125): floor((t_up - t_low) / slice_thickness) slices at most; a slice runs from its first
 *     event to lower_bound(ts + thickness) INCLUSIVE (the last event if that is end()); its pose is pose_fn at the stamp of its
 *     element count / 2; the next slice starts behind it.  More slices than max_poses_per_tick: ESVO_ERR_CAPACITY, no state change.
 *   matching on the device (esvo_map_match_em).  No match: ESVO_OK and nothing changes (the reference returns, :268-271).
 *   mode 0 (:273-305): esvo_map_fuse_matches_naive of the matches with the slice poses.
 *   mode 2 (:445-503): esvo_map_set_poses (slice medians, slice poses), esvo_map_refine with culling, esvo_map_push_frame,
 *     esvo_map_fuse -- the calls and policies of the BM mapper behind block matching.
 * The left selection must fit max_events_per_tick (ESVO_ERR_CAPACITY otherwise).  Not on sharded handles.
 * Ingest may run concurrently (the threading contract above): the selected ranges of both cameras are protected against eviction by
 * a concurrent push until they have been copied; events inside [t_low, t_up) staged while the call selects them make it fail with
 * ESVO_ERR_STATE (stage the events up to t_up first). */
int esvo_map_tick_em(esvo_handle h, const esvo_em_params_t* em, int mode, uint64_t t_low_ns, uint64_t t_up_ns,
                     esvo_em_pose_fn pose_fn, void* user);
/* The last tick's selection and slice table: slice s = slice_count[s] events from slice_begin[s] of the left selection, pose
 * stamp slice_t_ns[s], pose slice_T[16 s].  Each array may be NULL; non-NULL arrays need cap >= sel->n_slices. */
int esvo_map_em_get_selection(esvo_handle h, esvo_em_selection_t* sel, uint32_t* slice_begin, uint32_t* slice_count,
                              uint64_t* slice_t_ns, double* slice_T, size_t cap);
int esvo_map_em_stats(esvo_handle h, esvo_em_stats_t* out);
/* sizeof() of {esvo_em_params_t, esvo_em_selection_t, esvo_em_stats_t}, 0. */
void esvo_em_sizes(size_t out[4]);

/* ---- Mapper: the scale loop of the LM refinement -------------------------------------------------------------------
 *
 * With esvo_params_t::lm_scale_pass_limit != 0 the refinement kernels count the passes of the Student-t scale loop and, with a
 * limit below ESVO_LM_SCALE_COUNT_ONLY, abandon matches whose loop crawls.
 *   pass        one completed update s2 = sum / N with a non-zero sum.  An evaluation that takes the failure fill, or whose
 *               collapse is taken for granted (at most floor(0.94 N / (nu + 1)) non-zero residuals, none below 1e-6), has 0.
 *   over        an evaluation that has completed `limit` passes and whose loop test (|s2 - s1| / s1 > 5 %) asks for another.
 *   abandoned   the first evaluation the solver asks for that is over the limit abandons its match: no point, slot flag 0, not
 *               counted in last_solved / last_points.  Every other match gives the bits it gives with the limit 0.
 * Counted: every launch of the refinement on a plain handle (esvo_map_refine, esvo_map_tick, _tick_resident, esvo_map_front,
 * esvo_map_tick_em mode 2).  The evaluations are those the device computes: F(x0), F(x + h) and F(x + p); NumericalDiff's second
 * F(x) is the residual vector already held.  With the limit 0, and under LSnorm l2 (no scale loop), every field reads 0.
 * A band-sharded or tick-interleaved handle refuses a non-zero limit (esvo_shard_set_band, esvo_comm_init*, esvo_set_params:
 * ESVO_ERR_STATE).  The pair layout of small launches is not used while the guard is on (its second wave evaluates points the
 * solver may never ask for). */
typedef struct esvo_lm_stats_t {
  uint32_t enabled;                /* 1: the last refinement launch ran with a non-zero limit under the Student-t model */
  uint32_t last_max_passes_eval;   /* of the last completed launch: most passes of one evaluation */
  uint32_t last_max_passes_match;  /*   ... most passes of one match, summed over its evaluations */
  uint32_t last_abandoned;         /*   ... matches abandoned */
  uint64_t last_passes;            /*   ... passes, evaluations, evaluations that took the collapse for granted */
  uint64_t last_evals;
  uint64_t last_shortcut_evals;
  uint64_t total_passes;           /* since esvo_create / esvo_reset */
  uint64_t total_evals;
  uint64_t total_shortcut_evals;
  uint64_t total_abandoned;
} esvo_lm_stats_t;
/* Waits for outstanding refinement launches as esvo_get_stats does. */
int esvo_map_lm_stats(esvo_handle h, esvo_lm_stats_t* out);
/* sizeof(esvo_lm_stats_t), ESVO_LM_SCALE_COUNT_ONLY, 0, 0. */
void esvo_lm_sizes(size_t out[4]);

/* ---- Mapper: semi-global matching per tick, esvo_MVStereo mode 4 -------------------------------------------------
 *
 * esvo_MVStereo::MappingAtTime in MVStereoMode 4, PURE_SEMI_GLOBAL_MATCHING (esvo_MVStereo.cpp:311-376).  It is not the
 * bootstrap (esvo_map_init_sgm): the two share StereoSGBM and the event selection, and differ in every rule that decides which
 * points exist.  Per selected event, in the selection's order (createEdgeMask(..., true, 0), :1127-1170, and the loop :329-353):
 *   (x, y) = floor of the event's rectified coordinate; skipped when that pixel is off the image (an event off the sensor has no
 *   rectified coordinate and is skipped too); events on the same pixel are NOT merged; skipped when x < 48 (numDisparities);
 *   disp = D(y, x) / 16.0, skipped when disp < 0.  No inverse-depth range test, no minimum point count; a disparity of exactly 0
 *   is kept (inv_depth 0, p_cam not finite).
 * The DepthPoint of a kept event: row = x, col = y (`DepthPoint dp(x, y)`, the reference's own argument order), x = (x, y),
 * inv_depth = disp / (P(0,0) * baseline), p_cam = cam2World(x, inv_depth), variance 1e-6 (update(inv_depth, 0) + boundVariance),
 * residual 0, age = age_vis_threshold, the observation's pose; scale2 = nu = 0 (uninitialised memory in the reference).
 * The frame enters the window even when it is empty, frames leave from the front while there are more than max_fusion_frames,
 * and DepthFusion::naive_propagation (DepthFusion.cpp:234-327) of every frame, newest first, fills a new DepthFrame at the
 * observation's pose: every residual is 0, so a cell belongs to the first point that touches it.  A point whose propagated
 * coordinate is not finite touches no cell.  Nothing is cleaned or regularised.
 * Checked against the reference's own compiled mode-4 branch through tests/sgm_tick_restated.py. */

/* Counts of the last esvo_map_tick_sgm / esvo_map_push_disparity_frame at each filter, and HIP-event times of its stages. */
typedef struct esvo_sgm_stats_t {
  uint64_t events;          /* selected events (the seam: events handed in) */
  uint64_t on_image;        /* ... on the sensor, with their rectified pixel on the image */
  uint64_t matched_columns; /* ... with x >= 48 */
  uint64_t disp_ok;         /* ... with disparity >= 0 */
  uint64_t points;          /* DepthPoints of the frame (no further test: == disp_ok) */
  uint64_t zero_disp;       /* points with a disparity of exactly 0 */
  float ms_sgbm;            /* the StereoSGBM chain (0 for the seam) */
  float ms_points;          /* point kernel, scan, compaction */
  float ms_propagate;       /* naive propagation of the window */
  float pad_;
} esvo_sgm_stats_t;

/* The whole mode-4 tick on the events staged by esvo_ts_push_events and the observation set last (its stamp and pose:
 * esvo_map_set_observation).  Selection: dataTransferring's mode-4 branch (esvo_MVStereo.cpp:612-625) -- the walk of
 * esvo_map_init_sgm: newest first from lower_bound(t_obs) over the last 2 * BM_half_slice_thickness, at most
 * PROCESS_EVENT_NUM + 1 events.  StereoSGBM (0, 48, 11, 8*11*11, 32*11*11, -1, 0, 11) on the UN-smoothed Time-Surface pair --
 * ts_left / ts_right: host mono8 W*H, or NULL for the device-resident frames of esvo_ts_render.  n_points (nullable): points of
 * the new frame.  disp_out (nullable): the W*H int16 disparity image (x16, -16 = none).  Synchronous; one host read-back (the
 * point count); nothing is allocated after the first call.  esvo_stats_t: ticks, last_events_in, last_points,
 * last_window_frames, last_window_points as esvo_map_tick_bm_only fills them.
 * Refused without any change of state: no observation / sharded handle (ESVO_ERR_STATE), W <= 50 (ESVO_ERR_UNSUPPORTED), more
 * selected events than max_events_per_tick or a window that does not fit the ring (ESVO_ERR_CAPACITY), selected events already
 * overwritten in the event ring (ESVO_ERR_STATE). */
int esvo_map_tick_sgm(esvo_handle h, const uint8_t* ts_left, const uint8_t* ts_right, size_t* n_points, int16_t* disp_out);
/* The seam of that mode for a node that keeps its own StereoSGBM and dataTransferring: everything behind sgbm_->compute.
 * disp16: the disparity x 16 image (host W*H int16), or NULL for the device's last SGM result (esvo_map_tick_sgm,
 * esvo_map_init_sgm); ev[n]: vEventsPtr_left_SGM_ in the node's order.  Builds the points, pushes the frame, applies the window
 * policy and runs the naive propagation at the observation set last.  esvo_map_tick_sgm == selection + StereoSGBM + this. */
int esvo_map_push_disparity_frame(esvo_handle h, const int16_t* disp16, const esvo_event_t* ev, size_t n, size_t* n_points);
int esvo_map_sgm_stats(esvo_handle h, esvo_sgm_stats_t* out);
/* sizeof() of {esvo_sgm_stats_t}, numDisparities (48), 0, 0. */
void esvo_sgm_sizes(size_t out[4]);

/* ---- Time-Surface history ------------------------------------------------------------ */

/* The nodes' TS_history_ (a std::map of stereo pairs by stamp, TS_HISTORY_LENGTH 100) on the device.  The tracker registers
 * against the newest pair (esvo_Tracking.cpp:241-247), the mapper observes the second newest pair that has a pose
 * (esvo_Mapping.cpp:497-534): on one handle neither is "the last render", so the frames are kept by stamp and both pick theirs
 * without a Time Surface crossing the bus.  Off by default; with the history off no other call changes in any way.
 *
 * Retained, once the history is on: every frame that becomes a camera's resident frame -- esvo_ts_render,
 * esvo_ts_render_forward, both cameras of esvo_map_tick_resident -- and the frames given with esvo_ts_history_put, each under
 * its stamp.  Host images handed to esvo_map_set_observation or esvo_track_set_current are NOT retained.  An entry is a stamp
 * with up to two frames; it is complete when both cameras are present.  The reference's ExactTime synchroniser only ever
 * inserts pairs, so esvo_map_set_observation_at and both select calls see complete pairs only; esvo_track_set_current_at
 * needs the left frame only.
 * Eviction is the reference's (timeSurfaceCallback, esvo_Mapping.cpp:757-761): the entry is inserted in stamp order, then the
 * smallest stamps are erased while there are more than `length`.  A new stamp below every retained one on a full history is
 * therefore not retained (the render itself succeeds).  With per-pixel queues (max_event_queue_len > 0) stamps may arrive in
 * any order.
 * Deviation: a stamp and camera that is retained already is OVERWRITTEN by a new frame; the reference's emplace keeps the
 * first one, but a node cannot receive one stamp twice.
 * esvo_reset empties the history (esvo_Mapping::reset, :764-804), the slots stay allocated; esvo_set_params leaves it alone.
 * Every call below returns ESVO_ERR_STATE while the history is off, ESVO_ERR_INVALID_ARG for a NULL argument (where not
 * stated otherwise) or a cam outside 0..1.  A stamp that is not retained -- or not complete where a pair is needed -- is
 * ESVO_ERR_STATE with no change of state: the previous observation / current frame stays in place, and esvo_last_error names
 * the stamp and the retained range.
 * Not on band-sharded or tick-interleaved handles: esvo_ts_history_configure(length > 0) returns ESVO_ERR_UNSUPPORTED there,
 * and esvo_shard_set_band / esvo_comm_init / esvo_comm_init_callbacks return ESVO_ERR_UNSUPPORTED on a handle with the history on
 * (the band mode keeps esvo_comm_gather_ts).
 * Threads: the calls belong to the mapper group, except esvo_track_set_current_at (tracker group) and esvo_ts_history_list /
 * esvo_ts_history_select_observation, which any thread may call; esvo_ts_history_select takes no handle. */

/* TS_HISTORY_LENGTH (esvo_Mapping.h / esvo_Tracking.h: 100): `length` pairs are retained; 0 = off (the default).  The
 * slots -- length x 2 frames of W * H bytes, each starting on a multiple of 256 bytes -- are allocated here and freed by
 * length = 0, a reconfiguration or esvo_destroy.  Reconfiguring empties the history. */
int esvo_ts_history_configure(esvo_handle h, size_t length);
/* TS_history_'s keys: the retained stamps in ascending order; cams[i]: bit 0 left present, bit 1 right present.  *n receives
 * the count; t_ns and cams may be NULL (both NULL: count only), otherwise cap < count is ESVO_ERR_CAPACITY. */
int esvo_ts_history_list(esvo_handle h, uint64_t* t_ns, uint8_t* cams, size_t cap, size_t* n);
/* A retained frame copied out (W * H bytes) ... */
int esvo_ts_history_get(esvo_handle h, uint64_t t_ns, int cam, uint8_t* out_mono8);
/* ... and a host frame put in, as timeSurfaceCallback's TS_history_.emplace does (esvo_Mapping.cpp:737-761) for a
 * Time-Surface node in another process: one upload on arrival instead of one per use. */
int esvo_ts_history_put(esvo_handle h, uint64_t t_ns, int cam, const uint8_t* mono8);
/* esvo_map_set_observation on the retained pair of that stamp (TS_obs_ = *it_end, esvo_Mapping.cpp:512-519): equal, bit for
 * bit, to esvo_map_set_observation(h, t_ns, left, right, T_world_cam) with the host images of the two frames, SmoothTimeSurface
 * included (the blur reads the slot directly, as it reads the resident frame). */
int esvo_map_set_observation_at(esvo_handle h, uint64_t t_ns, const double T_world_cam[16]);
/* esvo_track_set_current on the retained left frame of that stamp (curDataTransferring's TS_history_.rbegin(),
 * esvo_Tracking.cpp:241-247, for the newest stamp): equal, bit for bit, to esvo_track_set_current(h, left, kernel_size) with
 * the host image, kernel_size 0 or 5.  No host wait: the read queues behind the frame's store on the device. */
int esvo_track_set_current_at(esvo_handle h, uint64_t t_ns, int kernel_size);
/* dataTransferring's choice of TS_obs_ (esvo_Mapping.cpp:497-534; the same in esvo_MVStereo.cpp:559-576).  Host code, no
 * handle: t_ns are the stamps of the complete pairs, ascending.  n <= 10: ESVO_AGAIN (:497, "to assure the
 * esvo_time_surface node has been working").  The walk starts at the second newest stamp (:503, "in case that the tf is
 * behind the most current TS") and goes down to the oldest inclusive; the newest is never taken.  initialization != 0
 * (ESVO_System_Status_ == "INITIALIZATION"): the second newest, T_world_cam = identity, pose_fn is not called (may be NULL).
 * Otherwise the first stamp for which pose_fn returns 1 (getPoseAt), with the pose it filled in.  Returns ESVO_OK and
 * *index, or ESVO_AGAIN where the node returns false. */
int esvo_ts_history_select(const uint64_t* t_ns, size_t n, int initialization, esvo_em_pose_fn pose_fn, void* user, size_t* index,
                           double T_world_cam[16]);
/* The same on the handle's retained complete pairs; *t_ns receives the chosen stamp (for esvo_map_set_observation_at).
 * pose_fn runs on the calling thread with none of the handle's locks held. */
int esvo_ts_history_select_observation(esvo_handle h, int initialization, esvo_em_pose_fn pose_fn, void* user, uint64_t* t_ns,
                                       double T_world_cam[16]);

/* ---- Outputs ------------------------------------------------------------------------ */

/* DepthMap iteration (SmartGrid.h:346-358) as consumed by the publishers
 * (esvo_Mapping.cpp:925-932).  Elements are returned in the reference's list order. */
int esvo_map_get_depth_points(esvo_handle h, esvo_depth_point_t* out, size_t cap, size_t* n);
/* The DepthMap of the newest COMMITTED tick (*t_ns: its stamp, 0 if none) without completing a pending one:
 * esvo_map_tick(k) commits tick k-1 and leaves tick k's front stage running, so a node that publishes after every
 * tick reads map k-1 here while tick k computes (one tick of latency for the overlap). */
int esvo_map_get_committed(esvo_handle h, esvo_depth_point_t* out, size_t cap, size_t* n, uint64_t* t_ns);
/* Replaces the loop of publishPointCloud (esvo_Mapping.cpp:925-932): p_world = R p_cam + t
 * as float32 xyz triples, the payload of /esvo_mapping/pointcloud_local. */
int esvo_map_get_pointcloud_xyz(esvo_handle h, float* out_xyz, size_t cap_points, size_t* n);
/* The same cloud built and KEPT on the device: replaces publishPointCloud's loop (esvo_Mapping.cpp:925-932) together with the
 * /esvo_mapping/pointcloud_local hop to the tracking node (esvo_Tracking.cpp:107-108, refDataTransferring :203-234) -- the
 * tracker takes its reference straight from this buffer (esvo_track_set_reference_from_cloud).
 * esvo_map_cloud_build completes a pending tick as esvo_map_get_pointcloud_xyz does, then writes the cloud of the current
 * DepthMap into a buffer the handle owns: the points, order (the reference's list order) and float bits of
 * esvo_map_get_pointcloud_xyz, with no element download and no host sort; *n (may be NULL) receives the point count, the one
 * value the host reads.  The buffer is a SNAPSHOT: later ticks leave it alone until the next build; esvo_reset empties it.
 * Mapper-group call; it may run while the tracker group registers against the previous snapshot (the two are ordered on the
 * device, neither waits on the host for the other).  ESVO_ERR_STATE on a sharded handle (esvo_comm_gather_pointcloud_xyz is
 * the band mode's cloud).
 * esvo_map_cloud_get copies the snapshot out, 12 bytes per point: *n = its point count (0 before the first build and after a
 * reset); out_xyz == NULL returns the count only; ESVO_ERR_CAPACITY when cap_points is too small.
 * esvo_map_cloud_device lends the snapshot to a HIP caller: *d_xyz = device pointer to *n float triples (NULL when there is
 * none), *t_ns (may be NULL) = stamp of the tick the snapshot was built from.  Stream rule: the snapshot is complete when
 * esvo_map_cloud_build returns, so any stream may read it from then on without an event; the pointer stays valid and its
 * contents unchanged until the next esvo_map_cloud_build, esvo_reset or esvo_destroy, and the caller must have waited for its
 * own reads (an event or a stream synchronisation of its own) before it makes one of these calls. */
int esvo_map_cloud_build(esvo_handle h, size_t* n);
int esvo_map_cloud_get(esvo_handle h, float* out_xyz, size_t cap_points, size_t* n);
int esvo_map_cloud_device(esvo_handle h, const float** d_xyz, size_t* n, uint64_t* t_ns);
/* ---- Debug images and global-cloud helpers ----
 * Replaces Visualization::plot_map / DrawPoint (Visualization.cpp:13-94) as esvo_Mapping::publishMappingResults calls
 * them for the topics Inverse_Depth_Map, Standard_Variance_Map, Age_Map and cost_map (esvo_Mapping.cpp:868-884): BGR8
 * images of H*W*3 bytes, each pointer may be NULL.  age_max_range is the yaml key of that name. */
int esvo_map_get_debug_images(esvo_handle h, double age_max_range, uint8_t* inv_depth_bgr, uint8_t* stdvar_bgr,
                              uint8_t* age_bgr, uint8_t* cost_bgr);
/* pc_near_ of publishPointCloud (esvo_Mapping.cpp:925-932): world points of the elements with |p_cam| < visualize_range. */
int esvo_map_get_pointcloud_near_xyz(esvo_handle h, double visualize_range, float* out_xyz, size_t cap_points, size_t* n);
/* pcl::VoxelGrid<pcl::PointXYZ> with setLeafSize(leaf, leaf, leaf) (esvo_Mapping.cpp:960-964): host code, no handle.
 * One centroid per occupied voxel, ascending voxel index; the node appends the last NumGPC_added_per_refresh - 1 of them
 * to its global cloud (:966-969). */
int esvo_voxel_filter_xyz(const float* xyz, size_t n, float leaf, float* out_xyz, size_t cap_points, size_t* n_out);
/* ---- The global point cloud (pc_global_), accumulated on the device ----
 * Replaces the global-cloud branch of publishPointCloud (esvo_Mapping.cpp:955-977): once per visualizeGPC_interval the near
 * part of the current map's cloud goes through pcl::VoxelGrid with a cubic leaf and the tail of the filtered cloud is appended
 * to pc_global_.  Near cloud, filter and append run on the device; the host reads counts and an error flag.  The two halves
 * are also calls of their own, equal bit for bit to the host helpers above (which stay the yardsticks).
 * All handle calls here are mapper-group calls; those that read the map complete a pending tick first, as
 * esvo_map_cloud_build does.  They use buffers of their own: neither the esvo_map_cloud_build snapshot nor anything a tick
 * reads is touched.  ESVO_ERR_STATE on a band-sharded or tick-interleaved handle. */
typedef struct esvo_gpc_params_t {
  double   visualize_range;        /* visualize_range (2.5) */
  double   interval_s;             /* visualizeGPC_interval (3) */
  uint64_t num_added_per_refresh;  /* NumGPC_added_per_refresh (1000); >= 1 */
  uint64_t capacity_points;        /* device capacity of the global cloud; 0 -> 5 000 000 (the node's reserve, :151) */
  float    leaf;                   /* 0.3f: the node hard-codes it (:964) */
  uint32_t reserved;
} esvo_gpc_params_t;

typedef struct esvo_gpc_stats_t {  /* last update + totals since configure */
  uint64_t updates, refreshes;     /* calls; calls the interval let through */
  uint64_t total_points;           /* size of the global cloud */
  uint32_t last_near, last_voxels, last_added, last_refreshed;
  double   t_last_pub;             /* t_last_pub_pc_ */
  float    ms_last;                /* device time of the last refresh (HIP events around it) */
  uint32_t pad;
} esvo_gpc_stats_t;

/* pc_near_ (:925-932) built on the device: the alive elements in list order with sqrt((x*x + y*y) + z*z) < visualize_range on
 * p_cam (f64, in that order), transformed by the observation's pose -- the points, order and float bits of
 * esvo_map_get_pointcloud_near_xyz; only the points cross the bus.  out_xyz == NULL returns the count only;
 * ESVO_ERR_CAPACITY when cap_points is too small. */
int esvo_map_cloud_near(esvo_handle h, double visualize_range, float* out_xyz, size_t cap_points, size_t* n);
/* The device twin of esvo_voxel_filter_xyz: host arrays in and out, all arithmetic on the device (bounds reduction, keys,
 * a stable radix sort of (key, input index), run heads, one sequential float sum per voxel in input order), the same bytes.
 * Rows with a coordinate that is not finite are dropped.  leaf <= 0: ESVO_ERR_INVALID_ARG.  A grid of more than 2^31 - 1
 * cells: ESVO_ERR_CAPACITY, nothing written.  out_xyz == NULL returns the count only; cap_points too small:
 * ESVO_ERR_CAPACITY.  The handle lends its device and scratch buffers (grown on demand); its map is not read. */
int esvo_map_voxel_filter(esvo_handle h, const float* xyz, size_t n, float leaf, float* out_xyz, size_t cap_points, size_t* n_out);
/* Allocates the device buffers of the global cloud (the only call of the five below that allocates), empties the cloud and
 * sets t_last_pub = 0.0 (:152).  ESVO_ERR_INVALID_ARG: num_added_per_refresh == 0 (the reference's `threshold - 1` is a size_t
 * and would wrap), leaf <= 0, a range or interval that is NaN. */
int esvo_map_gpc_configure(esvo_handle h, const esvo_gpc_params_t* prm);
/* The branch :956-977 on the current map.  now = toSec(t_ns).  If !(now - t_last_pub > interval_s): *refreshed = 0, nothing
 * else happens (the call is counted in stats.updates).  Otherwise: near cloud -> voxel filter with `leaf` -> L centroids ->
 * the last min(L, num_added_per_refresh) - 1 of them are appended to the global cloud; t_last_pub = now; *refreshed = 1.
 * Where the reference is undefined: L == 0 appends nothing and still counts as a refresh (the reference's size_t subtraction
 * wraps there).  An append beyond capacity_points fails with ESVO_ERR_CAPACITY and leaves the cloud, t_last_pub and the stats
 * as they were; so does a grid of more than 2^31 - 1 cells.  ESVO_ERR_STATE before esvo_map_gpc_configure.
 * The centroids never visit the host.  Synchronous: the cloud is complete when the call returns. */
int esvo_map_gpc_update(esvo_handle h, uint64_t t_ns, int* refreshed);
/* The global cloud: a copy (out_xyz == NULL: the count only), or the device buffer itself -- valid and unchanged until the
 * next esvo_map_gpc_update that refreshes, esvo_map_gpc_configure, esvo_reset or esvo_destroy.  Empty before configure.
 * esvo_reset empties the cloud and keeps t_last_pub, as esvo_Mapping::reset does (:779-780 clear the clouds, nothing resets
 * t_last_pub_pc_). */
int esvo_map_gpc_get(esvo_handle h, float* out_xyz, size_t cap_points, size_t* n);
int esvo_map_gpc_device(esvo_handle h, const float** d_xyz, size_t* n);
int esvo_map_gpc_stats(esvo_handle h, esvo_gpc_stats_t* out);
/* sizeof(esvo_gpc_params_t), sizeof(esvo_gpc_stats_t), the default capacity_points (5 000 000), 0. */
void esvo_gpc_sizes(size_t out[4]);
/* Replaces esvo_MVStereo::saveDepthMap (esvo_MVStereo.cpp:982-1000; the call sites at :302, :373, :521 are compiled out upstream
 * with `if (false)`: "to save the depth result, set it to true"): writes <save_dir><t_ns>.txt, one line "x y depth" per valid
 * element of the DepthMap in list order, formatted as Eigen's operator<< and the ofstream format it.  save_dir is used as a
 * prefix exactly as upstream does (it must end with the path separator).  n_written (nullable): lines written. */
int esvo_map_save_depth_map(esvo_handle h, const char* save_dir, uint64_t t_ns, size_t* n_written);
/* The newest frame of the fusion window (culled DepthPoints of the last tick). */
int esvo_map_get_last_frame(esvo_handle h, esvo_depth_point_t* out, size_t cap, size_t* n);
int esvo_get_stats(esvo_handle h, esvo_stats_t* out);
/* sizeof() of {event, calib, params, match, depth_point, stats}, 0, ABI version:
 * lets a foreign-language binding check its struct mirrors. */
void esvo_abi_sizes(size_t out[8]);

/* ---- Multi-GPU: one tick split over the GPUs by image row band ------------------------------------ */

/* Make this handle shard `shard` of `n_shards`: its per-cell work (fuse / clean / regularise) is the image rows
 * [row_begin, row_end).  (0, H, 0, 1) = unsharded.  How the per-event work (match + refine), the event ingest and the
 * Time-Surface raster are divided is esvo_shard_set_routing's choice; this call selects ESVO_ROUTE_BROADCAST. */
int esvo_shard_set_band(esvo_handle h, int row_begin, int row_end, int shard, int n_shards);
/* How a band handle divides the work that is not per cell.  Call after esvo_shard_set_band, before any event is staged
 * (or after esvo_reset): ESVO_ERR_STATE otherwise.
 *   ESVO_ROUTE_Y_RECT (what SURVEY.md §8(e) specifies; the default of esvo_amd/dist.py and bench.py):
 *     - ingest: esvo_ts_push_events* keeps, of the events it is handed, those this rank needs -- for both cameras the raw
 *       rows that the rectifying remap and the median of its rendered rows read (derived from the calibration maps), for
 *       the left camera also every event whose rectified row floor(y_rect) lies in the band.  Only they cross PCIe, sit in
 *       the device ring and are scattered; the host still walks every stamp (the reference's event selection,
 *       esvo_Mapping.cpp:562-574, counts the whole left stream).  The caller hands EVERY rank the full packets, exactly as a
 *       ROS topic would deliver them to eight subscribers.
 *     - raster: the Time Surfaces / the observation pair are rendered for the band + ts_halo_rows rows only (rounded
 *       outwards to whole 16-row tiles; + 2 rows under SmoothTimeSurface).  Rows outside are undefined in every image
 *       the handle returns.
 *     - match + refine: an event belongs to the rank that owns floor(y_rect) (the epipolar search is horizontal,
 *       EventBM.cpp:170-226, so block matching reads the band + patch_size_Y / 2 rows).  The refinement warps the patch by
 *       the camera motion since the event (DepthProblem.cpp:157-191) and may leave those rows: every evaluation is
 *       checked, a match whose blocks leave the rendered rows is COUNTED (stats.halo_violations, summed over all ranks by
 *       the second exchange), and once that count is non-zero every rank refuses its next tick with ESVO_ERR_HALO --
 *       never a silently different result.  Raise ts_halo_rows (DSEC / DAVIS hand-held sequences move < 10 rows in the
 *       10 ms a tick looks back) or fall back to ESVO_ROUTE_BROADCAST.
 *     - Denoising (ABI 7; esvo_Mapping.cpp:1046-1072): a rank decides the mask's verdict for the selected events whose RAW row lies
 *       in its band (its ring keeps one more raw row on either side), the verdicts travel as one bit per selected event
 *       (esvo_shard_tick_phase(h, 0) returns ESVO_AGAIN with that block due), and phase 0's second part matches the kept sequence
 *       of the unsharded tick.
 *     - a push that fails (ESVO_ERR_CAPACITY: event ring full) has consumed nothing -- not the events, not their stamps in the
 *       global sequence: render and hand the SAME packet in again, or the rank's global indices part from its peers'.
 *     Not available with per-pixel event queues, FORWARD mode, up-down stereo: ESVO_ERR_UNSUPPORTED.
 *   ESVO_ROUTE_BROADCAST (A/B switch; exact whatever the motion): every rank stages ALL events and renders the full Time
 *     Surfaces; the per-event work is the slots w with w % n_shards == shard of the tick's thread-stride order.
 * ts_halo_rows < 0: the default (24). */
enum { ESVO_ROUTE_BROADCAST = 0, ESVO_ROUTE_Y_RECT = 1 };
int esvo_shard_set_routing(esvo_handle h, int mode, int ts_halo_rows);
/* What the routing resolved to (each pointer may be NULL): rendered rectified rows, valid rows of the observation pair, the
 * raw rows whose events are kept per camera.  (0, H) everywhere for ESVO_ROUTE_BROADCAST. */
int esvo_shard_get_rows(esvo_handle h, int render_rows[2], int observation_rows[2], int source_rows_left[2], int source_rows_right[2]);
/* Three-phase tick for sharded operation.  The fusion window is replicated (every rank holds every frame; the DepthFrame
 * is rebuilt from it at every tick, so a band needs nothing of its neighbours' maps).  After phase 0 and after phase 1
 * the caller ALL-GATHERS one fixed-size block per rank (esvo_shard_exchange; ncclAllGather / torch.distributed
 * all_gather_into_tensor issued on the handle's stream, see esvo_amd/dist.py):
 *   phase 0: poses + event selection + block matching + LM refinement + culling of the rank's events
 *            -> exchange 1: (bit 0 matched, bit 1 point kept) of the tick's slots --
 *               Y_RECT:    two bits per slot of the WHOLE tick, own slots set: ceil(n / 16) 32-bit words rounded up to 8 bytes
 *               BROADCAST: one byte per OWN slot, slots shard, shard + n_shards ... back to back: ceil(n / n_shards)
 *                          bytes rounded up to 8
 *   phase 1: the tick's frame order (EventBM.cpp:289-308 and DepthProblemSolver.cpp:75-90 permutations, derived
 *            from all ranks' bits), own kept points packed with their final index
 *            -> exchange 2: [count (8 B) | points], 8 + K x sizeof(esvo_depth_point_t) bytes with K = the largest
 *               kept count among the ranks (every rank derives it from exchange 1)
 *   phase 2: every block's points to their place in the frame; window policy (identical on every rank), fusion +
 *            clean + regularisation of the band; the halo rows the band's neighbourhoods read
 *            (2 + RegularizationRadius) are recomputed locally, which is exact because the DepthFrame is rebuilt
 *            from the window at every tick.
 * The DepthMap stays sharded; esvo_map_get_depth_points returns the band's elements (seq = global
 * creation order, so bands merge by sorting on it).  stats.last_solved counts the shard's own problems. */
int esvo_shard_tick_phase(esvo_handle h, int phase, uint64_t t_ns, const uint64_t* pose_t_ns,
                          const double* pose_T, size_t m);
/* The exchange due before the next phase: all-gather block_bytes (a multiple of 8; 0 = nothing to do) from d_send of
 * every rank into d_recv, rank-major.  With n_shards == 1 d_recv aliases d_send and the call may be skipped. */
int esvo_shard_exchange(esvo_handle h, void** d_send, void** d_recv, size_t* block_bytes);

/* ---- Multi-GPU exchange behind the C-ABI: one process per GPU, RCCL over xGMI ------------------

 * The reference is a single-process CPU program (std::thread fan-out only); these calls exist because this
 * implementation can spread its per-tick work over the GPUs of a node.  RCCL is loaded (dlopen) by esvo_comm_unique_id /
 * esvo_comm_init only; the frame exchange of the tick-interleaved mode runs on a stream of its own, every other collective on
 * the handle's front stream.  All calls below are COLLECTIVE: every
 * rank makes them in the same order with the same arguments. */
#define ESVO_COMM_ID_BYTES 128
/* ncclGetUniqueId on one rank; hand the bytes to the others by any means (ROS parameter server, MPI, a file). */
int esvo_comm_unique_id(uint8_t id[ESVO_COMM_ID_BYTES]);
/* Which RCCL the calls above resolved: ncclGetVersion's code and the path of the shared object (dladdr).  The library is
 * loaded with dlopen on first use: ESVO_RCCL_PATH if set, else the librccl.so.1 already mapped into the process (a
 * process that imported torch carries torch's copy), else the loader path, else /opt/rocm/lib. */
int esvo_comm_rccl_info(int* version, char* path, size_t path_cap);
/* ncclCommInitRank on the handle's device. */
int esvo_comm_init(esvo_handle h, const uint8_t id[ESVO_COMM_ID_BYTES], int rank, int world);
/* The same with the collective supplied by the caller (another transport; tests that run several ranks on one GPU):
 * all_gather: bytes_per_rank from d_send into d_recv[rank * bytes_per_rank] on every rank.  It must be ordered after the work
 * already enqueued on hip_stream and must have completed (or be enqueued on hip_stream) when it returns 0. */
typedef int (*esvo_all_gather_fn)(void* user, const void* d_send, void* d_recv, size_t bytes_per_rank, void* hip_stream);
int esvo_comm_init_callbacks(esvo_handle h, int rank, int world, esvo_all_gather_fn all_gather, void* user);
int esvo_comm_destroy(esvo_handle h);
/* Tick-interleaved operation (throughput scales with the GPUs; the latency of one tick does not change): rank r maps
 * the ticks k = r (mod world) completely.  A tick depends on earlier ticks only through the frames of its fusion window
 * (MappingAtTime builds a new DepthFrame at every tick, esvo_Mapping.cpp:266-272,341-377), so after every `world` ticks the
 * ranks exchange that round's frames with ONE ncclAllGather (each block carries its point count: one host wait per
 * round, for an exchange enqueued a round earlier), push them into their windows in tick order and fuse at their own tick.
 * esvo_comm_tick replaces esvo_map_set_observation + esvo_map_tick: every rank calls it for every tick; the rank for which
 * esvo_comm_owns_next_tick() is 1 must have rendered both Time Surfaces of that tick (esvo_ts_render) beforehand. */
int esvo_comm_owns_next_tick(esvo_handle h);
int esvo_comm_tick(esvo_handle h, uint64_t t_ns, const double T_world_cam[16], const uint64_t* pose_t_ns, const double* pose_T,
                   size_t m);
/* The same with the owner's Time Surfaces rendered inside the call (= esvo_map_tick_resident's front: both cameras in one
 * launch per kernel); no esvo_ts_render beforehand. */
int esvo_comm_tick_resident(esvo_handle h, uint64_t t_ns, const double T_world_cam[16], const uint64_t* pose_t_ns,
                            const double* pose_T, size_t m);
/* Two rounds are in flight per rank (ABI 7): the call that completes round j enqueues that round's exchange on a stream of
 * its own -- pack, ncclAllGather, the blocks' counts to the host -- and then pushes + fuses round j - 1, whose exchange went
 * out a whole round earlier; the front stage of round j + 1 follows on the front and LM streams while exchange j travels.
 * The block length of a gather is the largest frame of the last four rounds + 25 % (the buffers' capacity until counts have
 * been seen; a frame that does not fit is gathered again with grown blocks, identically on every rank).  On a tick another
 * rank maps the call scatters that tick's events into this rank's SAE on the front stream (idle on such a tick), so an own
 * render only has its own tick's events left.  esvo_comm_flush completes a partial round and everything in flight. */
int esvo_comm_flush(esvo_handle h);
typedef struct esvo_comm_stats_t {
  uint64_t rounds;             /* rounds collected (frames pushed) */
  uint64_t gathers;            /* frame all-gathers issued (rounds + repeats after a regrow) */
  uint64_t regrows;            /* rounds that were gathered again because a frame exceeded its block */
  uint64_t bytes_sent;         /* bytes this rank contributed to those all-gathers (block length each) */
  uint64_t points_gathered;    /* depth points of all ranks' frames in the collected rounds (104 B each) */
  uint64_t host_wait_us;       /* host time spent waiting for the counts of a round (the one host wait per round): the slack the
                                  host has when the device sets the pace; near zero = the calling thread is the pace */
  uint32_t last_stride_points; /* block length of the last collected round, in points */
  uint32_t stride_cap_points;  /* what the exchange buffers hold per block */
} esvo_comm_stats_t;
int esvo_comm_get_stats(esvo_handle h, esvo_comm_stats_t* out);
/* The DepthMap of the newest tick on every rank (it lives on the rank that mapped it: all-gather of the newest maps). */
int esvo_comm_newest_map(esvo_handle h, esvo_depth_point_t* out, size_t cap, size_t* n, long long* tick_index);
/* One tick split over the ranks (esvo_shard_set_band + esvo_shard_set_routing first): the three phases of
 * esvo_shard_tick_phase with their two ncclAllGather exchanges, and the all-gather of the DepthMap bands, merged on the
 * creation order. */
int esvo_comm_shard_tick(esvo_handle h, uint64_t t_ns, const uint64_t* pose_t_ns, const double* pose_T, size_t m);
int esvo_comm_gather_map(esvo_handle h, esvo_depth_point_t* out, size_t cap, size_t* n);
/* ABI 7: the band exchange is device-resident -- the band's alive cells compacted on the device, their counts gathered first
 * (16 B per rank, the one host wait), then the elements with the largest band as block length, merged on the device by the
 * elements' global creation ids (a scatter by id, one scan, a gather).
 * esvo_comm_gather_pointcloud_xyz: publishPointCloud's cloud (esvo_Mapping.cpp:909-934) of the whole map on every rank -- the
 * points, order and float bits of esvo_map_get_pointcloud_xyz on one GPU: the tracker's reference cloud in the closed loop.
 * esvo_comm_gather_ts: routed band mode renders a rank's rows only, the tracker reads the whole left Time Surface: all-gather of
 * the bands' rows of camera cam's resident surface (standard partition: rank r owns rows [r ceil(H / world), ...)); afterwards
 * esvo_track_set_current(h, NULL, k) and esvo_map_init_sgm(h, NULL, NULL, ...) see the full image on every rank.  A no-op
 * without row routing. */
int esvo_comm_gather_pointcloud_xyz(esvo_handle h, float* out_xyz, size_t cap_points, size_t* n);
int esvo_comm_gather_ts(esvo_handle h, int cam);

/* ---- Tracker residual / Jacobian evaluation ---------------------- */

/* The adjacent consumer of the hot path: esvo_Tracking's RegProblemLM evaluates, for <= 2000 map points, a
 * bilinear fetch on the negated blurred left Time Surface (and on its Sobel derivatives for the analytical
 * Jacobian).  The device already holds that Time Surface, so these calls replace the per-point loops of
 * RegProblemLM.cpp and spare the tracker the TS download; the 6-DoF LM driver (Eigen, Cayley + SVD) stays on the
 * host, as north_star has it.  Supported: patch 1x1, kernelSize 0 or 5, l2 / Huber -- what every shipped
 * cfg/tracking yaml uses.  All calls are synchronous and run on a stream of their own. */
#define ESVO_TRACK_L2 0
#define ESVO_TRACK_HUBER 1
/* TimeSurfaceObservation::getTimeSurfaceNegative(kernelSize) + computeTsNegativeGrad
 * (TimeSurfaceObservation.h:118-147).  ts_left == NULL: the device-resident left Time Surface of the last
 * esvo_ts_render(h, 0, ...). */
int esvo_track_set_current(esvo_handle h, const uint8_t* ts_left, int kernel_size);
/* TS_negative_left_ (mono8, what the reprojection-map publisher draws on) and its derivatives as int16. */
int esvo_track_get_images(esvo_handle h, uint8_t* neg, int16_t* du, int16_t* dv);
/* The point loop of RegProblemLM::setProblem (RegProblemLM.cpp:44-56): p = R_world_ref^T (p_world - t_world_ref).
 * xyz_world: n x 3 float32 in the caller's order, i.e. after the stochastic swaps of :48-49 (rand() stays with
 * the caller). */
int esvo_track_set_reference(esvo_handle h, const float* xyz_world, size_t n, const double T_world_ref[16]);
/* The same loop (RegProblemLM.cpp:38-55) on the snapshot of esvo_map_cloud_build, in one launch on the tracker's stream:
 * position i of the reference takes cloud point order[i] -- what ref->vPointXYZPtr_[i] is after the swaps of :48-49
 * (esvo_track_stochastic_order) -- then p = R_world_ref^T (p_world - t_world_ref).  Equal bit for bit to
 * esvo_track_set_reference(h, cloud[order], n, T_world_ref); only the n indices travel.  order == NULL: the first
 * min(n, cloud) points in list order.  An index may repeat.  Refused with the previous reference left in place:
 * ESVO_ERR_STATE before any esvo_map_cloud_build or after esvo_reset, ESVO_ERR_INVALID_ARG for an index >= the cloud's
 * count.  Tracker-group call. */
int esvo_track_set_reference_from_cloud(esvo_handle h, const uint32_t* order, size_t n, const double T_world_ref[16]);
/* The stochastic swaps of setProblem (RegProblemLM.cpp:45-49) from the cloud's SIZE alone (host code, no handle): for
 * i < n_take, positions i and i + draws[i] % (n_cloud - i) of the identity over n_cloud are swapped; order[i] is what ends
 * up at position i.  draws[i] is the reference's rand() of that step, which stays with the caller.  n_take > n_cloud is
 * clamped (:39-40); O(n_take) time and memory.  esvo_hip::stochastic_order (esvo_hip.hpp) is the same function inline. */
int esvo_track_stochastic_order(size_t n_cloud, size_t n_take, const uint32_t* draws, uint32_t* order);
/* RegProblemLM::operator() (:91-136) on the batch [offset, offset+count) of setStochasticSampling (:71-88):
 * fvec[i] = sqrt(w_i) r_i, r_i = TS_negative(x_i) or 255 when the point does not reproject. */
int esvo_track_residuals(esvo_handle h, const double T_left_ref[16], size_t offset, size_t count, int ls_norm,
                         double huber_threshold, double* fvec, size_t* n_out);
/* RegProblemLM::df at x = 0 (:178-269) for the problem's current R_, t_: fjac is n_out x 6, column-major. */
int esvo_track_jacobian(esvo_handle h, const double R[9], const double t[3], size_t offset, size_t count,
                        double* fjac, size_t* n_out);
/* What one iteration of RegProblemSolverLM::solve_analytical consumes (RegProblemSolverLM.cpp:148-215: minimizeInit -> F(0),
 * minimizeOneStep -> df at 0, then a 6 x 6 system), in ONE launch and 43 doubles back: f = operator()(0) on the batch with its
 * Huber weights (RegProblemLM.cpp:121-131), J = df(0) (:178-269; the reference's Jacobian carries no weight), H = J^T J (6 x 6,
 * row-major, symmetric), b = J^T f, *cost = |f|^2.  R, t: the problem's R_, t_ as for esvo_track_jacobian (the warp of
 * operator()(0) is [R^T | -R^T t]).  The sums are taken in a fixed order (kernels_track.hip), reproduced by the CPU oracle. */
int esvo_track_normal_equations(esvo_handle h, const double R[9], const double t[3], size_t offset, size_t count, int ls_norm,
                                double huber_threshold, double H[36], double b[6], double* cost, size_t* n_out);
/* The same for n_poses (1..ESVO_TRACK_MAX_POSES) poses in ONE launch and one read-back: what Eigen's minimizeOneStep spends one
 * functor evaluation each on -- the trial points of its inner loop (a step per damping value until one is accepted) -- evaluated
 * together.  R: n_poses x 9, t: n_poses x 3, H: n_poses x 36, b: n_poses x 6, cost: n_poses; every pose's sums are the ones
 * esvo_track_normal_equations gives for it alone, bit for bit. */
#define ESVO_TRACK_MAX_POSES 4
int esvo_track_normal_equations_batch(esvo_handle h, int n_poses, const double* R, const double* t, size_t offset, size_t count,
                                      int ls_norm, double huber_threshold, double* H, double* b, double* cost, size_t* n_out);
/* The registration loop on top of it, host C++ inside the library (esvo_hip::gauss_newton_register of esvo_hip.hpp -- the same
 * code a C++ node calls directly): Levenberg-damped Gauss-Newton on (Cayley, translation) with the reference's motion update
 * (RegProblemLM::addMotionUpdate, :347-360: R <- orth(dR R), t <- dt + dR t), over the first n_points of the reference cloud;
 * a step is accepted when its actual cost reduction is at least 1e-4 of the predicted one (Eigen's ratio test), the damping
 * is raised tenfold otherwise and lowered tenfold after an accepted step; three trial dampings are evaluated per launch.
 * R, t: in = the start (R_, t_ of setProblem: identity / zero, or the previous frame's), out = the registered motion.
 * The reference's own driver is Eigen's LevenbergMarquardt (third-party, absent here); this one is what the closed-loop test
 * and bench.py use in its place. */
int esvo_track_register(esvo_handle h, size_t n_points, double R[9], double t[3], int ls_norm, double huber_threshold,
                        int max_iterations, double damping, double* rms, int* iterations);

/* The same registration with the batch schedule of the shipped configs, a record of what it did, and -- on_device = 1 -- the
 * whole loop in ONE kernel launch and one read-back: normal equations, the damped 6 x 6 solves, the Cayley update, the polar
 * factor and the accept test all run inside track_solve_kernel (one workgroup), in the host loop's expression order, so both
 * paths return the same bits.  The device path evaluates the trial dampings of an iteration lazily, in rising order: the
 * result is defined as the first acceptable one in that order, which is what the host's speculative launch of three returns. */
#define ESVO_TRACK_SOLVE_MAX_ITERATIONS 64
typedef struct esvo_track_solve_params_t {
  uint64_t n_points;        /* first n_points of the reference cloud (clamped to what esvo_track_set_reference holds) */
  uint64_t batch_size;      /* 0 or >= n_points: every iteration on all points (what esvo_track_register does);
                               else RegProblemLM::solve's schedule: offset = (it % max(n_points / batch_size, 1)) * batch_size */
  int32_t  ls_norm;         /* ESVO_TRACK_L2 / ESVO_TRACK_HUBER */
  int32_t  max_iterations;  /* 1 .. ESVO_TRACK_SOLVE_MAX_ITERATIONS */
  int32_t  on_device;       /* 0: gauss_newton_register on the host over esvo_track_normal_equations_batch
                               1: the whole loop in one kernel launch */
  int32_t  reserved;
  double   huber_threshold;
  double   damping;
} esvo_track_solve_params_t;

typedef struct esvo_track_iter_t {   /* one record per outer iteration */
  double   cost;        /* |f|^2 at the linearisation point of this iteration */
  double   lambda;      /* damping of the accepted trial, or the last one tried when none was accepted */
  double   step_norm;   /* |dx| of the accepted trial, 0 when none */
  uint32_t n;           /* points in this iteration's batch */
  uint32_t offset;      /* first point of the batch */
  int32_t  pick;        /* index 0..5 of the accepted trial in rising damping order (3..5 = second round), -1 none */
  int32_t  trials;      /* trial poses whose cost was needed to decide (1..6; in an iteration that ends on a singular damped
                           system: the trials before it, 0..5, and lambda is the singular system's damping) */
} esvo_track_iter_t;

typedef struct esvo_track_solve_info_t {
  double  rms;
  int32_t iterations;
  int32_t ok;           /* Registration::ok */
  int32_t stop;         /* 0 max_iterations, 1 step < 1e-6, 2 no trial acceptable, 3 failed (singular trial / evaluation) */
  int32_t launches;     /* kernel launches this call made (1 when on_device) */
} esvo_track_solve_info_t;

/* R, t: in = the start, out = what gauss_newton_register returns (its last accepted pose also when ok is 0).  info and trace may
 * be NULL; at most trace_cap records are written (info->iterations of them exist).  ESVO_ERR_STATE before
 * esvo_track_set_current, ESVO_ERR_INVALID_ARG for an unknown norm or max_iterations outside 1..64. */
int esvo_track_solve(esvo_handle h, const esvo_track_solve_params_t* prm, double R[9], double t[3],
                     esvo_track_solve_info_t* info, esvo_track_iter_t* trace, size_t trace_cap);
/* sizeof of esvo_track_solve_params_t, esvo_track_iter_t, esvo_track_solve_info_t, and ESVO_TRACK_SOLVE_MAX_ITERATIONS */
void esvo_track_sizes(size_t out[4]);
/* RegProblemSolverLM's reprojection map (RegProblemSolverLM.cpp:180-209; :106-135 per iteration of solve_numerical):
 * TS_negative_left_ of the last esvo_track_set_current in grey, the first min(n_points, reference size) points of the
 * reference (ResItems_ order) reprojected with [R^T | -R^T t] and painted as DrawPoint paints them (radius-1 filled circle,
 * jet colour of 1/z between inv_depth_min and inv_depth_max = invDepth_min_range / invDepth_max_range; later points over
 * earlier ones).  bgr_out: H x W x 3 bytes, or NULL to leave the image on the device.  n_inside (may be NULL): points whose
 * centre pixel is inside the image.  Tracker-group call.
 * None of the residual's tests applies (no bounds, no mask): the centre is ((int)x, (int)y) of the projection, truncated toward
 * zero, and each of the plus' five pixels is painted iff it lies inside the image.  1/z is the point's inverse depth in the
 * reference frame; the colour index floor((1/z - min) / (max - min) * 255) is clamped to 0..255 before it becomes an int.
 * Where the reference is undefined the point is skipped: a coordinate that is not finite or of magnitude >= 2^30, a NaN
 * index.  cv::circle's raster is restated, not pinned to OpenCV.  A reference of 0 points or n_points == 0 gives the grey
 * image and n_inside = 0.  ESVO_ERR_STATE before esvo_track_set_current; ESVO_ERR_INVALID_ARG: R or t NULL, a range that
 * is not finite, inv_depth_max == inv_depth_min.  Waits for the tracker's stream once, when bgr_out or n_inside is given. */
int esvo_track_reprojection_map(esvo_handle h, const double R[9], const double t[3], size_t n_points,
                                double inv_depth_min, double inv_depth_max, uint8_t* bgr_out, size_t* n_inside);
/* the image of the last such call on the device (valid until the next one or esvo_destroy); ESVO_ERR_STATE before any */
int esvo_track_reprojection_map_device(esvo_handle h, const uint8_t** d_bgr);

#ifdef __cplusplus
}
#endif
#endif /* ESVO_HIP_H */
