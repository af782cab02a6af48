// api_core.hip — lifecycle of the handle, parameters, ABI self-checks (see context.hpp).
#include "context.hpp"

namespace esvo_host {
thread_local std::string g_create_error;
}

namespace {

void invert3x3(const double* P, double* Kinv, double* Kinv_t) {
  const double a = P[0], b = P[1], cc = P[2], d = P[4], e = P[5], f = P[6], g = P[8], hh = P[9], i = P[10];
  const double det = a * (e * i - f * hh) - b * (d * i - f * g) + cc * (d * hh - e * g);
  const double id = 1.0 / det;
  Kinv[0] = (e * i - f * hh) * id; Kinv[1] = (cc * hh - b * i) * id; Kinv[2] = (b * f - cc * e) * id;
  Kinv[3] = (f * g - d * i) * id;  Kinv[4] = (a * i - cc * g) * id;  Kinv[5] = (cc * d - a * f) * id;
  Kinv[6] = (d * hh - e * g) * id; Kinv[7] = (b * g - a * hh) * id;  Kinv[8] = (a * e - b * d) * id;
  for (int r = 0; r < 3; ++r) Kinv_t[r] = (Kinv[r * 3 + 0] * P[3] + Kinv[r * 3 + 1] * P[7]) + Kinv[r * 3 + 2] * P[11];
}

int validate_params(const esvo_params_t* p, std::string& why) {
  if (p->ls_norm != ESVO_LSNORM_TDIST && p->ls_norm != ESVO_LSNORM_L2) { why = "LSnorm must be Tdist or l2 (DepthProblemSolver.cpp:121-131 exits on anything else)"; return ESVO_ERR_UNSUPPORTED; }
  if (p->bm_step < 1) { why = "BM_step must be >= 1"; return ESVO_ERR_INVALID_ARG; }
  // 15 x 7 (every shipped configuration) runs the register-layout kernels; any other size the general ones (kernels_lm_any.hip:
  // lane = column, three [rows][64] f64 arrays in LDS)
  if (p->patch_size_x < 1 || p->patch_size_x > 64 || p->patch_size_y < 1 || p->patch_size_y > 40) { why = "patch size must be within 1..64 x 1..40"; return ESVO_ERR_UNSUPPORTED; }
  if (p->median_blur_kernel_size < 0 || p->median_blur_kernel_size > 3) { why = "median_blur_kernel_size must be 0..3 (kernel 2k + 1)"; return ESVO_ERR_UNSUPPORTED; }
  if (p->max_event_queue_len < 0 || p->max_event_queue_len > TSQ_LMAX) { why = "max_event_queue_len must be 0 (one stamp per pixel) or 1..32"; return ESVO_ERR_UNSUPPORTED; }
  if (p->bm_max_disparity < p->bm_min_disparity || p->bm_min_disparity < 0) { why = "bad disparity range"; return ESVO_ERR_INVALID_ARG; }
  {  // both block-matching launchers size dynamic LDS from the range; past what a workgroup can be given the launch itself would fail
    const unsigned long long lds = esvo::bm_match_lds_bytes(p->patch_size_x, p->patch_size_y, p->bm_min_disparity, p->bm_max_disparity, p->bm_step, p->bm_updown);
    if (lds > esvo::BM_LDS_MAX_BYTES) {
      why = "disparity range too wide: block matching would need " + std::to_string(lds) + " bytes of LDS per workgroup for its strip of " +
            std::to_string((long long)p->bm_max_disparity - p->bm_min_disparity + 1) + " candidates, a workgroup gets " + std::to_string(esvo::BM_LDS_MAX_BYTES) + " at the most";
      return ESVO_ERR_UNSUPPORTED;
    }
  }
  if (p->td_nu <= 2.0 || p->td_scale <= 0) { why = "Tdist_nu must be > 2 and Tdist_scale > 0"; return ESVO_ERR_INVALID_ARG; }
  if (p->num_threads < 1 || p->num_threads > 64) { why = "num_threads out of range"; return ESVO_ERR_INVALID_ARG; }
  if (p->lm_max_iteration < 1) { why = "lm_max_iteration must be >= 1"; return ESVO_ERR_INVALID_ARG; }
  if (p->lm_scale_pass_limit < 0) { why = "lm_scale_pass_limit must be 0 (off), a positive pass limit or ESVO_LM_SCALE_COUNT_ONLY"; return ESVO_ERR_INVALID_ARG; }
  if (p->reg_radius < 0 || p->reg_radius > 31) { why = "RegularizationRadius out of range [0,31] (one 64-bit mask per tap row)"; return ESVO_ERR_INVALID_ARG; }
  return ESVO_OK;
}

// ---- esvo_create in steps (each returns a status; esvo_create destroys the half-built handle on the first that fails) ----------
#define CK(call) do { hipError_t _e = (call); if (_e != hipSuccess) { g_create_error = std::string(#call) + ": " + hipGetErrorString(_e); return ESVO_ERR_HIP; } } while (0)

// tiles of the fusion front (kernels_fuse.hip): FUSE_TILE x FUSE_TILE cells each
size_t fuse_front_tiles(const esvo_context* h) { return (size_t)((h->W + FUSE_TILE - 1) / FUSE_TILE) * ((h->H + FUSE_TILE - 1) / FUSE_TILE); }

// The device side of "as created": what esvo_create leaves behind, on the front stream, and esvo_reset puts back.  Everything else a
// tick reads it has written before, or (d_clk, esvo_reset) is cleared where it is read.
int zero_session_buffers(esvo_context* h, hipStream_t st) {
  const size_t npx = (size_t)h->W * h->H;
  for (int cam = 0; cam < 2; ++cam) {
    HIPCHK(hipMemsetAsync(h->d_sae[cam], 0, sizeof(u64) * npx, st));
    if (h->d_tsq[cam]) HIPCHK(hipMemsetAsync(h->d_tsq[cam], 0, sizeof(u64) * npx * (size_t)h->tsq_len, st));  // EventQueueMat semantics: a set of <= L keys per pixel, slot-major
  }
  HIPCHK(hipMemsetAsync(h->d_halo_viol, 0, sizeof(u32) * 2, st));
  HIPCHK(hipMemsetAsync(h->d_map, 0, map_buffer_bytes(npx), st));
  HIPCHK(hipMemsetAsync(h->d_map2, 0, map_buffer_bytes(npx), st));
  HIPCHK(hipMemsetAsync(h->d_tile_count, 0, sizeof(u32) * fuse_front_tiles(h), st));  // zero between ticks: fuse_turn_kernel clears what was read
  HIPCHK(hipMemsetAsync(h->d_fuse_ctr, 0, sizeof(u32) * 2112, st));
  if (h->d_rank_kept) HIPCHK(hipMemsetAsync(h->d_rank_kept, 0, sizeof(u32) * esvo_context::SHARD_MAX_RANKS, st));  // (band mode: allocated by its configuration)
  { int rcf = filter_zero_state(h, st); if (rcf) return rcf; }  // (the event filter's `last` images, where one is configured)
  { int rcs = survey_zero_state(h, st); if (rcs) return rcs; }  // (the event survey's counts and stats, where one is open)
  h->d_map_cur = h->d_map;
  return ESVO_OK;
}

// every development switch the handle reads (common.hpp, esvo_dev_switch: only with ESVO_DEV_SWITCHES=1), one line each
void read_dev_switches(esvo_context* h) {
  const char* e;
  if ((e = esvo_dev_switch("ESVO_LM_PAIR"))) h->lm_pair_forced = std::atoi(e) == 1 ? 1 : (std::atoi(e) == 0 ? 0 : -1);
  if ((e = esvo_dev_switch("ESVO_LM_QUEUES"))) h->lm_queues = std::atoi(e) == 1 ? 1 : (std::atoi(e) == 2 ? 2 : 0);
  if ((e = esvo_dev_switch("ESVO_TIMELINE"))) h->tl_on = std::atoi(e) != 0;
  if ((e = esvo_dev_switch("ESVO_LOWLAT"))) h->lat_mode = std::atoi(e) != 0;
  if ((e = esvo_dev_switch("ESVO_LOWLAT_TIMED_EVERY"))) h->lat_timed_every = std::max(1, std::atoi(e));
  if ((e = esvo_dev_switch("ESVO_REG_SPARSE"))) h->reg_sparse_forced = std::atoi(e) != 0 ? 1 : 0;
  if ((e = esvo_dev_switch("ESVO_PIPE_TIMED_EVERY"))) h->pipe_timed_every = std::max(1, std::atoi(e));
  if ((e = esvo_dev_switch("ESVO_LOWLAT_MAX_EVENTS"))) h->lat_max_events = (u32)std::strtoul(e, nullptr, 10);
  if (h->tsq_len > 0) h->tsq_tcap = (e = esvo_dev_switch("ESVO_TSQ_TILE_CAP")) ? (u32)std::max(1, std::atoi(e)) : 1024u;  // tests: force the overflow list
  if (h->max_ev > LM_TWO_QUEUES_MAX_EVENTS && (e = esvo_dev_switch("ESVO_LM_ORDER"))) h->lm_order_on = std::atoi(e) != 0;  // (only where the order buffers exist)
  if ((e = esvo_dev_switch("ESVO_BM_DEDUPE"))) h->bm_dedupe_on = std::atoi(e) != 0;
  if ((e = esvo_dev_switch("ESVO_BM_DEDUPE_MIN"))) h->bm_dedupe_min = (u32)std::max(1L, std::atol(e));
  if ((e = esvo_dev_switch("ESVO_CLK_PROBE"))) h->clk_probe = std::atoi(e) != 0;
  h->n_pose_slots = (e = esvo_dev_switch("ESVO_POSE_SLOTS0")) ? (u32)std::max(1, std::atoi(e)) : 1024u;  // tests: a smaller first allocation (alloc_window_and_map)
  if ((e = esvo_dev_switch("ESVO_FLT_TILE_CAP"))) h->flt_tcap = (u32)std::min<long>(std::max(1L, std::atol(e)), (long)FLT_TILE_CAP_MAX);  // tests: force the packet-reading route
  if ((e = esvo_dev_switch("ESVO_FUSE_TILE_CAP"))) h->fuse_tile_cap = (u32)std::max(1L, std::atol(e));
  if ((e = esvo_dev_switch("ESVO_FUSE_PMAX"))) h->fuse_pmax_plus1 = (u32)std::max(0L, std::atol(e)) + 1u;
  if ((e = esvo_dev_switch("ESVO_FUSE_TILE_REC"))) h->fuse_tile_rec = (u32)std::max(1L, std::atol(e));
  if ((e = esvo_dev_switch("ESVO_FUSE_LDS_CAP"))) h->fuse_lds_cap = (u32)std::max(0L, std::atol(e));
}

int create_streams(esvo_context* h) {
  int prio_lo = 0, prio_hi = 0;  // numerically lower = higher priority
  CK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  // Three stages on three streams share the chip.  The LM kernel is the bulk of the vector-ALU work and tolerates waiting
  // (two dense waves per SIMD); the matching stage and the fusion stage are short, latency-bound kernels that run one wave
  // per SIMD beside it.  They get the HIGH priority and the LM stream the LOWEST: whenever one of their waves is ready it
  // issues, the LM waves fill every other slot.  Measured in round 3: 1.40 ms per tick against 1.70 ms with the LM stream
  // high and the fusion stream low.  (Other priority assignments and a SPATIAL partition of the compute units by
  // hipExtStreamCreateWithCUMask were measured in rounds 3-4 -- all slower, 1.5-4 ms for the partition; profiles/HISTORY.md.)
  CK(hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, prio_hi));
  CK(hipStreamCreateWithPriority(&h->stream_b, hipStreamNonBlocking, prio_hi));
  h->own_stream = true;
  CK(hipStreamCreateWithPriority(&h->stream_l, hipStreamNonBlocking, prio_lo));
  CK(hipStreamCreateWithPriority(&h->stream_l1, hipStreamNonBlocking, prio_lo));
  CK(hipStreamCreateWithFlags(&h->stream_t, hipStreamNonBlocking));
  CK(hipStreamCreateWithFlags(&h->stream_i, hipStreamNonBlocking));
  return ESVO_OK;
}

// one camera: calibration -> device (the left camera's rectification table and mask, the fixed-point remap), then its Time Surface
int alloc_camera(esvo_context* h, int cam, const esvo_calib_t* c) {
  const size_t npx = (size_t)h->W * h->H;
  if (cam == 0) {
    CK(h->d_lut.alloc(npx));
    CK(hipMemcpy(h->d_lut, c->rect_lut, sizeof(float2) * npx, hipMemcpyHostToDevice));
    if (c->rect_mask) {
      CK(h->d_mask.alloc(npx));
      CK(hipMemcpy(h->d_mask, c->rect_mask, npx, hipMemcpyHostToDevice));
    }
  }
  std::vector<int2> fm(npx);
  for (size_t i = 0; i < npx; ++i) {  // OpenCV remap's INTER_BITS=5 coordinate quantisation (Appendix B.2)
    fm[i].x = (int)std::nearbyintf(c->map_x[i] * 32.f);
    fm[i].y = (int)std::nearbyintf(c->map_y[i] * 32.f);
  }
  CK(h->d_fixmap[cam].alloc(npx));
  CK(hipMemcpy(h->d_fixmap[cam], fm.data(), sizeof(int2) * npx, hipMemcpyHostToDevice));
  // per rectified row: the raw rows its bilinear taps reach (what a row band of the Time Surface needs of the SAE;
  // esvo_shard_set_routing).  A tap outside the image reads the constant 0 and needs nothing.
  h->fix_row_lo[cam].assign(h->H, h->H);
  h->fix_row_hi[cam].assign(h->H, -1);
  for (int y = 0; y < h->H; ++y)
    for (int x = 0; x < h->W; ++x) {
      const int2 m = fm[(size_t)y * h->W + x];
      const int ix = m.x >> 5, iy = m.y >> 5, fx = m.x & 31, fy = m.y & 31;
      if (ix + (fx ? 1 : 0) < 0 || ix >= h->W) continue;
      const int lo = std::max(iy, 0), hi = std::min(iy + (fy ? 1 : 0), h->H - 1);
      if (lo > hi) continue;
      h->fix_row_lo[cam][y] = std::min(h->fix_row_lo[cam][y], lo);
      h->fix_row_hi[cam][y] = std::max(h->fix_row_hi[cam][y], hi);
    }
  CK(h->d_sae[cam].alloc(npx));  // (the SAE and the queues are zeroed by zero_session_buffers)
  if (h->tsq_len > 0) CK(h->d_tsq[cam].alloc(npx * (size_t)h->tsq_len));
  CK(h->d_ts[cam].alloc(npx + 64));
  for (int k = 0; k < 2; ++k) CK(h->d_obs2[k][cam].alloc(npx + 64));
  h->d_obs[cam] = h->d_obs2[0][cam];
  return ESVO_OK;
}

// what the two cameras share: the queues' tile lists, raw surfaces, event rings, the tick's pose tables
int alloc_rings(esvo_context* h, const esvo_calib_t* left, const esvo_calib_t* right) {
  const size_t npx = (size_t)h->W * h->H;
  if (h->tsq_len > 0) {
    const size_t tiles = (size_t)((h->W + 7) / 8) * ((h->H + 7) / 8);
    CK(h->d_tsq_tcount.alloc(tiles)); CK(hipMemset(h->d_tsq_tcount, 0, sizeof(u32) * tiles));
    CK(h->d_tsq_tlist.alloc(tiles * h->tsq_tcap));
    CK(h->d_tsq_over.alloc((size_t)esvo_context::TSQ_ROUND));
    CK(h->d_tsq_over_count.alloc(1));
  }
  CK(h->d_raw.alloc(npx + 64)); CK(h->d_raw1.alloc(npx + 64));
  h->h_rect_lut[0].assign(left->rect_lut, left->rect_lut + 2 * npx);
  if (right->rect_lut) h->h_rect_lut[1].assign(right->rect_lut, right->rect_lut + 2 * npx);
  CK(h->d_obs_tmp.alloc(npx + 64));
  h->ring_cap = (u64)std::max<int64_t>(h->prm.event_ring_capacity, 1024);
  for (int cam = 0; cam < 2; ++cam) CK(h->d_ring[cam].alloc(h->ring_cap));
  h->max_poses = (u32)std::max(h->prm.max_poses_per_tick, 2);
  for (int k = 0; k < 2; ++k) CK(h->pose[k].d_T.alloc((size_t)h->max_poses * 17));  // [T | toSec]
  h->d_pose_T = h->pose[0].d_T;  // (pose_buf == 0; upload_poses re-points it)
  return ESVO_OK;
}

int alloc_tick_scratch(esvo_context* h) {
  const size_t npx = (size_t)h->W * h->H, E = h->max_ev;
  if (h->max_ev > 4000000u) FAIL(ESVO_ERR_CAPACITY, "max_events_per_tick too large (scan limit 4M)");
  if (npx > 4000000u) FAIL(ESVO_ERR_CAPACITY, "image too large (scan limit 4M pixels)");
  CK(h->d_tick_ev.alloc(E));
  CK(h->d_match_slots.alloc(E));
  CK(h->d_match_flags.alloc(E)); CK(h->d_match_prefix.alloc(E));
  for (int k = 0; k < 2; ++k) CK(h->front[k].d_matches.alloc(E));
  // (scratch of the split launch: 7 x 16 doubles per match -- only where the launch can be used)
  if (E >= LM_SPLIT_MIN_EVENTS) {
    // The split LM launch (kernels_lm.hip, LmSplit) executes 10 % fewer vector instructions (3.47e8 against 3.85e8 per launch
    // of the bench workload) but does not shorten the tick (1.40 against 1.38 ms): what it removes are the partially masked
    // instructions of lockstep execution, and the tick is bound by the chip's throughput at its sustained f64 clock.  It is
    // On the 1280x720 stress stream (4.9e5 events, 2.3e5 matches per tick: five times the waves) it does pay: 7.7 against
    // 8.4 ms per tick (profiles/r03_split_launch_other_workloads.txt).  So: used for launches bounded by >= 400 000 events.
    CK(h->d_lm_fvec0.alloc(E * 7 * 16)); CK(h->d_lm_fnorm0.alloc(E));
    CK(h->d_lm_meta.alloc(E)); CK(h->d_lm_order.alloc(E));
    CK(h->d_lm_hist.alloc(2 * 32 * 64));  // kernels_lm.hip: 2 x LM_SPLIT_STRIPES x LM_SPLIT_BINS
    CK(hipMemset(h->d_lm_hist, 0, sizeof(u32) * 2 * 32 * 64));
  }
  if (E > LM_TWO_QUEUES_MAX_EVENTS) {  // (= LM_WIDE_MAX: launches above it take the narrow layout) the processing order, context.hpp
    for (int k = 0; k < 2; ++k) { CK(h->front[k].d_lm_pix_order.alloc(E)); CK(h->d_lm_sort_rows[k].alloc(E)); }
    CK(h->d_lm_sort_hist.alloc(voxel_hist_words(E)));
  }
  if (h->bm_dedupe_on && E >= h->bm_dedupe_min) CK(h->d_bm_dedupe.alloc(npx + 4 + 2 * E));  // context.hpp: table | count | list | outcomes
  // (two blocks, one per front parity: two LM launches in flight -- the two LM queues -- must not share the probe's scratch, where
  //  a wave leaves its start stamps: a launch that read the other one's stamp added a wrapped difference to the sums)
  CK(h->d_clk.alloc(2 * clk_words(h->max_ev)));
  // All of it, once, so that no word is undefined; esvo_reset clears the CLK_SCRATCH sums at the head of each block only: the start
  // stamps behind them are written by the wave that reads them back (kernels_lm.hip), in every launch
  CK(hipMemset(h->d_clk, 0, sizeof(u64) * 2 * clk_words(h->max_ev)));
  int khz = 0;  // rate of s_memrealtime (wall_clock64): the constant reference clock the probe divides by
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess || khz <= 0) khz = 100000;
  h->stats.clk_ref_khz = (uint32_t)khz;
  for (int k = 0; k < 2; ++k) {
    CK(h->front[k].d_pt_slots.alloc(E));
    CK(h->front[k].d_pt_flags.alloc(E)); CK(h->front[k].d_pt_prefix.alloc(E));
    CK(h->front[k].d_scan_tmp_l.alloc(scan_scratch_elems(std::max(E, npx)) + 8));
  }
  CK(h->d_pts_tmp.alloc(E));
  for (int k = 0; k < 2; ++k) CK(h->front[k].d_stage.alloc(E));
  for (int k = 0; k < 2; ++k) CK(h->front[k].d_counters.alloc(CNT_ROW));
  for (int k = 0; k < 2; ++k) CK(hipMemset(h->front[k].d_counters, 0, sizeof(u32) * CNT_ROW));
  CK(h->h_counters.alloc(CNT_ROW * 2));
  std::memset(h->h_counters, 0, sizeof(u32) * CNT_ROW * 2);
  CK(h->h_pin.alloc(2 * ((size_t)h->max_poses * 17 + 16)));
  CK(h->d_scan_tmp.alloc(scan_scratch_elems(std::max(E, npx)) + 8)); CK(h->d_scan_tmp_b.alloc(scan_scratch_elems(std::max(E, npx)) + 8));
  CK(h->d_cnt_b.alloc(CNTB_ROW)); CK(hipMemset(h->d_cnt_b, 0, sizeof(u32) * CNTB_ROW));
  CK(h->h_cnt_b.alloc(CNTB_ROW * CNTB_ROWS));  // (common.hpp: CNTB_ROW_*)
  std::memset(h->h_cnt_b, 0, sizeof(u32) * CNTB_ROW * CNTB_ROWS);
  for (int k = 0; k < 2; ++k) { h->front[k].d_clk = h->d_clk + (size_t)k * clk_words(h->max_ev); h->front[k].h_counters = h->h_counters + CNT_ROW * k; h->back[k].h_cnt = h->h_cnt_b + CNTB_ROW * k; }  // the slots' views
  CK(h->d_halo_viol.alloc(2));
  return ESVO_OK;
}

int alloc_window_and_map(esvo_context* h) {
  const size_t npx = (size_t)h->W * h->H, E = h->max_ev;
  h->win_cap = (u32)std::max<int64_t>((int64_t)h->prm.max_window_points, (int64_t)E) + 2 * (u32)E;
  CK(h->d_win.alloc(h->win_cap));
  // CONST_POINTS keeps frames until their points exceed 1.5 maxNumFusionPoints (esvo_Mapping.cpp:346-353): every non-empty
  // frame holds at least one point, which bounds their number; empty frames are run-length records (context.hpp)
  h->max_frames = (u32)std::max(h->prm.max_fusion_frames + 2, 512);
  if (h->prm.fusion_strategy == ESVO_FUSION_CONST_POINTS)
    h->max_frames = std::max(h->max_frames, (u32)(1.5 * h->prm.max_fusion_points) + 4u);
  // pose-table slots of the window's non-empty frames: max_frames + 1 in the worst case (CONST_POINTS with one point per
  // frame: 1 GB of tables at 20 000 points x 256 poses), a handful in practice -- allocated for 1024 frames (read_dev_switches) and
  // doubled on demand (alloc_pose_slot, api_window.hip)
  h->slot_used.assign(h->max_frames + 1, 0);
  h->n_pose_slots = std::min<u32>(h->max_frames + 1, h->n_pose_slots);
  CK(h->d_frame_pose_T.alloc((size_t)h->n_pose_slots * h->max_poses * 16));
  CK(h->d_fr_table.alloc(2 * (3 * (size_t)h->max_frames + 1))); CK(h->h_fr_table.alloc(2 * (3 * (size_t)h->max_frames + 1)));
  for (int k = 0; k < 2; ++k) { h->back[k].d_fr_table = h->d_fr_table + k * (h->d_fr_table.cap() / 2); h->back[k].h_fr_table = h->h_fr_table + k * (h->h_fr_table.cap() / 2); }  // a half each
  // map
  CK(h->d_prop.alloc(h->win_cap));
  const size_t n_tiles = fuse_front_tiles(h);
  CK(h->d_tile_pts.alloc(n_tiles * h->fuse_tile_cap)); CK(h->d_over_pts.alloc(h->win_cap));
  CK(h->d_tile_count.alloc(n_tiles));
  CK(h->d_cell_count.alloc(npx)); CK(h->d_cell_offset.alloc(npx));
  h->fuse_slice_cap = (u32)((n_tiles + 63) / 64) * FUSE_TILE * FUSE_TILE;   // the cells of the tiles t with t % 64 == slice
  CK(h->d_cell_list.alloc((size_t)16 * 64 * h->fuse_slice_cap));
  CK(h->d_fuse_ctr.alloc(2112 + 64));
  // the 64 words behind the counters (common.hpp: FUSE_CTR_*, the last one at 2081) are padding no kernel addresses: zeroed here,
  // once, so that no word is undefined; the counters themselves by zero_session_buffers
  CK(hipMemset(h->d_fuse_ctr + 2112, 0, sizeof(u32) * 64));
  CK(h->d_rec_ids.alloc(n_tiles * h->fuse_tile_rec + (size_t)h->win_cap * 9));
  for (int k = 0; k < 2; ++k) CK(h->d_map_mem[k].alloc(map_buffer_bytes(npx)));  // cells + their dense flags (common.hpp: map_flags)
  h->d_map = reinterpret_cast<MapCell*>(h->d_map_mem[0].get()); h->d_map2 = reinterpret_cast<MapCell*>(h->d_map_mem[1].get());
  CK(h->d_owner_max.alloc(npx)); CK(h->d_owner_min.alloc(npx));
  CK(h->d_own_w.alloc(E)); CK(h->d_lkeep.alloc(E));
  h->codes_bytes = (E + 7) / 8 * 8;
  CK(h->d_codes.alloc(h->codes_bytes));
  CK(h->d_sel.alloc(E));
  CK(h->d_evmap.alloc(npx + 64));
  CK(h->d_reg_ab.alloc(npx)); CK(h->d_reg_cd.alloc(npx));
  CK(h->d_exp_flags.alloc(npx)); CK(h->d_exp_prefix.alloc(npx));
  CK(h->d_export.alloc(npx)); CK(h->d_export_cell.alloc(npx));
  return ESVO_OK;
}

int create_events_and_pools(esvo_context* h) {
  for (int k = 0; k < 2; ++k) CK(h->ts_ev[k].create());
  CK(h->ev_frame.create());  // (all of them, now: BE_RG1, FE_STG and a pose buffer's are waited for before they are first recorded)
  for (int k = 0; k < 2; ++k) CK(h->front[k].own_ev.create());
  for (int k = 0; k < 2; ++k) { CK(h->back[k].ev.create()); CK(h->pose[k].released.create()); }
  if (h->tl_on) { CK(h->tl_ref.create()); CK(hipEventRecord(h->tl_ref, h->stream)); CK(hipEventSynchronize(h->tl_ref)); }
  CK(h->evt_trk_read.create(hipEventDisableTiming));
  for (int cam = 0; cam < 2; ++cam) CK(h->evt_ingest[cam].create(hipEventDisableTiming));
  CK(h->h_pose_pool.alloc(16 * (size_t)h->max_poses * esvo_context::POSE_POOL));
  for (int i = 0; i < esvo_context::POSE_POOL; ++i) CK(h->pool_evt[i].create());
  for (int i = 0; i < 16; ++i) h->T_world_obs[i] = h->T_world_frame[i] = (i % 5 == 0) ? 1.0 : 0.0;
  return ESVO_OK;
}
#undef CK

}  // namespace

namespace esvo_host {

void fill_dev_params(esvo_context* h) {
  const esvo_params_t& p = h->prm;
  DevParams& d = h->dp;
  d.W = h->W; d.H = h->H;
  d.wx = p.patch_size_x; d.wy = p.patch_size_y;
  d.dmin = p.bm_min_disparity; d.dmax = p.bm_max_disparity; d.step = p.bm_step; d.updown = p.bm_updown ? 1 : 0;
  d.zncc_thr = p.bm_zncc_threshold;
  d.baseline_f = h->baseline * d.camL.P[0];
  d.td_nu = p.td_nu; d.td_scale = p.td_scale; d.td_scale2 = p.td_scale * p.td_scale;
  const double td_stdvar = std::sqrt(p.td_nu / (p.td_nu - 2) * (p.td_scale * p.td_scale));  // DepthProblem.h:34
  d.td_stdvar2 = td_stdvar * td_stdvar;
  d.lm_max_iter = p.lm_max_iteration; d.lm_maxfev = p.lm_max_iteration * 3;
  d.invdepth_min = p.invdepth_min; d.invdepth_max = p.invdepth_max;
  d.var_thr = p.stdvar_vis_threshold * p.stdvar_vis_threshold;
  d.cost_thr = (p.residual_vis_threshold * p.residual_vis_threshold) * (double)(p.patch_size_x * p.patch_size_y);
  d.age_thr = p.age_vis_threshold;
  d.fusion_radius = p.fusion_radius;
  d.reg_radius = p.reg_radius; d.reg_min_nb = p.reg_min_neighbours; d.reg_min_close = p.reg_min_close_neighbours;
  d.num_threads = p.num_threads;
  d.ls_norm = p.ls_norm;
}

// compute band of the per-cell stages: the owned rows + a halo of 2 rows for the displaced-element side
// effects (+ the regulariser's radius), see DevParams::cband_y0
void set_compute_band(esvo_context* h) {
  const int halo = 2 + (h->prm.regularization ? h->prm.reg_radius : 0);
  h->dp.cband_y0 = std::max(0, h->dp.band_y0 - halo);
  h->dp.cband_y1 = std::min(h->H, h->dp.band_y1 + halo);
}

// the reference's colour tables are jet on i / 255 (Visualization.cpp:128-226): 255 * channel =
// clamp(min(4 i + a, -4 i + b), 0, 255), stored in an 8-bit image by rounding half to even
void jet256_bgr(uint8_t jet[768]) {
  const double ab[3][2] = {{127.5, 637.5}, {-127.5, 892.5}, {-382.5, 1147.5}};  // B, G, R
  for (int i = 0; i < 256; ++i)
    for (int c = 0; c < 3; ++c) {
      double v = std::min(4.0 * i + ab[c][0], -4.0 * i + ab[c][1]);
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      jet[3 * i + c] = (uint8_t)std::nearbyint(v);
    }
}

}  // namespace esvo_host

// =================================================================================================
extern "C" {

void esvo_default_params(esvo_params_t* p) {
  std::memset(p, 0, sizeof(*p));
  p->decay_ms = 30; p->median_blur_kernel_size = 1; p->ignore_polarity = 1;
  p->patch_size_x = 25; p->patch_size_y = 25; p->ls_norm = ESVO_LSNORM_TDIST;
  p->td_nu = 0; p->td_scale = 0; p->lm_max_iteration = 10;
  p->reg_radius = 5; p->reg_min_neighbours = 8; p->reg_min_close_neighbours = 8;
  p->bm_min_disparity = 3; p->bm_max_disparity = 40; p->bm_step = 1; p->bm_zncc_threshold = 0.1;
  p->invdepth_min = 0.16; p->invdepth_max = 2.0; p->stdvar_vis_threshold = 0.005; p->residual_vis_threshold = 15;
  p->age_vis_threshold = 0; p->fusion_radius = 0; p->fusion_strategy = ESVO_FUSION_CONST_FRAMES;
  p->max_fusion_frames = 10; p->max_fusion_points = 2000; p->clean_requires_full_window = 1;
  p->process_event_num = 500; p->bm_half_slice_thickness = 0.001; p->num_threads = 4;
  p->max_events_per_tick = 1024; p->max_window_points = 20000; p->max_poses_per_tick = 256;
  p->event_ring_capacity = 1 << 24;
}

const char* esvo_last_error(esvo_handle h) { (void)h; return g_create_error.c_str(); }  // the calling thread's last error

int esvo_create(const esvo_params_t* params, const esvo_calib_t* left, const esvo_calib_t* right, int device,
                esvo_handle* out) {
  esvo_context* h = nullptr;
  if (!params || !left || !right || !out) FAIL(ESVO_ERR_INVALID_ARG, "null argument");
  if (left->width != right->width || left->height != right->height || left->width <= 0 || left->height <= 0)
    FAIL(ESVO_ERR_INVALID_ARG, "left/right image sizes differ or are empty");
  if (!left->rect_lut || !left->map_x || !left->map_y || !right->map_x || !right->map_y)
    FAIL(ESVO_ERR_INVALID_ARG, "calibration arrays missing");
  {
    std::string why;
    int rc = validate_params(params, why);
    if (rc) FAIL(rc, why);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    FAIL(ESVO_ERR_NO_DEVICE, "no HIP device visible: the ESVO hot path has no CPU fallback");
  if (device < 0 || device >= ndev) FAIL(ESVO_ERR_INVALID_ARG, "device ordinal out of range");
  HIPCHK(hipSetDevice(device));
  h = new esvo_context();
  h->prm = *params;
  h->device = device;
  h->W = left->width; h->H = left->height;
  std::memset(&h->stats, 0, sizeof(h->stats));
  std::memcpy(h->dp.camL.P, left->P, sizeof(double) * 12);
  std::memcpy(h->dp.camR.P, right->P, sizeof(double) * 12);
  invert3x3(left->P, h->dp.camL.Kinv, h->dp.camL.Kinv_t);
  invert3x3(right->P, h->dp.camR.Kinv, h->dp.camR.Kinv_t);
  {  // CameraSystem::computeBaseline, CameraSystem.cpp:161-166
    const double* t = h->dp.camR.Kinv_t;
    h->baseline = std::sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  }
  h->dp.band_y0 = 0; h->dp.band_y1 = h->H;
  h->dp.cband_y0 = 0; h->dp.cband_y1 = h->H;
  h->dp.ev_shard = 0; h->dp.ev_nshards = 1;
  fill_dev_params(h);
  h->tsq_len = params->max_event_queue_len;  // (0: one stamp per pixel)
  // + 1: the SGM bootstrap selects up to PROCESS_EVENT_NUM + 1 events (esvo_Mapping.cpp:547: `size() <= PROCESS_EVENT_NUM_`)
  h->max_ev = (u32)std::max(params->max_events_per_tick, params->process_event_num) + 1u;
  read_dev_switches(h);
  int rc = create_streams(h);
  for (int cam = 0; cam < 2 && !rc; ++cam) rc = alloc_camera(h, cam, cam ? right : left);
  if (!rc) rc = alloc_rings(h, left, right);
  if (!rc) rc = alloc_tick_scratch(h);
  if (!rc) rc = alloc_window_and_map(h);
  if (!rc) rc = create_events_and_pools(h);
  if (!rc) rc = zero_session_buffers(h, h->stream);
  if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) { g_create_error = "draining the front stream failed"; rc = ESVO_ERR_HIP; }
  if (rc) { esvo_destroy(h); return rc; }
  *out = h;
  return ESVO_OK;
}

int esvo_destroy(esvo_handle h) {
  if (!h) return ESVO_OK;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->stream_l) hipStreamSynchronize(h->stream_l);
  if (h->stream_l1) hipStreamSynchronize(h->stream_l1);
  if (h->stream_b) hipStreamSynchronize(h->stream_b);
  comm_release(h);
  em_release(h);
  gpc_release(h);
  // the handle's buffers and its own events go with it, before the streams as ever
  const hipStream_t streams[] = {h->own_stream ? h->stream : nullptr, h->stream_b, h->stream_l, h->stream_l1, h->stream_t, h->stream_i};
  delete h;
  for (hipStream_t s : streams) if (s) { hipStreamSynchronize(s); hipStreamDestroy(s); }
  return ESVO_OK;
}

int esvo_reset(esvo_handle h) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  // a reset excludes the other two groups as well: pushers in flight finish first (the tracker's images and reference stay:
  // context.hpp, "survives a reset")
  std::lock_guard<std::mutex> lp0(h->mu_push[0]), lp1(h->mu_push[1]), ltk(h->mu_track), lts(h->mu_ts), lr(h->mu_ring), lcl(h->mu_cloud);
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream_l)); HIPCHK(hipStreamSynchronize(h->stream_l1));
  HIPCHK(hipStreamSynchronize(h->stream_b));
  HIPCHK(hipStreamSynchronize(h->stream_t));
  HIPCHK(hipStreamSynchronize(h->stream_i));
  comm_reset(h);  // (drains the exchange stream of a handle with a communicator)
  // the session state (context.hpp): what is declared in these structs, and nothing else, starts again
  static_cast<IngestSession&>(*h) = IngestSession{};
  static_cast<TsSession&>(*h) = TsSession{};
  static_cast<SchedSession&>(*h) = SchedSession{};
  static_cast<MapSession&>(*h) = MapSession{};
  static_cast<CloudSession&>(*h) = CloudSession{};  // (every stream was drained above: no gather is in flight)
  // ... and what no default initialiser can say
  std::fill(h->slot_used.begin(), h->slot_used.end(), 0);  // (its size is fixed at esvo_create)
  std::memset(h->h_cnt_b + CNTB_ROW * CNTB_ROW_HALO, 0, sizeof(u32) * CNTB_ROW);
  hist_clear(h);  // esvo_Mapping::reset clears TS_history_ (:764-804); the slots stay allocated
  gpc_reset(h);
  { int rcz = zero_session_buffers(h, h->stream); if (rcz) return rcz; }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream_l)); HIPCHK(hipStreamSynchronize(h->stream_l1));
  HIPCHK(hipStreamSynchronize(h->stream_b));
  const uint32_t khz = h->stats.clk_ref_khz;  // (a property of the device: kept)
  std::memset(&h->stats, 0, sizeof(h->stats));
  h->stats.clk_ref_khz = khz;
  for (const FrontSlot& F : h->front) HIPCHK(hipMemset(F.d_clk, 0, sizeof(u64) * CLK_SCRATCH));  // the probe's sums (alloc_tick_scratch)
  for (const FrontSlot& F : h->front)  // the scale-loop guard's stripes, where a guarded launch has allocated them
    if (F.d_lm_guard) HIPCHK(hipMemset(F.d_lm_guard, 0, sizeof(u32) * LM_GUARD_STRIPES * LM_GUARD_WORDS));
  return ESVO_OK;
}

int esvo_set_params(esvo_handle h, const esvo_params_t* params) {
  if (!h || !params) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  std::string why;
  int rc = validate_params(params, why);
  if (rc) FAIL(rc, why);
  if ((u32)std::max(params->max_events_per_tick, params->process_event_num) > h->max_ev)
    FAIL(ESVO_ERR_CAPACITY, "process_event_num exceeds the capacity fixed at esvo_create");
  if (params->lm_scale_pass_limit != 0 && (h->sharded || h->comm))
    FAIL(ESVO_ERR_STATE, "handle is band-sharded or tick-interleaved: the LM scale-loop guard (lm_scale_pass_limit) is a single-GPU feature");
  {
    const u32 need = params->fusion_strategy == ESVO_FUSION_CONST_POINTS ? (u32)(1.5 * params->max_fusion_points) + 4u
                                                                         : (u32)params->max_fusion_frames + 2u;
    if (need > h->max_frames) FAIL(ESVO_ERR_CAPACITY, "fusion window (frames) exceeds the capacity fixed at esvo_create");
  }
  if (h->routed && (params->smooth_time_surface != h->prm.smooth_time_surface || params->median_blur_kernel_size != h->prm.median_blur_kernel_size ||
                    params->patch_size_y != h->prm.patch_size_y || params->denoising != h->prm.denoising || params->bm_updown))
    FAIL(ESVO_ERR_STATE, "the handle routes events by row (esvo_shard_set_routing): SmoothTimeSurface, median_blur_kernel_size, patch_size_Y and Denoising "
                         "fix the rows it renders and the events it keeps; esvo_reset + esvo_shard_set_routing to change them");
  esvo_params_t np = *params;
  np.max_events_per_tick = h->prm.max_events_per_tick;
  np.max_window_points = h->prm.max_window_points;
  np.max_poses_per_tick = h->prm.max_poses_per_tick;
  np.event_ring_capacity = h->prm.event_ring_capacity;
  if (np.max_event_queue_len != h->prm.max_event_queue_len) FAIL(ESVO_ERR_CAPACITY, "max_event_queue_len is fixed at esvo_create (the per-pixel queues are allocated there)");
  h->prm = np;
  fill_dev_params(h);
  set_compute_band(h);
  return ESVO_OK;
}

int esvo_set_stream(esvo_handle h, void* hip_stream) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  std::lock_guard<std::mutex> lp0(h->mu_push[0]), lp1(h->mu_push[1]);  // a pusher may be draining the front stream
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream_l)); HIPCHK(hipStreamSynchronize(h->stream_l1));
  HIPCHK(hipStreamSynchronize(h->stream_b));
  if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
  h->stream = reinterpret_cast<hipStream_t>(hip_stream);
  h->own_stream = false;
  return ESVO_OK;
}

int esvo_synchronize(esvo_handle h) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  const bool poll = h->lat_last;  // latency mode (context.hpp): the caller waits for a tick that ran alone -- polled, not slept
  HIPCHK(esvo_wait_stream(h->stream, poll));
  HIPCHK(esvo_wait_stream(h->stream_l, poll)); HIPCHK(esvo_wait_stream(h->stream_l1, poll));
  HIPCHK(esvo_wait_stream(h->stream_b, poll));
  return ESVO_OK;
}

}  // extern "C"

// sizeof() of every POD of the ABI (binding self-check)
extern "C" void esvo_abi_sizes(size_t out[8]) {
  out[0] = sizeof(esvo_event_t); out[1] = sizeof(esvo_calib_t); out[2] = sizeof(esvo_params_t);
  out[3] = sizeof(esvo_match_t); out[4] = sizeof(esvo_depth_point_t); out[5] = sizeof(esvo_stats_t);
  out[6] = 0; out[7] = ESVO_HIP_ABI_VERSION;
}

// sizeof() of the global cloud's PODs and its default capacity (api_gpc.hip)
extern "C" void esvo_gpc_sizes(size_t out[4]) {
  out[0] = sizeof(esvo_gpc_params_t); out[1] = sizeof(esvo_gpc_stats_t);
  out[2] = 5000000; out[3] = 0;
}

// ---- device self-test: div_by(a, make_recip(b)) == a / b and sqrt_moderate(x) == sqrt(x), bit for bit ----------
#include "fdiv.hpp"
namespace {
__device__ inline unsigned long long sm64(unsigned long long& s) {
  unsigned long long z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__global__ void selftest_div_kernel(unsigned long long n_per_thread, unsigned long long seed, unsigned long long* mismatches) {
  unsigned long long s = seed + 0x1234567ull * (blockIdx.x * blockDim.x + threadIdx.x + 1);
  unsigned long long bad = 0;
  for (unsigned long long i = 0; i < n_per_thread; ++i) {
    const unsigned long long ra = sm64(s), rb = sm64(s);
    // mantissas random; exponents: mostly moderate, sometimes extreme / zero / denormal
    const int mode = (int)(sm64(s) & 15);
    int ea = (int)(ra % 600) - 300 + 1023, eb = (int)(rb % 600) - 300 + 1023;
    if (mode == 0) ea = (int)(ra % 2046) + 1;
    if (mode == 1) eb = (int)(rb % 2046) + 1;
    if (mode == 2) ea = 0;
    if (mode == 3) eb = 0;
    unsigned long long ba = ((unsigned long long)ea << 52) | (ra >> 12);
    unsigned long long bb = ((unsigned long long)eb << 52) | (rb >> 12);
    if (mode == 4) ba = 0;  // a == 0
    if (mode == 5) ba |= 1ull << 63;
    if (mode == 6) bb |= 1ull << 63;
    const double a = __longlong_as_double((long long)ba), b = __longlong_as_double((long long)bb);
    const double q_ref = a / b;
    const double q = esvo::div_by(a, esvo::make_recip(b));
    const bool same = (__double_as_longlong(q) == __double_as_longlong(q_ref)) || (q != q && q_ref != q_ref);
    bad += !same;
    // sqrt_moderate(x) == sqrt(x) for x in [2^-700, 2^700]
    const int es = (int)(sm64(s) % 1400) - 700 + 1023;
    const double xs = __longlong_as_double((long long)(((unsigned long long)es << 52) | (ra >> 12)));
    bad += __double_as_longlong(esvo::sqrt_moderate(xs)) != __double_as_longlong(sqrt(xs));
  }
  if (bad) atomicAdd(mismatches, bad);
}
}  // namespace
namespace {
__global__ void debug_stall_kernel(unsigned long long ref_ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ref_ticks) __builtin_amdgcn_s_sleep(32);
}
}  // namespace
// tools only (tools/regime_probe.py, ESVO_TIMELINE=1): when every stage of the last `max_rows` ticks ran, in ms since esvo_create:
// rows of 12 -- front stage T0, BM0, BM1, S1, LM0, LM1, S2, CNT; back stage FU0, FU1, CL1, RG1 -- collected from the handle's HIP
// events as the ticks completed (no extra synchronisation while the run lasts; this call drains the handle).  Not part of the
// documented ABI.
extern "C" int esvo_debug_timeline(esvo_handle h, float* out, int max_rows, int* n_rows) {
  if (!h || !out || !n_rows) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  int rc = finalize_tick_stats(h);
  if (rc) return rc;
  const size_t n = std::min(h->tl_front.size(), h->tl_back.size());
  const size_t take = std::min<size_t>(n, (size_t)std::max(max_rows, 0));
  for (size_t k = 0; k < take; ++k) {
    const size_t i = n - take + k;
    for (int j = 0; j < 8; ++j) out[k * 12 + j] = h->tl_front[i][j];
    for (int j = 0; j < 4; ++j) out[k * 12 + 8 + j] = h->tl_back[i][j];
  }
  *n_rows = (int)take;
  return ESVO_OK;
}

// tools only (tools/regime_probe.py): occupy one of the handle's queues for `microseconds` with a kernel that does nothing --
// a stage of the tick pipeline falls behind by that much.  which: 0 front (Time Surfaces, block matching), 1 LM, 2 back (fusion,
// regulariser).  Not part of the documented ABI.
extern "C" int esvo_debug_stall(esvo_handle h, int which, unsigned microseconds) {
  if (!h || which < 0 || which > 2) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  const unsigned long long ticks = (unsigned long long)microseconds * (h->stats.clk_ref_khz ? h->stats.clk_ref_khz : 100000u) / 1000ull;
  hipStream_t s = which == 0 ? h->stream : (which == 1 ? h->stream_l : h->stream_b);
  hipLaunchKernelGGL(debug_stall_kernel, dim3(1), dim3(1), 0, s, ticks);
  HIPCHK(hipGetLastError());
  return ESVO_OK;
}

extern "C" int esvo_selftest_division(unsigned long long n, unsigned long long seed, unsigned long long* mismatches) {
  esvo_context* h = nullptr;
  DevBuf<unsigned long long> d;
  HIPCHK(d.alloc(1));
  HIPCHK(hipMemset(d, 0, sizeof(unsigned long long)));
  const unsigned threads = 256, blocks = 1024;
  const unsigned long long per = (n + (unsigned long long)threads * blocks - 1) / ((unsigned long long)threads * blocks);
  hipLaunchKernelGGL(selftest_div_kernel, dim3(blocks), dim3(threads), 0, 0, per, seed, d);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(mismatches, d, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return ESVO_OK;
}
