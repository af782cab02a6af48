// api_modes.hip — the synchronous esvo_MVStereo modes: PURE_BLOCK_MATCHING (1), PURE_SEMI_GLOBAL_MATCHING (4) and the SGM
// initialisation (see context.hpp).
#include "context.hpp"

// ---- esvo_MVStereo's PURE_BLOCK_MATCHING mode (MVStereoMode 1, esvo_MVStereo.cpp:383-432) -------------------------------------
// Event selection + (denoising) + block matching as in every tick; then vEMP2vDP (:1072-1094) instead of the nonlinear
// refinement, a window of maxNumFusionFrames frames whatever the fusion strategy (:419-421), and
// DepthFusion::naive_propagation of every frame, newest first, into a new DepthFrame (:422-423) -- no culling, no clean, no
// regularisation.  Synchronous (a visualisation baseline: nothing is pipelined).
extern "C" int esvo_map_tick_bm_only(esvo_handle h, uint64_t t_ns, const uint64_t* pose_t_ns, const double* pose_T, size_t m) {
  if (!h || !pose_t_ns || !pose_T) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (!h->obs_set) FAIL(ESVO_ERR_STATE, "esvo_map_set_observation has not been called");
  if (h->sharded) FAIL(ESVO_ERR_STATE, "handle is sharded");
  HIPCHK(hipSetDevice(h->device));
  int rc = flush_pending_tick(h);
  if (rc) return rc;
  // phase 0 up to the match list (tick_phase0 also enqueues the LM kernel, which this mode does not run), on the front stream
  if (m > h->max_poses) FAIL(ESVO_ERR_CAPACITY, "pose table larger than max_poses_per_tick");
  u32 n = 0;
  u64 first = 0;
  rc = select_events(h, t_ns, &first, &n);
  if (!rc) rc = upload_poses(h, pose_t_ns, pose_T, m, h->front[h->fpar ^ 1].d_counters);
  if (rc) return rc;
  // This mode keeps maxNumFusionFrames frames of up to PROCESS_EVENT_NUM un-culled matches whatever the fusion strategy, while
  // the window ring is sized for the normal policy (max_window_points): a CONST_POINTS preset with a small point budget and
  // many frames can run out of ring.  Find that out HERE, before any tick state flips: the frame that leaves at this tick
  // leaves first (push_back + pop_front while size > max == pop while size >= max, then push), and the ring must take a
  // frame of n points (n = the selected events bounds the matches).
  // (probed on a COPY of the window: a refused tick, or one that fails further down, has dropped no frame)
  const size_t keep_below = (size_t)std::max(1, h->prm.max_fusion_frames);
  if (window_probe_after_pops(h, keep_below, n) != ESVO_OK)
    FAIL(ESVO_ERR_CAPACITY, "PURE_BLOCK_MATCHING window (maxNumFusionFrames frames of up to PROCESS_EVENT_NUM matches) "
                            "does not fit the fusion window ring: raise max_window_points");
  switch_front_parity(h);
  FrontSlot& F = h->front_cur();
  HIPCHK(hipStreamWaitEvent(h->stream, h->back[h->par].ev.e[BE_RG1], 0));
  hipEventRecord(F.ev->e[FE_T0], h->stream);
  const u32* sel = nullptr;
  if (h->prm.denoising && n) {
    rc = denoise_select(h, n, &n);
    if (rc) return rc;
    sel = h->d_sel;
  }
  u32 n_matches = 0;
  if (n) {
    rc = run_bm(h, h->d_ring[0], h->sh_first, h->ring_cap, 1, n, sel);
    if (rc) return rc;
    rc = run_order_matches(h, n, false);
    if (rc) return rc;
    launch_matches_to_points(F.d_matches, F.d_counters + CNT_MATCHES, n, h->d_pts_tmp, h->dp, h->stream);
    HIPCHK(hipGetLastError());
    rc = read_counters(h);
    if (rc) return rc;
    n_matches = h->h_counters[CNT_MATCHES];
    collect_bm_failures(h, h->h_counters, true);
  }
  esvo_stats_t& s = h->stats;
  s.last_events_in = n; s.last_matches = n_matches; s.last_solved = 0; s.last_points = n_matches;
  s.total_events_in += n; s.total_matches += n_matches; s.total_points += n_matches;
  // dqvDepthPoints_.push_back(vdp_em); while (size > maxNumFusionFrames_) pop_front()
  rc = back_after_front(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream_b));  // the ring space may still be read by a fusion in flight
  rc = commit_naive_frame(h, h->d_pts_tmp, n_matches, nullptr, h->n_pose, h->pose_buf);  // (the probe above guarantees the space)
  if (rc) return rc;
  h->committed_t_ns = t_ns;
  s.ticks++;
  window_stats(h);
  return ESVO_OK;
}

// The stage-wise seam of the same mode: what follows match_all_HyperThread in PURE_BLOCK_MATCHING (esvo_MVStereo.cpp:411-423)
// on matches the caller holds (esvo_map_match gave them): vEMP2vDP, dqvDepthPoints_.push_back + pop to maxNumFusionFrames_,
// naive_propagation of the window (newest first) into a new DepthFrame at the observation's pose.  Synchronous.
extern "C" int esvo_map_fuse_matches_naive(esvo_handle h, const esvo_match_t* matches, size_t n, const double* pose_T, size_t m) {
  if (!h || (n && !matches) || (m && !pose_T)) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (!h->obs_set) FAIL(ESVO_ERR_STATE, "esvo_map_set_observation has not been called");
  if (h->sharded) FAIL(ESVO_ERR_STATE, "handle is sharded");
  if (n > h->max_ev) FAIL(ESVO_ERR_CAPACITY, "more matches than max_events_per_tick");
  if (m > h->max_poses) FAIL(ESVO_ERR_CAPACITY, "pose table larger than max_poses_per_tick");
  for (size_t i = 0; i < n; ++i)
    if (matches[i].pose_idx >= m) FAIL(ESVO_ERR_INVALID_ARG, "match refers to a pose outside the pose table");
  HIPCHK(hipSetDevice(h->device));
  int rc = flush_pending_tick(h);
  if (rc) return rc;
  rc = drain_lm_and_back(h);  // the staging buffers and the ring may still be read by work in flight
  if (rc) return rc;
  const u32 n32 = (u32)n;
  FrontSlot& F = h->front_cur();
  if (n) {
    HIPCHK(hipMemcpyAsync(F.d_matches, matches, sizeof(esvo_match_t) * n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(F.d_counters, &n32, sizeof(u32), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // n32 / matches are borrowed
    launch_matches_to_points(F.d_matches, F.d_counters + CNT_MATCHES, n32, h->d_pts_tmp, h->dp, h->stream);
    HIPCHK(hipGetLastError());
  }
  // the frame that leaves at this call leaves first (its ring space is free: stream_b was drained above) -- probed on a copy
  // of the window, popped for real only when nothing can fail any more before the frame is committed
  rc = window_probe_after_pops(h, (size_t)std::max(1, h->prm.max_fusion_frames), n32);
  if (rc) return rc;
  rc = back_after_front(h);
  if (rc) return rc;
  static const double ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  rc = commit_naive_frame(h, h->d_pts_tmp, n32, m ? pose_T : ident, (u32)m, 0);
  if (rc) return rc;
  h->committed_t_ns = h->obs_t_ns;
  h->stats.last_points = n32;
  window_stats(h);
  return ESVO_OK;
}

namespace esvo_host {
// scratch of the SGM chain and of the SGM modes: allocated on first use, released by esvo_destroy
static int sgm_alloc(esvo_context* h) {
  const size_t npx = (size_t)h->W * h->H;
  if (!h->sgm_ok) {
    const size_t nvol = (size_t)h->H * (h->W - 48) * 48;
    for (auto& b : h->d_sgm_plane) HIPCHK(b.alloc(npx));
    for (auto& b : h->d_sgm_vol) HIPCHK(b.alloc(nvol));
    HIPCHK(h->d_sgm_d1.alloc(npx));
    HIPCHK(h->d_sgm_d1b.alloc(npx));
    HIPCHK(h->d_sgm_d2key.alloc(npx));
    h->sgm = SgmScratch{h->d_sgm_plane[0], h->d_sgm_plane[1], h->d_sgm_plane[2], h->d_sgm_plane[3],
                        {h->d_sgm_vol[0], h->d_sgm_vol[1], h->d_sgm_vol[2], h->d_sgm_vol[3], h->d_sgm_vol[4], h->d_sgm_vol[5]},
                        h->d_sgm_d1, h->d_sgm_d1b, h->d_sgm_d2key};
    HIPCHK(h->d_sgm_img[0].alloc(npx));
    HIPCHK(h->d_sgm_img[1].alloc(npx));
    HIPCHK(h->d_sgm_disp.alloc(npx));
    HIPCHK(h->d_sgm_pair.alloc(8 * (size_t)h->max_ev));
    HIPCHK(h->d_sgm_T.alloc(16));
    for (DevEvent& e : h->evt_sgm) HIPCHK(e.create());
    h->sgm_ok = true;
  }
  return ESVO_OK;
}
// the SGM event selection (esvo_Mapping.cpp:541-551, esvo_MVStereo.cpp:612-625): newest first from lower_bound(t), 2 *
// BM_half_slice_thickness back, at most PROCESS_EVENT_NUM + 1; a refusal changes nothing
static int sgm_select(esvo_context* h, u64* first_out, u32* n_out) {
  u64 first = 0;
  u32 n = 0;
  std::lock_guard<std::mutex> lr(h->mu_ring);
  ingest_fence(h, 0);
  const double t_end = ns_to_sec(h->obs_t_ns);
  const double t_begin = ns_to_sec(ros_time_from_sec(std::max(0.0, t_end - 2 * h->prm.bm_half_slice_thickness)));
  const u64 it_end = lower_bound_sec(h, 0, t_end), it_begin = lower_bound_sec(h, 0, t_begin);
  const u64 staged_end = h->ring_base[0] + h->ts_host[0].size();
  u64 avail = it_end - it_begin;
  first = it_end;
  if (it_end == staged_end && avail > 0) { first = it_end - 1; avail -= 1; }  // end() is skipped (oracle definition)
  n = (u32)std::min<u64>(avail, (u64)h->prm.process_event_num + 1);
  if (n > h->max_ev) FAIL(ESVO_ERR_CAPACITY, "more events than max_events_per_tick");
  if (n && first - (n - 1) < h->ring_reserved[0] - std::min<u64>(h->ring_reserved[0], h->ring_cap))
    FAIL(ESVO_ERR_STATE, "selected events were already overwritten in the event ring");
  if (n) { h->sh_first_prev = h->sh_first; h->sh_first = first; }  // the ingest thread's overwrite guard protects this selection like a tick's
  *first_out = first;
  *n_out = n;
  return ESVO_OK;
}
// the refusals the SGM calls share; W <= 50: the SGM chain matches the columns x >= numDisparities only
static int sgm_mode_checks(esvo_context* h) {
  if (!h->obs_set) FAIL(ESVO_ERR_STATE, "esvo_map_set_observation has not been called (time stamp and pose of the Time-Surface pair)");
  if (h->sharded) FAIL(ESVO_ERR_STATE, "handle is sharded");
  if (h->W <= 48 + 2) FAIL(ESVO_ERR_UNSUPPORTED, "image narrower than numDisparities");
  return ESVO_OK;
}
// the pair the SGM chain reads: a host image staged on the front stream, or (null) the camera's device-resident Time Surface
static int sgm_stage_images(esvo_context* h, const uint8_t* ts_left, const uint8_t* ts_right, const uint8_t* img[2]) {
  const uint8_t* src[2] = {ts_left, ts_right};
  for (int cam = 0; cam < 2; ++cam) {
    if (src[cam]) {
      HIPCHK(hipMemcpyAsync(h->d_sgm_img[cam], src[cam], (size_t)h->W * h->H, hipMemcpyHostToDevice, h->stream));
      img[cam] = h->d_sgm_img[cam];
    } else {
      if (!h->ts_valid[cam]) FAIL(ESVO_ERR_STATE, "no device-resident Time Surface: call esvo_ts_render first");
      img[cam] = h->d_ts[cam];
    }
  }
  return ESVO_OK;
}
}  // namespace esvo_host

// ---- SGM initialisation -----------------------------------------------------------------------
// Replaces esvo_Mapping::InitializationAtTime (esvo_Mapping.cpp:433-492) with the SGM branch of dataTransferring (:537-552):
// cv::StereoSGBM on the UN-smoothed Time-Surface pair, the rectified pixels of the newest <= PROCESS_EVENT_NUM + 1 left
// events of the last 2 * BM_half_slice_thickness as edge mask, one Gaussian DepthPoint (variance 1e-6, age =
// age_vis_threshold) per masked event with a disparity inside the inverse-depth range; if at least min_points
// (INIT_SGM_DP_NUM_THRESHOLD) come out they open the fusion window and DepthFusion::naive_propagation fills the DepthFrame.
extern "C" int esvo_map_init_sgm(esvo_handle h, const uint8_t* ts_left, const uint8_t* ts_right, size_t min_points, size_t* n_points,
                                 int16_t* disp_out) {
  if (!h || !n_points) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  int rc = sgm_mode_checks(h);
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->device));
  rc = flush_pending_tick(h);
  if (rc) return rc;
  const size_t npx = (size_t)h->W * h->H;
  rc = sgm_alloc(h);
  if (rc) return rc;
  const uint8_t* img[2];
  rc = sgm_stage_images(h, ts_left, ts_right, img);
  if (!rc) rc = drain_lm_and_back(h);  // the DepthMap and the window are rebuilt below
  if (rc) return rc;
  launch_sgbm(img[0], img[1], h->sgm, h->d_sgm_disp, h->W, h->H, h->stream);
  HIPCHK(hipGetLastError());
  h->sgm_disp_valid = true;
  // the SGM event selection (esvo_Mapping.cpp:541-551): newest first from lower_bound(t), 2 * BM_half_slice_thickness back
  u64 first = 0;
  u32 n = 0;
  rc = sgm_select(h, &first, &n);
  if (rc) return rc;
  FrontSlot& F = h->front_cur();
  HIPCHK(hipMemsetAsync(F.d_counters, 0, sizeof(u32) * CNT_ROW, h->stream));
  u32 count = 0;
  if (n) {
    HIPCHK(hipStreamWaitEvent(h->stream, h->back[h->par].ev.e[BE_RG1], 0));
    launch_sgm_points(h->d_ring[0], first, h->ring_cap, n, h->d_lut, h->d_sgm_disp, F.d_pt_slots, F.d_pt_flags, h->dp, h->stream);
    launch_exclusive_scan_u32(F.d_pt_flags, F.d_pt_prefix, F.d_counters + CNT_POINTS, h->d_scan_tmp, n, h->stream);
    HIPCHK(hipMemcpyAsync(F.d_counters + CNT_MATCHES, &n, sizeof(u32), hipMemcpyHostToDevice, h->stream));  // compaction bound (n_in of compact_points), behind the memset above
    launch_compact_points(F.d_pt_slots, F.d_pt_flags, F.d_pt_prefix, F.d_counters + CNT_MATCHES, n, h->d_pts_tmp, h->stream);
    rc = read_counters(h);
    if (rc) return rc;
    count = h->h_counters[CNT_POINTS];
  }
  if (disp_out) {
    HIPCHK(hipMemcpyAsync(disp_out, h->d_sgm_disp, npx * sizeof(int16_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  *n_points = 0;
  if (count < min_points) return ESVO_OK;  // InitializationAtTime returns false: nothing is pushed (:482-483)
  u32 off;
  rc = window_reserve(h, count, &off);
  if (rc) return rc;
  rc = back_after_front(h);
  if (rc) return rc;
  if (count) HIPCHK(hipMemcpyAsync(h->d_win + off, h->d_pts_tmp, sizeof(DevPoint) * count, hipMemcpyDeviceToDevice, h->stream_b));
  rc = commit_frame(h, off, count, h->T_world_obs, 1, 0, false);  // dqvDepthPoints_.push_back(vdp_sgm): no window policy (:485)
  if (rc) return rc;
  // DepthFusion::naive_propagation into a new DepthFrame at the observation's pose (:436-440, :486)
  std::memcpy(h->T_world_frame, h->T_world_obs, sizeof(double) * 16);
  double Tfw[16], Tfo[16];
  rigid_inverse(h->T_world_frame, Tfw);
  mat4_mul(Tfw, h->T_world_obs, Tfo);
  HIPCHK(hipMemcpy(h->d_sgm_T, Tfo, sizeof(double) * 16, hipMemcpyHostToDevice));
  launch_sgm_naive(h->d_win + off, count, h->d_sgm_T, h->d_owner_max, h->d_sgm_pair, h->d_sgm_pair + 4 * (size_t)h->max_ev, h->d_cnt_b + CNTB_RECORDS,
                   h->d_scan_tmp_b, h->d_map, h->dp, h->stream_b);
  HIPCHK(hipGetLastError());
  rc = drain_lm_and_back(h);
  if (rc) return rc;
  h->d_map_cur = h->d_map;
  h->map_id_bound = 4u * count;  // (creation ids: ranks of the winning (point, k) pairs, kernels_sgm.hip)
  h->committed_t_ns = h->obs_t_ns;
  h->stats.last_points = count;
  h->stats.last_window_frames = (u32)h->n_window_frames;
  *n_points = count;
  return ESVO_OK;
}

// ---- esvo_MVStereo's PURE_SEMI_GLOBAL_MATCHING mode (MVStereoMode 4, esvo_MVStereo.cpp:311-376) ------------------------------
namespace esvo_host {
// Everything behind sgbm_->compute, on h->d_sgm_disp and the n events ev[(first -/+ k) % cap]: the mode's DepthPoints (:329-353),
// dqvDepthPoints_.push_back + pop to maxNumFusionFrames_ (:357-359), naive_propagation of every frame, newest first, into a new
// DepthFrame at the observation's pose (:360-361).  The caller has drained the other streams and probed the window ring for n points.
static int sgm_frame_and_propagate(esvo_context* h, const esvo_event_t* d_ev, u64 first, u64 cap, int reverse, u32 n, u32* count_out) {
  FrontSlot& F = h->front_cur();
  u32* cnt = F.d_counters + CNT_SCRATCH;  // the mode's four statistics words (common.hpp)
  HIPCHK(hipMemsetAsync(F.d_counters, 0, sizeof(u32) * CNT_ROW, h->stream));
  HIPCHK(hipEventRecord(h->evt_sgm[1], h->stream));
  u32 count = 0;
  esvo_sgm_stats_t& g = h->sgm_stats;
  g.events = n; g.on_image = g.matched_columns = g.disp_ok = g.points = g.zero_disp = 0;
  int rc;
  if (n) {
    launch_sgm_tick_points(d_ev, first, cap, reverse, n, h->d_lut, h->d_sgm_disp, F.d_pt_slots, F.d_pt_flags, cnt, h->dp, h->stream);
    launch_exclusive_scan_u32(F.d_pt_flags, F.d_pt_prefix, F.d_counters + CNT_POINTS, h->d_scan_tmp, n, h->stream);
    HIPCHK(hipMemcpyAsync(F.d_counters + CNT_MATCHES, &n, sizeof(u32), hipMemcpyHostToDevice, h->stream));  // compaction bound (n_in of compact_points), behind the memset above
    launch_compact_points(F.d_pt_slots, F.d_pt_flags, F.d_pt_prefix, F.d_counters + CNT_MATCHES, n, h->d_pts_tmp, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->evt_sgm[2], h->stream));
    rc = read_counters(h);  // the one host read of the tick
    if (rc) return rc;
    count = h->h_counters[CNT_POINTS];
    const u32* gw = h->h_counters + CNT_SCRATCH;
    g.on_image = gw[0]; g.matched_columns = gw[1]; g.disp_ok = gw[2]; g.zero_disp = gw[3];
    g.points = count;
  } else {
    HIPCHK(hipEventRecord(h->evt_sgm[2], h->stream));
  }
  rc = back_after_front(h);
  if (rc) return rc;
  // count <= n, for which the caller probed the ring; dp.updatePose(T_world_cam) of the observation: one pose per frame
  rc = commit_naive_frame(h, h->d_pts_tmp, count, h->T_world_obs, 1, 0);
  if (rc) return rc;
  const bool timed = h->back[h->par ^ 1].timed;  // (the parity that fusion took)
  h->committed_t_ns = h->obs_t_ns;
  g.ms_points = g.ms_propagate = 0.f;
  if (hipEventElapsedTime(&g.ms_points, h->evt_sgm[1], h->evt_sgm[2]) != hipSuccess) (void)hipGetLastError();
  if (timed) g.ms_propagate = h->stats.ms_kernel[4];
  esvo_stats_t& s = h->stats;
  s.last_events_in = n; s.last_matches = 0; s.last_solved = 0; s.last_points = count;
  s.total_events_in += n; s.total_points += count;
  window_stats(h);
  *count_out = count;
  return ESVO_OK;
}
}  // namespace esvo_host

extern "C" int esvo_map_tick_sgm(esvo_handle h, const uint8_t* ts_left, const uint8_t* ts_right, size_t* n_points, int16_t* disp_out) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  int rc = sgm_mode_checks(h);
  if (rc) return rc;
  const uint8_t* src[2] = {ts_left, ts_right};
  for (int cam = 0; cam < 2; ++cam)
    if (!src[cam] && !h->ts_valid[cam]) FAIL(ESVO_ERR_STATE, "no device-resident Time Surface: call esvo_ts_render first");
  HIPCHK(hipSetDevice(h->device));
  rc = flush_pending_tick(h);
  if (rc) return rc;
  rc = sgm_alloc(h);
  if (rc) return rc;
  const u64 sh_first = h->sh_first, sh_first_prev = h->sh_first_prev;
  u64 first = 0;
  u32 n = 0;
  rc = sgm_select(h, &first, &n);
  if (rc) return rc;
  // maxNumFusionFrames frames of up to PROCESS_EVENT_NUM + 1 points whatever the fusion strategy: found out HERE whether the ring
  // takes them (on a copy of the window), before anything changes -- as esvo_map_tick_bm_only does
  if (window_probe_after_pops(h, (size_t)std::max(1, h->prm.max_fusion_frames), n) != ESVO_OK) {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    h->sh_first = sh_first; h->sh_first_prev = sh_first_prev;
    FAIL(ESVO_ERR_CAPACITY, "PURE_SEMI_GLOBAL_MATCHING window (maxNumFusionFrames frames of up to PROCESS_EVENT_NUM + 1 points) "
                            "does not fit the fusion window ring: raise max_window_points");
  }
  const uint8_t* img[2];
  rc = sgm_stage_images(h, ts_left, ts_right, img);  // (cannot refuse: checked above)
  if (!rc) rc = drain_lm_and_back(h);  // the DepthMap and the window are rebuilt below
  if (rc) return rc;
  HIPCHK(hipEventRecord(h->evt_sgm[0], h->stream));
  launch_sgbm(img[0], img[1], h->sgm, h->d_sgm_disp, h->W, h->H, h->stream);
  HIPCHK(hipGetLastError());
  h->sgm_disp_valid = true;
  if (disp_out) HIPCHK(hipMemcpyAsync(disp_out, h->d_sgm_disp, (size_t)h->W * h->H * sizeof(int16_t), hipMemcpyDeviceToHost, h->stream));
  u32 count = 0;
  rc = sgm_frame_and_propagate(h, h->d_ring[0], first, h->ring_cap, 1, n, &count);
  if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }  // (disp_out and the images are borrowed)
  HIPCHK(hipStreamSynchronize(h->stream));  // disp_out / the borrowed images (n == 0: nothing else waited for the front stream)
  h->sgm_stats.ms_sgbm = 0.f;
  if (hipEventElapsedTime(&h->sgm_stats.ms_sgbm, h->evt_sgm[0], h->evt_sgm[1]) != hipSuccess) (void)hipGetLastError();
  h->stats.ticks++;
  if (n_points) *n_points = count;
  return ESVO_OK;
}

extern "C" int esvo_map_push_disparity_frame(esvo_handle h, const int16_t* disp16, const esvo_event_t* ev, size_t n, size_t* n_points) {
  if (!h || (n && !ev)) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  int rc = sgm_mode_checks(h);
  if (rc) return rc;
  if (n > h->max_ev) FAIL(ESVO_ERR_CAPACITY, "more events than max_events_per_tick");
  if (!disp16 && !h->sgm_disp_valid) FAIL(ESVO_ERR_STATE, "no disparity image on the device: hand one in, or call esvo_map_tick_sgm / esvo_map_init_sgm first");
  HIPCHK(hipSetDevice(h->device));
  rc = flush_pending_tick(h);
  if (rc) return rc;
  rc = sgm_alloc(h);
  if (rc) return rc;
  const u32 n32 = (u32)n;
  rc = window_probe_after_pops(h, (size_t)std::max(1, h->prm.max_fusion_frames), n32);
  if (rc) return rc;
  rc = drain_lm_and_back(h);  // the staging buffers and the ring may still be read by work in flight
  if (rc) return rc;
  if (disp16) {
    HIPCHK(hipMemcpyAsync(h->d_sgm_disp, disp16, (size_t)h->W * h->H * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
    h->sgm_disp_valid = true;
  }
  if (n) HIPCHK(hipMemcpyAsync(h->d_tick_ev, ev, sizeof(esvo_event_t) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // disp16 / ev are borrowed
  u32 count = 0;
  rc = sgm_frame_and_propagate(h, h->d_tick_ev, 0, (u64)h->max_ev, 0, n32, &count);
  if (rc) return rc;
  h->sgm_stats.ms_sgbm = 0.f;
  if (n_points) *n_points = count;
  return ESVO_OK;
}

extern "C" int esvo_map_sgm_stats(esvo_handle h, esvo_sgm_stats_t* out) {
  if (!h || !out) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  *out = h->sgm_stats;
  return ESVO_OK;
}

extern "C" void esvo_sgm_sizes(size_t out[4]) {
  out[0] = sizeof(esvo_sgm_stats_t);
  out[1] = 48;
  out[2] = out[3] = 0;
}
