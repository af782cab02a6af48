// api_map.hip — the mapper's tick pipeline: stage launch wrappers, the stage-wise calls, the fused (lazily completed,
// two-stream) tick and its scheduling policies, the device-resident front stage (see context.hpp).
#include "context.hpp"

namespace esvo_host {

// lower_bound over the staged time stamps with the reference's toSec() comparison
// (tools::EventBuffer_lower_bound, utils.h:51-56); returns an absolute index
u64 lower_bound_sec(const esvo_context* h, int cam, double t) {
  const auto& v = h->ts_host[cam];
  size_t lo = 0, hi = v.size();
  while (lo < hi) {
    size_t mid = (lo + hi) / 2;
    if (ns_to_sec(v[mid]) < t) lo = mid + 1; else hi = mid;
  }
  return h->ring_base[cam] + lo;
}
// ros::Time(double)  (TimeBase::fromSec)
u64 ros_time_from_sec(double t) {
  long long sec64 = (long long)std::floor(t);
  u32 sec = (u32)sec64;
  u32 nsec = (u32)std::round((t - sec) * 1e9);
  sec += (nsec / 1000000000ul);
  nsec %= 1000000000ul;
  return (u64)sec * 1000000000ull + nsec;
}

int upload_poses(esvo_context* h, const uint64_t* pose_t_ns, const double* pose_T, size_t m, u32* d_zero_row) {
  if (m > h->max_poses) FAIL(ESVO_ERR_CAPACITY, "pose table larger than max_poses_per_tick");
  // staged through pinned memory (two alternating slots): no host synchronisation on the tick path
  h->pin_slot ^= 1;
  double* pin = h->h_pin + (size_t)h->pin_slot * ((size_t)h->max_poses * 17 + 16);
  double* T = pin;            // [T (16 m) | toSec (m)]: one contiguous upload
  double* sec = pin + 16 * m;
  for (size_t i = 0; i < m; ++i) sec[i] = ns_to_sec(pose_t_ns[i]);
  std::memcpy(T, pose_T, sizeof(double) * 16 * m);
  h->h_pose_T.assign(pose_T, pose_T + 16 * m);
  h->n_pose = (u32)m;
  // the back stage copies the previous table of this buffer into its frame slot: not before that is done
  h->pose_buf ^= 1;
  h->d_pose_T = h->pose[h->pose_buf].d_T;
  HIPCHK(hipStreamWaitEvent(h->stream, h->pose[h->pose_buf].released, 0));
  h->d_pose_sec = h->d_pose_T + 16 * m;
  // d_zero_row: the counter row of the tick that follows, cleared by the same launch
  launch_upload_words(T, h->d_pose_T, sizeof(double) * 17 * m, h->stream, d_zero_row, CNT_ROW);
  return ESVO_OK;
}

// BM over n events starting at absolute ring index `first` (reverse walk) or over d_tick_ev:
// flags + match records in slot (thread-stride) order
int run_bm(esvo_context* h, const esvo_event_t* d_ev, u64 first, u64 cap, int reverse, u32 n, const u32* sel) {
  FrontSlot& F = h->front_cur();
  BmArgs a;
  a.ev = d_ev; a.n = n; a.ev_first = first; a.ev_cap = cap; a.ev_reverse = reverse; a.sel = sel;
  a.tsL = h->d_obs[0]; a.tsR = h->d_obs[1];
  a.lut = h->d_lut; a.mask = h->d_mask;
  a.pose_sec = h->d_pose_sec; a.n_pose = h->n_pose;
  a.out_slots = h->d_match_slots; a.out_flags = h->d_match_flags;
  a.fail_counters = F.d_counters;
  if (h->stage_events_on) hipEventRecord(F.ev->e[FE_BM0], h->stream);
  // a throughput slice: one search per distinct raw pixel (kernels_bm.hip; the lone-tick latency path gains no launch)
  if (h->d_bm_dedupe && n >= h->bm_dedupe_min && n <= h->max_ev && !h->sharded && bm_dedupe_applies(a, h->dp)) {
    u32* owner = h->d_bm_dedupe;
    u32* n_uniq = owner + (size_t)h->W * h->H;
    u32* uniq_w = n_uniq + 4;
    launch_bm_match_dedupe(a, h->dp, owner, uniq_w, n_uniq, uniq_w + h->max_ev, h->stream);
  } else {
    launch_bm_match(a, h->dp, h->stream);
  }
  if (h->stage_events_on) hipEventRecord(F.ev->e[FE_BM1], h->stream);
  HIPCHK(hipGetLastError());
  return ESVO_OK;
}
// stable compaction of the match slots into vEMP order.  Sharded mode: the flags are this rank's own
// ones, the list is its dense local list (count -> CNT_OWN_MATCHES) and slot_of remembers each entry's slot.
// by_index (latency mode): the list as indices into the slots -- d_own_w -- which the wide LM layout reads; no record is copied
int run_order_matches(esvo_context* h, u32 n, bool local, bool by_index) {
  FrontSlot& F = h->front_cur();
  if (scan_compact_is_small(n)) {  // a small tick: one launch (scan.hip)
    by_index = by_index && !local;
    launch_scan_compact_matches_small(h->d_match_flags, h->d_match_prefix, F.d_counters + (local ? CNT_OWN_MATCHES : CNT_MATCHES), n, h->d_match_slots,
                                      by_index ? nullptr : F.d_matches, (local || by_index) ? h->d_own_w : nullptr, h->stream);
  } else {
    launch_exclusive_scan_u32(h->d_match_flags, h->d_match_prefix, F.d_counters + (local ? CNT_OWN_MATCHES : CNT_MATCHES), h->d_scan_tmp, n, h->stream);
    launch_compact_matches(h->d_match_slots, h->d_match_flags, h->d_match_prefix, n, F.d_matches, local ? h->d_own_w : nullptr,
                           h->stream);
  }
  if (h->stage_events_on) hipEventRecord(F.ev->e[FE_S1], h->stream);
  HIPCHK(hipGetLastError());
  return ESVO_OK;
}
int run_match(esvo_context* h, const esvo_event_t* d_ev, u64 first, u64 cap, int reverse, u32 n) {
  int rc = run_bm(h, d_ev, first, cap, reverse, n);
  if (rc) return rc;
  return run_order_matches(h, n, false);
}

// which LM layout the next lazy tick uses (context.hpp: lm_pair_*): -1 not a candidate, else 0 wide / 1 pair
static int lm_pair_policy(esvo_context* h, u32 n_events) {
  if (lm_guard_wanted(h)) return -1;  // the guard has no pair layout (kernels_lm.hip)
  if (n_events == 0 || n_events > esvo::LM_PAIR_MAX_EVENTS || h->prm.ls_norm == ESVO_LSNORM_L2) return -1;
  if (h->lm_pair_forced >= 0) return h->lm_pair_forced;
  const u32 k = h->lm_pair_decisions++;
  if (k < 8u || h->lm_pair_n[0] == 0u || h->lm_pair_n[1] == 0u) return (int)(k & 1u);
  auto recent_min = [&](int mode) {
    float m = 1e30f;
    for (u32 i = 0; i < 4u && i < h->lm_pair_n[mode]; ++i) m = std::min(m, h->lm_pair_ms[mode][i]);
    return m;
  };
  // The samples are FE_LM0..FE_LM1 intervals on the lowest-priority stream: contention with the other stages only ever ADDS
  // time, so the minimum of the recent four is the estimate least touched by it; and the layout in use is left only for one
  // that is 5 % faster by that estimate (hysteresis: two layouts within noise of each other do not alternate run to run).
  if (h->lm_pair_current < 0) h->lm_pair_current = recent_min(1) < recent_min(0) ? 1 : 0;
  else if (recent_min(h->lm_pair_current ^ 1) < 0.95f * recent_min(h->lm_pair_current)) h->lm_pair_current ^= 1;
  return (k % 64u == 63u) ? h->lm_pair_current ^ 1 : h->lm_pair_current;  // (a periodic sample of the other one keeps its estimate fresh)
}
// The processing order of the LM launch that follows (kernels_lm.hip): on the front queue, behind the match compaction of the
// tick -- the count stays on the device.  Launches that do not read an order (wide, pair, dense, band, split) get none (nullptr).
static const u32* run_lm_order(esvo_context* h, u32 max_matches) {
  FrontSlot& F = h->front_cur();
  const bool split = h->d_lm_fvec0 != nullptr && max_matches >= esvo::LM_SPLIT_MIN_EVENTS && !lm_guard_wanted(h);  // (guarded: the ordered launch)
  if (!h->lm_order_on || !h->front[0].d_lm_pix_order || !lm_launch_is_ordered(max_matches, false, false, split, h->dp)) return nullptr;
  u32* order = F.d_lm_pix_order;
  u64* const rows[2] = {h->d_lm_sort_rows[0], h->d_lm_sort_rows[1]};
  launch_lm_pixel_order(F.d_matches, F.d_counters + CNT_MATCHES, max_matches, 0, h->d_obs[0], h->d_obs[1], h->dp, rows, h->d_lm_sort_hist,
                        h->d_scan_tmp, order, h->stream);
  return order;
}
// order: what run_lm_order built for this launch; by_index: the match list is d_own_w (indices into d_match_slots), not d_matches
int run_lm(esvo_context* h, u32 max_matches, int cull, bool dense, hipStream_t st, int pair, const u32* order, bool by_index) {
  FrontSlot& F = h->front_cur();
  if (!st) st = h->stream;
  if (F.gather_guard) {  // a back stage's first launch reads this parity's solver slots (latency mode, tick_phase2): not
    F.gather_guard = false;  // before it is done (an event long complete when ticks are waited for one by one)
    HIPCHK(hipStreamWaitEvent(st, F.ev->e[FE_STG], 0));
  }
  u32* flags = dense ? h->d_lkeep : F.d_pt_flags;  // the kernel writes every flag of its launch range
  LmArgs a;
  a.matches = F.d_matches; a.n_matches = F.d_counters + (dense ? CNT_OWN_MATCHES : CNT_MATCHES); a.max_matches = max_matches;
  a.match_index = nullptr;
  a.order = dense ? nullptr : order;
  if (by_index && !dense) { a.matches = h->d_match_slots; a.match_index = h->d_own_w; }
  a.tsL = h->d_obs[0]; a.tsR = h->d_obs[1];
  a.pose_T = h->d_pose_T; std::memcpy(a.T_world_obs, h->T_world_obs, sizeof(double) * 16);
  a.out_slots = F.d_pt_slots; a.out_flags = flags; a.cull = cull; a.dense = dense ? 1 : 0;
  // the scale-loop guard: a plain handle's launches only (a dense launch is a rank's share); its stripes exist from the first such launch on
  LmGuard guard;
  if (!dense && lm_guard_wanted(h)) {
    if (!F.d_lm_guard) {
      HIPCHK(F.d_lm_guard.alloc((size_t)esvo::LM_GUARD_STRIPES * esvo::LM_GUARD_WORDS));
      HIPCHK(hipMemsetAsync(F.d_lm_guard, 0, sizeof(u32) * esvo::LM_GUARD_STRIPES * esvo::LM_GUARD_WORDS, st));
    }
    guard.stripes = F.d_lm_guard;
    guard.limit = h->prm.lm_scale_pass_limit;
  }
  F.tk.lm_guard = guard.limit != 0;
  const bool split = h->d_lm_fvec0 != nullptr && max_matches >= esvo::LM_SPLIT_MIN_EVENTS && !F.tk.lm_guard;
  a.split_fvec0 = split ? h->d_lm_fvec0 : nullptr; a.split_fnorm0 = h->d_lm_fnorm0; a.split_meta = h->d_lm_meta;
  a.split_order = h->d_lm_order; a.split_hist = h->d_lm_hist;
  a.pair = pair >= 0 ? pair : (h->lm_pair_forced == 1 && max_matches <= esvo::LM_PAIR_MAX_EVENTS ? 1 : 0);
  if (F.tk.lm_guard) a.pair = 0;  // (a forced ESVO_LM_PAIR loses to the guard)
  a.clk = h->clk_probe ? F.d_clk : nullptr;  // (a block per front parity: api_core.hip)
  if (h->routed && dense) { a.halo_viol = F.d_counters + CNT_SCRATCH; a.vy0 = h->oband_y0; a.vy1 = h->oband_y1; }
  const bool timed_lm = h->stage_events_on || F.tk.timed_lm;
  if (timed_lm) hipEventRecord(F.ev->e[FE_LM0], st);
  launch_lm_refine(a, h->dp, F.d_counters + CNT_SOLVED, st, guard);
  // (FE_LM1 is also what the point compaction waits for when it runs on the other LM queue: tick_phase0)
  if (timed_lm || F.tk.cnt_stream != st) hipEventRecord(F.ev->e[FE_LM1], st);
  HIPCHK(hipGetLastError());
  return ESVO_OK;
}
// stable compaction of the solver slots: the culled points go to `dst` in the reference's order
// host_row (latency mode): where the small compaction leaves the tick's counter row itself (TickState::host_row_sent)
int run_order_points(esvo_context* h, u32 max_matches, DevPoint* dst, hipStream_t st, u32* host_row) {
  FrontSlot& F = h->front_cur();
  u32* scratch = (st && st != h->stream) ? F.d_scan_tmp_l : h->d_scan_tmp;  // the LM stage scans beside the next tick's BM
  if (!st) st = h->stream;
  if (F.tk.lm_guard) launch_lm_guard_fold(F.d_lm_guard, F.d_counters, st);  // (before the small compaction copies the row to the host)
  if (scan_compact_is_small(max_matches)) {
    // (the refinement kernel writes a flag for every slot of its launch, 0 beyond the match count: no count to clip to)
    launch_scan_compact_points_small(F.d_pt_flags, F.d_pt_prefix, F.d_counters + CNT_POINTS, max_matches, F.d_pt_slots, dst, st,
                                     F.d_counters, host_row, host_row ? (u32)CNT_ROW : 0u);
    F.tk.host_row_sent = host_row != nullptr;
  } else {
    launch_exclusive_scan_u32(F.d_pt_flags, F.d_pt_prefix, F.d_counters + CNT_POINTS, scratch, max_matches, st);
    launch_compact_points(F.d_pt_slots, F.d_pt_flags, F.d_pt_prefix, F.d_counters + CNT_MATCHES, max_matches, dst, st);
  }
  if (h->stage_events_on) hipEventRecord(F.ev->e[FE_S2], st);
  HIPCHK(hipGetLastError());
  return ESVO_OK;
}
int run_refine(esvo_context* h, u32 max_matches, int cull, DevPoint* dst) {
  HIPCHK(hipMemsetAsync(h->front_cur().d_counters + CNT_SOLVED, 0, sizeof(u32), h->stream));  // n_solved (a tick zeroes all counters at once)
  const u32* order = run_lm_order(h, max_matches);
  int rc = run_lm(h, max_matches, cull, false, nullptr, -1, order);
  if (rc) return rc;
  return run_order_points(h, max_matches, dst);
}

// EventBM's per-reason failure counters (EventBM.h:89) from a counter row read back from the device
void collect_bm_failures(esvo_context* h, const u32* row, bool accumulate) {
  u32 r[3] = {0, 0, 0};
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < CNT_STRIPES; ++i) r[k] += row[CNT_BM_FAIL + k * CNT_STRIPES + i];
  esvo_stats_t& s = h->stats;
  s.last_bm_info_noise_low = r[0]; s.last_bm_coarse_fail = r[1]; s.last_bm_fine_fail = r[2];
  if (accumulate) { s.total_bm_info_noise_low += r[0]; s.total_bm_coarse_fail += r[1]; s.total_bm_fine_fail += r[2]; }
}
bool lm_guard_wanted(const esvo_context* h) {
  return h->prm.lm_scale_pass_limit != 0 && h->prm.ls_norm != ESVO_LSNORM_L2 && !h->sharded && !h->comm;
}
void collect_lm_guard(esvo_context* h, const u32* row, bool guarded) {
  esvo_lm_stats_t& s = h->lm_stats;
  s.last_max_passes_eval = guarded ? row[CNT_LM_MAX_EVAL] : 0;
  s.last_max_passes_match = guarded ? row[CNT_LM_MAX_MATCH] : 0;
  s.last_abandoned = guarded ? row[CNT_LM_ABANDONED] : 0;
  s.last_passes = guarded ? row[CNT_LM_PASSES] : 0;
  s.last_evals = guarded ? row[CNT_LM_EVALS] : 0;
  s.last_shortcut_evals = guarded ? row[CNT_LM_SHORTCUT] : 0;
  s.total_passes += s.last_passes; s.total_evals += s.last_evals; s.total_shortcut_evals += s.last_shortcut_evals;
  s.total_abandoned += s.last_abandoned;
}
int read_counters(esvo_context* h) {
  HIPCHK(hipMemcpyAsync(h->h_counters, h->front_cur().d_counters, sizeof(u32) * CNT_ROW, hipMemcpyDeviceToHost, h->stream));  // (row 0, whatever the parity)
  HIPCHK(hipStreamSynchronize(h->stream));
  return ESVO_OK;
}

// a new observation goes into the OTHER pair of buffers: an LM stage still in flight keeps reading its own
// (the one before that has finished: the call that enqueued it completed its predecessor, context.hpp)
void begin_observation(esvo_context* h) {
  h->obs_par ^= 1;
  h->d_obs[0] = h->d_obs2[h->obs_par][0];
  h->d_obs[1] = h->d_obs2[h->obs_par][1];
  // (observations set twice between two ticks: the pending tick's LM stage reads this very pair -- write behind it)
  if (h->tick_pending && h->front_cur().tk.obs_par == h->obs_par)
    hipStreamWaitEvent(h->stream, h->front_cur().ev->e[FE_CNT], 0);
}
// nothing was rendered into the pair begin_observation switched to: the previous observation stays current
void revert_observation(esvo_context* h) {
  h->obs_par ^= 1;
  h->d_obs[0] = h->d_obs2[h->obs_par][0];
  h->d_obs[1] = h->d_obs2[h->obs_par][1];
}
}  // namespace esvo_host

extern "C" {

// ---- Mapper: stage-wise ---------------------------------------------------------------------------
int esvo_map_set_observation(esvo_handle h, uint64_t t_ns, const uint8_t* ts_left, const uint8_t* ts_right,
                             const double T_world_cam[16]) {
  if (!h || !T_world_cam) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  const size_t npx = (size_t)h->W * h->H;
  const uint8_t* src[2] = {ts_left, ts_right};
  begin_observation(h);
  for (int cam = 0; cam < 2; ++cam) {
    uint8_t* dst = h->prm.smooth_time_surface ? h->d_obs_tmp : h->d_obs[cam];
    if (src[cam]) {
      HIPCHK(hipMemcpyAsync(dst, src[cam], npx, hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
    } else {
      if (!h->ts_valid[cam]) FAIL(ESVO_ERR_STATE, "no device-resident Time Surface: call esvo_ts_render first");
      if (h->prm.smooth_time_surface) dst = h->d_ts[cam];  // the blur reads the resident surface directly
      else HIPCHK(hipMemcpyAsync(dst, h->d_ts[cam], npx, hipMemcpyDeviceToDevice, h->stream));
    }
    // createMatchProblem applies GaussianBlurTS(5) when SmoothTimeSurface (EventBM.cpp:68-72)
    if (h->prm.smooth_time_surface)
      launch_gaussian5(dst, h->d_obs[cam], h->W, h->H, h->stream, h->routed ? h->oband_y0 : 0, h->routed ? h->oband_y1 : -1);
  }
  std::memcpy(h->T_world_obs, T_world_cam, sizeof(double) * 16);  // handed to the LM kernel by value
  h->obs_t_ns = t_ns;
  h->obs_set = true;
  return ESVO_OK;
}

int esvo_map_set_poses(esvo_handle h, const uint64_t* pose_t_ns, const double* pose_T, size_t m) {
  if (!h || (m && (!pose_t_ns || !pose_T))) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  return upload_poses(h, pose_t_ns, pose_T, m);
}

int esvo_map_match(esvo_handle h, const esvo_event_t* ev, size_t n, const uint64_t* pose_t_ns, const double* pose_T,
                   size_t m, esvo_match_t* out, size_t cap, size_t* n_out) {
  if (!h || (n && !ev) || !n_out) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (!h->obs_set) FAIL(ESVO_ERR_STATE, "esvo_map_set_observation has not been called");
  if (n > h->max_ev) FAIL(ESVO_ERR_CAPACITY, "more events than max_events_per_tick");
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  if (pose_t_ns) { int rc = upload_poses(h, pose_t_ns, pose_T, m); if (rc) return rc; }
  FrontSlot& F = h->front_cur();
  *n_out = 0;
  if (n == 0) { HIPCHK(hipMemsetAsync(F.d_counters, 0, sizeof(u32), h->stream)); return ESVO_OK; }
  HIPCHK(hipMemcpyAsync(h->d_tick_ev, ev, sizeof(esvo_event_t) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(F.d_counters + CNT_BM_FAIL, 0, sizeof(u32) * 3 * CNT_STRIPES, h->stream));
  int rc = run_match(h, h->d_tick_ev, 0, (u64)h->max_ev, 0, (u32)n);
  if (rc) return rc;
  rc = read_counters(h);
  if (rc) return rc;
  const u32 nm = h->h_counters[CNT_MATCHES];
  *n_out = nm;
  h->stats.last_events_in = (u32)n;
  h->stats.last_matches = nm;
  collect_bm_failures(h, h->h_counters, false);
  if (out && nm) {
    if (nm > cap) FAIL(ESVO_ERR_CAPACITY, "output array too small for the matches");
    HIPCHK(hipMemcpy(out, F.d_matches, sizeof(esvo_match_t) * nm, hipMemcpyDeviceToHost));
  }
  return ESVO_OK;
}

int esvo_map_refine(esvo_handle h, const esvo_match_t* matches, size_t n, int cull, esvo_depth_point_t* out, size_t cap,
                    size_t* n_out) {
  if (!h || (n && !matches) || !n_out) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (!h->obs_set) FAIL(ESVO_ERR_STATE, "esvo_map_set_observation has not been called");
  if (n > h->max_ev) FAIL(ESVO_ERR_CAPACITY, "more matches than max_events_per_tick");
  for (size_t i = 0; i < n; ++i)
    if (matches[i].pose_idx >= h->n_pose) FAIL(ESVO_ERR_INVALID_ARG, "match refers to a pose outside the pose table");
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  *n_out = 0;
  if (n == 0) return ESVO_OK;
  const u32 n32 = (u32)n;
  HIPCHK(hipMemcpyAsync(h->front_cur().d_matches, matches, sizeof(esvo_match_t) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->front_cur().d_counters, &n32, sizeof(u32), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  int rc = run_refine(h, n32, cull, h->d_pts_tmp);
  if (rc) return rc;
  rc = read_counters(h);
  if (rc) return rc;
  const u32 np = h->h_counters[CNT_POINTS];
  *n_out = np;
  h->stats.last_solved = h->h_counters[CNT_SOLVED];
  h->stats.last_points = np;
  collect_lm_guard(h, h->h_counters, h->front_cur().tk.lm_guard);
  if (out && np) {
    if (np > cap) FAIL(ESVO_ERR_CAPACITY, "output array too small for the depth points");
    HIPCHK(hipMemcpy(out, h->d_pts_tmp, sizeof(esvo_depth_point_t) * np, hipMemcpyDeviceToHost));
  }
  return ESVO_OK;
}

}  // extern "C"

// ---- Mapper: fused tick ---------------------------------------------------------------------------
namespace esvo_host {
// event selection, esvo_Mapping.cpp:562-574 (Appendix A-3): walk back from lower_bound(t_end) to
// lower_bound(t_begin), newest first, at most PROCESS_EVENT_NUM
int select_events(esvo_context* h, uint64_t t_ns, u64* first_out, u32* n_out) {
  std::lock_guard<std::mutex> lr(h->mu_ring);  // the ingest thread appends to ts_host / advances the ring meanwhile
  ingest_fence(h, 0);  // block matching reads the left camera's ring on the front stream
  const double t_end = ns_to_sec(t_ns);
  const u64 t_begin_ns = ros_time_from_sec(std::max(0.0, t_end - 10 * h->prm.bm_half_slice_thickness));
  const double t_begin = ns_to_sec(t_begin_ns);
  u64 it_end = lower_bound_sec(h, 0, t_end);
  const u64 it_begin = lower_bound_sec(h, 0, t_begin);
  const u64 staged_end = h->ring_base[0] + h->ts_host[0].size();
  u64 avail = it_end - it_begin;
  u64 first = it_end;
  if (it_end == staged_end && avail > 0) { first = it_end - 1; avail -= 1; }  // end() is skipped (oracle definition)
  const u32 n = (u32)std::min<u64>(avail, (u64)h->prm.process_event_num);
  if (n > h->max_ev) FAIL(ESVO_ERR_CAPACITY, "more events than max_events_per_tick");
  // (against ring_reserved: a pusher on another thread may be overwriting the slots of its block right now)
  if (n && first - (n - 1) < h->ring_reserved[0] - std::min<u64>(h->ring_reserved[0], h->ring_cap))
    FAIL(ESVO_ERR_STATE, "selected events were already overwritten in the event ring");
  *first_out = first;
  *n_out = n;
  h->sh_first_prev = h->sh_first;  // the previous tick's front stage may still be in flight on the front stream (lazy ticks)
  h->sh_first = first;             // under mu_ring: what the ingest thread's overwrite guard reads
  return ESVO_OK;
}

// Denoising (esvo_Mapping.cpp:282-296): mask from the n selected events, keep those on it, in order (d_sel: their walk positions).
// One extra read-back (the kept count sizes the BM launch); only the small DAVIS configs use it.
int denoise_select(esvo_context* h, u32 n, u32* n_kept) {
  launch_denoise_flags(h->d_ring[0], h->sh_first, h->ring_cap, n, h->d_evmap, h->d_match_flags, h->W, h->H, h->stream);
  launch_exclusive_scan_u32(h->d_match_flags, h->d_match_prefix, h->front_cur().d_counters + CNT_DENOISE_KEPT, h->d_scan_tmp, n, h->stream);
  launch_denoise_select(h->d_match_flags, h->d_match_prefix, n, h->d_sel, h->stream);
  int rc = read_counters(h);
  if (rc) return rc;
  *n_kept = h->h_counters[CNT_DENOISE_KEPT];
  return ESVO_OK;
}

// phase 0 (front stage): poses, event selection, block matching + LM of the events of this handle's shard
int tick_phase0(esvo_context* h, uint64_t t_ns, const uint64_t* pose_t_ns, const double* pose_T, size_t m, FrontOpts opt) {
  // Everything that can refuse the tick (pose table too large, events beyond the capacity or already overwritten in
  // the ring) is checked BEFORE any per-tick state is switched: a refused tick must leave no trace, in particular not in
  // the pose-table double buffer, which the LM stage of a still pending tick reads and whose content the back stage
  // copies into that tick's frame slot.
  if (h->dn_pending) {  // phase 0 called again behind the exchange of the denoising bits (ESVO_AGAIN)
    h->stage_events_on = h->front_cur().tk.timed;
    return routed_denoise_resume(h);
  }
  if (m > h->max_poses) FAIL(ESVO_ERR_CAPACITY, "pose table larger than max_poses_per_tick");
  if (h->routed && h->halo_error)
    FAIL(ESVO_ERR_HALO, "a refinement of an earlier tick read outside the Time-Surface rows some rank renders (stats.halo_violations): "
                        "raise ts_halo_rows or use ESVO_ROUTE_BROADCAST");
  u32 n = 0, n_loc = 0, n_own = 0, g_first = 0;
  u64 first = 0;
  int rc = h->routed ? select_events_routed(h, t_ns, &n, &g_first, &first, &n_loc, &n_own) : select_events(h, t_ns, &first, &n);
  if (rc) return rc;
  // (the counter row of this tick's parity -- last used two ticks ago, collected since -- is cleared with the pose upload)
  rc = upload_poses(h, pose_t_ns, pose_T, m, h->front[h->fpar ^ 1].d_counters);
  if (rc) return rc;
  switch_front_parity(h);
  FrontSlot& F = h->front_cur();
  TickState& tk = F.tk;
  tk.n = n; tk.off = 0; tk.points = 0; tk.t_ns = t_ns;
  tk.n_loc = n_loc; tk.n_own = n_own; tk.g_first = g_first;
  tk.lm_stream = tk.cnt_stream = h->stream;
  tk.lm_pair = -1;
  tk.lm_guard = false;
  // latency mode: nothing of an earlier tick is pending, so this tick has nothing to run beside -- its LM launch stays in the front
  // queue (one cross-queue hand-off less on the path the caller waits for), the host polls for its counters and its end, and its
  // stage timings are sampled, not recorded tick by tick (context.hpp)
  tk.lat = opt.lat && !h->sharded && n && n <= h->lat_max_events;
  tk.gather = tk.lm_two = false;
  // (sampled for every tick that runs alone, whatever its size; a band-sharded tick is waited for phase by phase)
  tk.timed = (opt.lat || h->sharded) ? esvo_stage_timed(h) : true;
  if (opt.pipe && !h->sharded && !h->comm && !h->tl_on && n && n <= h->lat_max_events) {
    // a small tick that overlaps the previous one (esvo_map_tick's lazy path): host-paced -- one tick in pipe_timed_every is timed
    tk.timed = h->pipe_seq % h->pipe_timed_every == 0u;
    h->pipe_seq++;
  }
  tk.timed_lm = tk.timed;
  h->stage_events_on = tk.timed;  // (esvo_map_tick's scope switches it back on)
  tk.obs_par = h->obs_par;
  tk.pose_buf = h->pose_buf; tk.n_pose = h->n_pose;
  std::memcpy(tk.T_world_obs, h->T_world_obs, sizeof(double) * 16);
  // two ticks in flight at most: what this tick's front stage overwrites (ring space of popped frames, the pose
  // table buffer) was last read by the back stage two ticks ago.
  // (For the ordinary tick this device-side wait is only a throttle: the tick writes parity buffers that are released by events of
  // their own -- FE_STG, PoseBuf::released, the collected FE_CNT -- and the host never runs more than two back stages ahead.  Off since
  // round 5: it ties every front stage to the END of a back stage, which is what makes a lagging back chain stay behind -- see
  // pipeline_resync.  Sharded ticks keep it: their frame goes straight into the ring.)
  if (h->sharded) HIPCHK(hipStreamWaitEvent(h->stream, h->back[h->par].ev.e[BE_RG1], 0));
  if (tk.timed) hipEventRecord(F.ev->e[FE_T0], h->stream);
  const u32* sel = nullptr;
  if (h->prm.denoising && n && !h->routed) {
    rc = denoise_select(h, n, &n);
    if (rc) return rc;
    tk.n = n;
    sel = h->d_sel;
  }
  h->xchg_send = h->xchg_recv = nullptr;
  h->xchg_block = 0;
  if (n && !h->sharded) {
    rc = run_bm(h, h->d_ring[0], h->sh_first, h->ring_cap, 1, n, sel);
    if (rc) return rc;
    // latency mode: the compacted match list is not materialised -- the scan leaves the kept slots' indices and the (wide) LM
    // layout reads the block matcher's slots through them (one workgroup copying 48-byte records: 17 us for DSEC's 10 000 slots)
    const bool by_index = tk.lat && scan_compact_is_small(n) && lm_launch_is_wide(n, h->dp);
    rc = run_order_matches(h, n, false, by_index);
    if (rc) return rc;
    const u32* order = run_lm_order(h, n);
    hipStream_t sl = h->stream;
    if (opt.split && !tk.lat) {  // the LM stage on its own stream, behind this tick's matches
      HIPCHK(hipEventRecord(F.ev->e[FE_A1], h->stream));
      // launches in the latency-bound (wide) layout alternate between the two LM queues; the split launch's scratch and
      // the throughput layout (which fills the chip by itself) stay on one
      const bool split_scratch = h->d_lm_fvec0 != nullptr && n >= esvo::LM_SPLIT_MIN_EVENTS;
      if (h->ema_lm_ms > 0.f && h->ema_back_ms > 0.f)
        h->lm_two_on = h->ema_lm_ms > (h->lm_two_on ? 0.7f : 0.9f) * h->ema_back_ms;  // (context.hpp: round 6's thresholds)
      tk.lm_two = (h->lm_queues == 2 || (h->lm_queues == 0 && h->lm_two_on)) && n <= esvo::LM_TWO_QUEUES_MAX_EVENTS && !split_scratch;
      sl = (tk.lm_two && h->fpar) ? h->stream_l1 : h->stream_l;
      HIPCHK(hipStreamWaitEvent(sl, F.ev->e[FE_A1], 0));
    }
    if (h->resync.lm_wait_back) {  // pipeline_resync: this LM launch starts together with the back stage after the newest enqueued one
      h->resync.lm_wait_back = false;
      HIPCHK(hipStreamWaitEvent(sl, h->back[h->par ^ 1].ev.e[BE_RG1], 0));
    }
    tk.lm_stream = tk.cnt_stream = sl;
    // With ONE LM queue, what follows the launch on the device (point compaction, counters) goes to the idle second queue: the
    // next tick's launch -- enqueued before this one has finished -- then follows this one directly instead of waiting out
    // ~40 us of small dependent launches at the head of the stream that paces the pipeline.
    // (only while ticks overlap -- the previous one is still pending: a tick that is waited for gains nothing from it and would pay
    //  one more cross-queue hand-off)
    if (opt.split && !tk.lat && h->tick_pending && (sl == h->stream_l || sl == h->stream_l1) && !tk.lm_two)
      tk.cnt_stream = sl == h->stream_l ? h->stream_l1 : h->stream_l;
    tk.lm_pair = lm_pair_policy(h, n);
    // (the layout policy's feedback is the LM launch time: sampled ticks aside, whenever it explores or tries the other layout)
    if (tk.lm_pair >= 0 && h->lm_pair_forced < 0 && tk.lm_pair != h->lm_pair_current) tk.timed_lm = true;
    rc = run_lm(h, n, 1, false, sl, tk.lm_pair, order, by_index);
    if (rc) return rc;
  } else if (n) {  // the band mode's front stage (api_shard.hip)
    return shard_front(h, tk, n, sel);
  }
  return ESVO_OK;
}
// phase 1a (front stage, enqueue only): the tick's frame (culled points in the reference's order) goes straight
// into the window ring (capacity for the worst case: n points); the counters follow into the pinned row of the
// tick's parity and FE_CNT marks "frame and counters ready"
int tick_phase1_enqueue(esvo_context* h) {
  FrontSlot& F = h->front_cur();
  TickState& tk = F.tk;
  const u32 n = tk.n;
  int rc = ESVO_OK;
  tk.host_row_sent = false;
  if (h->sharded) {  // committed right away: straight into the ring (worst case n points)
    rc = window_reserve(h, n, &tk.off);
    if (rc) return rc;
  }
  h->xchg_send = h->xchg_recv = nullptr;
  h->xchg_block = 0;
  if (n && !h->sharded) {
    // the frame waits in the staging buffer of its parity until the tick is committed and its size is known; the
    // buffer's previous frame (two ticks ago) has been copied into the ring by then
    if (tk.cnt_stream != tk.lm_stream) HIPCHK(hipStreamWaitEvent(tk.cnt_stream, F.ev->e[FE_LM1], 0));
    HIPCHK(hipStreamWaitEvent(tk.cnt_stream, F.ev->e[FE_STG], 0));
    // latency mode: the compaction kernel leaves the counter row in the pinned host row itself (no copy operation behind it)
    u32* host_row = tk.lat ? F.h_counters : nullptr;
    // ... and only scans: the frame stays in the solver slots until the back stage's first launch -- which knows where in the window
    // ring it goes -- compacts it straight into place (one copy of the records instead of two, and that one over the whole grid)
    tk.gather = tk.lat && scan_compact_is_small(n);
    rc = run_order_points(h, n, tk.gather ? nullptr : F.d_stage, tk.cnt_stream, host_row);
    if (rc) return rc;
  } else if (n) {  // the band mode's frame order (api_shard.hip); the frame itself is filled after exchange 2 (tick_phase2)
    rc = shard_order_points(h, tk);
    if (rc) return rc;
  }
  hipStream_t sc = (n && !h->sharded) ? tk.cnt_stream : h->stream;
  if (!tk.host_row_sent)
    HIPCHK(hipMemcpyAsync(F.h_counters, F.d_counters, sizeof(u32) * CNT_ROW, hipMemcpyDeviceToHost, sc));
  HIPCHK(hipEventRecord(F.ev->e[FE_CNT], sc));
  h->tick_pending = true;
  return ESVO_OK;
}
// phase 1b (host): wait for the counters of the tick of parity fp (one small D2H per tick: the window policy
// needs the point count), book-keeping, front-stage timings
int tick_phase1_collect(esvo_context* h, int fp) {
  return collect_front_stats(h, h->front[fp].tk, h->front[fp].h_counters, *h->front[fp].ev);
}
// the same for a front stage whose counters and events live elsewhere --
// the tick-interleaved mode keeps them per own tick, four deep, so that a tick can be collected after the front stage two
// own ticks later has been enqueued on the same parity
int collect_front_stats(esvo_context* h, TickState& tk, const u32* cnt, const FrontEvents& ev) {
  HIPCHK(esvo_wait_event(ev.e[FE_CNT], tk.lat));
  const u32 n = tk.n;
  const u32 n_points = n ? cnt[CNT_POINTS] : 0;
  esvo_stats_t& s = h->stats;
  s.last_events_in = n;
  s.last_matches = cnt[CNT_MATCHES];
  s.last_solved = cnt[CNT_SOLVED];  // sharded: this rank's share
  s.last_points = n_points;
  s.total_events_in += n;
  s.total_matches += cnt[CNT_MATCHES];
  s.total_points += n_points;
  collect_bm_failures(h, cnt, true);
  collect_lm_guard(h, cnt, n && tk.lm_guard);
  tk.points = n_points;
  if (tk.timed) {
    s.ms_bm = s.ms_refine = 0;
    s.ms_kernel[2] = s.ms_kernel[3] = 0;
  }
  if (n && !tk.timed && tk.timed_lm && tk.lm_pair >= 0) {  // an unsampled tick whose LM launch was timed for the layout policy alone
    float lm = 0.f;
    if (hipEventElapsedTime(&lm, ev.e[FE_LM0], ev.e[FE_LM1]) == hipSuccess && lm > 0.f) {
      h->lm_pair_ms[tk.lm_pair][h->lm_pair_n[tk.lm_pair] & 3u] = lm;
      h->lm_pair_n[tk.lm_pair]++;
    } else {
      (void)hipGetLastError();
    }
  }
  if (n && tk.timed) {
    s.stage_timing_samples++;
    hipEventElapsedTime(&s.ms_bm, ev.e[FE_T0], ev.e[FE_S1]);
    hipEventElapsedTime(&s.ms_refine, ev.e[FE_S1], ev.e[FE_S2]);
    hipEventElapsedTime(&s.ms_kernel[2], ev.e[FE_BM0], ev.e[FE_BM1]);
    hipEventElapsedTime(&s.ms_kernel[3], ev.e[FE_LM0], ev.e[FE_LM1]);
    s.sum_ms_kernel[2] += s.ms_kernel[2];
    s.sum_ms_kernel[3] += s.ms_kernel[3];
    h->ema_lm_ms = h->ema_lm_ms > 0.f ? 0.75f * h->ema_lm_ms + 0.25f * s.ms_kernel[3] : s.ms_kernel[3];
    if (tk.lm_pair >= 0 && s.ms_kernel[3] > 0.f) {  // feedback for lm_pair_policy
      h->lm_pair_ms[tk.lm_pair][h->lm_pair_n[tk.lm_pair] & 3u] = s.ms_kernel[3];  // ring of the last four
      h->lm_pair_n[tk.lm_pair]++;
    }
  }
  if (h->tl_on && h->tl_ref && n && tk.timed) {
    std::array<float, 8> row;  // FE_T0 .. FE_CNT
    for (int i = 0; i < 8; ++i) { row[i] = -1.f; if (hipEventElapsedTime(&row[i], h->tl_ref, ev.e[i]) != hipSuccess) (void)hipGetLastError(); }
    h->tl_front.push_back(row);
  }
  tk.max_kept = (h->sharded && n) ? cnt[CNT_MAX_KEPT] : 0;
  // exchange 2: [count | kept points], block length from the largest kept count among the ranks.  Routed band mode: the count
  // word also carries the rank's halo violations, so the exchange takes place whenever the tick had events -- a tick whose
  // violating matches were all culled (no kept point anywhere) still reports them (n is the global selection: every rank agrees)
  if (h->sharded && (n_points || (h->routed && n))) {
    h->xchg_send = h->d_pts_send;
    h->xchg_recv = h->dp.ev_nshards > 1 ? h->d_pts_all : h->d_pts_send;
    h->xchg_block = 8 + (size_t)tk.max_kept * sizeof(DevPoint);
  }
  return ESVO_OK;
}
// The tick pipeline has two stable operating points (profiles/r05_regime_timeline.txt: the stage times of both).  Normally LM
// launches run back to back and a tick's back stage (fusion 0.6 ms, then the regulariser) starts the moment its frame is ready,
// i.e. together with the NEXT LM launch: the regulariser runs beside that launch's draining tail (0.6-0.7 ms) and the back chain
// (1.25-1.3 ms) keeps pace with the LM chain (1.27-1.3).  If the back chain ever falls behind by a few milliseconds (a stall of
// its queue does it on demand; a hiccup did it in 2 of 25 sustained runs of round 4) it stays behind: the host, which may not run
// more than two back stages ahead, then issues every front stage when a back stage ENDS, so each LM launch begins ~0.4 ms into a
// fusion stage and the regulariser spends its whole launch beside the LM kernel at full occupancy -- 1.03 instead of 0.69 ms --
// which makes the back chain 1.6 ms per tick: the pace-setter, for good.
// The way back: when the symptom shows (the tick period well above the LM launch time while the back stage fills the period, three
// ticks running) the NEXT LM launch is made to wait, once, for the end of the newest enqueued back stage.  The following back
// stage and that LM launch then start together -- the fast state's alignment, one tick of lag further back, which the window
// policy does not care about.  A workload whose back chain is the slower one by nature (a reference-faithful DSEC tick) shows the
// same symptom; there the wait buys nothing, which the period after it shows, and the attempt is not repeated for 5000 ticks.
static int pipeline_resync(esvo_context* h, float wait_ms, double now_ms) {
  (void)wait_ms;
  esvo_context::Resync& r = h->resync;
  if (r.last_ms > 0.0) { const float dt = (float)(now_ms - r.last_ms); r.period_ema = r.period_ema > 0.f ? 0.8f * r.period_ema + 0.2f * dt : dt; }
  r.last_ms = now_ms;
  if (r.check_in > 0 && --r.check_in == 0)   // did the last attempt shorten the tick?  if not, the back chain IS the pace: stop trying
    r.cooldown = (r.period_ema > 0.93f * r.period_before) ? 5000u : 50u;
  if (r.cooldown > 0) { --r.cooldown; r.streak = 0; return ESVO_OK; }
  if (r.check_in > 0) return ESVO_OK;
  const bool symptom = h->ema_lm_ms > 0.f && h->ema_back_ms > 0.f && r.period_ema > 1.2f * (h->ema_lm_ms + 0.05f) &&
                       h->ema_back_ms > 0.85f * r.period_ema;
  r.streak = symptom ? r.streak + 1 : 0;
  if (r.streak < 3) return ESVO_OK;
  r.streak = 0;
  r.period_before = r.period_ema;
  r.check_in = 24;
  r.lm_wait_back = true;   // consumed by the next tick_phase0
  h->stats.pipeline_resyncs++;
  return ESVO_OK;
}
// phase 2 (back stage): window policy, fusion + clean + regularisation of this band (halo rows recomputed locally),
// enqueued on the back stream behind the frame of the tick of parity fp.  Nothing here waits for the GPU except for
// the back stage of two ticks ago (long finished), whose pinned table and event set are reused; its timings are
// collected then.
int tick_phase2(esvo_context* h, int fp) {
  FrontSlot& F = h->front[fp];
  TickState& tk = F.tk;
  h->xchg_send = h->xchg_recv = nullptr;
  h->xchg_block = 0;
  if (h->sharded) {  // the band mode's frame out of exchange 2, the back stream behind it (api_shard.hip)
    int rc = shard_scatter_frame(h, tk);
    if (rc) return rc;
  } else {
    HIPCHK(hipStreamWaitEvent(h->stream_b, F.ev->e[FE_CNT], 0));
  }
  const int par = h->par;
  h->par ^= 1;
  const auto t_wait0 = std::chrono::steady_clock::now();
  HIPCHK(hipEventSynchronize(h->back[par].ev.e[BE_RG1]));
  if (!h->sharded) {
    const auto t_wait1 = std::chrono::steady_clock::now();
    int rcr = pipeline_resync(h, std::chrono::duration<float, std::milli>(t_wait1 - t_wait0).count(),
                              std::chrono::duration<double, std::milli>(t_wait1.time_since_epoch()).count());
    if (rcr) return rcr;
  }
  collect_back(h, par);
  int rc;
  if (!h->sharded) {  // now that the size is known: exact ring space, frame copied behind the fusion that may still read it
    rc = window_reserve(h, tk.points, &tk.off);
    if (rc) return rc;
    if (tk.lat) {  // the copy rides on run_fuse's first launch (context.hpp, DeferredCopies)
      h->pro = esvo_context::DeferredCopies();
      h->pro.active = true;
      h->pro.a_src = F.d_stage; h->pro.a_dst = h->d_win + tk.off; h->pro.a_bytes = sizeof(DevPoint) * tk.points;
      h->pro.ev_a = F.ev->e[FE_STG];
      if (tk.gather && tk.points) {
        h->pro.a_src = F.d_pt_slots; h->pro.a_flags = F.d_pt_flags; h->pro.a_prefix = F.d_pt_prefix; h->pro.a_slots = tk.n;
        F.gather_guard = true;  // the next LM launch of this parity waits for FE_STG (tick_phase0)
      }
    } else {
      if (tk.points)
        HIPCHK(hipMemcpyAsync(h->d_win + tk.off, F.d_stage, sizeof(DevPoint) * tk.points, hipMemcpyDeviceToDevice, h->stream_b));
      HIPCHK(hipEventRecord(F.ev->e[FE_STG], h->stream_b));
    }
  }
  rc = commit_frame(h, tk.off, tk.points, nullptr, tk.n_pose, tk.pose_buf);
  if (rc) { (void)flush_deferred_copies(h); return rc; }
  {
    StageEventsScope timed_scope(h, tk.timed);
    rc = run_fuse(h, par, tk.T_world_obs);
  }
  if (rc) { (void)flush_deferred_copies(h); return rc; }
  h->stats.ticks++;
  if (h->sharded) h->lat_ticks++;
  window_stats(h);
  h->stats_pending = true;
  h->tick_pending = false;
  h->committed_t_ns = tk.t_ns;
  return ESVO_OK;
}
// complete the tick whose front stage is enqueued but which is not committed yet (unsharded ticks are lazy)
int flush_pending_tick(esvo_context* h) {
  if (!h->tick_pending || h->sharded) return ESVO_OK;
  const int fp = h->fpar;
  h->tick_pending = false;  // also when completing it fails (e.g. window ring full): the error is reported once
  int rc = tick_phase1_collect(h, fp);
  if (rc) return rc;
  return tick_phase2(h, fp);
}
// drain the back stream and collect what is pending (older parity first)
int finalize_tick_stats(esvo_context* h) {
  int rcf = flush_pending_tick(h);
  if (rcf) return rcf;
  if (!h->stats_pending && !h->back_pending[0] && !h->back_pending[1]) return ESVO_OK;
  const bool tick_done = h->stats_pending;
  h->stats_pending = false;
  const bool poll = h->lat_last;  // the newest tick ran in latency mode: somebody is waiting for exactly this
  HIPCHK(esvo_wait_stream(h->stream, poll));
  HIPCHK(esvo_wait_stream(h->stream_l, poll)); HIPCHK(esvo_wait_stream(h->stream_l1, poll));
  HIPCHK(esvo_wait_stream(h->stream_b, poll));
  collect_ts_timing(h);
  collect_back(h, h->par);
  collect_back(h, h->par ^ 1);
  if (tick_done && h->front_cur().tk.timed && h->back[h->par ^ 1].timed) hipEventElapsedTime(&h->stats.ms_tick_total, h->front_cur().ev->e[FE_T0], h->back[h->par ^ 1].ev.e[BE_RG1]);
  return ESVO_OK;
}
}  // namespace esvo_host

extern "C" int esvo_map_tick_resident(esvo_handle h, uint64_t t_ns, const double T_world_cam[16], const uint64_t* pose_t_ns,
                                      const double* pose_T, size_t m) {
  if (!h || !T_world_cam || !pose_t_ns || !pose_T) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  // = esvo_ts_render x2 + esvo_map_set_observation + esvo_map_tick with both cameras in one launch per kernel; an
  // un-smoothed observation is written by the remap itself (no device-to-device copies)
  begin_observation(h);
  uint8_t* obs[2] = {h->d_obs[0], h->d_obs[1]};
  int rc = ts_render_pair(h, t_ns, h->prm.smooth_time_surface ? nullptr : obs);
  if (rc) { revert_observation(h); return rc; }
  if (h->prm.smooth_time_surface)  // createMatchProblem applies GaussianBlurTS(5) when SmoothTimeSurface (EventBM.cpp:68-72)
    launch_gaussian5_pair(h->d_ts[0], h->d_ts[1], h->d_obs[0], h->d_obs[1], h->W, h->H, h->stream, h->routed ? h->oband_y0 : 0,
                          h->routed ? h->oband_y1 : -1);
  HIPCHK(hipGetLastError());
  std::memcpy(h->T_world_obs, T_world_cam, sizeof(double) * 16);
  h->obs_t_ns = t_ns;
  h->obs_set = true;
  return esvo_map_tick(h, t_ns, pose_t_ns, pose_T, m);
}

extern "C" int esvo_map_tick(esvo_handle h, uint64_t t_ns, const uint64_t* pose_t_ns, const double* pose_T, size_t m) {
  if (!h || !pose_t_ns || !pose_T) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (!h->obs_set) FAIL(ESVO_ERR_STATE, "esvo_map_set_observation has not been called");
  if (h->sharded) FAIL(ESVO_ERR_STATE, "handle is sharded: drive it with esvo_shard_tick_phase");
  HIPCHK(hipSetDevice(h->device));
  // the previous tick (if still pending) is completed AFTER this tick's front stage is enqueued: its point count
  // arrived long ago, and the front stream never runs dry while the host works
  if (h->prm.denoising) {  // its kept-event count is read back inside phase 0: no point in deferring anything
    int rcp = flush_pending_tick(h);
    if (rcp) return rcp;
  }
  const bool prev = h->tick_pending;
  const int prev_fp = h->fpar;
  // only the lazy tick path splits; latency mode when the tick runs alone, host-paced sampling when it overlaps the previous one
  int rc = tick_phase0(h, t_ns, pose_t_ns, pose_T, m, FrontOpts{!h->prm.denoising, h->lat_mode && !prev, h->lat_mode && prev});
  if (!rc) rc = tick_phase1_enqueue(h);
  h->stage_events_on = true;
  if (!rc) {
    h->lat_last = h->front_cur().tk.lat;
    if (!prev) h->lat_ticks++;
  }
  if (rc) {  // the failed tick leaves no trace: the previous one (if pending) stays pending on ITS parity and is
    h->fpar = prev_fp;  // completed -- with its own counters and staging buffer -- by the next call that needs it
    return rc;
  }
  if (prev) {
    rc = tick_phase1_collect(h, prev_fp);
    if (!rc) rc = tick_phase2(h, prev_fp);
    h->tick_pending = true;  // this tick (its front stage is enqueued whatever happened to the previous one)
    if (rc) return rc;
  }
  return ESVO_OK;
}

// ---- device-resident stage calls: the building blocks of tick-interleaved multi-GPU operation ---------------------
// (rank r maps the ticks k with k % N == r completely; a tick needs nothing from the previous DepthMaps -- the
// DepthFrame is rebuilt from the window at every tick, esvo_Mapping.cpp:266-272 -- only the frames of the last
// ticks, which the ranks all-gather; see esvo_amd/dist.py)
extern "C" int esvo_map_front(esvo_handle h, uint64_t t_ns, const uint64_t* pose_t_ns, const double* pose_T, size_t m,
                              size_t* n_points) {
  if (!h || !pose_t_ns || !pose_T || !n_points) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (!h->obs_set) FAIL(ESVO_ERR_STATE, "esvo_map_set_observation has not been called");
  if (h->sharded) FAIL(ESVO_ERR_STATE, "handle is sharded by slot/band: esvo_map_front maps whole ticks");
  HIPCHK(hipSetDevice(h->device));
  int rc = flush_pending_tick(h);
  if (rc) return rc;
  rc = tick_phase0(h, t_ns, pose_t_ns, pose_T, m);
  if (rc) return rc;
  FrontSlot& F = h->front_cur();
  const u32 n = F.tk.n;
  if (n) { rc = run_order_points(h, n, h->d_pts_tmp); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(F.h_counters, F.d_counters, sizeof(u32) * CNT_ROW, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipEventRecord(F.ev->e[FE_CNT], h->stream));
  rc = tick_phase1_collect(h, h->fpar);
  if (rc) return rc;
  *n_points = F.tk.points;
  return ESVO_OK;
}

extern "C" int esvo_map_front_frame(esvo_handle h, const esvo_depth_point_t** d_frame) {
  if (!h || !d_frame) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  *d_frame = h->d_pts_tmp;
  return ESVO_OK;
}
