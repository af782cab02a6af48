// api_window.hip — the fusion window (ring, pose slots, window policy) and the back stage: fusion + clean + regularisation
// on the back stream, its counters, the map export (see context.hpp).
#include "context.hpp"

namespace esvo_host {

// back-stage counters into row `row` of the pinned table (CNTB_ROW_*)
static int read_counters_b(esvo_context* h, int row, bool sync) {
  HIPCHK(hipMemcpyAsync(h->h_cnt_b + CNTB_ROW * row, h->d_cnt_b, sizeof(u32) * CNTB_ROW, hipMemcpyDeviceToHost, h->stream_b));
  if (sync) HIPCHK(hipStreamSynchronize(h->stream_b));
  return ESVO_OK;
}
// the back stage starts when everything enqueued on the front stream so far is done
int back_after_front(esvo_context* h) {
  HIPCHK(hipEventRecord(h->ev_frame, h->stream));
  HIPCHK(hipStreamWaitEvent(h->stream_b, h->ev_frame, 0));
  return ESVO_OK;
}
// timings and counters of a finished back stage
void collect_back(esvo_context* h, int par) {
  if (!h->back_pending[par]) return;
  h->back_pending[par] = false;
  const BackSlot& B = h->back[par];
  esvo_stats_t& s = h->stats;
  s.last_fusions = B.h_cnt[CNTB_FUSIONS];
  if (h->routed && h->h_cnt_b[CNTB_ROW * CNTB_ROW_HALO + par]) {  // (the running total over all ranks: identical on every rank at this point of the call sequence)
    s.halo_violations = h->h_cnt_b[CNTB_ROW * CNTB_ROW_HALO + par];
    h->halo_error = true;
  }
  if (h->prm.regularization) s.last_map_size = B.h_cnt[CNTB_REG_ELEMS];  // alive cells of the band (exports refresh it)
  if (!B.timed) return;  // latency mode: this back stage's timings were not sampled (context.hpp, lat_ticks)
  float fu = 0, cl = 0, rg = 0;
  hipEventElapsedTime(&fu, B.ev.e[BE_FU0], B.ev.e[BE_FU1]);
  hipEventElapsedTime(&cl, B.ev.e[BE_FU1], B.ev.e[BE_CL1]);
  hipEventElapsedTime(&rg, B.ev.e[BE_CL1], B.ev.e[BE_RG1]);
  s.ms_fusion = fu + cl;
  s.ms_regularization = rg;
  s.ms_kernel[4] = fu; s.ms_kernel[5] = cl; s.ms_kernel[6] = rg;
  s.sum_ms_kernel[4] += fu; s.sum_ms_kernel[5] += cl; s.sum_ms_kernel[6] += rg;
  h->ema_back_ms = h->ema_back_ms > 0.f ? 0.75f * h->ema_back_ms + 0.25f * (fu + cl + rg) : fu + cl + rg;
  if (h->tl_on && h->tl_ref) {
    std::array<float, 4> row;  // BE_FU0 .. BE_RG1
    for (int i = 0; i < 4; ++i) { row[i] = -1.f; if (hipEventElapsedTime(&row[i], h->tl_ref, B.ev.e[i]) != hipSuccess) (void)hipGetLastError(); }
    h->tl_back.push_back(row);
  }
}

// place a frame of n points in the window ring (frames stay contiguous: [oldest frame, newest frame) modulo the wrap)
// (`frames`: the window to place it behind -- the handle's own, or a copy on which a caller has already dropped the frames that
// will leave, to learn whether a frame fits BEFORE it changes anything)
static int window_reserve_in(esvo_context* h, const std::deque<FrameRec>& frames, u32 n, u32* off_out) {
  u32 off = 0;
  const FrameRec* first = nullptr;  // oldest and newest frames that occupy ring space (empty frames hold none)
  const FrameRec* last = nullptr;
  for (const FrameRec& f : frames)
    if (f.count) { if (!first) first = &f; last = &f; }
  if (first) {
    const FrameRec& back = *last;
    const FrameRec& front = *first;
    const u32 tail = back.off + back.count;
    if (back.off >= front.off) {  // not wrapped: [front.off, tail)
      if (tail + n <= h->win_cap) off = tail;
      else if (n <= front.off) off = 0;
      else FAIL(ESVO_ERR_CAPACITY, "fusion window ring full (raise max_window_points)");
    } else {  // wrapped: free space is [tail, front.off)
      if (tail + n <= front.off) off = tail;
      else FAIL(ESVO_ERR_CAPACITY, "fusion window ring full (raise max_window_points)");
    }
  } else if (n > h->win_cap) {
    FAIL(ESVO_ERR_CAPACITY, "frame larger than the fusion window ring");
  }
  *off_out = off;
  return ESVO_OK;
}
int window_reserve(esvo_context* h, u32 n, u32* off_out) { return window_reserve_in(h, h->frames, n, off_out); }
// would a frame of n points fit once the window has been cut down to fewer than `keep_below` frames (the pops themselves are
// left to the caller, after its last fallible step)?
int window_probe_after_pops(esvo_context* h, size_t keep_below, u32 n) {
  std::deque<FrameRec> fr = h->frames;
  size_t nwf = h->n_window_frames;
  while (nwf && nwf >= keep_below) {
    nwf--;
    if (fr.front().run > 1) fr.front().run--; else fr.pop_front();
  }
  u32 off;
  return window_reserve_in(h, fr, n, &off);
}
static int alloc_pose_slot(esvo_context* h, u32* slot) {
  for (u32 i = 0; i < h->n_pose_slots; ++i)
    if (!h->slot_used[i]) { h->slot_used[i] = 1; *slot = i; return ESVO_OK; }
  // every allocated slot holds a frame of the window: double the table (a rare, synchronising step; kernels take the pointer
  // at launch, so nothing in flight may still read the old one)
  const u32 cap = h->max_frames + 1;
  if (h->n_pose_slots >= cap) FAIL(ESVO_ERR_CAPACITY, "no free pose-table slot (too many frames in the fusion window)");
  const u32 n_new = (u32)std::min<u64>(cap, 2ull * h->n_pose_slots);
  HIPCHK(hipStreamSynchronize(h->stream));
  int rc = drain_lm_and_back(h);
  if (rc) return rc;
  DevBuf<double> d_new;
  const size_t per = (size_t)h->max_poses * 16;
  if (d_new.alloc(per * n_new) != hipSuccess) {
    (void)hipGetLastError();
    FAIL(ESVO_ERR_CAPACITY, "out of device memory growing the pose-table slots");
  }
  if (hipMemcpy(d_new, h->d_frame_pose_T, sizeof(double) * per * h->n_pose_slots, hipMemcpyDeviceToDevice) != hipSuccess) {
    (void)hipGetLastError();  // (d_new goes with this scope: the old table stays in place and in use)
    FAIL(ESVO_ERR_HIP, "copying the pose-table slots into the grown table failed");
  }
  std::swap(d_new, h->d_frame_pose_T);  // the copy succeeded: from here on the handle owns the new table whatever the free says
  HIPCHK(d_new.release());
  *slot = h->n_pose_slots;
  h->slot_used[*slot] = 1;
  h->n_pose_slots = n_new;
  return ESVO_OK;
}
static void pop_front_frame(esvo_context* h) {
  FrameRec& f = h->frames.front();
  h->n_window_frames--;
  if (f.run > 1) { f.run--; return; }
  if (f.slot != NO_SLOT) h->slot_used[f.slot] = 0;
  h->frames.pop_front();
}
// window policy, esvo_Mapping.cpp:341-368
static void apply_window_policy(esvo_context* h) {
  if (h->prm.fusion_strategy == ESVO_FUSION_CONST_POINTS) {
    auto total = [&]() { size_t s = 0; for (auto& f : h->frames) s += f.count; return s; };
    size_t np = total();
    while ((double)np > 1.5 * (double)h->prm.max_fusion_points) { pop_front_frame(h); np = total(); }
  } else {
    while (h->n_window_frames > (size_t)h->prm.max_fusion_frames) pop_front_frame(h);
  }
}

// latency mode (context.hpp, DeferredCopies): the copies a tick's back stage opens with, if run_fuse did not get to carry them in
// its first launch (an error on the way), are enqueued the plain way -- the events behind them release buffers the next ticks wait for
int flush_deferred_copies(esvo_context* h) {
  esvo_context::DeferredCopies d = h->pro;
  h->pro = esvo_context::DeferredCopies();
  if (!d.active) return ESVO_OK;
  if (d.a_flags) launch_back_prologue(nullptr, nullptr, 0, d.a_src, d.a_dst, d.a_bytes, nullptr, nullptr, 0, h->stream_b, d.a_flags, d.a_prefix, d.a_slots);
  else if (d.a_bytes) HIPCHK(hipMemcpyAsync(d.a_dst, d.a_src, d.a_bytes, hipMemcpyDeviceToDevice, h->stream_b));
  if (d.ev_a) HIPCHK(hipEventRecord(d.ev_a, h->stream_b));
  if (d.b_bytes) HIPCHK(hipMemcpyAsync(d.b_dst, d.b_src, d.b_bytes, hipMemcpyDeviceToDevice, h->stream_b));
  if (d.ev_b) HIPCHK(hipEventRecord(d.ev_b, h->stream_b));
  return ESVO_OK;
}
// pose table of the frame: from the host (stage-wise API) or, in a tick, the front stage's device table
int commit_frame(esvo_context* h, u32 off, u32 count, const double* pose_T_host, u32 m, int pose_buf, bool apply_policy) {
  if (count == 0) {  // an empty frame: no pose table, no ring space; consecutive ones share a record
    if (!h->frames.empty() && h->frames.back().count == 0) h->frames.back().run++;
    else h->frames.push_back(FrameRec{off, 0, NO_SLOT, 1});
    h->n_window_frames++;
    if (apply_policy) apply_window_policy(h);
    return ESVO_OK;
  }
  u32 slot;
  int rc = alloc_pose_slot(h, &slot);  // before the frame enters the deque: a failure leaves the window as it was
  if (rc) return rc;
  if (m) {
    double* dst = h->d_frame_pose_T + (size_t)slot * h->max_poses * 16;
    if (pose_T_host) {  // through a pinned slot: an async copy from pageable memory would stall the host behind the stream
      const int ps = h->pool_next;
      h->pool_next = (ps + 1) % esvo_context::POSE_POOL;
      HIPCHK(hipEventSynchronize(h->pool_evt[ps]));
      double* pin = h->h_pose_pool + (size_t)ps * h->max_poses * 16;
      std::memcpy(pin, pose_T_host, sizeof(double) * 16 * m);
      HIPCHK(hipMemcpyAsync(dst, pin, sizeof(double) * 16 * m, hipMemcpyHostToDevice, h->stream_b));
      HIPCHK(hipEventRecord(h->pool_evt[ps], h->stream_b));
    } else if (h->pro.active) {  // latency mode: carried by run_fuse's first launch
      h->pro.b_src = h->pose[pose_buf].d_T; h->pro.b_dst = dst; h->pro.b_bytes = sizeof(double) * 16 * m;
      h->pro.ev_b = h->pose[pose_buf].released;
    } else {
      HIPCHK(hipMemcpyAsync(dst, h->pose[pose_buf].d_T, sizeof(double) * 16 * m, hipMemcpyDeviceToDevice, h->stream_b));
      HIPCHK(hipEventRecord(h->pose[pose_buf].released, h->stream_b));
    }
  }
  h->frames.push_back(FrameRec{off, count, slot, 1});
  h->n_window_frames++;
  if (apply_policy) apply_window_policy(h);
  return ESVO_OK;
}

// fusion loop + clean + regularisation on the current window, on the back stream; `par` selects the
// pinned frame table and the event set (two ticks may be in flight)
int run_fuse(esvo_context* h, int par, const double* T_world_obs, bool naive) {
  // frames newest -> oldest (esvo_Mapping.cpp:372-377)
  // The table is laid out COMPACTLY for the frames in use -- [cum (nf + 1) | off (nf) | slot (nf)] -- so that one small
  // upload carries it (max_frames is sized for the worst case of CONST_POINTS, one point per frame; a tick uses a handful).
  BackSlot& B = h->back[par];
  u32* host = B.h_fr_table;
  u32 nf = 0;
  for (size_t q = h->frames.size(); q-- > 0;)
    if (h->frames[q].count) ++nf;  // empty frames contribute no point (DepthFusion::update loops over none)
  if (nf > h->max_frames) { (void)flush_deferred_copies(h); FAIL(ESVO_ERR_CAPACITY, "too many non-empty frames in the fusion window"); }
  u32* cum = host;
  u32* off = host + (nf + 1);
  u32* slot = off + nf;
  u32 total = 0, i = 0;
  for (size_t q = h->frames.size(); q-- > 0;) {
    const FrameRec& f = h->frames[q];
    if (f.count == 0) continue;
    cum[i] = total; off[i] = f.off; slot[i] = f.slot;
    total += f.count;
    ++i;
  }
  cum[nf] = total;
  hipStream_t sb = h->stream_b;
  hipEvent_t tail_ev[2] = {nullptr, nullptr};
  u32* dtab = B.d_fr_table;
  if (h->pro.active) {  // latency mode: the frame's points and its pose table travel with the table (one launch, not three operations)
    const esvo_context::DeferredCopies d = h->pro;
    h->pro = esvo_context::DeferredCopies();
    launch_back_prologue(host, dtab, sizeof(u32) * (3 * (size_t)nf + 1), d.a_src, d.a_dst, d.a_bytes, d.b_src, d.b_dst, d.b_bytes, sb,
                         d.a_flags, d.a_prefix, d.a_slots);
    // "staging buffer / pose table free again": recorded at the END of this back stage, not here between two dependent launches
    // (~5 us each); who waits for them -- the front stage two ticks on -- comes long after either point
    tail_ev[0] = d.ev_a; tail_ev[1] = d.ev_b;
  } else {
    launch_upload_words(host, dtab, sizeof(u32) * (3 * (size_t)nf + 1), sb);
  }
  std::memcpy(h->T_world_frame, T_world_obs, sizeof(double) * 16);  // new DepthFrame at the TS pose (:268-272)
  FuseArgs a;
  a.win = h->d_win;
  a.fr_cum = dtab; a.fr_off = dtab + (nf + 1); a.fr_slot = a.fr_off + nf;
  a.n_frames = nf; a.n_pts = total;
  a.frame_pose_T = h->d_frame_pose_T; a.max_poses = h->max_poses;
  rigid_inverse(h->T_world_frame, a.T_frame_world);
  a.prop = h->d_prop;
  a.tile_count = h->d_tile_count; a.tile_pts = h->d_tile_pts; a.tile_cap = h->fuse_tile_cap;
  a.over_pts = h->d_over_pts; a.over_count = h->d_fuse_ctr + FUSE_CTR_OVER_COUNT;
  a.rec_ids = h->d_rec_ids; a.tile_rec = h->fuse_tile_rec; a.rec_cursor = h->d_fuse_ctr + FUSE_CTR_REC_CURSOR;
  a.cell_count = h->d_cell_count; a.cell_offset = h->d_cell_offset; a.cell_list = h->d_cell_list; a.slice_cap = h->fuse_slice_cap;
  a.class_count = h->d_fuse_ctr; a.class_total = h->d_fuse_ctr + FUSE_CTR_CLASS_TOTAL;
  a.lds_cap = h->fuse_lds_cap; a.pmax_plus1 = h->fuse_pmax_plus1; a.d_total = h->d_cnt_b + CNTB_RECORDS;
  a.map = h->d_map; a.d_num_fusion = h->d_cnt_b + CNTB_FUSIONS;
  a.n_touched = h->d_cnt_b + CNTB_TOUCHED;
  a.naive = naive ? 1 : 0;
  a.owner_max = h->prm.regularization ? h->d_owner_max : nullptr;
  a.owner_min = h->d_owner_min; a.n_reg_elems = h->prm.regularization ? h->d_cnt_b + CNTB_REG_ELEMS : nullptr;
  if (total > h->win_cap) {
    for (hipEvent_t e : tail_ev) if (e) hipEventRecord(e, sb);
    FAIL(ESVO_ERR_CAPACITY, "window points exceed capacity");
  }
  const bool timed = h->stage_events_on;
  B.timed = timed;
  if (timed) hipEventRecord(B.ev.e[BE_FU0], sb);
  launch_fuse(a, h->dp, sb);
  if (timed) hipEventRecord(B.ev.e[BE_FU1], sb);
  h->d_map_cur = h->d_map;
  // the ids this fusion numbered (kernels_fuse.hip: record id q K + k, launch_fuse's K): what esvo_map_cloud_build scans over
  h->map_id_bound = total * ((naive || h->dp.fusion_radius == 0) ? 4u : 9u);
  // (naive propagation, esvo_MVStereo.cpp:416-428: the map is published as it is, neither cleaned nor regularised)
  const bool do_clean = naive ? false : (h->prm.clean_requires_full_window ? (h->n_window_frames >= (size_t)h->prm.max_fusion_frames) : true);
  if (do_clean) launch_clean(h->d_map, h->dp, sb);
  if (timed) hipEventRecord(B.ev.e[BE_CL1], sb);
  if (h->prm.regularization && !naive) {
    launch_reg_view(h->d_map, h->d_map2, h->d_owner_max, h->d_owner_min, h->d_reg_ab, h->d_reg_cd, h->d_cnt_b + CNTB_REG_ELEMS, h->dp, sb);
    // (the tile kernel's layout for sparse maps when the newest known element count -- the previous tick's -- is below a tenth of
    //  the band's cells: scheduling only, same bits; ESVO_REG_SPARSE = 0 / 1 forces never / always)
    const u64 band_cells = (u64)std::max(h->dp.band_y1 - h->dp.band_y0, 1) * (u64)h->W;
    const bool sparse = h->reg_sparse_forced >= 0 ? h->reg_sparse_forced == 1 : (u64)h->stats.last_map_size * 10u < band_cells;
    launch_reg_apply(h->d_map, h->d_map2, h->d_owner_max, h->d_owner_min, h->d_reg_ab, h->d_reg_cd, h->d_cnt_b + CNTB_REG_ELEMS, h->dp, sb, sparse);
    h->d_map_cur = h->d_map2;
  }
  HIPCHK(hipMemcpyAsync(B.h_cnt, h->d_cnt_b, sizeof(u32) * CNTB_ROW, hipMemcpyDeviceToHost, sb));
  if (h->routed) HIPCHK(hipMemcpyAsync(h->h_cnt_b + CNTB_ROW * CNTB_ROW_HALO + par, h->d_halo_viol, sizeof(u32), hipMemcpyDeviceToHost, sb));
  hipEventRecord(B.ev.e[BE_RG1], sb);  // also "back stage of this parity done"
  for (hipEvent_t e : tail_ev) if (e) hipEventRecord(e, sb);
  HIPCHK(hipGetLastError());
  h->back_pending[par] = true;
  return ESVO_OK;
}

int export_map(esvo_context* h, std::vector<esvo_depth_point_t>& out, std::vector<u32>* cells) {
  launch_map_compact(h->d_map_cur, h->d_exp_flags, h->d_exp_prefix, h->d_cnt_b + CNTB_MAP, h->d_scan_tmp_b, h->d_export,
                     h->d_export_cell, h->dp, h->stream_b);
  int rc = read_counters_b(h, CNTB_ROW_EXPORT, true);
  if (rc) return rc;
  const u32 n = h->h_cnt_b[CNTB_ROW * CNTB_ROW_EXPORT + CNTB_MAP];
  out.resize(n);
  std::vector<u32> cell(n);
  if (n) {
    HIPCHK(hipMemcpy(out.data(), h->d_export, sizeof(esvo_depth_point_t) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cell.data(), h->d_export_cell, sizeof(u32) * n, hipMemcpyDeviceToHost));
  }
  // the reference iterates its element list in creation order
  std::vector<u32> order(n);
  for (u32 i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return out[a].seq < out[b].seq; });
  std::vector<esvo_depth_point_t> sorted(n);
  if (cells) cells->resize(n);
  for (u32 i = 0; i < n; ++i) {
    sorted[i] = out[order[i]];
    if (!h->sharded) sorted[i].seq = i;  // sharded: keep the global creation id so that bands can be merged
    if (cells) (*cells)[i] = cell[order[i]];
  }
  out.swap(sorted);
  h->stats.last_map_size = n;
  return ESVO_OK;
}
void window_stats(esvo_context* h) {
  h->stats.last_window_frames = (u32)h->n_window_frames;
  u32 np = 0;
  for (auto& f : h->frames) np += f.count;
  h->stats.last_window_points = np;
}
// the LM queues and the back stream have run dry
int drain_lm_and_back(esvo_context* h) {
  HIPCHK(hipStreamSynchronize(h->stream_l)); HIPCHK(hipStreamSynchronize(h->stream_l1));
  HIPCHK(hipStreamSynchronize(h->stream_b));
  return ESVO_OK;
}
// The back stage, now: the next back parity is taken (*par_out) and flipped, the back stage that used it two ticks ago is waited for
// and collected (its pinned table and event set are reused), the window is fused at the pose T_world_obs.
int fuse_window_now(esvo_context* h, const double* T_world_obs, bool naive, int* par_out) {
  const int par = h->par;
  h->par ^= 1;
  if (par_out) *par_out = par;
  HIPCHK(hipEventSynchronize(h->back[par].ev.e[BE_RG1]));
  collect_back(h, par);
  return run_fuse(h, par, T_world_obs, naive);
}
// A frame of the synchronous esvo_MVStereo modes (api_modes.hip): `count` points at d_src enter a window of maxNumFusionFrames
// frames whatever the fusion strategy, and DepthFusion::naive_propagation runs over it, waited for.  The frame that leaves at this
// tick leaves first (push_back + pop_front while size > max == pop while size >= max, then push) -- the caller has every fallible
// step of its front stage behind it, has probed the ring for the frame (window_probe_after_pops) and drained the back stream.
int commit_naive_frame(esvo_context* h, const DevPoint* d_src, u32 count, const double* pose_T_host, u32 m, int pose_buf) {
  const size_t keep_below = (size_t)std::max(1, h->prm.max_fusion_frames);
  while (h->n_window_frames && h->n_window_frames >= keep_below) pop_front_frame(h);
  u32 off;
  int rc = window_reserve(h, count, &off);
  if (rc) return rc;
  if (count) HIPCHK(hipMemcpyAsync(h->d_win + off, d_src, sizeof(DevPoint) * count, hipMemcpyDeviceToDevice, h->stream_b));
  rc = commit_frame(h, off, count, pose_T_host, m, pose_buf, false);
  if (rc) return rc;
  while (h->n_window_frames > (size_t)h->prm.max_fusion_frames) pop_front_frame(h);
  int par;
  rc = fuse_window_now(h, h->T_world_obs, true, &par);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream_b));
  collect_back(h, par);
  return ESVO_OK;
}
}  // namespace esvo_host

extern "C" {

int esvo_map_push_frame(esvo_handle h, const esvo_depth_point_t* pts, size_t n, const double* pose_T, size_t m) {
  if (!h || (n && !pts) || (m && !pose_T)) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (m > h->max_poses) FAIL(ESVO_ERR_CAPACITY, "pose table larger than max_poses_per_tick");
  for (size_t i = 0; i < n; ++i)
    if (pts[i].pose_idx >= m) FAIL(ESVO_ERR_INVALID_ARG, "depth point refers to a pose outside the frame's pose table");
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  u32 off;
  int rc = window_reserve(h, (u32)n, &off);
  if (rc) return rc;
  rc = drain_lm_and_back(h);  // the ring space may have been read by a fusion still in flight
  if (rc) return rc;
  if (n) HIPCHK(hipMemcpyAsync(h->d_win + off, pts, sizeof(esvo_depth_point_t) * n, hipMemcpyHostToDevice, h->stream));
  static const double ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  rc = commit_frame(h, off, (u32)n, m ? pose_T : ident, (u32)m);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return drain_lm_and_back(h);
}

int esvo_map_fuse(esvo_handle h, size_t* n_fusions) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (!h->obs_set) FAIL(ESVO_ERR_STATE, "esvo_map_set_observation has not been called");
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  int rc = back_after_front(h);
  if (rc) return rc;
  int par;
  rc = fuse_window_now(h, h->T_world_obs, false, &par);
  if (rc) return rc;
  h->committed_t_ns = h->obs_t_ns;
  rc = drain_lm_and_back(h);
  if (rc) return rc;
  collect_back(h, par);
  window_stats(h);
  if (n_fusions) *n_fusions = h->stats.last_fusions;
  return ESVO_OK;
}

int esvo_map_push_frame_device(esvo_handle h, const esvo_depth_point_t* d_pts, size_t n, const double* pose_T, size_t m) {
  if (!h || (n && !d_pts) || (m && !pose_T)) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (m > h->max_poses) FAIL(ESVO_ERR_CAPACITY, "pose table larger than max_poses_per_tick");
  HIPCHK(hipSetDevice(h->device));
  int rc = flush_pending_tick(h);
  if (rc) return rc;
  u32 off;
  rc = window_reserve(h, (u32)n, &off);
  if (rc) return rc;
  // the points were produced on the front stream (or by a collective the caller issued there); the copy runs on the
  // back stream, behind any fusion that still reads ring space freed by earlier pops
  rc = back_after_front(h);
  if (rc) return rc;
  if (n) HIPCHK(hipMemcpyAsync(h->d_win + off, d_pts, sizeof(esvo_depth_point_t) * n, hipMemcpyDeviceToDevice, h->stream_b));
  static const double ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  return commit_frame(h, off, (u32)n, m ? pose_T : ident, (u32)m);
}

int esvo_map_fuse_async(esvo_handle h) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (!h->obs_set) FAIL(ESVO_ERR_STATE, "esvo_map_set_observation has not been called");
  HIPCHK(hipSetDevice(h->device));
  int rc = flush_pending_tick(h);
  if (rc) return rc;
  rc = back_after_front(h);
  if (rc) return rc;
  rc = fuse_window_now(h, h->T_world_obs);
  if (rc) return rc;
  h->committed_t_ns = h->obs_t_ns;
  h->stats.ticks++;
  window_stats(h);
  h->stats_pending = true;
  return ESVO_OK;
}

}  // extern "C"
