// api_shard.hip — the band mode: slot- / row-routed front stages of a sharded tick, its phases, the shard configuration
// (see context.hpp).
#include "context.hpp"

namespace esvo_host {

// The same selection on a routed band handle: the walk is defined on the WHOLE left stream (glob_ts: every stamp, kept on the
// host), the rank's ring holds the events of its rows.  n / g_first: size of the global selection and the global index of its
// newest event; loc_first / n_loc: the newest of them in this rank's ring (absolute local index) and how many the ring holds.
int select_events_routed(esvo_context* h, uint64_t t_ns, u32* n_out, u32* g_first_out, u64* loc_first_out, u32* n_loc_out, u32* n_own_out) {
  std::lock_guard<std::mutex> lr(h->mu_ring);
  ingest_fence(h, 0);
  const double t_end = ns_to_sec(t_ns);
  const u64 t_begin_ns = ros_time_from_sec(std::max(0.0, t_end - 10 * h->prm.bm_half_slice_thickness));
  const double t_begin = ns_to_sec(t_begin_ns);
  auto lower = [&](double t) {
    const auto& v = h->glob_ts;
    size_t lo = 0, hi = v.size();
    while (lo < hi) {
      const size_t mid = (lo + hi) / 2;
      if (ns_to_sec(v[mid]) < t) lo = mid + 1; else hi = mid;
    }
    return h->glob_base + lo;
  };
  const u64 it_end = lower(t_end), it_begin = lower(t_begin);
  const u64 staged_end = h->glob_base + h->glob_ts.size();
  u64 avail = it_end - it_begin;
  u64 first = it_end;
  if (it_end == staged_end && avail > 0) { first = it_end - 1; avail -= 1; }  // end() is skipped (oracle definition)
  const u32 n = (u32)std::min<u64>(avail, (u64)h->prm.process_event_num);
  if (n > h->max_ev) FAIL(ESVO_ERR_CAPACITY, "more events than max_events_per_tick");
  *n_out = n;
  *g_first_out = (u32)first;
  *loc_first_out = 0;
  *n_loc_out = 0;
  *n_own_out = 0;
  if (n == 0) return ESVO_OK;
  // the kept events with a global index in [first - n + 1, first]
  const auto& kg = h->kept_g;
  const size_t lo = std::lower_bound(kg.begin(), kg.end(), first - (n - 1)) - kg.begin();
  const size_t hi = std::upper_bound(kg.begin(), kg.end(), first) - kg.begin();
  if (hi <= lo) return ESVO_OK;
  const u64 loc_first = h->ring_base[0] + hi - 1;
  const u32 n_loc = (u32)(hi - lo);
  if (loc_first - (n_loc - 1) < h->ring_reserved[0] - std::min<u64>(h->ring_reserved[0], h->ring_cap))
    FAIL(ESVO_ERR_STATE, "selected events were already overwritten in the event ring");
  *loc_first_out = loc_first;
  *n_loc_out = n_loc;
  *n_own_out = (u32)((hi < h->own_before.size() ? h->own_before[hi] : h->own_total) - h->own_before[lo]);
  h->sh_first_prev = h->sh_first;
  h->sh_first = loc_first;
  return ESVO_OK;
}

// block length of exchange 1 (kernels_shard.hip): the bytes of a rank's own slots, whole 64-bit words
static inline size_t shard_codes_block(u32 n, u32 N) { return (((size_t)n + N - 1) / N + 7) / 8 * 8; }
// the same in routed band mode: two bits per slot of the whole tick, whole 64-bit words
static inline size_t shard_codes_block_routed(u32 n) { return (((size_t)n + 15) / 16 * 4 + 7) / 8 * 8; }

// Routed band mode, phase 0 proper: the events of the band's rows (the rank's own ring): BM over them, dense local list of the own
// matches, LM + cull on it, then the (matched, kept) bits of the own slots in a block that spans the whole tick.
// keep_flags / keep_prefix (Denoising): per walk position of the RAW selection (n_raw events) whether the event is kept and how
// many kept ones precede it -- the slots are those of the kept sequence (n of them), as on one GPU.
static int routed_front(esvo_context* h, TickState& tk, u32 n, const u32* keep_flags, const u32* keep_prefix, u32 n_raw = 0) {
  FrontSlot& F = h->front_cur();
  const u32 N = (u32)h->dp.ev_nshards;
  const u32 n_loc = tk.n_loc, n_own = tk.n_own;
  int rc;
  if (n_loc) {
    BmArgs a;
    a.ev = h->d_ring[0]; a.n = n; a.ev_first = h->sh_first; a.ev_cap = h->ring_cap; a.ev_reverse = 1; a.sel = nullptr;
    a.gidx = h->d_ring_gidx; a.g_first = tk.g_first; a.n_loc = n_loc;
    a.keep_flags = keep_flags; a.keep_prefix = keep_prefix; a.n_raw = keep_flags ? n_raw : n;
    a.tsL = h->d_obs[0]; a.tsR = h->d_obs[1];
    a.lut = h->d_lut; a.mask = h->d_mask;
    a.pose_sec = h->d_pose_sec; a.n_pose = h->n_pose;
    a.out_slots = h->d_match_slots; a.out_flags = h->d_match_flags;
    a.fail_counters = F.d_counters;
    if (h->stage_events_on) hipEventRecord(F.ev->e[FE_BM0], h->stream);
    launch_bm_match(a, h->dp, h->stream);
    if (h->stage_events_on) hipEventRecord(F.ev->e[FE_BM1], h->stream);
    HIPCHK(hipGetLastError());
    // dense list of the own matches (count -> CNT_OWN_MATCHES); the slot of each follows from its walk position (shard_codes_routed)
    if (scan_compact_is_small(n_loc)) {
      launch_scan_compact_matches_small(h->d_match_flags, h->d_match_prefix, F.d_counters + CNT_OWN_MATCHES, n_loc, h->d_match_slots, F.d_matches, nullptr,
                                        h->stream);
    } else {
      launch_exclusive_scan_u32(h->d_match_flags, h->d_match_prefix, F.d_counters + CNT_OWN_MATCHES, h->d_scan_tmp, n_loc, h->stream);
      launch_compact_matches(h->d_match_slots, h->d_match_flags, h->d_match_prefix, n_loc, F.d_matches, nullptr, h->stream);
    }
    if (h->stage_events_on) hipEventRecord(F.ev->e[FE_S1], h->stream);
    HIPCHK(hipGetLastError());
    // (the ring also holds the raster's halo events: the launch -- and with it the kernel's layout -- is bounded by the OWN
    //  events of the selection, counted at ingest)
    rc = run_lm(h, n_own, 1, true);
    if (rc) return rc;
  } else {  // no event of this tick in the band: the stage events the statistics read are still recorded
    if (h->stage_events_on)
      for (int e : {FE_BM0, FE_BM1, FE_S1, FE_LM0, FE_LM1}) hipEventRecord(F.ev->e[e], h->stream);
  }
  const size_t nb = shard_codes_block_routed(n);
  HIPCHK(hipMemsetAsync(h->d_codes_send, 0, nb, h->stream));
  launch_shard_codes_routed(F.d_matches, h->d_lkeep, F.d_counters + CNT_OWN_MATCHES, n_own, n, (u32)h->dp.num_threads, h->d_own_w,
                            reinterpret_cast<u32*>(h->d_codes_send.get()), h->stream);
  HIPCHK(hipGetLastError());
  h->xchg_send = h->d_codes_send;
  h->xchg_recv = N > 1 ? h->d_codes_all : h->d_codes_send;
  h->xchg_block = nb;
  return ESVO_OK;
}
// Denoising on a routed band handle (esvo_Mapping.cpp:1046-1072: the mask is the 3 x 3 median of the selected events' map; an
// event is kept when its pixel is set in it).  An event's flag needs the selected events of its raw row and the two next to it; a
// rank's ring holds the raw rows of its band + 1 (keep_px bit 2, esvo_shard_set_routing), so it computes the flags of the events
// whose RAW row lies in its band -- every selected event has exactly one such rank -- and the ranks all-gather them as one bit per
// walk position of the selection.  The kept sequence (which events, in which order, how many) is then the one-GPU one on every rank.
static inline size_t denoise_bits_block(u32 n) { return (((size_t)n + 31) / 32 * 4 + 7) / 8 * 8; }
static int routed_denoise_begin(esvo_context* h, TickState& tk) {
  const u32 N = (u32)h->dp.ev_nshards;
  const size_t nb = denoise_bits_block(tk.n);
  HIPCHK(hipMemsetAsync(h->d_codes_send, 0, nb, h->stream));
  launch_denoise_bits_routed(h->d_ring[0], h->sh_first, h->ring_cap, tk.n_loc, h->d_ring_gidx, tk.g_first, tk.n, h->d_evmap, h->W, h->H,
                             h->dp.band_y0, h->dp.band_y1, reinterpret_cast<u32*>(h->d_codes_send.get()), h->stream);
  HIPCHK(hipGetLastError());
  h->xchg_send = h->d_codes_send;
  h->xchg_recv = N > 1 ? h->d_codes_all : h->d_codes_send;
  h->xchg_block = nb;
  h->dn_pending = true;
  return ESVO_OK;
}
int routed_denoise_resume(esvo_context* h) {
  h->dn_pending = false;
  TickState& tk = h->front_cur().tk;
  const u32 N = (u32)h->dp.ev_nshards, n_raw = tk.n;
  if (!h->d_dn_flags) {
    HIPCHK(h->d_dn_flags.alloc(2 * (size_t)h->max_ev));
  }
  u32* flags = h->d_dn_flags;
  u32* prefix = h->d_dn_flags + h->max_ev;
  launch_denoise_bits_unpack(reinterpret_cast<const u32*>((N > 1 ? h->d_codes_all : h->d_codes_send).get()), (u32)(denoise_bits_block(n_raw) / 4), N, n_raw,
                             flags, h->stream);
  launch_exclusive_scan_u32(flags, prefix, h->front_cur().d_counters + CNT_DENOISE_KEPT, h->d_scan_tmp, n_raw, h->stream);
  int rc = read_counters(h);  // the kept count sizes everything behind it (as on one GPU: one read-back)
  if (rc) return rc;
  const u32 n = tk.n = h->h_counters[CNT_DENOISE_KEPT];
  h->xchg_send = h->xchg_recv = nullptr;
  h->xchg_block = 0;
  if (!n) return ESVO_OK;
  return routed_front(h, tk, n, flags, prefix, n_raw);
}

// phase 0 of a sharded tick behind the event selection (tick_phase0): the routed front stage, or:
int shard_front(esvo_context* h, TickState& tk, u32 n, const u32* sel) {
  int rc;
  if (h->routed) {
    if (h->prm.denoising) {  // the denoising mask first: its bits are exchanged, phase 0 is called again behind that (ESVO_AGAIN)
      rc = routed_denoise_begin(h, tk);
      return rc ? rc : (int)ESVO_AGAIN;
    }
    return routed_front(h, tk, n, nullptr, nullptr);
  }
  // own slots only (w % n_shards == shard): BM, dense local list, LM + cull on it, then the (matched, kept)
  // byte of every own slot, back to back: this rank's block of the caller's all-gather
  const u32 N = (u32)h->dp.ev_nshards, r = (u32)h->dp.ev_shard;
  const u32 own = n > r ? (n - r + N - 1) / N : 0;
  HIPCHK(hipMemsetAsync(h->d_match_flags, 0, sizeof(u32) * n, h->stream));
  rc = run_bm(h, h->d_ring[0], h->sh_first, h->ring_cap, 1, n, sel);
  if (rc) return rc;
  rc = run_order_matches(h, n, true);
  if (rc) return rc;
  rc = run_lm(h, own, 1, true);
  if (rc) return rc;
  const size_t nb = shard_codes_block(n, N);
  HIPCHK(hipMemsetAsync(h->d_codes_send, 0, nb, h->stream));
  launch_shard_codes(h->d_own_w, h->d_lkeep, h->front_cur().d_counters + CNT_OWN_MATCHES, own, N, h->d_codes_send, h->stream);
  HIPCHK(hipGetLastError());
  h->xchg_send = h->d_codes_send;
  h->xchg_recv = N > 1 ? h->d_codes_all : h->d_codes_send;
  h->xchg_block = nb;
  return ESVO_OK;
}
// phase 1 of a sharded tick (tick_phase1_enqueue): the frame's order from the exchanged codes, the rank's block of exchange 2
int shard_order_points(esvo_context* h, TickState& tk) {
  FrontSlot& F = h->front_cur();
  const u32 n = tk.n;
  const u32 N = (u32)h->dp.ev_nshards, r = (u32)h->dp.ev_shard, T = (u32)h->dp.num_threads;
  const u32 own = h->routed ? tk.n_own : (n > r ? (n - r + N - 1) / N : 0);
  // Six dependent launches for a routed tick above the single-workgroup scans' size (round 6; thirteen before): unpack (+ the
  // matched slots per scan tile), down-sweep of the matched bits (+ clearing the keep flags), keep flags by solver slot (+ clearing
  // the exchange block's cursor), their scan (2), pack.  This chain is the same on every rank whatever the number of ranks -- the
  // part of a band-mode tick that does not shrink.
  const bool tiled = h->routed && !scan_is_small(n);
  if (h->routed)
    launch_shard_unpack_routed(reinterpret_cast<const u32*>((N > 1 ? h->d_codes_all : h->d_codes_send).get()), (u32)(shard_codes_block_routed(n) / 4), N,
                               n, h->d_codes, h->d_rank_kept, tiled ? h->d_scan_tmp : nullptr, h->stream);
  else
    launch_shard_unpack_codes(N > 1 ? h->d_codes_all : h->d_codes_send, (u32)shard_codes_block(n, N), N, n, h->d_codes, h->d_rank_kept,
                              h->stream);
  if (tiled) launch_scan_down_code_bit0(h->d_codes, h->d_match_prefix, F.d_counters + CNT_MATCHES, h->d_scan_tmp, n, F.d_pt_flags, h->stream);
  else launch_exclusive_scan_code_bit0(h->d_codes, h->d_match_prefix, F.d_counters + CNT_MATCHES, h->d_scan_tmp, n, F.d_pt_flags, h->stream);
  launch_shard_keep_flags(h->d_codes, h->d_match_prefix, F.d_counters + CNT_MATCHES, n, T, F.d_pt_flags, h->d_pts_send, h->stream);
  launch_exclusive_scan_u32(F.d_pt_flags, F.d_pt_prefix, F.d_counters + CNT_POINTS, h->d_scan_tmp, n, h->stream);
  launch_shard_pack(h->d_own_w, h->d_lkeep, F.d_pt_slots, F.d_counters + CNT_OWN_MATCHES, own, h->d_match_prefix, F.d_counters + CNT_MATCHES,
                    F.d_pt_prefix, T, h->d_pts_send, own, n, h->d_rank_kept, N, F.d_counters + CNT_MAX_KEPT, h->stream,
                    h->routed ? F.d_counters + CNT_SCRATCH : nullptr);
  if (tk.timed) hipEventRecord(F.ev->e[FE_S2], h->stream);
  HIPCHK(hipGetLastError());
  return ESVO_OK;
}
// what opens phase 2 of a sharded tick (tick_phase2)
int shard_scatter_frame(esvo_context* h, TickState& tk) {
  const u32 N = (u32)h->dp.ev_nshards;
  launch_shard_scatter(N > 1 ? h->d_pts_all : h->d_pts_send, 1 + (size_t)tk.max_kept * (sizeof(DevPoint) / 8), N, tk.max_kept,
                       h->d_win + tk.off, tk.n, h->stream, h->routed ? h->d_halo_viol : nullptr);
  HIPCHK(hipGetLastError());
  return back_after_front(h);
}
}  // namespace esvo_host

extern "C" int esvo_shard_tick_phase(esvo_handle h, int phase, uint64_t t_ns, const uint64_t* pose_t_ns, const double* pose_T,
                                     size_t m) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (!h->obs_set) FAIL(ESVO_ERR_STATE, "esvo_map_set_observation has not been called");
  if (!h->sharded) FAIL(ESVO_ERR_STATE, "call esvo_shard_set_band first");
  HIPCHK(hipSetDevice(h->device));
  // (stage-timing events are sampled, context.hpp lat_ticks: phase 0 decides for the tick; switched back on when the call returns)
  StageEventsScope timed_scope(h, phase == 0 ? true : h->front_cur().tk.timed);
  switch (phase) {
    case 0:
      if (!h->dn_pending && (!pose_t_ns || !pose_T)) return ESVO_ERR_INVALID_ARG;
      return tick_phase0(h, t_ns, pose_t_ns, pose_T, m);  // (ESVO_AGAIN: exchange, then phase 0 once more -- Denoising on a routed handle)
    case 1: {
      int rc = tick_phase1_enqueue(h);
      if (rc) return rc;
      return tick_phase1_collect(h, h->fpar);
    }
    case 2: return tick_phase2(h, h->fpar);
    default: FAIL(ESVO_ERR_INVALID_ARG, "phase must be 0..2");
  }
}

extern "C" {
// ---- Multi-GPU row-band sharding ------------------------------------------------------------------
namespace {
bool rings_empty(esvo_context* h) {
  std::lock_guard<std::mutex> lr(h->mu_ring);
  return h->ring_next[0] == 0 && h->ring_next[1] == 0 && h->glob_ts.empty();
}
}  // namespace

int esvo_shard_set_band(esvo_handle h, int row_begin, int row_end, int shard, int n_shards) {
  if (!h || row_begin < 0 || row_end > h->H || row_begin >= row_end || n_shards < 1 || shard < 0 || shard >= n_shards ||
      n_shards > (int)esvo_context::SHARD_MAX_RANKS)
    return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (h->hist_len) FAIL(ESVO_ERR_UNSUPPORTED, "the handle keeps a Time-Surface history: esvo_ts_history_configure(h, 0) before sharding it");
  if (h->prm.lm_scale_pass_limit != 0)
    FAIL(ESVO_ERR_STATE, "the handle runs the LM scale-loop guard (lm_scale_pass_limit != 0), a single-GPU feature: set the limit to 0 before sharding it");
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  if (h->routed && !rings_empty(h))
    FAIL(ESVO_ERR_STATE, "the handle routes events by row and holds staged events: esvo_reset before changing its band");
  h->routed = false;  // (esvo_shard_set_routing follows)
  h->dp.ev_shard = shard;
  h->dp.ev_nshards = n_shards;
  h->dp.band_y0 = row_begin;
  h->dp.band_y1 = row_end;
  set_compute_band(h);
  h->sharded = !(row_begin == 0 && row_end == h->H) || n_shards > 1;
  if (h->sharded && !h->d_rank_kept) {  // exchange blocks, sized for any rank count up to SHARD_MAX_RANKS (lazily: unsharded handles never pay)
    const size_t E = h->max_ev, R = esvo_context::SHARD_MAX_RANKS, WP = sizeof(DevPoint) / 8;
    HIPCHK(hipSetDevice(h->device));
    // (d_rank_kept, the guard above, is allocated LAST: a failure in the chain frees what came before and leaves the guard null)
    if (h->d_codes_send.alloc((E + 7) / 8 * 8) || h->d_codes_all.alloc(E + 8 * R) || h->d_pts_send.alloc(1 + E * WP) ||
        h->d_pts_all.alloc(R + (E + R) * WP) || h->d_rank_kept.alloc(R)) {
      (void)hipGetLastError();
      (void)h->d_codes_send.release(); (void)h->d_codes_all.release(); (void)h->d_pts_send.release(); (void)h->d_pts_all.release();
      (void)h->d_rank_kept.release(); (void)h->d_ring_gidx.release();
      h->sharded = false;
      h->dp.ev_shard = 0; h->dp.ev_nshards = 1; h->dp.band_y0 = 0; h->dp.band_y1 = h->H;
      set_compute_band(h);
      FAIL(ESVO_ERR_CAPACITY, "out of device memory for the shard exchange blocks");
    }
    HIPCHK(hipMemset(h->d_rank_kept, 0, sizeof(u32) * R));
  }
  return ESVO_OK;
}

int esvo_shard_set_routing(esvo_handle h, int mode, int ts_halo_rows) {
  if (!h || (mode != ESVO_ROUTE_BROADCAST && mode != ESVO_ROUTE_Y_RECT)) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  if (!h->sharded) FAIL(ESVO_ERR_STATE, "call esvo_shard_set_band first");
  if (!rings_empty(h)) FAIL(ESVO_ERR_STATE, "events are already staged: choose the routing before the first esvo_ts_push_events (or esvo_reset)");
  if (mode == ESVO_ROUTE_BROADCAST) { h->routed = false; return ESVO_OK; }
  if (h->flt[0].on || h->flt[1].on) FAIL(ESVO_ERR_UNSUPPORTED, "an event filter is configured (esvo_ts_filter_configure): it needs the whole stream, row routing filters packets on the host -- use ESVO_ROUTE_BROADCAST");
  const esvo_params_t& p = h->prm;
  if (h->tsq_len) FAIL(ESVO_ERR_UNSUPPORTED, "per-pixel event queues (max_event_queue_len) are not routed: use ESVO_ROUTE_BROADCAST");
  if (p.bm_updown) FAIL(ESVO_ERR_UNSUPPORTED, "up-down stereo searches along y, across the bands: use ESVO_ROUTE_BROADCAST");
  const int H = h->H, W = h->W;
  const int hy = (p.patch_size_y - 1) / 2;
  int halo = ts_halo_rows < 0 ? 24 : ts_halo_rows;
  // block matching reads the band + hy rows; the refinement's blocks reach one row further before any motion
  if (halo < hy + 2) FAIL(ESVO_ERR_INVALID_ARG, "ts_halo_rows must be at least patch_size_Y / 2 + 2");
  // rows of the observation pair that must hold data, in whole 4-row tiles of the blur; the Time-Surface rows they are made
  // from (+ 2 under SmoothTimeSurface: GaussianBlurTS(5)), in whole tiles of the render kernel
  const int o0 = std::max(0, h->dp.band_y0 - halo) / 4 * 4;
  const int o1 = std::min(H, (std::min(H, h->dp.band_y1 + halo) + 3) / 4 * 4);
  const int pad = p.smooth_time_surface ? 2 : 0;
  const int r0 = std::max(0, o0 - pad) / TS_TILE_ROWS * TS_TILE_ROWS;
  const int r1 = std::min(H, (std::min(H, o1 + pad) + TS_TILE_ROWS - 1) / TS_TILE_ROWS * TS_TILE_ROWS);
  const int k = std::max(0, p.median_blur_kernel_size);
  for (int cam = 0; cam < 2; ++cam) {  // raw rows the remap taps of [r0, r1) reach, + the median's ring
    int lo = H, hi = -1;
    for (int y = r0; y < r1; ++y) { lo = std::min(lo, h->fix_row_lo[cam][y]); hi = std::max(hi, h->fix_row_hi[cam][y]); }
    h->sband_y0[cam] = hi < lo ? 0 : std::max(0, lo - k);
    h->sband_y1[cam] = hi < lo ? 0 : std::min(H, hi + k + 1);
  }
  h->keep_px.assign((size_t)W * H, 0);
  const float* lut = h->h_rect_lut[0].data();
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      uint8_t f = (y >= h->sband_y0[0] && y < h->sband_y1[0]) ? 1 : 0;
      const int yb = (int)std::floor((double)lut[2 * ((size_t)y * W + x) + 1]);  // kernels_bm.hip: the rank that owns floor(y_rect)
      if (yb >= h->dp.band_y0 && yb < h->dp.band_y1) f |= 2;
      // Denoising: the rank decides the mask's verdict for the events whose RAW row is in its band; the 3 x 3 median reads the
      // selected events of one more row on either side (routed_denoise_begin)
      if (p.denoising && y >= h->dp.band_y0 - 1 && y < h->dp.band_y1 + 1) f |= 4;
      h->keep_px[(size_t)y * W + x] = f;
    }
  HIPCHK(hipSetDevice(h->device));
  if (!h->d_ring_gidx) HIPCHK(h->d_ring_gidx.alloc(h->ring_cap));
  {  // exchange 1 spans the whole tick in this mode: n_shards blocks of two bits per slot
    const size_t need = (size_t)h->dp.ev_nshards * shard_codes_block_routed(h->max_ev);
    if (need > (size_t)h->max_ev + 8 * esvo_context::SHARD_MAX_RANKS) {
      HIPCHK(hipStreamSynchronize(h->stream));
      DevBuf<uint8_t> d_new;  // (allocated before the old blocks go: they stay intact where this fails)
      if (d_new.alloc(need) != hipSuccess) { (void)hipGetLastError(); FAIL(ESVO_ERR_CAPACITY, "out of device memory for the routed exchange blocks"); }
      h->d_codes_all = std::move(d_new);
    }
  }
  h->ts_halo = halo;
  h->oband_y0 = o0; h->oband_y1 = o1;
  h->rband_y0 = r0; h->rband_y1 = r1;
  h->routed = true;
  return ESVO_OK;
}

int esvo_shard_get_rows(esvo_handle h, int render_rows[2], int observation_rows[2], int source_rows_left[2], int source_rows_right[2]) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  const bool r = h->routed;
  if (render_rows) { render_rows[0] = r ? h->rband_y0 : 0; render_rows[1] = r ? h->rband_y1 : h->H; }
  if (observation_rows) { observation_rows[0] = r ? h->oband_y0 : 0; observation_rows[1] = r ? h->oband_y1 : h->H; }
  if (source_rows_left) { source_rows_left[0] = r ? h->sband_y0[0] : 0; source_rows_left[1] = r ? h->sband_y1[0] : h->H; }
  if (source_rows_right) { source_rows_right[0] = r ? h->sband_y0[1] : 0; source_rows_right[1] = r ? h->sband_y1[1] : h->H; }
  return ESVO_OK;
}

int esvo_shard_exchange(esvo_handle h, void** d_send, void** d_recv, size_t* block_bytes) {
  if (!h || !d_send || !d_recv || !block_bytes) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  *d_send = h->xchg_send;
  *d_recv = h->xchg_recv;
  *block_bytes = h->xchg_block;
  return ESVO_OK;
}

}  // extern "C"
