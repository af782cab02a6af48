// api_em.hip — event-to-event matching (EventMatcher), esvo_MVStereo modes 0 and 2: the host-array seam
// (esvo_map_match_em), the fused tick on the staged events (esvo_map_tick_em) and its read-outs.  Kernels: kernels_em.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "context.hpp"
#include "em.hpp"

// (global namespace: esvo_context holds an EmState*)
struct EmSlice {
  u32 begin, count;
  u64 t_ns;
  double T[16];
};

struct EmState {
  // device buffers (grown on demand)
  DevBuf<esvo_event_t> d_left, d_right;
  DevBuf<u32> d_slice_of, d_cnt_tp, d_cnt_ep, d_off, d_flags, d_prefix;  // cap_ev elements each, as d_slots and d_out
  DevBuf<esvo_match_t> d_slots, d_out;
  size_t cap_ev = 0;
  DevBuf<double> d_T;
  DevBuf<u32> d_pair_ev, d_pair_r, d_pair_ok;  // cap_pairs elements each, as d_pair_cost
  DevBuf<double> d_pair_cost;
  size_t cap_pairs = 0;
  DevBuf<u32> d_scan;
  DevBuf<u32> d_tot;  // [0] epipolar pairs [1] unused [2] patch ok [3] matches
  DevBuf<unsigned long long> d_tot64;  // [0] epipolar pairs [1] time + polarity pairs, 64-bit
  DevBuf<float2> d_lut_r;
  DevEvent ev0, ev1;
  // last tick
  esvo_em_selection_t sel{};
  std::vector<EmSlice> slices;
  esvo_em_stats_t stats{};
};

namespace esvo_host {

void em_release(esvo_context* h) {
  delete h->em;
  h->em = nullptr;
}

// the state, the right camera's rectification table on the device, the checks every EM call shares
static int em_prepare(esvo_context* h, const esvo_em_params_t* em) {
  HIPCHK(hipSetDevice(h->device));  // before anything below allocates on first use
  if (!h->obs_set) FAIL(ESVO_ERR_STATE, "esvo_map_set_observation has not been called");
  if (h->sharded) FAIL(ESVO_ERR_STATE, "handle is sharded");
  if (h->prm.smooth_time_surface)
    FAIL(ESVO_ERR_UNSUPPORTED, "event matching reads the un-smoothed Time Surfaces; the observation holds the smoothed pair");
  if (!(em->time_threshold >= 0.0) || !(em->epipolar_threshold >= 0.0) || em->num_event_matching < 0)
    FAIL(ESVO_ERR_INVALID_ARG, "invalid esvo_em_params_t");
  const size_t npx = (size_t)h->W * h->H;
  if (h->h_rect_lut[1].size() != 2 * npx) FAIL(ESVO_ERR_STATE, "event matching needs the right camera's rect_lut (esvo_create)");
  if (!h->em) {
    h->em = new EmState();
    HIPCHK(h->em->ev0.create());
    HIPCHK(h->em->ev1.create());
    HIPCHK(h->em->d_tot.alloc(4));
    HIPCHK(h->em->d_tot64.alloc(2));
  }
  EmState* e = h->em;
  if (!e->d_lut_r) {
    HIPCHK(e->d_lut_r.alloc(npx));
    HIPCHK(hipMemcpy(e->d_lut_r, h->h_rect_lut[1].data(), sizeof(float2) * npx, hipMemcpyHostToDevice));
  }
  return ESVO_OK;
}

static int em_reserve_events(esvo_context* h, size_t n_left, size_t n_right) {
  EmState* e = h->em;
  HIPCHK(e->d_left.grow(n_left));
  HIPCHK(e->d_right.grow(n_right));
  return ESVO_OK;
}

// Matching of n events (d_left[first + i]) against d_right[0, n_right): candidates, pair costs, argmin, compaction into
// e->d_out in the stride-N order.  slice_of[i], slice poses T_world[16 s].  Synchronous; fills e->stats.
static int em_match_device(esvo_context* h, const esvo_em_params_t* em, u32 first, u32 n, const std::vector<u32>& slice_of,
                           const double* slice_T, size_t n_slices, u32 n_right, u32* n_matches) {
  EmState* e = h->em;
  *n_matches = 0;
  e->stats = esvo_em_stats_t{};
  e->stats.events = n;
  e->stats.right_events = n_right;
  e->stats.slices = n_slices;
  if (n == 0) return ESVO_OK;
  if (n > e->cap_ev) {
    HIPCHK(e->d_slice_of.grow(n)); HIPCHK(e->d_cnt_tp.grow(n)); HIPCHK(e->d_cnt_ep.grow(n));
    HIPCHK(e->d_off.grow(n)); HIPCHK(e->d_flags.grow(n)); HIPCHK(e->d_prefix.grow(n));
    HIPCHK(e->d_slots.grow(n)); HIPCHK(e->d_out.grow(n));
    e->cap_ev = n;
  }
  HIPCHK(e->d_T.grow(n_slices * 12));
  // T_left_rv = T_obs^-1 T_slice with the rigid inverse and 4x4 product of DepthProblem's restatement (common.hpp)
  std::vector<double> T_lr(n_slices * 12);
  double Tlw[16], Tlv[16];
  rigid_inverse(h->T_world_obs, Tlw);
  for (size_t s = 0; s < n_slices; ++s) {
    mat4_mul(Tlw, slice_T + 16 * s, Tlv);
    std::copy(Tlv, Tlv + 12, T_lr.begin() + 12 * s);
  }
  auto scan_need = [](size_t m) { return scan_scratch_elems(m); };
  HIPCHK(e->d_scan.grow(scan_need(n)));
  hipStream_t st = h->stream;
  HIPCHK(hipMemcpyAsync(e->d_slice_of, slice_of.data(), sizeof(u32) * n, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(e->d_T, T_lr.data(), sizeof(double) * 12 * n_slices, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(e->d_tot, 0, sizeof(u32) * 4, st));

  EmArgs a{};
  a.left = e->d_left + first; a.n = n; a.event_base = first; a.slice_of = e->d_slice_of; a.T_lr = e->d_T;
  a.right = e->d_right; a.n_right = n_right;
  a.lut_l = h->d_lut; a.lut_r = e->d_lut_r;
  a.tsL = h->d_obs[0]; a.tsR = h->d_obs[1];
  a.W = h->W; a.H = h->H; a.wx = h->prm.patch_size_x; a.wy = h->prm.patch_size_y;
  a.num_threads = (u32)std::max(1, h->prm.num_threads);
  a.half_T = em->time_threshold / 2;
  a.epi_thr = em->epipolar_threshold; a.ncc_thr = em->ncc_threshold;
  a.bf = h->dp.baseline_f;
  a.camL = h->dp.camL; a.camR = h->dp.camR;
  a.cnt_tp = e->d_cnt_tp; a.cnt_ep = e->d_cnt_ep; a.pair_off = e->d_off;
  a.slots = e->d_slots; a.flags = e->d_flags;
  HIPCHK(hipEventRecord(e->ev0, st));
  launch_em_candidates(a, 0, st);
  launch_exclusive_scan_u32(e->d_cnt_ep, e->d_off, e->d_tot + 0, e->d_scan, n, st);
  launch_em_sum64(e->d_cnt_ep, e->d_cnt_tp, n, e->d_tot64, st);
  HIPCHK(hipGetLastError());
  u32 tot[4];
  unsigned long long tot64[2];
  HIPCHK(hipMemcpyAsync(tot64, e->d_tot64, sizeof(tot64), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  e->stats.time_polarity = tot64[1];
  e->stats.epipolar = tot64[0];
  // pair indices and offsets are 32-bit: refuse a call with more pairs than that (the u32 scan total has wrapped)
  if (tot64[0] > 0xffffffffull) FAIL(ESVO_ERR_CAPACITY, "more than 2^32 - 1 (event, candidate) pairs pass the epipolar test");
  const u32 n_pairs = (u32)tot64[0];
  if (n_pairs > e->cap_pairs) {
    HIPCHK(e->d_pair_ev.grow(n_pairs)); HIPCHK(e->d_pair_r.grow(n_pairs));
    HIPCHK(e->d_pair_ok.grow(n_pairs)); HIPCHK(e->d_pair_cost.grow(n_pairs));
    e->cap_pairs = n_pairs;
  }
  HIPCHK(e->d_scan.grow(scan_need(n_pairs)));
  a.n_pairs = n_pairs; a.pair_ev = e->d_pair_ev; a.pair_r = e->d_pair_r; a.pair_cost = e->d_pair_cost; a.pair_ok = e->d_pair_ok;
  launch_em_candidates(a, 1, st);
  launch_em_pair_cost(a, st);
  if (n_pairs) launch_exclusive_scan_u32(e->d_pair_ok, e->d_pair_ok, e->d_tot + 2, e->d_scan, n_pairs, st);
  launch_em_argmin(a, st);
  launch_exclusive_scan_u32(e->d_flags, e->d_prefix, e->d_tot + 3, e->d_scan, n, st);
  launch_em_compact(e->d_slots, e->d_flags, e->d_prefix, n, e->d_out, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e->ev1, st));
  HIPCHK(hipMemcpyAsync(tot, e->d_tot, sizeof(u32) * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e->ev0, e->ev1);
  e->stats.patch_ok = tot[2];
  e->stats.matches = tot[3];
  e->stats.ms_match = ms;
  *n_matches = tot[3];
  return ESVO_OK;
}

// Holds the EM selection's ring ranges against eviction (esvo_context::em_guard_lo) from the moment the gather is enqueued until
// it has completed; on an early return it waits for the front stream before lifting the guard.
struct EmGuard {
  esvo_context* h;
  bool armed = false;
  explicit EmGuard(esvo_context* hh) : h(hh) {}
  void release() {
    if (!armed) return;
    std::lock_guard<std::mutex> lr(h->mu_ring);
    h->em_guard_lo[0] = h->em_guard_lo[1] = ~0ull;
    armed = false;
  }
  ~EmGuard() {
    if (armed) (void)hipStreamSynchronize(h->stream);
    release();
  }
};

// EventVecPtr_lower_bound over the stamps of a selection (toSec() comparison, std::lower_bound's halving)
static size_t em_lower_bound_ns(const std::vector<u64>& ts, double t) {
  size_t first = 0, len = ts.size();
  while (len > 0) {
    const size_t half = len >> 1, mid = first + half;
    if (ns_to_sec(ts[mid]) < t) { first = mid + 1; len = len - half - 1; }
    else len = half;
  }
  return first;
}

// copy [first, first + n) of camera cam's ring into dst (two pieces where the ring wraps)
static int em_gather_ring(esvo_context* h, int cam, u64 first, u32 n, esvo_event_t* dst) {
  for (const RingSpan& s : ring_spans(h->ring_cap, first, n))
    HIPCHK(hipMemcpyAsync(dst + s.at, h->d_ring[cam] + s.slot, sizeof(esvo_event_t) * s.count, hipMemcpyDeviceToDevice, h->stream));
  return ESVO_OK;
}

}  // namespace esvo_host

extern "C" {

int esvo_map_match_em(esvo_handle h, const esvo_em_params_t* em, const esvo_event_t* left_ev, size_t n_left,
                      const uint32_t* slice_begin, const uint32_t* slice_count, const double* slice_T, size_t n_slices,
                      const esvo_event_t* right_ev, size_t n_right, esvo_match_t* out, size_t cap, size_t* n_out) {
  if (!h || !em || !n_out || (n_left && !left_ev) || (n_right && !right_ev) ||
      (n_slices && (!slice_begin || !slice_count || !slice_T)))
    return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  *n_out = 0;
  int rc = em_prepare(h, em);
  if (rc) return rc;
  if (n_left > 0xffffffffull || n_right > 0xffffffffull) FAIL(ESVO_ERR_CAPACITY, "more than 2^32 - 1 events");
  // match_all_HyperThread: the slices' event counts, taken contiguously from the first slice's first event
  u64 total = 0;
  for (size_t s = 0; s < n_slices; ++s) total += slice_count[s];
  const u32 first = n_slices ? slice_begin[0] : 0;
  if (n_slices && (u64)first + total > n_left) FAIL(ESVO_ERR_INVALID_ARG, "slices reach beyond the left events");
  std::vector<u32> slice_of;
  slice_of.reserve(total);
  for (size_t s = 0; s < n_slices; ++s) slice_of.insert(slice_of.end(), slice_count[s], (u32)s);
  rc = flush_pending_tick(h);
  if (rc) return rc;
  rc = em_reserve_events(h, n_left, n_right);
  if (rc) return rc;
  EmState* e = h->em;
  if (n_left) HIPCHK(hipMemcpyAsync(e->d_left, left_ev, sizeof(esvo_event_t) * n_left, hipMemcpyHostToDevice, h->stream));
  if (n_right) HIPCHK(hipMemcpyAsync(e->d_right, right_ev, sizeof(esvo_event_t) * n_right, hipMemcpyHostToDevice, h->stream));
  u32 nm = 0;
  rc = em_match_device(h, em, first, (u32)total, slice_of, slice_T, n_slices, (u32)n_right, &nm);
  if (rc) return rc;
  *n_out = nm;
  if (out && nm) {
    if (nm > cap) FAIL(ESVO_ERR_CAPACITY, "output array too small for the matches");
    HIPCHK(hipMemcpy(out, e->d_out, sizeof(esvo_match_t) * nm, hipMemcpyDeviceToHost));
  }
  return ESVO_OK;
}

int esvo_map_tick_em(esvo_handle h, const esvo_em_params_t* em, int mode, uint64_t t_low_ns, uint64_t t_up_ns,
                     esvo_em_pose_fn pose_fn, void* user) {
  if (!h || !em || (mode != 0 && mode != 2)) return ESVO_ERR_INVALID_ARG;
  if (!(em->slice_thickness > 0.0)) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  int rc = em_prepare(h, em);
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->device));
  rc = flush_pending_tick(h);
  if (rc) return rc;
  // ---- selection (dataTransferring's EM branch, esvo_MVStereo.cpp:579-609); caller holds mu_ring
  const double t_low = ns_to_sec(t_low_ns), t_up = ns_to_sec(t_up_ns);
  const u64 cap1 = (u64)em->num_event_matching + 1;  // the loop pushes while size <= EM_NUM_EVENT_MATCHING
  auto select = [&](u64 first[2], u32 cnt[2]) -> int {
    for (int cam = 0; cam < 2; ++cam) {
      ingest_fence(h, cam);
      const u64 lo = lower_bound_sec(h, cam, t_low);
      const u64 ub = lower_bound_sec(h, cam, t_up);
      const u64 avail = ub > lo + 1 ? ub - 1 - lo : 0;  // [lo, lower_bound(t_up) - 1)
      first[cam] = lo;
      cnt[cam] = (u32)std::min<u64>(avail, cap1);
      if (cnt[cam] && lo < h->ring_reserved[cam] - std::min<u64>(h->ring_reserved[cam], h->ring_cap))
        FAIL(ESVO_ERR_STATE, "selected events were already overwritten in the event ring");
    }
    return ESVO_OK;
  };
  u64 first[2] = {0, 0};
  u32 cnt[2] = {0, 0};
  std::vector<u64> left_ts;
  {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    rc = select(first, cnt);
    if (rc) return rc;
    if (cnt[0] && cnt[1]) {
      const auto& v = h->ts_host[0];
      const size_t off = (size_t)(first[0] - h->ring_base[0]);
      left_ts.assign(v.begin() + off, v.begin() + off + cnt[0]);
    }
  }
  if (cnt[0] && cnt[1] && cnt[0] > h->max_ev)
    FAIL(ESVO_ERR_CAPACITY, "EM left selection (up to EM_NUM_EVENT_MATCHING + 1 events) exceeds max_events_per_tick");
  // ---- slicing (eventSlicingForEM, esvo_MVStereo.cpp:1096-1125)
  std::vector<EmSlice> slices;
  if (cnt[0] && cnt[1]) {
    const size_t num_slice = (size_t)std::floor((t_up - t_low) / em->slice_thickness);
    size_t it = 0;
    const size_t end = left_ts.size();
    for (size_t i = 0; i < num_slice; ++i) {
      EmSlice s{};
      const double t_end = ns_to_sec(ros_time_from_sec(ns_to_sec(left_ts[it]) + em->slice_thickness));
      size_t it_end = em_lower_bound_ns(left_ts, t_end);
      if (it_end == end) it_end--;
      s.begin = (u32)it;
      s.count = (u32)(it_end - it + 1);
      s.t_ns = left_ts[it + s.count / 2];
      slices.push_back(s);
      it = it_end + 1;
      if (it == end) break;
      if (slices.size() > h->max_poses) break;  // refused below; stop walking
    }
    if (slices.size() > h->max_poses) FAIL(ESVO_ERR_CAPACITY, "more EM slices than max_poses_per_tick");
  }
  EmState* e = h->em;
  auto record = [&]() {
    e->sel = esvo_em_selection_t{};
    e->sel.t_low_ns = t_low_ns; e->sel.t_up_ns = t_up_ns;
    e->sel.left_first = first[0]; e->sel.right_first = first[1];
    e->sel.left_count = cnt[0]; e->sel.right_count = cnt[1];
    e->sel.n_slices = (u32)slices.size();
    e->slices = slices;
    e->stats = esvo_em_stats_t{};
  };
  if (!cnt[0] || !cnt[1]) { record(); return ESVO_OK; }  // no tick
  static const double ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (auto& s : slices) {
    if (!(pose_fn && pose_fn(user, s.t_ns, s.T))) std::copy(ident, ident + 16, s.T);
  }
  rc = em_reserve_events(h, cnt[0], cnt[1]);
  if (rc) return rc;
  // ---- the selected events into the matcher's buffers.  Under mu_ring again: the selection is re-validated, the gather is
  // ENQUEUED on the front stream before the lock is released and both cameras' selected ranges are registered with the ingest
  // side (esvo_context::em_guard_lo): a push that would evict them drains the front stream first (push_begin, api_ingest.hip), so
  // the copies always read the events that were selected.  The guard is lifted once the copies have completed.
  EmGuard guard(h);
  {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    u64 f2[2];
    u32 c2[2];
    rc = select(f2, c2);
    if (rc) return rc;
    if (f2[0] != first[0] || f2[1] != first[1] || c2[0] != cnt[0] || c2[1] != cnt[1])
      FAIL(ESVO_ERR_STATE, "events inside the tick's window were staged while the tick selected them");
    h->em_guard_lo[0] = first[0];
    h->em_guard_lo[1] = first[1];
    guard.armed = true;
    rc = em_gather_ring(h, 0, first[0], cnt[0], e->d_left);
    if (!rc) rc = em_gather_ring(h, 1, first[1], cnt[1], e->d_right);
    if (rc) return rc;
  }
  record();
  std::vector<u32> slice_of;
  std::vector<double> T(16 * slices.size());
  std::vector<uint64_t> stamps(slices.size());
  for (size_t s = 0; s < slices.size(); ++s) {
    slice_of.insert(slice_of.end(), slices[s].count, (u32)s);
    std::copy(slices[s].T, slices[s].T + 16, T.begin() + 16 * s);
    stamps[s] = slices[s].t_ns;
  }
  u32 nm = 0;
  rc = em_match_device(h, em, 0, (u32)slice_of.size(), slice_of, T.data(), slices.size(), cnt[1], &nm);
  if (rc) return rc;
  guard.release();  // em_match_device waited for the stream: the gathers are complete
  if (nm == 0) return ESVO_OK;  // if (vEMP.size() == 0) return;  (esvo_MVStereo.cpp:268-271)
  std::vector<esvo_match_t> m(nm);
  HIPCHK(hipMemcpy(m.data(), e->d_out, sizeof(esvo_match_t) * nm, hipMemcpyDeviceToHost));
  if (mode == 0) {
    rc = esvo_map_fuse_matches_naive(h, m.data(), nm, T.data(), slices.size());
    if (rc) return rc;
    h->stats.last_matches = nm;
  } else {
    rc = esvo_map_set_poses(h, stamps.data(), T.data(), slices.size());
    if (rc) return rc;
    std::vector<esvo_depth_point_t> pts(nm);
    size_t np = 0;
    rc = esvo_map_refine(h, m.data(), nm, 1, pts.data(), pts.size(), &np);
    if (!rc) rc = esvo_map_push_frame(h, pts.data(), np, T.data(), slices.size());
    if (!rc) rc = esvo_map_fuse(h, nullptr);
    if (rc) return rc;
    h->stats.last_matches = nm;
  }
  h->stats.ticks++;
  return ESVO_OK;
}

int esvo_map_em_get_selection(esvo_handle h, esvo_em_selection_t* sel, uint32_t* slice_begin, uint32_t* slice_count,
                              uint64_t* slice_t_ns, double* slice_T, size_t cap) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  const EmState* e = h->em;
  const size_t ns = e ? e->slices.size() : 0;
  if (sel) *sel = e ? e->sel : esvo_em_selection_t{};
  if ((slice_begin || slice_count || slice_t_ns || slice_T) && ns > cap) FAIL(ESVO_ERR_CAPACITY, "slice arrays too small");
  for (size_t s = 0; s < ns; ++s) {
    if (slice_begin) slice_begin[s] = e->slices[s].begin;
    if (slice_count) slice_count[s] = e->slices[s].count;
    if (slice_t_ns) slice_t_ns[s] = e->slices[s].t_ns;
    if (slice_T) std::copy(e->slices[s].T, e->slices[s].T + 16, slice_T + 16 * s);
  }
  return ESVO_OK;
}

int esvo_map_em_stats(esvo_handle h, esvo_em_stats_t* out) {
  if (!h || !out) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  *out = h->em ? h->em->stats : esvo_em_stats_t{};
  return ESVO_OK;
}

void esvo_em_sizes(size_t out[4]) {
  out[0] = sizeof(esvo_em_params_t);
  out[1] = sizeof(esvo_em_selection_t);
  out[2] = sizeof(esvo_em_stats_t);
  out[3] = 0;
}

}  // extern "C"
