// api_track.hip — tracker residual / Jacobian evaluation on the device-resident Time Surface (see context.hpp).
#include "context.hpp"
#include "../../include/esvo_hip.hpp"  // esvo_hip::gauss_newton_register: the host-side driver esvo_track_register runs

// ---- Tracker residual / Jacobian evaluation ---------------------------------------
extern "C" {
int esvo_track_set_current(esvo_handle h, const uint8_t* ts_left, int kernel_size) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> _trk_lock(h->mu_track);
  if (kernel_size != 0 && kernel_size != 5)
    FAIL(ESVO_ERR_UNSUPPORTED, "tracker kernelSize must be 0 or 5 (the shipped configs); other sizes take OpenCV's float kernel path");
  HIPCHK(hipSetDevice(h->device));
  const size_t npx = (size_t)h->W * h->H;
  if (!h->d_trk_neg) {
    HIPCHK(h->d_trk_blur.alloc(npx));
    HIPCHK(h->d_trk_neg.alloc(npx));
    HIPCHK(h->d_trk_du.alloc(npx));
    HIPCHK(h->d_trk_dv.alloc(npx));
  }
  const uint8_t* src = h->d_ts[0];
  if (ts_left) {  // host image (TS node in another process)
    HIPCHK(hipMemcpyAsync(h->d_trk_neg, ts_left, npx, hipMemcpyHostToDevice, h->stream_t));
    src = h->d_trk_neg;  // staged here, consumed by the blur / copy below before track_images writes it
    if (kernel_size == 5) launch_gaussian5(src, h->d_trk_blur, h->W, h->H, h->stream_t);
    else HIPCHK(hipMemcpyAsync(h->d_trk_blur, src, npx, hipMemcpyDeviceToDevice, h->stream_t));
  } else {
    // The resident left surface belongs to the mapper group, whose thread may render the next one at any moment: the read
    // is enqueued behind the newest render (TE_R1) and marked, under mu_ts, so that the next render queues behind it.
    std::lock_guard<std::mutex> lt(h->mu_ts);
    if (!h->ts_valid[0]) FAIL(ESVO_ERR_STATE, "no device-resident left Time Surface: call esvo_ts_render(h, 0, ...) first");
    // (a render that runs alone records TE_R1 only once the tracker has shown up -- context.hpp, trk_used; renders are enqueued
    //  under mu_ts, held here: the first call drains the front stream instead, every later render has recorded the event)
    if (!h->trk_used.exchange(true)) HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamWaitEvent(h->stream_t, h->ts_ev[0].e[TE_R1], 0));  // the render of camera 0 on the front stream
    if (kernel_size == 5) launch_gaussian5(src, h->d_trk_blur, h->W, h->H, h->stream_t);
    else HIPCHK(hipMemcpyAsync(h->d_trk_blur, src, npx, hipMemcpyDeviceToDevice, h->stream_t));
    HIPCHK(hipEventRecord(h->evt_trk_read, h->stream_t));
    h->trk_read_pending = true;
  }
  launch_track_images(h->d_trk_blur, h->d_trk_neg, h->d_trk_du, h->d_trk_dv, h->W, h->H, h->stream_t);
  HIPCHK(hipGetLastError());
  // a host image is borrowed for the call; the resident surface needs no host wait (the evaluation calls run on this stream)
  if (ts_left) HIPCHK(hipStreamSynchronize(h->stream_t));
  h->trk_cur = true;
  return ESVO_OK;
}

int esvo_track_get_images(esvo_handle h, uint8_t* neg, int16_t* du, int16_t* dv) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> _trk_lock(h->mu_track);
  if (!h->trk_cur) FAIL(ESVO_ERR_STATE, "esvo_track_set_current has not been called");
  HIPCHK(hipSetDevice(h->device));
  const size_t npx = (size_t)h->W * h->H;
  if (neg) HIPCHK(hipMemcpyAsync(neg, h->d_trk_neg, npx, hipMemcpyDeviceToHost, h->stream_t));
  if (du) HIPCHK(hipMemcpyAsync(du, h->d_trk_du, npx * sizeof(int16_t), hipMemcpyDeviceToHost, h->stream_t));
  if (dv) HIPCHK(hipMemcpyAsync(dv, h->d_trk_dv, npx * sizeof(int16_t), hipMemcpyDeviceToHost, h->stream_t));
  HIPCHK(hipStreamSynchronize(h->stream_t));
  return ESVO_OK;
}

// room for a reference of n points (caller holds mu_track)
static int track_reserve(esvo_context* h, size_t n) {
  if (n > h->trk_cap) {
    HIPCHK(hipStreamSynchronize(h->stream_t));
    (void)h->d_trk_xyz.release(); (void)h->d_trk_pts.release(); (void)h->d_trk_out.release(); (void)h->h_trk_xyz.release();
    h->trk_cap = 0; h->trk_n = 0;
    const size_t cap = std::max<size_t>(n, 4096);
    HIPCHK(h->h_trk_xyz.alloc(cap * 3));
    HIPCHK(h->d_trk_xyz.alloc(cap * 3));
    HIPCHK(h->d_trk_pts.alloc(cap * 3));
    HIPCHK(h->d_trk_out.alloc(cap * 6));
    h->trk_cap = cap;
  }
  return ESVO_OK;
}

int esvo_track_set_reference(esvo_handle h, const float* xyz_world, size_t n, const double T_world_ref[16]) {
  if (!h || (n && !xyz_world) || !T_world_ref) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> _trk_lock(h->mu_track);
  HIPCHK(hipSetDevice(h->device));
  { int rc = track_reserve(h, n); if (rc) return rc; }
  h->trk_n = n;
  if (n) {
    TrackRef r;
    std::memcpy(r.T, T_world_ref, sizeof(r.T));
    // xyz_world is borrowed for the call: it is copied into a pinned staging buffer (24 KB for 2000 points) instead of waiting
    // for the device -- the previous upload out of that buffer finished long ago (every evaluation call ends with a wait on
    // this stream), the stream wait below only covers a caller that sets two references in a row
    if (h->trk_xyz_inflight) HIPCHK(hipStreamSynchronize(h->stream_t));
    std::memcpy(h->h_trk_xyz, xyz_world, n * 3 * sizeof(float));
    h->trk_xyz_inflight = true;
    HIPCHK(hipMemcpyAsync(h->d_trk_xyz, h->h_trk_xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream_t));
    launch_track_reference(h->d_trk_xyz, (u32)n, r, h->d_trk_pts, h->stream_t);
    HIPCHK(hipGetLastError());
  }
  return ESVO_OK;
}

// setProblem's point loop on the device-resident cloud of esvo_map_cloud_build: nothing but the indices travels
int esvo_track_set_reference_from_cloud(esvo_handle h, const uint32_t* order, size_t n, const double T_world_ref[16]) {
  if (!h || !T_world_ref) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> _trk_lock(h->mu_track);
  HIPCHK(hipSetDevice(h->device));
  // The snapshot cannot change under this call's feet: a build fills the OTHER buffer, and the one after it -- the first that
  // writes this one again -- queues behind evt_cloud_read.  cloud_cur / cloud_n are re-read under mu_cloud where the gather is
  // enqueued; a build that has published meanwhile only makes this call gather out of the newer snapshot, so the indices are
  // checked there, against the count of the buffer that is read.
  size_t cloud_n = 0;
  {
    std::lock_guard<std::mutex> lc(h->mu_cloud);
    if (h->cloud_cur < 0) FAIL(ESVO_ERR_STATE, "no device-resident point cloud: call esvo_map_cloud_build first");
    cloud_n = h->cloud_n;
  }
  if (!order) n = std::min(n, cloud_n);  // numPoints_ = min(size, MAX_REGISTRATION_POINTS_), :38-40
  if (n > 0xffffffffull) FAIL(ESVO_ERR_CAPACITY, "more reference points than 32-bit indices address");
  if (n > h->trk_cap) {  // (before anything else changes: the reserve drops the previous reference's buffers)
    if (order)
      for (size_t i = 0; i < n; ++i)
        if (order[i] >= cloud_n) FAIL(ESVO_ERR_INVALID_ARG, "order holds an index beyond the cloud's point count");
    int rc = track_reserve(h, n);
    if (rc) return rc;
  }
  if (order && n) {
    // the indices go through the pinned staging buffer the xyz take on the host route (4 of its 12 bytes per point) into
    // d_trk_xyz, which this route does not otherwise use
    if (h->trk_xyz_inflight) HIPCHK(hipStreamSynchronize(h->stream_t));
  }
  TrackRef r;
  std::memcpy(r.T, T_world_ref, sizeof(r.T));
  std::lock_guard<std::mutex> lc(h->mu_cloud);
  if (h->cloud_cur < 0) FAIL(ESVO_ERR_STATE, "no device-resident point cloud: call esvo_map_cloud_build first");
  const int cb = h->cloud_cur;
  cloud_n = h->cloud_n;
  if (!order) n = std::min(n, cloud_n);
  else
    for (size_t i = 0; i < n; ++i)
      if (order[i] >= cloud_n) FAIL(ESVO_ERR_INVALID_ARG, "order holds an index beyond the cloud's point count");
  h->trk_n = n;
  if (n == 0) return ESVO_OK;
  const u32* d_order = nullptr;
  if (order) {
    std::memcpy(h->h_trk_xyz, order, n * sizeof(u32));
    h->trk_xyz_inflight = true;
    HIPCHK(hipMemcpyAsync(h->d_trk_xyz, h->h_trk_xyz, n * sizeof(u32), hipMemcpyHostToDevice, h->stream_t));
    d_order = reinterpret_cast<const u32*>(h->d_trk_xyz.get());
  }
  HIPCHK(hipStreamWaitEvent(h->stream_t, h->evt_cloud_built[cb], 0));
  launch_track_reference_gather(h->d_cloud_xyz[cb], d_order, (u32)n, r, h->d_trk_pts, h->stream_t);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->evt_cloud_read[cb], h->stream_t));
  h->cloud_read_pending[cb] = true;
  return ESVO_OK;
}

// the order the stochastic swaps of RegProblemLM::setProblem (:48-49) leave, from the draws alone (host code, no handle)
int esvo_track_stochastic_order(size_t n_cloud, size_t n_take, const uint32_t* draws, uint32_t* order) {
  esvo_context* h = nullptr;
  n_take = std::min(n_take, n_cloud);
  if (n_take && (!draws || !order)) return ESVO_ERR_INVALID_ARG;
  if (n_cloud > 0xffffffffull) FAIL(ESVO_ERR_CAPACITY, "more cloud points than 32-bit indices address");
  esvo_hip::stochastic_order(n_cloud, n_take, draws, order);
  return ESVO_OK;
}
}  // extern "C"

namespace {
void fill_track_args(esvo_context* h, TrackArgs& a) {
  a.pts = h->d_trk_pts; a.neg = h->d_trk_neg; a.du = h->d_trk_du; a.dv = h->d_trk_dv; a.mask = h->d_mask;
  std::memcpy(a.P, h->dp.camL.P, sizeof(a.P));
  a.W = h->W; a.H = h->H;
}
}  // namespace

extern "C" {
int esvo_track_residuals(esvo_handle h, const double T_left_ref[16], size_t offset, size_t count, int ls_norm,
                         double huber_threshold, double* fvec, size_t* n_out) {
  if (!h || !T_left_ref || !n_out || (ls_norm != ESVO_TRACK_L2 && ls_norm != ESVO_TRACK_HUBER)) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> _trk_lock(h->mu_track);
  if (!h->trk_cur) FAIL(ESVO_ERR_STATE, "esvo_track_set_current has not been called");
  HIPCHK(hipSetDevice(h->device));
  const size_t m = offset >= h->trk_n ? 0 : std::min(count, h->trk_n - offset);  // setStochasticSampling, :71-88
  *n_out = m;
  if (m == 0) return ESVO_OK;
  if (!fvec) return ESVO_ERR_INVALID_ARG;
  TrackArgs a;
  fill_track_args(h, a);
  TrackPose pose;
  std::memcpy(pose.T, T_left_ref, sizeof(pose.T));
  std::memset(pose.Jc, 0, sizeof(pose.Jc));
  launch_track_residuals(a, pose, (u32)offset, (u32)m, ls_norm == ESVO_TRACK_HUBER, huber_threshold, h->d_trk_out, h->stream_t);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(fvec, h->d_trk_out, m * sizeof(double), hipMemcpyDeviceToHost, h->stream_t));
  HIPCHK(hipStreamSynchronize(h->stream_t));
  h->trk_xyz_inflight = false;
  return ESVO_OK;
}

int esvo_track_jacobian(esvo_handle h, const double R[9], const double t[3], size_t offset, size_t count, double* fjac,
                        size_t* n_out) {
  if (!h || !R || !t || !n_out) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> _trk_lock(h->mu_track);
  if (!h->trk_cur) FAIL(ESVO_ERR_STATE, "esvo_track_set_current has not been called");
  HIPCHK(hipSetDevice(h->device));
  const size_t m = offset >= h->trk_n ? 0 : std::min(count, h->trk_n - offset);
  *n_out = m;
  if (m == 0) return ESVO_OK;
  if (!fjac) return ESVO_ERR_INVALID_ARG;
  TrackArgs a;
  fill_track_args(h, a);
  TrackPose pose;  // T_left_ref = [R^T | -R^T t] (:203-205), J_constPart = R^T diag(1/P11, 1/P22; 0) (:189-194)
  std::memset(pose.T, 0, sizeof(pose.T));
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) pose.T[r * 4 + c] = R[c * 3 + r];
    pose.T[r * 4 + 3] = (-R[0 * 3 + r] * t[0] + -R[1 * 3 + r] * t[1]) + -R[2 * 3 + r] * t[2];
  }
  pose.T[15] = 1.0;
  const double iP11 = 1.0 / a.P[0], iP22 = 1.0 / a.P[5];
  for (int r = 0; r < 3; ++r) { pose.Jc[r * 2 + 0] = R[0 * 3 + r] * iP11; pose.Jc[r * 2 + 1] = R[1 * 3 + r] * iP22; }
  launch_track_jacobian(a, pose, (u32)offset, (u32)m, h->d_trk_out, h->stream_t);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(fjac, h->d_trk_out, m * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream_t));
  HIPCHK(hipStreamSynchronize(h->stream_t));
  h->trk_xyz_inflight = false;
  return ESVO_OK;
}

static_assert(ESVO_TRACK_MAX_POSES == TRK_NE_MAX_POSES, "the ABI's pose limit is the kernel's");
static_assert(ESVO_TRACK_SOLVE_MAX_ITERATIONS == TRK_SOLVE_MAX_ITERATIONS, "the ABI's iteration limit is the kernel's");
// f = operator()(0), J = df(0) and their products in one launch: H = J^T J (6 x 6, row-major, symmetric), b = J^T f, cost = |f|^2;
// n_poses of them (one workgroup each) share the launch and the read-back
int esvo_track_normal_equations_batch(esvo_handle h, int n_poses, const double* R, const double* t, size_t offset, size_t count,
                                      int ls_norm, double huber_threshold, double* H, double* b, double* cost, size_t* n_out) {
  if (!h || !R || !t || !H || !b || !n_out || n_poses < 1 || n_poses > ESVO_TRACK_MAX_POSES ||
      (ls_norm != ESVO_TRACK_L2 && ls_norm != ESVO_TRACK_HUBER))
    return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> _trk_lock(h->mu_track);
  if (!h->trk_cur) FAIL(ESVO_ERR_STATE, "esvo_track_set_current has not been called");
  HIPCHK(hipSetDevice(h->device));
  const size_t m = offset >= h->trk_n ? 0 : std::min(count, h->trk_n - offset);
  *n_out = m;
  std::memset(H, 0, sizeof(double) * 36 * n_poses);
  std::memset(b, 0, sizeof(double) * 6 * n_poses);
  if (cost) std::memset(cost, 0, sizeof(double) * n_poses);
  if (m == 0) return ESVO_OK;
  if (!h->h_trk_ne) HIPCHK(h->h_trk_ne.alloc(TRK_NE_TERMS * TRK_NE_MAX_POSES));
  TrackArgs a;
  fill_track_args(h, a);
  TrackPoseSet set;  // as esvo_track_jacobian: T_left_ref = [R^T | -R^T t] (RegProblemLM.cpp:203-205), J_constPart (:189-194)
  std::memset(&set, 0, sizeof(set));
  const double iP11 = 1.0 / a.P[0], iP22 = 1.0 / a.P[5];
  for (int q = 0; q < n_poses; ++q) {
    TrackPose& pose = set.p[q];
    const double *Rq = R + 9 * q, *tq = t + 3 * q;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) pose.T[r * 4 + c] = Rq[c * 3 + r];
      pose.T[r * 4 + 3] = (-Rq[0 * 3 + r] * tq[0] + -Rq[1 * 3 + r] * tq[1]) + -Rq[2 * 3 + r] * tq[2];
    }
    pose.T[15] = 1.0;
    for (int r = 0; r < 3; ++r) { pose.Jc[r * 2 + 0] = Rq[0 * 3 + r] * iP11; pose.Jc[r * 2 + 1] = Rq[1 * 3 + r] * iP22; }
  }
  // The kernel's one write per pose (28 sums) goes straight into the pinned host row -- no copy operation behind the launch -- and the
  // host polls for the end of the launch (10-20 us of kernel: sleeping on the completion interrupt would cost as much again).  One
  // of these round trips per iteration is the whole latency of the tracker's loop.
  launch_track_normal(a, set, n_poses, (u32)offset, (u32)m, ls_norm == ESVO_TRACK_HUBER, huber_threshold, h->h_trk_ne, h->stream_t);
  HIPCHK(hipGetLastError());
  HIPCHK(esvo_wait_stream(h->stream_t, true));
  h->trk_xyz_inflight = false;
  for (int q = 0; q < n_poses; ++q) {
    const double* s = h->h_trk_ne + (size_t)q * TRK_NE_TERMS;
    double* Hq = H + 36 * q;
    int n = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) { Hq[i * 6 + j] = Hq[j * 6 + i] = s[n]; ++n; }
    for (int i = 0; i < 6; ++i) b[6 * q + i] = s[21 + i];
    if (cost) cost[q] = s[27];
  }
  return ESVO_OK;
}
int esvo_track_normal_equations(esvo_handle h, const double R[9], const double t[3], size_t offset, size_t count, int ls_norm,
                                double huber_threshold, double H[36], double b[6], double* cost, size_t* n_out) {
  return esvo_track_normal_equations_batch(h, 1, R, t, offset, count, ls_norm, huber_threshold, H, b, cost, n_out);
}

// The registration of one frame: esvo_hip::gauss_newton_register (include/esvo_hip.hpp, host C++) over
// esvo_track_normal_equations_batch -- the (up to three) trial steps of an iteration in one launch, 224 bytes back per trial.
int esvo_track_register(esvo_handle h, size_t n_points, double R[9], double t[3], int ls_norm, double huber_threshold,
                        int max_iterations, double damping, double* rms, int* iterations) {
  if (!h || !R || !t || max_iterations < 1) return ESVO_ERR_INVALID_ARG;
  int rc = ESVO_OK;
  auto ne = [&](int, int k, const double* Rc, const double* tc, double* H, double* b, double* cost, size_t* n) {
    rc = esvo_track_normal_equations_batch(h, k, Rc, tc, 0, n_points, ls_norm, huber_threshold, H, b, cost, n);
    return rc == ESVO_OK;
  };
  const esvo_hip::Registration res = esvo_hip::gauss_newton_register(ne, R, t, max_iterations, damping);
  if (rc) return rc;
  std::memcpy(R, res.R, sizeof(res.R));
  std::memcpy(t, res.t, sizeof(res.t));
  if (rms) *rms = res.rms;
  if (iterations) *iterations = res.iterations;
  return ESVO_OK;
}
// esvo_track_register with the batch schedule, a trace, and -- on_device -- the whole loop in one launch (kernels_track.hip)
int esvo_track_solve(esvo_handle h, const esvo_track_solve_params_t* prm, double R[9], double t[3], esvo_track_solve_info_t* info,
                     esvo_track_iter_t* trace, size_t trace_cap) {
  if (!h || !prm || !R || !t || (prm->ls_norm != ESVO_TRACK_L2 && prm->ls_norm != ESVO_TRACK_HUBER) || prm->max_iterations < 1 ||
      prm->max_iterations > ESVO_TRACK_SOLVE_MAX_ITERATIONS)
    return ESVO_ERR_INVALID_ARG;
  if (!trace) trace_cap = 0;
  size_t N = 0;
  {
    std::lock_guard<std::mutex> _trk_lock(h->mu_track);
    if (!h->trk_cur) FAIL(ESVO_ERR_STATE, "esvo_track_set_current has not been called");
    N = std::min<size_t>(prm->n_points, h->trk_n);
  }
  const size_t B = prm->batch_size;
  const bool batches = B != 0 && B < N;
  const size_t n_batches = batches ? std::max<size_t>(N / B, 1) : 1;
  if (!prm->on_device) {  // today's path: the host loop over one launch per evaluation, plus the recorder
    int rc = ESVO_OK, launches = 0;
    auto ne = [&](int it, int k, const double* Rc, const double* tc, double* H, double* b, double* cost, size_t* n) {
      rc = esvo_track_normal_equations_batch(h, k, Rc, tc, batches ? ((size_t)it % n_batches) * B : 0, batches ? B : N, prm->ls_norm,
                                             prm->huber_threshold, H, b, cost, n);
      if (rc == ESVO_OK && *n) ++launches;
      return rc == ESVO_OK;
    };
    esvo_track_iter_t rec[ESVO_TRACK_SOLVE_MAX_ITERATIONS];
    esvo_hip::RegistrationTrace tr;
    tr.rec = rec; tr.cap = ESVO_TRACK_SOLVE_MAX_ITERATIONS;
    const esvo_hip::Registration res = esvo_hip::gauss_newton_register(ne, R, t, prm->max_iterations, prm->damping, !batches, &tr);
    if (rc) return rc;
    std::memcpy(R, res.R, sizeof(res.R));
    std::memcpy(t, res.t, sizeof(res.t));
    if (info) { info->rms = res.rms; info->iterations = res.iterations; info->ok = res.ok ? 1 : 0; info->stop = tr.stop; info->launches = launches; }
    for (size_t it = 0; it < std::min<size_t>(trace_cap, (size_t)res.iterations); ++it) {
      trace[it] = rec[it];
      trace[it].offset = batches ? (uint32_t)((it % n_batches) * B) : 0u;
    }
    return ESVO_OK;
  }
  std::lock_guard<std::mutex> _trk_lock(h->mu_track);
  if (!h->trk_cur) FAIL(ESVO_ERR_STATE, "esvo_track_set_current has not been called");
  HIPCHK(hipSetDevice(h->device));
  N = std::min<size_t>(prm->n_points, h->trk_n);  // (a reference set between the two locks)
  if (!h->h_trk_solve) HIPCHK(h->h_trk_solve.alloc(1));
  TrackArgs a;
  fill_track_args(h, a);
  TrackSolveArgs s;
  std::memcpy(s.R0, R, sizeof(s.R0));
  std::memcpy(s.t0, t, sizeof(s.t0));
  s.huber_threshold = prm->huber_threshold; s.damping = prm->damping;
  s.n_points = (u32)N; s.batch = (u32)std::min<size_t>(B, N);  // (>= N: one batch, as 0)
  s.huber = prm->ls_norm == ESVO_TRACK_HUBER; s.max_iterations = prm->max_iterations;
  // one launch, one write phase into the pinned block, and the host polls for the end of the launch as the per-evaluation path does
  launch_track_solve(a, s, h->h_trk_solve, h->stream_t);
  HIPCHK(hipGetLastError());
  HIPCHK(esvo_wait_stream(h->stream_t, true));
  h->trk_xyz_inflight = false;
  const TrackSolveOut& o = *h->h_trk_solve;
  std::memcpy(R, o.R, sizeof(o.R));
  std::memcpy(t, o.t, sizeof(o.t));
  if (info) *info = o.info;
  for (size_t it = 0; it < std::min<size_t>(trace_cap, (size_t)o.info.iterations); ++it) trace[it] = o.trace[it];
  return ESVO_OK;
}

// The visualisation block of RegProblemSolverLM (RegProblemSolverLM.cpp:180-209) on the tracker's own stream and buffers
// (kernels_track_viz.hip states the image); nothing of the mapper group is touched, so esvo_map_get_debug_images may run beside it.
int esvo_track_reprojection_map(esvo_handle h, const double R[9], const double t[3], size_t n_points, double inv_depth_min,
                                double inv_depth_max, uint8_t* bgr_out, size_t* n_inside) {
  if (!h || !R || !t || !std::isfinite(inv_depth_min) || !std::isfinite(inv_depth_max) || inv_depth_max == inv_depth_min)
    return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> _trk_lock(h->mu_track);
  if (!h->trk_cur) FAIL(ESVO_ERR_STATE, "esvo_track_set_current has not been called");
  HIPCHK(hipSetDevice(h->device));
  const size_t npx = (size_t)h->W * h->H;
  if (!h->d_trk_viz_cnt) {
    if (!h->d_trk_viz_bgr) HIPCHK(h->d_trk_viz_bgr.alloc((npx + 3) / 4 * 12));
    if (!h->d_trk_viz_owner) HIPCHK(h->d_trk_viz_owner.alloc((npx + 3) / 4 * 4));
    if (!h->d_trk_viz_jet) HIPCHK(h->d_trk_viz_jet.alloc(768));
    uint8_t jet[768];
    jet256_bgr(jet);
    HIPCHK(hipMemsetAsync(h->d_trk_viz_owner, 0, (npx + 3) / 4 * 4 * sizeof(u32), h->stream_t));  // the only clear: every call leaves it 0
    HIPCHK(hipMemcpyAsync(h->d_trk_viz_jet, jet, 768, hipMemcpyHostToDevice, h->stream_t));
    HIPCHK(hipStreamSynchronize(h->stream_t));  // (jet lives on this frame)
    HIPCHK(h->d_trk_viz_cnt.alloc(1));  // last: marks the set complete
  }
  TrackArgs a;
  fill_track_args(h, a);
  TrackPose pose;  // T_left_ref = [R^T | -R^T t] exactly as esvo_track_jacobian builds it (:191-192)
  std::memset(&pose, 0, sizeof(pose));
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) pose.T[r * 4 + c] = R[c * 3 + r];
    pose.T[r * 4 + 3] = (-R[0 * 3 + r] * t[0] + -R[1 * 3 + r] * t[1]) + -R[2 * 3 + r] * t[2];
  }
  pose.T[15] = 1.0;
  const u32 n = (u32)std::min<size_t>(std::min<size_t>(n_points, h->trk_n), 0xffffffffull);  // numVisualization, :194
  launch_track_reprojection_map(a, pose, n, inv_depth_min, inv_depth_max, h->d_trk_viz_jet, h->d_trk_viz_owner, h->d_trk_viz_bgr,
                                h->d_trk_viz_cnt, h->stream_t);
  HIPCHK(hipGetLastError());
  h->trk_viz_valid = true;
  u32 cnt = 0;
  if (bgr_out) HIPCHK(hipMemcpyAsync(bgr_out, h->d_trk_viz_bgr, npx * 3, hipMemcpyDeviceToHost, h->stream_t));
  if (n_inside) HIPCHK(hipMemcpyAsync(&cnt, h->d_trk_viz_cnt, sizeof(u32), hipMemcpyDeviceToHost, h->stream_t));
  if (bgr_out || n_inside) {
    HIPCHK(hipStreamSynchronize(h->stream_t));
    h->trk_xyz_inflight = false;
  }
  if (n_inside) *n_inside = cnt;
  return ESVO_OK;
}

int esvo_track_reprojection_map_device(esvo_handle h, const uint8_t** d_bgr) {
  if (!h || !d_bgr) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> _trk_lock(h->mu_track);
  if (!h->trk_viz_valid) FAIL(ESVO_ERR_STATE, "esvo_track_reprojection_map has not been called");
  *d_bgr = h->d_trk_viz_bgr;
  return ESVO_OK;
}

void esvo_track_sizes(size_t out[4]) {
  out[0] = sizeof(esvo_track_solve_params_t);
  out[1] = sizeof(esvo_track_iter_t);
  out[2] = sizeof(esvo_track_solve_info_t);
  out[3] = ESVO_TRACK_SOLVE_MAX_ITERATIONS;
}
}  // extern "C"
