// api_out.hip — what leaves the mapper: DepthMap, point clouds, debug images, the last frame, statistics (see context.hpp).
#include "context.hpp"

extern "C" {
// ---- Outputs -----------------------------------------------------------------------------------------
int esvo_map_get_depth_points(esvo_handle h, esvo_depth_point_t* out, size_t cap, size_t* n) {
  if (!h || !n) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  std::vector<esvo_depth_point_t> v;
  int rc = export_map(h, v, nullptr);
  if (rc) return rc;
  *n = v.size();
  if (out) {
    if (v.size() > cap) FAIL(ESVO_ERR_CAPACITY, "output array too small for the DepthMap");
    if (!v.empty()) std::memcpy(out, v.data(), sizeof(esvo_depth_point_t) * v.size());
  }
  return ESVO_OK;
}

int esvo_map_get_committed(esvo_handle h, esvo_depth_point_t* out, size_t cap, size_t* n, uint64_t* t_ns) {
  if (!h || !n) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  if (t_ns) *t_ns = h->committed_t_ns;
  *n = 0;
  if (h->committed_t_ns == 0) return ESVO_OK;
  std::vector<esvo_depth_point_t> v;
  int rc = export_map(h, v, nullptr);  // back stream only: a pending tick's front stage keeps running
  if (rc) return rc;
  *n = v.size();
  if (out) {
    if (v.size() > cap) FAIL(ESVO_ERR_CAPACITY, "output array too small for the DepthMap");
    std::memcpy(out, v.data(), sizeof(esvo_depth_point_t) * v.size());
  }
  return ESVO_OK;
}

int esvo_map_get_pointcloud_xyz(esvo_handle h, float* out_xyz, size_t cap_points, size_t* n) {
  if (!h || !n) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  std::vector<esvo_depth_point_t> v;
  int rc = export_map(h, v, nullptr);
  if (rc) return rc;
  *n = v.size();
  if (out_xyz) {
    if (v.size() > cap_points) FAIL(ESVO_ERR_CAPACITY, "output array too small for the point cloud");
    const double* T = h->T_world_frame;  // publishPointCloud, esvo_Mapping.cpp:925-932
    for (size_t i = 0; i < v.size(); ++i)
      for (int r = 0; r < 3; ++r)
        out_xyz[3 * i + r] = (float)(((T[r * 4 + 0] * v[i].p_cam[0] + T[r * 4 + 1] * v[i].p_cam[1]) + T[r * 4 + 2] * v[i].p_cam[2]) + T[r * 4 + 3]);
  }
  return ESVO_OK;
}

// The same cloud built and kept on the device (kernels_cloud.hip; context.hpp: cloud_*): no element leaves the device, the
// host reads two counters.
int esvo_map_cloud_build(esvo_handle h, size_t* n) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (h->sharded) FAIL(ESVO_ERR_STATE, "handle is sharded");
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  const size_t npx = (size_t)h->W * h->H;
  if (!h->d_cloud_xyz[1]) {  // first build: nothing of this state is in use yet
    for (int k = 0; k < 2; ++k) {
      if (!h->d_cloud_xyz[k]) HIPCHK(h->d_cloud_xyz[k].alloc(npx * 3));
      HIPCHK(h->evt_cloud_built[k].create(hipEventDisableTiming));
      HIPCHK(h->evt_cloud_read[k].create(hipEventDisableTiming));
    }
    if (!h->d_cloud_cnt) HIPCHK(h->d_cloud_cnt.alloc(2));
    if (!h->h_cloud_cnt) HIPCHK(h->h_cloud_cnt.alloc(2));
  }
  const u32 id_n = h->map_id_bound;
  if (id_n > h->cloud_id_cap) {  // (the id arrays are read on the back stream only, by earlier builds: all complete -- every build waits for its count)
    (void)h->d_cloud_ids.release(); (void)h->d_cloud_scan.release();
    h->cloud_id_cap = 0;
    const size_t cap = std::max<size_t>((size_t)id_n + id_n / 4, 4096);
    HIPCHK(h->d_cloud_ids.alloc(3 * cap));
    HIPCHK(h->d_cloud_scan.alloc(scan_scratch_elems(cap) + 8));
    h->cloud_id_cap = cap;
  }
  int w;
  {
    std::lock_guard<std::mutex> lc(h->mu_cloud);
    w = h->cloud_cur < 0 ? 0 : h->cloud_cur ^ 1;  // not the current one: the tracker may be gathering out of that right now
    if (h->cloud_read_pending[w]) {  // its last gather out of this buffer (two builds ago): waited for on the device
      HIPCHK(hipStreamWaitEvent(h->stream_b, h->evt_cloud_read[w], 0));
      h->cloud_read_pending[w] = false;
    }
  }
  u32* present = h->d_cloud_ids;
  launch_map_cloud(h->d_map_cur, id_n, present, present + h->cloud_id_cap, present + 2 * h->cloud_id_cap, h->d_cloud_cnt, h->d_cloud_scan,
                   h->T_world_frame, h->d_cloud_xyz[w], (u32)npx, h->dp, h->stream_b);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h->h_cloud_cnt, h->d_cloud_cnt, sizeof(u32) * 2, hipMemcpyDeviceToHost, h->stream_b));
  HIPCHK(hipEventRecord(h->evt_cloud_built[w], h->stream_b));
  HIPCHK(esvo_wait_stream(h->stream_b, true));
  if (h->h_cloud_cnt[1]) FAIL(ESVO_ERR_STATE, "DepthMap elements carry creation ids beyond the bound of the last fusion (internal error)");
  const size_t cnt = h->h_cloud_cnt[0];
  {
    std::lock_guard<std::mutex> lc(h->mu_cloud);
    h->cloud_cur = w;
    h->cloud_n = cnt;
    h->cloud_t_ns = h->committed_t_ns;
  }
  h->stats.last_map_size = (u32)cnt;  // (as the host read-out does)
  if (n) *n = cnt;
  return ESVO_OK;
}

int esvo_map_cloud_get(esvo_handle h, float* out_xyz, size_t cap_points, size_t* n) {
  if (!h || !n) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);  // (no build meanwhile: the snapshot is complete and stays where it is)
  HIPCHK(hipSetDevice(h->device));
  const size_t cnt = h->cloud_cur < 0 ? 0 : h->cloud_n;
  *n = cnt;
  if (!out_xyz || !cnt) return ESVO_OK;
  if (cnt > cap_points) FAIL(ESVO_ERR_CAPACITY, "output array too small for the point cloud");
  HIPCHK(hipMemcpy(out_xyz, h->d_cloud_xyz[h->cloud_cur], cnt * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return ESVO_OK;
}

int esvo_map_cloud_device(esvo_handle h, const float** d_xyz, size_t* n, uint64_t* t_ns) {
  if (!h || !d_xyz || !n) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  const bool have = h->cloud_cur >= 0;
  *d_xyz = have ? h->d_cloud_xyz[h->cloud_cur] : nullptr;
  *n = have ? h->cloud_n : 0;
  if (t_ns) *t_ns = have ? h->cloud_t_ns : 0;
  return ESVO_OK;
}

// pc_near_ of publishPointCloud (esvo_Mapping.cpp:925-932): what the global-cloud voxel filter is fed
int esvo_map_get_pointcloud_near_xyz(esvo_handle h, double visualize_range, float* out_xyz, size_t cap_points, size_t* n) {
  if (!h || !n) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  std::vector<esvo_depth_point_t> v;
  int rc = export_map(h, v, nullptr);
  if (rc) return rc;
  const double* T = h->T_world_frame;
  size_t k = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    const double* q = v[i].p_cam;
    if (!(std::sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) < visualize_range)) continue;
    if (out_xyz) {
      if (k >= cap_points) FAIL(ESVO_ERR_CAPACITY, "output array too small for the point cloud");
      for (int r = 0; r < 3; ++r)
        out_xyz[3 * k + r] = (float)(((T[r * 4 + 0] * q[0] + T[r * 4 + 1] * q[1]) + T[r * 4 + 2] * q[2]) + T[r * 4 + 3]);
    }
    ++k;
  }
  *n = k;
  return ESVO_OK;
}

// pcl::VoxelGrid<PointXYZ> with a cubic leaf (esvo_Mapping.cpp:960-964): host code, as in the reference -- it runs on a
// few ten thousand points once per visualizeGPC_interval.  Float arithmetic throughout; one centroid per occupied voxel
// in ascending voxel index (x fastest); the points of a voxel are summed in input order.
int esvo_voxel_filter_xyz(const float* xyz, size_t n, float leaf, float* out_xyz, size_t cap_points, size_t* n_out) {
  esvo_context* h = nullptr;
  if ((n && !xyz) || !n_out || !(leaf > 0)) return ESVO_ERR_INVALID_ARG;
  std::vector<size_t> fin;
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    const float* p = xyz + 3 * i;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
    if (fin.empty()) for (int c = 0; c < 3; ++c) mn[c] = mx[c] = p[c];
    for (int c = 0; c < 3; ++c) { mn[c] = std::min(mn[c], p[c]); mx[c] = std::max(mx[c], p[c]); }
    fin.push_back(i);
  }
  *n_out = 0;
  if (fin.empty()) return ESVO_OK;
  const float inv = 1.0f / leaf;
  long long minb[3], divb[3];
  for (int c = 0; c < 3; ++c) {
    minb[c] = (long long)std::floor(mn[c] * inv);
    divb[c] = (long long)std::floor(mx[c] * inv) - minb[c] + 1;
  }
  if ((double)divb[0] * (double)divb[1] * (double)divb[2] > 2147483647.0)
    FAIL(ESVO_ERR_CAPACITY, "leaf size too small for the extent of the cloud (voxel index overflows, as in pcl::VoxelGrid)");
  std::vector<std::pair<long long, size_t>> idx;
  idx.reserve(fin.size());
  for (size_t i : fin) {
    const float* p = xyz + 3 * i;
    const long long a = (long long)std::floor(p[0] * inv) - minb[0], b = (long long)std::floor(p[1] * inv) - minb[1],
                    c = (long long)std::floor(p[2] * inv) - minb[2];
    idx.emplace_back(a + b * divb[0] + c * divb[0] * divb[1], i);
  }
  std::stable_sort(idx.begin(), idx.end(),
                   [](const std::pair<long long, size_t>& x, const std::pair<long long, size_t>& y) { return x.first < y.first; });
  size_t k = 0;
  for (size_t a = 0; a < idx.size();) {
    size_t b = a;
    float c[3] = {0, 0, 0};
    while (b < idx.size() && idx[b].first == idx[a].first) {
      for (int d = 0; d < 3; ++d) c[d] += xyz[3 * idx[b].second + d];
      ++b;
    }
    if (out_xyz) {
      if (k >= cap_points) FAIL(ESVO_ERR_CAPACITY, "output array too small for the filtered cloud");
      for (int d = 0; d < 3; ++d) out_xyz[3 * k + d] = c[d] / (float)(b - a);
    }
    ++k;
    a = b;
  }
  *n_out = k;
  return ESVO_OK;
}

// Visualization::plot_map x 4 with publishMappingResults' arguments (esvo_Mapping.cpp:868-884)
int esvo_map_get_debug_images(esvo_handle h, double age_max_range, uint8_t* inv_depth_bgr, uint8_t* stdvar_bgr, uint8_t* age_bgr,
                              uint8_t* cost_bgr) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  const size_t npx = (size_t)h->W * h->H;
  if (!h->d_viz_bgr) {
    HIPCHK(h->d_viz_bgr.alloc(npx * 3));
    HIPCHK(h->d_viz_owner.alloc(npx));
    HIPCHK(h->d_viz_jet.alloc(768));
    uint8_t jet[768];
    jet256_bgr(jet);
    HIPCHK(hipMemcpy(h->d_viz_jet, jet, 768, hipMemcpyHostToDevice));
  }
  const esvo_params_t& p = h->prm;
  const double cost_thr = p.residual_vis_threshold * p.residual_vis_threshold * (p.patch_size_x * p.patch_size_y);  // esvo_Mapping.cpp:97
  struct { uint8_t* out; int type; double mx, mn, t1, t2; } img[4] = {
      {inv_depth_bgr, 0, p.invdepth_max, p.invdepth_min, p.stdvar_vis_threshold, p.age_vis_threshold},
      {stdvar_bgr, 1, p.stdvar_vis_threshold, 0.0, p.stdvar_vis_threshold, 0.0},
      {age_bgr, 3, age_max_range, 0.0, p.age_vis_threshold, 0.0},
      {cost_bgr, 2, cost_thr, 0.0, cost_thr, 0.0}};
  for (auto& im : img) {
    if (!im.out) continue;
    launch_debug_image(h->d_map_cur, h->d_viz_owner, h->d_viz_bgr, h->d_viz_jet, im.type, im.mx, im.mn, im.t1, im.t2, h->dp, h->stream_b);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(im.out, h->d_viz_bgr, npx * 3, hipMemcpyDeviceToHost, h->stream_b));
    int rc = drain_lm_and_back(h);
    if (rc) return rc;
  }
  return ESVO_OK;
}

// esvo_MVStereo::saveDepthMap (esvo_MVStereo.cpp:982-1000), the reference's only DepthMap dump: the file <save_dir><t_ns>.txt with
// one line per valid element (inverse depth > -1e-6, DepthPoint::valid() without arguments) in list order:
//     of << it->x().transpose() << " " << it->p_cam()(2) << "\n"
// Eigen's operator<< with the default IOFormat prints the 1 x 2 row vector with the stream's precision (6 significant digits,
// general format) and ALIGNED columns: both coefficients right-aligned to the longer one's width, separated by one blank; the
// depth follows as a plain double.  (Eigen is third-party and absent here: restated from its documented default format.)
int esvo_map_save_depth_map(esvo_handle h, const char* save_dir, uint64_t t_ns, size_t* n_written) {
  if (!h || !save_dir) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  std::vector<esvo_depth_point_t> v;
  int rc = export_map(h, v, nullptr);
  if (rc) return rc;
  const std::string path = std::string(save_dir) + std::to_string((unsigned long long)t_ns) + ".txt";
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) FAIL(ESVO_ERR_INVALID_ARG, "cannot open " + path);
  size_t n = 0;
  for (const esvo_depth_point_t& e : v) {
    if (!(e.inv_depth > -1e-6)) continue;
    char a[64], b[64];
    std::snprintf(a, sizeof(a), "%g", e.x[0]);
    std::snprintf(b, sizeof(b), "%g", e.x[1]);
    const int w = (int)std::max(std::strlen(a), std::strlen(b));
    std::fprintf(f, "%*s %*s %g\n", w, a, w, b, e.p_cam[2]);
    ++n;
  }
  std::fclose(f);
  if (n_written) *n_written = n;
  return ESVO_OK;
}

int esvo_map_get_last_frame(esvo_handle h, esvo_depth_point_t* out, size_t cap, size_t* n) {
  if (!h || !n) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  *n = 0;
  if (h->frames.empty()) return ESVO_OK;
  const FrameRec& f = h->frames.back();
  *n = f.count;
  if (out && f.count) {
    if (f.count > cap) FAIL(ESVO_ERR_CAPACITY, "output array too small for the frame");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->stream_b));  // (the frame was copied into the ring on the back stream)
    HIPCHK(hipMemcpy(out, h->d_win + f.off, sizeof(esvo_depth_point_t) * f.count, hipMemcpyDeviceToHost));
  }
  return ESVO_OK;
}

int esvo_get_stats(esvo_handle h, esvo_stats_t* out) {
  if (!h || !out) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  int rc = finalize_tick_stats(h);
  if (rc) return rc;
  {  // the LM kernel's clock probe (every stream is drained here): running sums since esvo_create / esvo_reset
    u64 acc[CLK_SCRATCH], acc1[CLK_SCRATCH];
    HIPCHK(hipMemcpy(acc, h->d_clk, sizeof(acc), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(acc1, h->d_clk + clk_words(h->max_ev), sizeof(acc1), hipMemcpyDeviceToHost));
    for (u32 x = 0; x < CLK_XCDS; ++x) { h->stats.clk_cycles[x] = acc[2 * x] + acc1[2 * x]; h->stats.clk_ref_ticks[x] = acc[2 * x + 1] + acc1[2 * x + 1]; }
    h->stats.clk_samples = acc[CLK_SAMPLES] + acc1[CLK_SAMPLES];
  }
  std::lock_guard<std::mutex> lr(h->mu_ring);  // events_staged is written by the ingest thread
  *out = h->stats;
  return ESVO_OK;
}

int esvo_map_lm_stats(esvo_handle h, esvo_lm_stats_t* out) {
  if (!h || !out) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  int rc = finalize_tick_stats(h);  // (completes a pending tick: its counter row is collected there)
  if (rc) return rc;
  *out = esvo_lm_stats_t{};
  if (!lm_guard_wanted(h)) return ESVO_OK;  // limit 0, or no scale loop (l2): every field reads 0
  *out = h->lm_stats;
  out->enabled = 1;
  return ESVO_OK;
}

void esvo_lm_sizes(size_t out[4]) {
  out[0] = sizeof(esvo_lm_stats_t); out[1] = (size_t)ESVO_LM_SCALE_COUNT_ONLY;
  out[2] = 0; out[3] = 0;
}

}  // extern "C"
