// api_gpc.hip — the mapper's global point cloud (pc_global_, esvo_Mapping.cpp:955-977) accumulated on the device: the near
// cloud (esvo_map_cloud_near; kernels_cloud.hip), the voxel filter (esvo_map_voxel_filter; kernels_voxel.hip) and the branch
// itself (esvo_map_gpc_configure / _update / _get / _device / _stats).  Everything runs on the back stream, behind whatever
// wrote the current map; the buffers are this file's own, so the esvo_map_cloud_build snapshot and the ticks never see it.
#include <algorithm>
#include <cmath>

#include "context.hpp"

// (global namespace: esvo_context holds a GpcState*)
struct GpcState {
  // near cloud: ids scratch [3][id_cap] present | prefix | where, its scan scratch, the cloud itself (3 floats per point)
  DevBuf<u32> d_ids;
  size_t id_cap = 0;
  DevBuf<u32> d_id_scan;
  DevBuf<float> d_near;
  DevBuf<u32> d_cnt;             // [0] near elements [1] cells whose id was outside the bound
  // voxel filter, for vox_cap rows
  DevBuf<u64> d_pairs[2];
  DevBuf<u32> d_heads;           // [2][vox_cap] heads | rank
  DevBuf<u32> d_hist;
  DevBuf<u32> d_vox_scan;
  DevBuf<float> d_cent;
  size_t vox_cap = 0;
  DevBuf<float> d_in;            // esvo_map_voxel_filter's upload
  DevBuf<VoxelGrid> d_grid;
  struct Pinned { VoxelGrid grid; u32 cnt[2]; };
  PinBuf<Pinned> h_pin;
  // the global cloud
  bool configured = false;
  esvo_gpc_params_t prm{};
  DevBuf<float> d_global;        // 3 floats per point of the capacity
  DevEvent ev0, ev1;
  esvo_gpc_stats_t stats{};
};

namespace esvo_host {

void gpc_release(esvo_context* h) {
  delete h->gpc;
  h->gpc = nullptr;
}

// esvo_reset: pc_global_->clear() (esvo_Mapping.cpp:780); t_last_pub_pc_ is not reset there, so it stays
void gpc_reset(esvo_context* h) {
  if (!h->gpc) return;
  h->gpc->stats.total_points = 0;
}

static int gpc_state(esvo_context* h) {
  if (h->sharded || h->comm) FAIL(ESVO_ERR_STATE, "handle is band-sharded or tick-interleaved: the global cloud is a single-GPU read-out");
  HIPCHK(hipSetDevice(h->device));
  if (h->gpc) return ESVO_OK;
  GpcState* g = new GpcState();
  h->gpc = g;  // (released by esvo_destroy whatever fails below)
  HIPCHK(g->d_cnt.alloc(2));
  HIPCHK(g->d_grid.alloc(1));
  HIPCHK(g->h_pin.alloc(1));
  HIPCHK(g->ev0.create());
  HIPCHK(g->ev1.create());
  return ESVO_OK;
}

// the work on the back stream is complete whenever a call of this file returns, so its scratch may be replaced here
static int gpc_reserve_near(esvo_context* h, size_t id_n) {
  GpcState* g = h->gpc;
  const size_t npx = (size_t)h->W * h->H;
  HIPCHK(g->d_near.grow(npx * 3));
  if (id_n > g->id_cap || !g->d_ids) {
    const size_t cap = std::max<size_t>(id_n, 4096);
    g->id_cap = 0;
    HIPCHK(g->d_ids.grow(3 * cap));
    HIPCHK(g->d_id_scan.grow(scan_scratch_elems(cap) + 8));
    g->id_cap = cap;
  }
  return ESVO_OK;
}

static int gpc_reserve_voxel(esvo_context* h, size_t n) {
  GpcState* g = h->gpc;
  if (n <= g->vox_cap && g->d_cent) return ESVO_OK;
  const size_t cap = std::max<size_t>(n, 4096);
  g->vox_cap = 0;
  HIPCHK(g->d_pairs[0].grow(cap));
  HIPCHK(g->d_pairs[1].grow(cap));
  HIPCHK(g->d_heads.grow(2 * cap));
  HIPCHK(g->d_hist.grow(voxel_hist_words(cap)));
  HIPCHK(g->d_vox_scan.grow(scan_scratch_elems(std::max(cap, voxel_hist_words(cap))) + 8));
  HIPCHK(g->d_cent.grow(cap * 3));
  g->vox_cap = cap;
  return ESVO_OK;
}

// the near cloud of the current map into d_near; *n_near: its size.  One host read (two counters).
static int gpc_near(esvo_context* h, double range, size_t* n_near) {
  GpcState* g = h->gpc;
  const u32 id_n = h->map_id_bound;
  u32* present = g->d_ids;
  launch_map_cloud_near(h->d_map_cur, id_n, range, present, present + g->id_cap, present + 2 * g->id_cap, g->d_cnt, g->d_id_scan,
                        h->T_world_frame, g->d_near, (u32)(g->d_near.cap() / 3), h->dp, h->stream_b);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(g->h_pin->cnt, g->d_cnt, sizeof(u32) * 2, hipMemcpyDeviceToHost, h->stream_b));
  HIPCHK(esvo_wait_stream(h->stream_b, true));
  if (g->h_pin->cnt[1]) FAIL(ESVO_ERR_STATE, "DepthMap elements carry creation ids beyond the bound of the last fusion (internal error)");
  *n_near = g->h_pin->cnt[0];
  return ESVO_OK;
}

// d_xyz[n] (device) -> d_cent[*n_vox] centroids.  Two host reads: the grid (finite rows, cell count, the too-large flag) in
// front of the sort, which picks the number of radix passes from it, and the voxel count behind it.
static int gpc_voxel(esvo_context* h, const float* d_xyz, size_t n, float leaf, size_t* n_vox) {
  GpcState* g = h->gpc;
  hipStream_t s = h->stream_b;
  *n_vox = 0;
  if (n == 0) return ESVO_OK;
  launch_voxel_bounds(d_xyz, (u32)n, leaf, g->d_grid, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&g->h_pin->grid, g->d_grid, sizeof(VoxelGrid), hipMemcpyDeviceToHost, s));
  HIPCHK(esvo_wait_stream(s, true));
  const VoxelGrid& grid = g->h_pin->grid;
  if (grid.n_finite == 0) return ESVO_OK;
  if (grid.too_large) FAIL(ESVO_ERR_CAPACITY, "leaf size too small for the extent of the cloud (voxel index overflows, as in pcl::VoxelGrid)");
  const u32 n_finite = grid.n_finite;
  u64* const pairs[2] = {g->d_pairs[0], g->d_pairs[1]};
  const u64* sorted = launch_voxel_sort(d_xyz, (u32)n, g->d_grid, grid.key_bits, pairs, g->d_hist, g->d_vox_scan, s);
  launch_voxel_centroids(d_xyz, sorted, n_finite, g->d_heads, g->d_heads + g->vox_cap, g->d_grid, g->d_vox_scan, g->d_cent, (u32)g->vox_cap, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&g->h_pin->grid.n_voxels, &g->d_grid->n_voxels, sizeof(u32), hipMemcpyDeviceToHost, s));
  HIPCHK(esvo_wait_stream(s, true));
  *n_vox = g->h_pin->grid.n_voxels;
  return ESVO_OK;
}

}  // namespace esvo_host

extern "C" {

int esvo_map_cloud_near(esvo_handle h, double visualize_range, float* out_xyz, size_t cap_points, size_t* n) {
  if (!h || !n) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  { int rc = gpc_state(h); if (rc) return rc; }
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  { int rc = gpc_reserve_near(h, h->map_id_bound); if (rc) return rc; }
  size_t cnt = 0;
  { int rc = gpc_near(h, visualize_range, &cnt); if (rc) return rc; }
  *n = cnt;
  if (!out_xyz || !cnt) return ESVO_OK;
  if (cnt > cap_points) FAIL(ESVO_ERR_CAPACITY, "output array too small for the point cloud");
  HIPCHK(hipMemcpy(out_xyz, h->gpc->d_near, cnt * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return ESVO_OK;
}

int esvo_map_voxel_filter(esvo_handle h, const float* xyz, size_t n, float leaf, float* out_xyz, size_t cap_points, size_t* n_out) {
  if (!h || (n && !xyz) || !n_out || !(leaf > 0)) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (n > 0x7fffffffull) FAIL(ESVO_ERR_CAPACITY, "more rows than 31-bit indices address");
  { int rc = gpc_state(h); if (rc) return rc; }
  *n_out = 0;
  if (n == 0) return ESVO_OK;
  GpcState* g = h->gpc;
  HIPCHK(g->d_in.grow(n * 3));
  { int rc = gpc_reserve_voxel(h, n); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(g->d_in, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream_b));
  size_t k = 0;
  { int rc = gpc_voxel(h, g->d_in, n, leaf, &k); if (rc) return rc; }
  *n_out = k;
  if (!out_xyz || !k) return ESVO_OK;
  if (k > cap_points) FAIL(ESVO_ERR_CAPACITY, "output array too small for the filtered cloud");
  HIPCHK(hipMemcpy(out_xyz, g->d_cent, k * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return ESVO_OK;
}

int esvo_map_gpc_configure(esvo_handle h, const esvo_gpc_params_t* prm) {
  if (!h || !prm) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (prm->num_added_per_refresh == 0) FAIL(ESVO_ERR_INVALID_ARG, "num_added_per_refresh must be at least 1 (the reference's `threshold - 1` wraps at 0)");
  if (!(prm->leaf > 0) || std::isnan(prm->visualize_range) || std::isnan(prm->interval_s))
    FAIL(ESVO_ERR_INVALID_ARG, "invalid esvo_gpc_params_t");
  { int rc = gpc_state(h); if (rc) return rc; }
  GpcState* g = h->gpc;
  g->configured = false;
  // every buffer an update needs, at its largest: a map holds one element per pixel at most, and a fusion numbers at most
  // 9 ids per point of the window ring (run_fuse; esvo_map_init_sgm: 4 per point)
  const size_t npx = (size_t)h->W * h->H;
  { int rc = gpc_reserve_near(h, 9 * (size_t)h->win_cap); if (rc) return rc; }
  { int rc = gpc_reserve_voxel(h, npx); if (rc) return rc; }
  const size_t cap = prm->capacity_points ? (size_t)prm->capacity_points : (size_t)5000000;
  if (cap * 3 != g->d_global.cap()) HIPCHK(g->d_global.alloc(cap * 3));
  g->prm = *prm;
  g->prm.capacity_points = cap;
  g->stats = esvo_gpc_stats_t{};  // (t_last_pub = 0.0, esvo_Mapping.cpp:152)
  g->configured = true;
  return ESVO_OK;
}

int esvo_map_gpc_update(esvo_handle h, uint64_t t_ns, int* refreshed) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (h->sharded || h->comm) FAIL(ESVO_ERR_STATE, "handle is band-sharded or tick-interleaved: the global cloud is a single-GPU read-out");
  GpcState* g = h->gpc;
  if (!g || !g->configured) FAIL(ESVO_ERR_STATE, "esvo_map_gpc_configure has not been called");
  HIPCHK(hipSetDevice(h->device));
  { int rcp = flush_pending_tick(h); if (rcp) return rcp; }
  const double now = ns_to_sec(t_ns);
  if (!(now - g->stats.t_last_pub > g->prm.interval_s)) {  // :956
    g->stats.updates += 1;
    g->stats.last_refreshed = 0;
    if (refreshed) *refreshed = 0;
    return ESVO_OK;
  }
  if (h->map_id_bound > g->id_cap) FAIL(ESVO_ERR_STATE, "creation ids beyond 9 per window point (internal error)");
  HIPCHK(hipEventRecord(g->ev0, h->stream_b));
  size_t n_near = 0, L = 0;
  { int rc = gpc_near(h, g->prm.visualize_range, &n_near); if (rc) return rc; }
  { int rc = gpc_voxel(h, g->d_near, n_near, g->prm.leaf, &L); if (rc) return rc; }
  // :966-969: the last min(L, NumGPC_added_per_refresh) - 1 centroids
  const size_t add = L ? (size_t)std::min<u64>((u64)L, g->prm.num_added_per_refresh) - 1 : 0;
  const size_t total = (size_t)g->stats.total_points;
  if (total + add > g->d_global.cap() / 3) FAIL(ESVO_ERR_CAPACITY, "the global cloud is full (esvo_gpc_params_t::capacity_points)");
  if (add)
    HIPCHK(hipMemcpyAsync(g->d_global + 3 * total, g->d_cent + 3 * (L - add), add * 3 * sizeof(float), hipMemcpyDeviceToDevice, h->stream_b));
  HIPCHK(hipEventRecord(g->ev1, h->stream_b));
  HIPCHK(esvo_wait_stream(h->stream_b, true));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, g->ev0, g->ev1));
  g->stats.updates += 1;
  g->stats.refreshes += 1;
  g->stats.total_points = total + add;
  g->stats.last_near = (u32)n_near;
  g->stats.last_voxels = (u32)L;
  g->stats.last_added = (u32)add;
  g->stats.last_refreshed = 1;
  g->stats.t_last_pub = now;
  g->stats.ms_last = ms;
  if (refreshed) *refreshed = 1;
  return ESVO_OK;
}

int esvo_map_gpc_get(esvo_handle h, float* out_xyz, size_t cap_points, size_t* n) {
  if (!h || !n) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  const GpcState* g = h->gpc;
  const size_t cnt = (g && g->configured) ? (size_t)g->stats.total_points : 0;
  *n = cnt;
  if (!out_xyz || !cnt) return ESVO_OK;
  if (cnt > cap_points) FAIL(ESVO_ERR_CAPACITY, "output array too small for the global point cloud");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpy(out_xyz, g->d_global, cnt * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return ESVO_OK;
}

int esvo_map_gpc_device(esvo_handle h, const float** d_xyz, size_t* n) {
  if (!h || !d_xyz || !n) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  const GpcState* g = h->gpc;
  const bool have = g && g->configured;
  *d_xyz = have ? g->d_global : nullptr;
  *n = have ? (size_t)g->stats.total_points : 0;
  return ESVO_OK;
}

int esvo_map_gpc_stats(esvo_handle h, esvo_gpc_stats_t* out) {
  if (!h || !out) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  const GpcState* g = h->gpc;
  *out = (g && g->configured) ? g->stats : esvo_gpc_stats_t{};
  return ESVO_OK;
}

}  // extern "C"
