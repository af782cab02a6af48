// kernels_cloud.hip — publishPointCloud's cloud (esvo_Mapping.cpp:925-932) of the current DepthMap, built and kept on the
// device (esvo_map_cloud_build, api_out.hip): the points, order and float bits of esvo_map_get_pointcloud_xyz without the
// element download and the host sort of export_map.
//
// The reference iterates its element list, which is in creation order; an element carries the id of the record that created
// it (MapCell::seq), so the list is the alive cells in ascending id.  Ids are bounded by what the last fusion numbered
// (`id_n`, recorded by run_fuse / esvo_map_init_sgm when they number them -- NOT derived from the window, which may shrink
// between the fusion and the read-out: esvo_map_push_frame applies the window policy without fusing).  So the order is a
// scatter of (present, cell) by id, one exclusive scan over [0, id_n) and a gather: O(cells + ids), no comparison sort, and
// 24 B of p_cam read per element where the host path moves the 104-byte record three times.
//
// Ids are UNIQUE among the alive cells on every route that leaves a map, which is what lets one word per id hold the cell:
//   * run_fuse (the mapper tick, esvo_map_fuse, esvo_map_tick_em, esvo_map_tick_sgm, esvo_map_tick_bm_only and
//     esvo_map_fuse_matches_naive -- the last three with the naive model): an element is created by the record (point q, cell k)
//     with id q K + k (kernels_fuse.hip, fuse_record case 1), and a record addresses exactly one cell; later records of the
//     cell -- fusion, the replace branch, the naive model's overwrite -- keep the creating id.  id < total points x K.
//   * ... followed by the regulariser (the map is d_map2 then): only the OWNER element of a believed cell b survives, one per
//     b, and takes owner_min[b], the smallest id among the elements that believe b (reg_apply_kernel).  Every element
//     believes one cell, so these sets are disjoint over b and their minima distinct; they are ids of the fusion: same bound.
//   * esvo_map_init_sgm: the id is the rank of the cell's winning (point, k) pair in a scan over the pairs (sgm_naive_create):
//     distinct by construction, below 4 x points.
// An id outside [0, id_n) cannot occur; the mark kernel counts such cells instead of writing (the build then fails instead of
// returning a cloud with points missing).
#include "common.hpp"

namespace esvo {

// pass 1, one thread per cell of the band: present[id] = 1, where[id] = cell   (present was cleared by the caller)
__global__ void __launch_bounds__(256) cloud_mark_kernel(const MapCell* __restrict__ map, int ncell, int W, int band0, int band1, u32 id_n,
                                                         u32* __restrict__ present, u32* __restrict__ where, u32* __restrict__ n_out_of_range) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= ncell) return;
  const int row = cell / W;
  if (row < band0 || row >= band1 || !(map_flags(map, ncell)[cell] & CELL_ALIVE)) return;
  const u32 id = map[cell].seq;
  if (id >= id_n) { atomicAdd(n_out_of_range, 1u); return; }
  present[id] = 1u;
  where[id] = (u32)cell;
}

// pass 3, one thread per id: p_world = T_world_frame p_cam as float, un-fused -- the operations of the host loop in
// esvo_map_get_pointcloud_xyz in their order (band_xyz_kernel of api_comm.hip does the same for the merged bands)
struct CloudPose { double T[12]; };
__global__ void __launch_bounds__(256) cloud_xyz_kernel(const MapCell* __restrict__ map, const u32* __restrict__ present,
                                                        const u32* __restrict__ prefix, const u32* __restrict__ where, u32 id_n, u32 cap_points,
                                                        CloudPose P, float* __restrict__ xyz) {
  const u32 id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= id_n || !present[id]) return;
  const u32 i = prefix[id];
  if (i >= cap_points) return;  // (one element per cell at most: cannot happen)
  const MapCell& c = map[where[id]];
  const double a = c.p_cam[0], b = c.p_cam[1], d = c.p_cam[2];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    xyz[3 * (size_t)i + r] =
        (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P.T[r * 4 + 0], a), __dmul_rn(P.T[r * 4 + 1], b)), __dmul_rn(P.T[r * 4 + 2], d)), P.T[r * 4 + 3]);
}

// pc_near_ (esvo_Mapping.cpp:925-932: `if (p_cam.norm() < visualize_range)`): the same mark with the predicate of
// esvo_map_get_pointcloud_near_xyz in it -- sqrt((x x + y y) + z z) < range in f64, in that order -- so that the scan and the
// gather leave the near elements in list order
__global__ void __launch_bounds__(256) cloud_mark_near_kernel(const MapCell* __restrict__ map, int ncell, int W, int band0, int band1, u32 id_n,
                                                              double range, u32* __restrict__ present, u32* __restrict__ where,
                                                              u32* __restrict__ n_out_of_range) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= ncell) return;
  const int row = cell / W;
  if (row < band0 || row >= band1 || !(map_flags(map, ncell)[cell] & CELL_ALIVE)) return;
  const u32 id = map[cell].seq;
  if (id >= id_n) { atomicAdd(n_out_of_range, 1u); return; }
  const double x = map[cell].p_cam[0], y = map[cell].p_cam[1], z = map[cell].p_cam[2];
  if (!(__dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z))) < range)) return;
  present[id] = 1u;
  where[id] = (u32)cell;
}

// ids [0, id_n): present | prefix | where are id_n words each; counts: [0] elements (the scan's total) [1] cells with an id
// outside the range (cleared here); scan_tmp: scan_scratch_elems(id_n) words; xyz: cap_points x 3 floats
void launch_map_cloud(const MapCell* map, u32 id_n, u32* present, u32* prefix, u32* where, u32* counts, u32* scan_tmp, const double* T_world_frame,
                      float* xyz, u32 cap_points, const DevParams& p, hipStream_t s) {
  const int ncell = p.W * p.H;
  hipMemsetAsync(counts, 0, sizeof(u32) * 2, s);
  if (id_n == 0) return;
  hipMemsetAsync(present, 0, sizeof(u32) * (size_t)id_n, s);
  hipLaunchKernelGGL(cloud_mark_kernel, dim3((ncell + 255) / 256), dim3(256), 0, s, map, ncell, p.W, p.band_y0, p.band_y1, id_n, present, where,
                     counts + 1);
  launch_exclusive_scan_u32(present, prefix, counts, scan_tmp, (size_t)id_n, s);
  CloudPose P;
  for (int i = 0; i < 12; ++i) P.T[i] = T_world_frame[i];
  hipLaunchKernelGGL(cloud_xyz_kernel, dim3((id_n + 255) / 256), dim3(256), 0, s, map, present, prefix, where, id_n, cap_points, P, xyz);
}

// the near cloud: launch_map_cloud with cloud_mark_near_kernel as its first pass (same scratch, same counts)
void launch_map_cloud_near(const MapCell* map, u32 id_n, double range, u32* present, u32* prefix, u32* where, u32* counts, u32* scan_tmp,
                           const double* T_world_frame, float* xyz, u32 cap_points, const DevParams& p, hipStream_t s) {
  const int ncell = p.W * p.H;
  hipMemsetAsync(counts, 0, sizeof(u32) * 2, s);
  if (id_n == 0) return;
  hipMemsetAsync(present, 0, sizeof(u32) * (size_t)id_n, s);
  hipLaunchKernelGGL(cloud_mark_near_kernel, dim3((ncell + 255) / 256), dim3(256), 0, s, map, ncell, p.W, p.band_y0, p.band_y1, id_n, range, present,
                     where, counts + 1);
  launch_exclusive_scan_u32(present, prefix, counts, scan_tmp, (size_t)id_n, s);
  CloudPose P;
  for (int i = 0; i < 12; ++i) P.T[i] = T_world_frame[i];
  hipLaunchKernelGGL(cloud_xyz_kernel, dim3((id_n + 255) / 256), dim3(256), 0, s, map, present, prefix, where, id_n, cap_points, P, xyz);
}

}  // namespace esvo
