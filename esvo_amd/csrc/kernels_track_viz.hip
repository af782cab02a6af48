// kernels_track_viz.hip — the tracker's reprojection map (Reproj_Map_Left).
//
// Replaces the visualisation block of RegProblemSolverLM::solve_analytical (esvo_core/src/core/RegProblemSolverLM.cpp:180-209;
// :106-135 is the same block, once per iteration of solve_numerical) with Visualization::DrawPoint
// (esvo_core/src/tools/Visualization.cpp:74-94) as it is called there.  The image is what the sequential loop
// `for i in 0..n-1: DrawPoint(...)` leaves, whatever order the threads run in:
//
//   base     every pixel is (neg, neg, neg): eigen2cv -> convertTo(CV_8UC1) -> GRAY2BGR on integer-valued doubles (:185-188)
//   project  pl[r] = ((T[r,0] p0 + T[r,1] p1) + T[r,2] p2) + T[r,3] with T = T_left_ref = [R^T | -R^T t] (:191-198), hm the same
//            with P, x = hm[0] / hm[2], y = hm[1] / hm[2] (world2Cam, :200) -- the expressions of trk_reproject
//            (kernels_track.hip) in their order, and NONE of its tests: no bounds, no mask, no isValidPatch
//   centre   cx = (int)x, cy = (int)y: cv::Point from doubles truncates toward zero (Visualization.cpp:90-92), x = -0.6 is
//            column 0.  Where that conversion is undefined -- x or y not finite, or of magnitude >= 2^30 -- the point is skipped
//   colour   val = 1.0 / p[2], p[2] the z of the point in the REFERENCE frame (:201-202);
//            v = floor((val - min_range) / (max_range - min_range) * 255.0) in f64 (Visualization.cpp:82), clamped to 0..255 in
//            f64 BEFORE the conversion to int (:83-86; the reference converts first, which is undefined for a huge v);
//            a NaN v skips the point; colour = jet[3 index .. + 2], the mapper's 256 BGR triples
//   sprite   cv::circle(img, centre, 1, colour, FILLED) (:93): the 5-pixel plus of kernels_viz.hip, each of the five pixels
//            painted if and only if it lies inside the image -- a centre one pixel outside still paints one arm
//   overlap  the point with the largest index i among those covering a pixel wins: the mark pass takes
//            atomicMax(owner[pix], i + 1), the paint pass lets exactly the owner paint (the scheme of viz_kernel)
//   counter  n_inside = the points that were not skipped and whose centre pixel lies inside the image
//
// cv::circle's raster is restated here, not pinned to OpenCV (as for the mapper's debug images).
//
// The paint pass runs per pixel, four pixels a thread: one 16-byte load of owner, one dword of neg, three dword stores of
// BGR.  It recomputes the owner's colour from pts and zeroes owner as it reads it, so that buffer is cleared once, where it
// is allocated, and every call leaves it clean for the next.
#include "common.hpp"

namespace esvo {

// colour index of DrawPoint for the reference point p; false where v is NaN
__device__ inline bool trk_viz_index(const double* __restrict__ p, double min_range, double max_range, int& index) {
  const double val = 1.0 / p[2];
  double v = floor((val - min_range) / (max_range - min_range) * 255.0);
  if (v != v) return false;
  v = v > 255.0 ? 255.0 : (v < 0.0 ? 0.0 : v);
  index = (int)v;
  return true;
}

// n threads: every point that is drawn claims its five pixels with its list position
__global__ void __launch_bounds__(256) track_viz_mark_kernel(TrackArgs a, TrackPose pose, u32 n, double min_range, double max_range,
                                                             u32* __restrict__ owner, u32* __restrict__ n_inside) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  bool inside = false;
  if (i < n) {
    const double* p = a.pts + 3 * (size_t)i;
    const double* T = pose.T;
    double pl[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) pl[r] = ((T[r * 4 + 0] * p[0] + T[r * 4 + 1] * p[1]) + T[r * 4 + 2] * p[2]) + T[r * 4 + 3];
    double hm[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) hm[r] = ((a.P[r * 4 + 0] * pl[0] + a.P[r * 4 + 1] * pl[1]) + a.P[r * 4 + 2] * pl[2]) + a.P[r * 4 + 3];
    const double x = hm[0] / hm[2], y = hm[1] / hm[2];
    int index;
    // (a NaN fails the comparison, an infinity the bound)
    if (fabs(x) < 1073741824.0 && fabs(y) < 1073741824.0 && trk_viz_index(p, min_range, max_range, index)) {
      const int cx = (int)x, cy = (int)y;
      inside = cx >= 0 && cx < a.W && cy >= 0 && cy < a.H;
      const int dx[5] = {0, -1, 1, 0, 0}, dy[5] = {0, 0, 0, -1, 1};
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int px = cx + dx[k], py = cy + dy[k];
        if (px < 0 || px >= a.W || py < 0 || py >= a.H) continue;
        atomicMax(&owner[py * a.W + px], i + 1u);
      }
    }
  }
  const unsigned long long m = __ballot(inside);  // one add per wave
  if (m != 0ull && (threadIdx.x & 63) == (u32)(__ffsll((long long)m) - 1)) atomicAdd(n_inside, (u32)__popcll(m));
}

__device__ inline u32 trk_viz_pixel(u32 o, u32 grey, const double* __restrict__ pts, const uint8_t* __restrict__ jet, double min_range,
                                    double max_range) {
  u32 b = grey, g = grey, r = grey;
  int index;
  if (o != 0u && trk_viz_index(pts + 3 * (size_t)(o - 1u), min_range, max_range, index)) {
    b = jet[3 * index + 0]; g = jet[3 * index + 1]; r = jet[3 * index + 2];
  }
  return b | (g << 8) | (r << 16);
}

// one thread per four pixels: grey base or the owner's colour, and owner back to 0
__global__ void __launch_bounds__(256) track_viz_paint_kernel(const uint8_t* __restrict__ neg, const double* __restrict__ pts,
                                                              const uint8_t* __restrict__ jet, double min_range, double max_range,
                                                              u32* __restrict__ owner, uint8_t* __restrict__ bgr, u32 npx) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 p0 = 4u * q;
  if (p0 >= npx) return;
  if (p0 + 4u <= npx) {
    uint4* ow = reinterpret_cast<uint4*>(owner) + q;
    const uint4 o = *ow;
    const u32 g4 = reinterpret_cast<const u32*>(neg)[q];
    if ((o.x | o.y | o.z | o.w) != 0u) *ow = make_uint4(0u, 0u, 0u, 0u);
    const u32 c0 = trk_viz_pixel(o.x, g4 & 255u, pts, jet, min_range, max_range);
    const u32 c1 = trk_viz_pixel(o.y, (g4 >> 8) & 255u, pts, jet, min_range, max_range);
    const u32 c2 = trk_viz_pixel(o.z, (g4 >> 16) & 255u, pts, jet, min_range, max_range);
    const u32 c3 = trk_viz_pixel(o.w, g4 >> 24, pts, jet, min_range, max_range);
    u32* out = reinterpret_cast<u32*>(bgr) + 3 * (size_t)q;  // 12 bytes: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
    out[0] = c0 | (c1 << 24);
    out[1] = (c1 >> 8) | (c2 << 16);
    out[2] = (c2 >> 16) | (c3 << 8);
  } else {  // the last 1..3 pixels of an image whose pixel count is no multiple of 4
    for (u32 pix = p0; pix < npx; ++pix) {
      const u32 c = trk_viz_pixel(owner[pix], neg[pix], pts, jet, min_range, max_range);
      owner[pix] = 0u;
      bgr[3 * (size_t)pix + 0] = (uint8_t)(c & 255u);
      bgr[3 * (size_t)pix + 1] = (uint8_t)((c >> 8) & 255u);
      bgr[3 * (size_t)pix + 2] = (uint8_t)(c >> 16);
    }
  }
}

// owner: W * H words, all 0 on entry and on exit; n_inside is zeroed here.  n <= the number of points behind a.pts.
void launch_track_reprojection_map(const TrackArgs& a, const TrackPose& pose, u32 n, double min_range, double max_range,
                                   const uint8_t* jet, u32* owner, uint8_t* bgr, u32* n_inside, hipStream_t s) {
  const u32 npx = (u32)a.W * (u32)a.H;
  hipMemsetAsync(n_inside, 0, sizeof(u32), s);
  if (n) hipLaunchKernelGGL(track_viz_mark_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, pose, n, min_range, max_range, owner, n_inside);
  const u32 nq = (npx + 3u) / 4u;
  hipLaunchKernelGGL(track_viz_paint_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, a.neg, a.pts, jet, min_range, max_range, owner, bgr,
                     npx);
}

}  // namespace esvo
