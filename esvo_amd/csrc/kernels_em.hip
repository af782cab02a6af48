// kernels_em.hip — event-to-event stereo matching (EventMatcher, the [26] baseline of esvo_MVStereo modes 0 and 2).
//
// EventMatcher::match_an_event (EventMatcher.cpp:60-163) per left event, split into three launches so that waves stay full
// whatever the candidate counts are:
//   em_candidates  one lane per left event: the right-event time window (two std::lower_bound over the right selection,
//                  EventMatcher.cpp:66-69), the time + polarity test (:71-85) and the epipolar test (:90-104).  Run twice:
//                  once to count the survivors, once (after an exclusive scan of the counts) to write (event, candidate)
//                  pairs in right-queue order.
//   em_pair_cost   one lane per pair: triangulation, warping2 (:271-301), patchInterpolation2 of both Time Surfaces
//                  (:303-346) and zncc_cost (:248-269).  Patches are never stored: each of the three sequential passes of
//                  zncc_cost (sum -> mean, sum of squares -> norm, sum of products) recomputes the bilinear samples, in
//                  column-major order, so every reduction has the reference's (stand-in Eigen's) summation order.
//   em_argmin      one lane per output slot of the stride-N thread order (match_all_HyperThread, :184-246): the strict-<
//                  argmin from 1.0 over the event's pairs in order, the threshold, the match record.
// Everything is f64 and built with -ffp-contract=off: each expression below is the reference's, operation by operation.
// Kernels write with ordinary vector stores only; no atomics.  Events off the sensor (x >= W or y >= H) are skipped before any
// rectification-table read: a left one gets no candidate, a right one is no candidate.
#include "common.hpp"
#include "em.hpp"

namespace esvo {

// ros::Time(double).toSec()  (roscpp TimeBase::fromSec: floor, round half away from zero)
__device__ inline double ros_time_round_sec(double t) {
  u32 sec = (u32)(long long)floor(t);
  u32 nsec = (u32)round((t - (double)sec) * 1e9);
  sec += nsec / 1000000000u;
  nsec %= 1000000000u;
  return time_to_sec(sec, nsec);
}

// std::lower_bound with the comparison of tools::EventVecPtr_lower_bound (utils.h:43-48): the same halving, so the range is
// the reference's on any input order
__device__ inline u32 em_lower_bound(const esvo_event_t* ev, u32 n, double t) {
  u32 first = 0, len = n;
  while (len > 0) {
    const u32 half = len >> 1;
    const u32 mid = first + half;
    const esvo_event_t e = ev[mid];
    if (time_to_sec(e.sec, e.nsec) < t) { first = mid + 1; len = len - half - 1; }
    else len = half;
  }
  return first;
}

__global__ void __launch_bounds__(256) em_candidates_kernel(EmArgs a, int emit) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const esvo_event_t ev = a.left[i];
  // an event off the sensor has no rectified coordinate: it takes part in nothing (block matching's rule, kernels_bm.hip)
  if (ev.x >= a.W || ev.y >= a.H) {
    if (!emit) { a.cnt_tp[i] = 0; a.cnt_ep[i] = 0; }
    return;
  }
  const double ts = time_to_sec(ev.sec, ev.nsec);
  const double t_lo = ros_time_round_sec(ts - a.half_T);
  const double t_up = ros_time_round_sec(ts + a.half_T);
  const u32 lo = em_lower_bound(a.right, a.n_right, t_lo);
  const u32 hi = em_lower_bound(a.right, a.n_right, t_up);
  const float2 fl = a.lut_l[(size_t)ev.y * a.W + ev.x];
  const double xl = (double)fl.x, yl = (double)fl.y;
  u32 n_tp = 0, n_ep = 0;
  const u32 base = emit ? a.pair_off[i] : 0;
  for (u32 j = lo; j < hi; ++j) {
    const esvo_event_t r = a.right[j];
    if (r.x >= a.W || r.y >= a.H) continue;  // off the sensor: never a candidate
    const double tr = time_to_sec(r.sec, r.nsec);
    if (!(tr >= t_lo && tr <= t_up) || r.polarity != ev.polarity) continue;
    ++n_tp;
    const float2 fr = a.lut_r[(size_t)r.y * a.W + r.x];
    if (fabs(yl - (double)fr.y) <= a.epi_thr && (double)fr.x < xl) {
      if (emit) { a.pair_ev[base + n_ep] = i; a.pair_r[base + n_ep] = j; }
      ++n_ep;
    }
  }
  if (!emit) {
    a.cnt_tp[i] = n_tp;
    a.cnt_ep[i] = n_ep;
  }
}

// bilinear sample (r, c) of patchInterpolation2's patch: F = q3 R(r) + q4 R(r+1), R(r) = q1 S(r, c) + q2 S(r, c+1)
struct EmPatch {
  const uint8_t* p;  // image pointer at the patch's upper-left source pixel
  int W;
  double q1, q2, q3, q4;
  __device__ inline double at(int r, int c) const {
    const uint8_t* s0 = p + (size_t)r * W + c;
    const uint8_t* s1 = s0 + W;
    const double r0 = q1 * (double)s0[0] + q2 * (double)s0[1];
    const double r1 = q1 * (double)s1[0] + q2 * (double)s1[1];
    return q3 * r0 + q4 * r1;
  }
};

// warping2's bounds test on one projection (EventMatcher.cpp:291-298; (w - 1) / 2 is integer division of size_t)
__device__ inline bool em_in_bounds(double u, double v, const EmArgs& a) {
  const int hx = (a.wx - 1) / 2, hy = (a.wy - 1) / 2;
  return !(u < (double)hx || u > (double)(a.W - hx) || v < (double)hy || v > (double)(a.H - hy));
}

// patchInterpolation2's checks and weights (EventMatcher.cpp:303-346)
__device__ inline bool em_patch(const uint8_t* img, double u, double v, const EmArgs& a, EmPatch& out) {
  const int hx = (a.wx - 1) / 2, hy = (a.wy - 1) / 2;
  const double fu = floor(u), fv = floor(v);
  const int ulx = (int)(fu - (double)hx), uly = (int)(fv - (double)hy);
  const int drx = (int)(fu + (double)hx), dry = (int)(fv + (double)hy);
  if (ulx < 0 || uly < 0) return false;
  if (drx >= a.W || dry >= a.H) return false;
  if (uly + a.wy >= a.H || ulx + a.wx >= a.W) return false;
  const int lx = (int)fu, ly = (int)fv;
  out.q1 = (double)(lx + 1) - u;
  out.q2 = u - (double)lx;
  out.q3 = (double)(ly + 1) - v;
  out.q4 = v - (double)ly;
  out.p = img + (size_t)uly * a.W + ulx;
  out.W = a.W;
  return true;
}

__global__ void __launch_bounds__(256) em_pair_cost_kernel(EmArgs a) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.n_pairs) return;
  const u32 i = a.pair_ev[q];
  const esvo_event_t ev = a.left[i];
  const esvo_event_t r = a.right[a.pair_r[q]];
  const float2 fl = a.lut_l[(size_t)ev.y * a.W + ev.x];
  const float2 fr = a.lut_r[(size_t)r.y * a.W + r.x];
  const double xl = (double)fl.x, yl = (double)fl.y;
  // triangulation: depth = b * f / disparity; warping2 takes 1.0 / depth
  const double disparity = xl - (double)fr.x;
  const double depth = a.bf / disparity;
  const double inv = 1.0 / depth;
  double p_rv[3];
  cam2World(a.camL, xl, yl, inv, p_rv);
  const double* T = a.T_lr + (size_t)a.slice_of[i] * 12;
  double p_left[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) p_left[k] = ((T[k * 4 + 0] * p_rv[0] + T[k * 4 + 1] * p_rv[1]) + T[k * 4 + 2] * p_rv[2]) + T[k * 4 + 3];
  double u1, v1, u2, v2;
  world2Cam(a.camL, p_left, u1, v1);
  world2Cam(a.camR, p_left, u2, v2);
  double cost = INFINITY;  // a candidate that fails warping or a patch is skipped: never below min_cost
  u32 ok = 0;
  EmPatch L, R;
  if (em_in_bounds(u1, v1, a) && em_in_bounds(u2, v2, a) && em_patch(a.tsL, u1, v1, a, L) && em_patch(a.tsR, u2, v2, a, R)) {
    ok = 1;
    const int wx = a.wx, wy = a.wy;
    double sl = 0.0, sr = 0.0;
    for (int c = 0; c < wx; ++c)
      for (int rr = 0; rr < wy; ++rr) { sl += L.at(rr, c); sr += R.at(rr, c); }
    const double area = (double)(wx * wy);
    const double ml = sl / area, mr = sr / area;
    double ql = 0.0, qr = 0.0;
    for (int c = 0; c < wx; ++c)
      for (int rr = 0; rr < wy; ++rr) {
        const double dl = L.at(rr, c) - ml, dr = R.at(rr, c) - mr;
        ql += dl * dl;
        qr += dr * dr;
      }
    const double nl = sqrt(ql) + 1e-6, nr = sqrt(qr) + 1e-6;
    double s = 0.0;
    for (int c = 0; c < wx; ++c)
      for (int rr = 0; rr < wy; ++rr) s += ((L.at(rr, c) - ml) / nl) * ((R.at(rr, c) - mr) / nr);
    cost = 0.5 * (1 - s);
  }
  a.pair_cost[q] = cost;
  a.pair_ok[q] = ok;
}

__global__ void __launch_bounds__(256) em_argmin_kernel(EmArgs a) {
  const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.n) return;
  const u32 i = stride_item(w, a.n, a.num_threads);
  const u32 n_ep = a.cnt_ep[i];
  u32 matched = 0;
  if (n_ep) {
    const u32 base = a.pair_off[i];
    double min_cost = 1.0;
    u32 best = 0;
    bool updated = false;
    for (u32 k = 0; k < n_ep; ++k) {
      const double c = a.pair_cost[base + k];
      if (c < min_cost) { min_cost = c; best = k; updated = true; }
    }
    if (!(min_cost > a.ncc_thr)) {
      const esvo_event_t ev = a.left[i];
      const esvo_event_t r = a.right[a.pair_r[base + best]];
      const float2 fl = a.lut_l[(size_t)ev.y * a.W + ev.x];
      const float2 fr = a.lut_r[(size_t)r.y * a.W + r.x];
      const double xl = (double)fl.x;
      const double disparity = xl - (double)fr.x;
      const double best_depth = updated ? a.bf / disparity : 0.0;  // no candidate below 1: best_depth keeps its 0
      esvo_match_t m;
      m.x_left[0] = xl;
      m.x_left[1] = (double)fl.y;
      m.inv_depth = 1.0 / best_depth;
      m.cost = min_cost;
      m.disp = disparity;
      m.event_idx = a.event_base + i;
      m.pose_idx = a.slice_of[i];
      a.slots[w] = m;
      matched = 1;
    }
  }
  a.flags[w] = matched;
}

__global__ void __launch_bounds__(256) em_compact_kernel(const esvo_match_t* slots, const u32* flags, const u32* prefix, u32 n,
                                                         esvo_match_t* out) {
  const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n || !flags[w]) return;
  out[prefix[w]] = slots[w];
}

// 64-bit totals of two per-event count arrays (one workgroup; the u32 scans of the counts would wrap above 2^32 - 1)
__global__ void __launch_bounds__(256) em_sum64_kernel(const u32* a, const u32* b, u32 n, unsigned long long* out) {
  __shared__ unsigned long long sa[256], sb[256];
  unsigned long long va = 0, vb = 0;
  for (u32 i = threadIdx.x; i < n; i += 256) { va += a[i]; vb += b[i]; }
  sa[threadIdx.x] = va;
  sb[threadIdx.x] = vb;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { sa[threadIdx.x] += sa[threadIdx.x + w]; sb[threadIdx.x] += sb[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = sa[0]; out[1] = sb[0]; }
}

void launch_em_sum64(const u32* a, const u32* b, u32 n, unsigned long long* out, hipStream_t s) {
  hipLaunchKernelGGL(em_sum64_kernel, dim3(1), dim3(256), 0, s, a, b, n, out);
}
void launch_em_candidates(const EmArgs& a, int emit, hipStream_t s) {
  if (!a.n) return;
  hipLaunchKernelGGL(em_candidates_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a, emit);
}
void launch_em_pair_cost(const EmArgs& a, hipStream_t s) {
  if (!a.n_pairs) return;
  hipLaunchKernelGGL(em_pair_cost_kernel, dim3((a.n_pairs + 255) / 256), dim3(256), 0, s, a);
}
void launch_em_argmin(const EmArgs& a, hipStream_t s) {
  if (!a.n) return;
  hipLaunchKernelGGL(em_argmin_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}
void launch_em_compact(const esvo_match_t* slots, const u32* flags, const u32* prefix, u32 n, esvo_match_t* out, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(em_compact_kernel, dim3((n + 255) / 256), dim3(256), 0, s, slots, flags, prefix, n, out);
}

}  // namespace esvo
