// em.hpp — event-to-event matching (EventMatcher, esvo_MVStereo modes 0 and 2): kernel arguments shared by kernels_em.hip and
// api_em.hip.
#pragma once
#include "common.hpp"

namespace esvo {

struct EmArgs {
  const esvo_event_t* left;   // the events to match: left[i], i < n (the slices' events, contiguous from slice 0's first)
  u32 n;
  u32 event_base;             // esvo_match_t.event_idx = event_base + i (position in the left selection)
  const u32* slice_of;        // [n] slice of event i
  const double* T_lr;         // [slices x 12] T_left_rv = T_obs^-1 T_slice, rows 0..2 of the 4x4, row-major
  const esvo_event_t* right;  // the right selection (candidate queue)
  u32 n_right;
  const float2* lut_l;        // rectified coordinates, raw pixel -> (x, y)
  const float2* lut_r;
  const uint8_t* tsL;         // the observation's un-smoothed Time Surfaces (mono8)
  const uint8_t* tsR;
  int W, H, wx, wy;
  u32 num_threads;            // stride-N output order
  double half_T;              // EM_Time_THRESHOLD / 2
  double epi_thr, ncc_thr;
  double bf;                  // baseline * P_left(0,0)
  CamConst camL, camR;
  // per event
  u32* cnt_tp;                // candidates that pass time + polarity
  u32* cnt_ep;                // ... and the epipolar test
  u32* pair_off;              // exclusive scan of cnt_ep
  // per pair
  u32 n_pairs;
  u32* pair_ev;
  u32* pair_r;
  double* pair_cost;          // +inf where warping / a patch failed
  u32* pair_ok;
  // per output slot
  esvo_match_t* slots;
  u32* flags;
};

void launch_em_candidates(const EmArgs& a, int emit, hipStream_t s);
void launch_em_pair_cost(const EmArgs& a, hipStream_t s);
void launch_em_argmin(const EmArgs& a, hipStream_t s);
void launch_em_sum64(const u32* a, const u32* b, u32 n, unsigned long long* out, hipStream_t s);
void launch_em_compact(const esvo_match_t* slots, const u32* flags, const u32* prefix, u32 n, esvo_match_t* out, hipStream_t s);

}  // namespace esvo
