// kernels_survey.hip — the event survey of the ingest path (include/esvo_hip.h, esvo_ts_survey_begin): per-pixel event counts kept on
// the device while a stream is pushed, and the hot-pixel mask derived from them by an exact integer rule.
//
// Counting.  What the survey exists to find is its own worst case: a stuck pixel puts thousands of events of one packet on one
// address, and one global atomic per event serialises there.  So a workgroup takes SRV_CHUNK consecutive events, forms the keys
// pixel << 1 | polarity (0xffffffff: outside the image), sorts them in LDS (bitonic, as flt_walk_kernel sorts its tile list) and issues
// ONE atomicAdd per run of equal keys, with the run's length: global memory receives at most one update per (pixel, polarity) per
// chunk, whatever the packet looks like.  The order of the packet plays no part, so the kernel serves unsorted packets as well.
// The stamps' range and the outside count are reduced per wave: one 64-bit atomicMin, atomicMax and add per wave.
//
// The mask.  c = counts[0] + counts[1] per pixel; the baseline B, the rank-th smallest c, comes from an exact radix select: four
// passes over the 32-bit values, most significant byte first, each a 256-bin histogram of the values that share the bytes found so
// far (LDS histogram per workgroup, merged into the global one per workgroup), and a one-workgroup step that walks the bins to the
// one holding the rank.  Nothing is sorted and nothing comes down between the passes.  The last kernel applies the rule per pixel
// and reduces the report per wave.
#include "common.hpp"

namespace esvo {

namespace {
__device__ inline u64 wave_min_u64(u64 v) {
  for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d, ESVO_WAVE); v = o < v ? o : v; }
  return v;
}
__device__ inline u64 wave_max_u64(u64 v) {
  for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d, ESVO_WAVE); v = o > v ? o : v; }
  return v;
}
__device__ inline u64 wave_sum_u64(u64 v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, ESVO_WAVE);
  return v;
}

__global__ void __launch_bounds__(256) srv_count_kernel(SurveyArgs a) {
  __shared__ u32 s_key[SRV_CHUNK];
  const u32 tid = threadIdx.x, base = blockIdx.x * SRV_CHUNK;
  const u32 cnt = min(SRV_CHUNK, a.n - base);  // (the grid covers n exactly: base < n)
  u32 N = 64u;                                 // the chunk padded to a power of two
  while (N < cnt) N <<= 1;
  const u32 npx = (u32)a.W * (u32)a.H;
  u64 t_min = ~0ull, t_max = 0ull;
  u32 n_in = 0u, n_out = 0u;
  for (u32 k = tid; k < N; k += 256u) {
    u32 key = 0xffffffffu;
    if (k < cnt) {
      const u32 i = base + k;
      const u32 x = a.x[i], y = a.y[i];
      if (x < (u32)a.W && y < (u32)a.H) {
        key = ((y * (u32)a.W + x) << 1) | columns_polarity(a.p, i, a.p_type);
        const u64 t = a.t[i];
        t_min = t < t_min ? t : t_min; t_max = t > t_max ? t : t_max;
        ++n_in;
      } else ++n_out;
    }
    s_key[k] = key;
  }
  __syncthreads();
  for (u32 k = 2; k <= N; k <<= 1)
    for (u32 j = k >> 1; j > 0; j >>= 1) {
      for (u32 q = tid; q < N / 2; q += 256u) {
        const u32 lo = 2u * q - (q & (j - 1u)), hi = lo + j;
        const u32 va = s_key[lo], vb = s_key[hi];
        if ((va > vb) == ((lo & k) == 0u)) { s_key[lo] = vb; s_key[hi] = va; }
      }
      __syncthreads();
    }
  // the first entry of every run adds the run's length: its end is the first entry above the key (binary search, the list is sorted)
  for (u32 k = tid; k < N; k += 256u) {
    const u32 key = s_key[k];
    if (key == 0xffffffffu || (k > 0u && s_key[k - 1u] == key)) continue;
    u32 lo = k + 1u, hi = N;  // the end lies in [lo, hi]
    while (lo < hi) {
      const u32 mid = (lo + hi) >> 1;
      if (s_key[mid] == key) lo = mid + 1u; else hi = mid;
    }
    atomicAdd(&a.counts[(size_t)(key & 1u) * npx + (key >> 1)], lo - k);
  }
  // per wave: the stamps' range, the counted and the outside events
  const u64 w_min = wave_min_u64(t_min), w_max = wave_max_u64(t_max);
  const u64 w_in = wave_sum_u64((u64)n_in), w_out = wave_sum_u64((u64)n_out);
  if ((tid & (ESVO_WAVE - 1)) == 0) {
    if (w_in) {
      atomicMin(reinterpret_cast<unsigned long long*>(&a.stats[SRV_S_T_FIRST]), (unsigned long long)w_min);
      atomicMax(reinterpret_cast<unsigned long long*>(&a.stats[SRV_S_T_LAST]), (unsigned long long)w_max);
      atomicAdd(reinterpret_cast<unsigned long long*>(&a.stats[SRV_S_IN]), (unsigned long long)w_in);
    }
    if (w_out) atomicAdd(reinterpret_cast<unsigned long long*>(&a.stats[SRV_S_OUTSIDE]), (unsigned long long)w_out);
  }
}

__global__ void __launch_bounds__(256) srv_first_bad_kernel(const u64* __restrict__ t, u32 n, u32* __restrict__ sel) {
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    if (t[i] == COL_BAD_STAMP) atomicMin(&sel[SRV_SEL_FIRST_BAD], i);
}
__global__ void srv_first_bad_init_kernel(u32* sel) { sel[SRV_SEL_FIRST_BAD] = 0xffffffffu; }

// ---- the mask ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) srv_select_init_kernel(u32* sel, u64* report, u32 rank) {
  sel[SRV_SEL_HIST + threadIdx.x] = 0u;
  if (threadIdx.x == 0) { sel[SRV_SEL_PREFIX] = 0u; sel[SRV_SEL_RANK] = rank; }
  if (threadIdx.x < SRV_REPORT_WORDS) report[threadIdx.x] = 0ull;
}
// the histogram of byte `shift / 8` of the values whose higher bytes equal the prefix found so far
__global__ void __launch_bounds__(256) srv_select_hist_kernel(const u32* __restrict__ counts, u32 npx, int shift, u32* sel) {
  __shared__ u32 s_h[256];
  s_h[threadIdx.x] = 0u;
  __syncthreads();
  const u32 prefix = sel[SRV_SEL_PREFIX], high = shift == 24 ? 0u : ~0u << (shift + 8);
  // a thread flushes a run of equal digits with one LDS atomic: a dark image (every value 0) costs each thread one, not one per pixel
  u32 run_digit = 0u, run = 0u;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) {
    const u32 c = counts[i] + counts[npx + i];
    if ((c & high) != prefix) continue;
    const u32 d = (c >> shift) & 255u;
    if (d != run_digit && run) { atomicAdd(&s_h[run_digit], run); run = 0u; }
    run_digit = d; ++run;
  }
  if (run) atomicAdd(&s_h[run_digit], run);
  __syncthreads();
  if (s_h[threadIdx.x]) atomicAdd(&sel[SRV_SEL_HIST + threadIdx.x], s_h[threadIdx.x]);
}
// one workgroup: the bin that holds the rank becomes the next byte of the prefix; the histogram is cleared for the next pass
__global__ void __launch_bounds__(256) srv_select_pick_kernel(u32* sel, int shift) {
  __shared__ u32 s_h[256];
  s_h[threadIdx.x] = sel[SRV_SEL_HIST + threadIdx.x];
  sel[SRV_SEL_HIST + threadIdx.x] = 0u;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 rank = sel[SRV_SEL_RANK], d = 0u;
    while (d < 255u && rank >= s_h[d]) { rank -= s_h[d]; ++d; }
    sel[SRV_SEL_PREFIX] |= d << shift;
    sel[SRV_SEL_RANK] = rank;
  }
}
__global__ void __launch_bounds__(256) srv_mask_kernel(const u32* __restrict__ counts, u32 npx, u32 min_count, u32 factor, int rate_on, u32 rate_count,
                                                       const u32* __restrict__ sel, uint8_t* __restrict__ mask, u64* report) {
  const u32 B = sel[SRV_SEL_PREFIX];
  u64 n_hot = 0ull, ev_hot = 0ull, best = 0ull;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) {
    const u32 c = counts[i] + counts[npx + i];
    const bool hot = c >= min_count && ((factor != 0u && (u64)c > (u64)factor * (u64)B) || (rate_on && c > rate_count));
    mask[i] = hot ? (uint8_t)1 : (uint8_t)0;
    if (hot) { ++n_hot; ev_hot += c; }
    const u64 key = ((u64)c << 32) | (u64)(0xffffffffu - i);  // the largest count, the smallest pixel that holds it
    best = key > best ? key : best;
  }
  n_hot = wave_sum_u64(n_hot); ev_hot = wave_sum_u64(ev_hot); best = wave_max_u64(best);
  if ((threadIdx.x & (ESVO_WAVE - 1)) == 0) {
    if (n_hot) {
      atomicAdd(reinterpret_cast<unsigned long long*>(&report[SRV_R_HOT]), (unsigned long long)n_hot);
      atomicAdd(reinterpret_cast<unsigned long long*>(&report[SRV_R_EVENTS]), (unsigned long long)ev_hot);
    }
    atomicMax(reinterpret_cast<unsigned long long*>(&report[SRV_R_MAX]), (unsigned long long)best);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) report[SRV_R_BASELINE] = B;
}
__global__ void __launch_bounds__(256) srv_mask_or_kernel(uint8_t* __restrict__ into, const uint8_t* __restrict__ from, u32 npx) {
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) into[i] = (into[i] | from[i]) ? (uint8_t)1 : (uint8_t)0;
}
}  // namespace

void launch_survey_count(const SurveyArgs& a, hipStream_t s) {
  if (a.n == 0) return;
  hipLaunchKernelGGL(srv_count_kernel, dim3((a.n + SRV_CHUNK - 1u) / SRV_CHUNK), dim3(256), 0, s, a);
}
void launch_survey_first_bad(const u64* t, u32 n, u32* sel, hipStream_t s) {
  hipLaunchKernelGGL(srv_first_bad_init_kernel, dim3(1), dim3(1), 0, s, sel);
  if (n) hipLaunchKernelGGL(srv_first_bad_kernel, dim3(min((n + 255u) / 256u, 1024u)), dim3(256), 0, s, t, n, sel);
}
void launch_survey_mask(const u32* counts, u32 npx, u32 rank, u32 min_count, u32 factor, bool rate_on, u32 rate_count, u32* sel, uint8_t* mask,
                        u64* report, hipStream_t s) {
  const dim3 grid(min((npx + 255u) / 256u, 1024u));
  hipLaunchKernelGGL(srv_select_init_kernel, dim3(1), dim3(256), 0, s, sel, report, rank);
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(srv_select_hist_kernel, grid, dim3(256), 0, s, counts, npx, shift, sel);
    hipLaunchKernelGGL(srv_select_pick_kernel, dim3(1), dim3(256), 0, s, sel, shift);
  }
  hipLaunchKernelGGL(srv_mask_kernel, grid, dim3(256), 0, s, counts, npx, min_count, factor, rate_on ? 1 : 0, rate_count, sel, mask, report);
}
void launch_survey_mask_or(uint8_t* into, const uint8_t* from, u32 npx, hipStream_t s) {
  hipLaunchKernelGGL(srv_mask_or_kernel, dim3(min((npx + 255u) / 256u, 1024u)), dim3(256), 0, s, into, from, npx);
}

}  // namespace esvo
