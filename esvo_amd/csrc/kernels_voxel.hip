// kernels_voxel.hip — pcl::VoxelGrid<PointXYZ> with a cubic leaf (esvo_Mapping.cpp:960-964) on the device: the points, order
// and float bits of esvo_voxel_filter_xyz (api_out.hip), which stays the host yardstick.
//
//   bounds    per-axis min / max over the rows whose three coordinates are finite, and their count (ordered-integer atomics)
//   grid      one thread: inv = 1 / leaf, minb = floor(min inv), div = floor(max inv) - minb + 1, the cell count and its bit width
//   keys      (key << 32 | input index) per row; key = (ix - minb.x) + (iy - minb.y) div.x + (iz - minb.z) div.x div.y, and the
//             CELL COUNT for a row that is not finite: one more than the largest key, so those rows sort behind all others
//   sort      LSD radix sort of the pairs by key, 8 bits per pass, as many passes as the cell count has bits.  Every pass is
//             STABLE -- tile histogram, one exclusive scan over [digit][tile] (scan.hip), scatter by rank within the tile --
//             and the pairs start in input order, so the rows of a voxel end up in input order.  The sort by itself is
//             launch_radix_sort_pairs, which the LM launch's processing order uses as well (kernels_lm.hip)
//   heads     flag per sorted position: first row of its voxel; their exclusive scan numbers the voxels in ascending key
//   centroids one thread per voxel walks its run: a sequential float sum per axis from 0 in input order, then / (float)count
//
// The centroid of a voxel depends on the ORDER of its rows (float addition), which is why the sort must be stable and the sum a
// chain; neither the number of passes nor the tile size changes a bit of the result.  All arithmetic is float, un-fused.
#include <algorithm>

#include "common.hpp"
#include "scan.hpp"

namespace esvo {

static constexpr int VOX_B = 256;                  // threads per block of the sort kernels (4 waves)
static constexpr int VOX_ROUNDS = 8;               // rows per thread
static constexpr int VOX_TILE = VOX_B * VOX_ROUNDS;  // rows per block and radix pass

// floats as unsigned integers in the same order (-0 sorts below +0; both floor to cell 0, so which one wins does not matter)
__device__ inline u32 vox_ordered(float f) {
  const u32 u = __float_as_uint(f);
  return u ^ (((u32)((int)u >> 31)) | 0x80000000u);
}
__device__ inline float vox_unordered(u32 k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ inline bool vox_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

__global__ void voxel_init_kernel(VoxelGrid* g) {
  for (int c = 0; c < 3; ++c) { g->mn[c] = 0xffffffffu; g->mx[c] = 0u; g->minb[c] = 0; g->div[c] = 0; }
  g->n_finite = g->too_large = g->cells = g->key_bits = g->n_voxels = 0u;
  g->inv = 0.f;
}

__global__ void __launch_bounds__(256) voxel_bounds_kernel(const float* __restrict__ xyz, u32 n, VoxelGrid* __restrict__ g) {
  u32 mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u}, cnt = 0;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    if (!vox_finite(p[0]) || !vox_finite(p[1]) || !vox_finite(p[2])) continue;
    ++cnt;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const u32 k = vox_ordered(p[c]);
      mn[c] = min(mn[c], k);
      mx[c] = max(mx[c], k);
    }
  }
#pragma unroll
  for (int d = 1; d < ESVO_WAVE; d <<= 1) {
    cnt += __shfl_xor(cnt, d, ESVO_WAVE);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      mn[c] = min(mn[c], (u32)__shfl_xor(mn[c], d, ESVO_WAVE));
      mx[c] = max(mx[c], (u32)__shfl_xor(mx[c], d, ESVO_WAVE));
    }
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicAdd(&g->n_finite, cnt);
    for (int c = 0; c < 3; ++c) { atomicMin(&g->mn[c], mn[c]); atomicMax(&g->mx[c], mx[c]); }
  }
}

__global__ void voxel_grid_kernel(float leaf, VoxelGrid* g) {
  if (g->n_finite == 0u) return;
  const float inv = __fdiv_rn(1.0f, leaf);
  g->inv = inv;
  for (int c = 0; c < 3; ++c) {
    g->minb[c] = (long long)floorf(__fmul_rn(vox_unordered(g->mn[c]), inv));
    g->div[c] = (long long)floorf(__fmul_rn(vox_unordered(g->mx[c]), inv)) - g->minb[c] + 1;
  }
  if (__dmul_rn(__dmul_rn((double)g->div[0], (double)g->div[1]), (double)g->div[2]) > 2147483647.0) { g->too_large = 1u; return; }
  const u32 cells = (u32)(g->div[0] * g->div[1] * g->div[2]);
  g->cells = cells;
  g->key_bits = 32u - (u32)__clz((int)cells);  // bits of the LARGEST key in use: the cell count itself (rows that are not finite)
}

__global__ void __launch_bounds__(256) voxel_keys_kernel(const float* __restrict__ xyz, u32 n, const VoxelGrid* __restrict__ g,
                                                         u64* __restrict__ pairs) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
  u32 key = g->cells;
  if (vox_finite(p[0]) && vox_finite(p[1]) && vox_finite(p[2])) {
    const float inv = g->inv;
    const long long a = (long long)floorf(__fmul_rn(p[0], inv)) - g->minb[0], b = (long long)floorf(__fmul_rn(p[1], inv)) - g->minb[1],
                    c = (long long)floorf(__fmul_rn(p[2], inv)) - g->minb[2];
    key = (u32)(a + b * g->div[0] + c * g->div[0] * g->div[1]);
  }
  pairs[i] = ((u64)key << 32) | i;
}

__device__ inline u32 vox_digit(u64 pair, u32 shift) { return (u32)(pair >> (32u + shift)) & 255u; }

// hist[digit * n_tiles + tile] = rows of the tile with that digit
// (n_dev, nullable: the row count lives on the device and n bounds it -- the grid, and with it the layout of hist, follow the bound)
__global__ void __launch_bounds__(VOX_B) voxel_hist_kernel(const u64* __restrict__ pairs, u32 n, const u32* __restrict__ n_dev, u32 shift,
                                                           u32* __restrict__ hist) {
  __shared__ u32 cnt[256];
  if (n_dev) n = min(n, *n_dev);
  cnt[threadIdx.x] = 0u;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * VOX_TILE;
  for (int r = 0; r < VOX_ROUNDS; ++r) {
    const size_t i = base + (size_t)r * VOX_B + threadIdx.x;
    if (i < n) atomicAdd(&cnt[vox_digit(pairs[i], shift)], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = cnt[threadIdx.x];
}

// offs: the exclusive scan of hist -- where the tile's first row with that digit goes.  A row's place is that plus the rows
// of the tile in front of it with the same digit: those of earlier rounds (base), of earlier waves of its round (wcnt) and of
// lower lanes of its wave (the match mask), which keeps equal digits in their order.
// out_index (non-null in the last pass of a sort whose caller wants the permutation alone): the row's index goes there, not the pair
__global__ void __launch_bounds__(VOX_B) voxel_scatter_kernel(const u64* __restrict__ in, u64* __restrict__ out, u32 n,
                                                              const u32* __restrict__ n_dev, u32 shift, const u32* __restrict__ offs,
                                                              u32* __restrict__ out_index) {
  constexpr int NW = VOX_B / ESVO_WAVE;
  if (n_dev) n = min(n, *n_dev);
  __shared__ u32 base[256];
  __shared__ u32 wcnt[NW][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  base[threadIdx.x] = offs[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
  const size_t first = (size_t)blockIdx.x * VOX_TILE;
  for (int r = 0; r < VOX_ROUNDS; ++r) {
#pragma unroll
    for (int w = 0; w < NW; ++w) wcnt[w][threadIdx.x] = 0u;
    __syncthreads();
    const size_t i = first + (size_t)r * VOX_B + threadIdx.x;
    const bool valid = i < n;
    const u64 pair = valid ? in[i] : 0ull;
    const u32 d = vox_digit(pair, shift);
    u64 same = __ballot(valid);  // lanes of this wave that hold a row with the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const u64 m = __ballot((d >> b) & 1u);
      same &= ((d >> b) & 1u) ? m : ~m;
    }
    const u32 rank = (u32)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank == 0u) wcnt[wave][d] = (u32)__popcll(same);
    __syncthreads();
    if (valid) {
      u32 pos = base[d] + rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
      if (pos < n) {  // (a permutation of [0, n): always)
        if (out_index) out_index[pos] = (u32)pair;
        else out[pos] = pair;
      }
    }
    __syncthreads();
    u32 add = 0u;
#pragma unroll
    for (int w = 0; w < NW; ++w) add += wcnt[w][threadIdx.x];
    base[threadIdx.x] += add;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) voxel_heads_kernel(const u64* __restrict__ sorted, u32 n_finite, u32* __restrict__ heads) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_finite) return;
  heads[j] = (j == 0u || (u32)(sorted[j] >> 32) != (u32)(sorted[j - 1] >> 32)) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) voxel_centroid_kernel(const float* __restrict__ xyz, const u64* __restrict__ sorted,
                                                             const u32* __restrict__ heads, const u32* __restrict__ rank, u32 n_finite,
                                                             u32 cap_points, float* __restrict__ out) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_finite || !heads[j]) return;
  const u32 v = rank[j];
  if (v >= cap_points) return;
  const u32 key = (u32)(sorted[j] >> 32);
  float c[3] = {0.f, 0.f, 0.f};
  u32 b = j;
  for (; b < n_finite; ++b) {
    const u64 pr = sorted[b];
    if ((u32)(pr >> 32) != key) break;
    const size_t i = (size_t)(u32)pr;
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] = __fadd_rn(c[d], xyz[3 * i + d]);
  }
  const float cnt = (float)(b - j);
#pragma unroll
  for (int d = 0; d < 3; ++d) out[3 * (size_t)v + d] = __fdiv_rn(c[d], cnt);
}

u32 voxel_tiles(size_t n) { return (u32)((n + VOX_TILE - 1) / VOX_TILE); }
size_t voxel_hist_words(size_t n) { return 256 * (size_t)std::max<u32>(voxel_tiles(n), 1u); }

void launch_voxel_bounds(const float* xyz, u32 n, float leaf, VoxelGrid* grid, hipStream_t s) {
  hipLaunchKernelGGL(voxel_init_kernel, dim3(1), dim3(1), 0, s, grid);
  if (n == 0) return;
  const u32 blocks = std::min<u32>((n + 255u) / 256u, 1024u);
  hipLaunchKernelGGL(voxel_bounds_kernel, dim3(blocks), dim3(256), 0, s, xyz, n, grid);
  hipLaunchKernelGGL(voxel_grid_kernel, dim3(1), dim3(1), 0, s, leaf, grid);
}

// The sort by itself: stable LSD radix sort of the rows (key << 32 | index) in pairs[0] by the low key_bits bits of their keys,
// 8 bits per pass.  n bounds the row count and sizes the launches; n_dev (nullable) is the count itself where it lives on the
// device -- rows behind it are neither read nor written.  pairs[0] / pairs[1]: n words of 64 bits each; hist:
// voxel_hist_words(n); scan_tmp: scan_scratch_elems of that.  Returns the buffer that holds the sorted pairs -- or, with
// out_index (n words) and at least one pass, nullptr: the last pass then writes the sorted rows' indices there and nothing else.
const u64* launch_radix_sort_pairs(u64* const pairs[2], u32 n, const u32* n_dev, u32 key_bits, u32* hist, u32* scan_tmp, u32* out_index,
                                   hipStream_t s) {
  const u32 tiles = voxel_tiles(n);
  int cur = 0;
  for (u32 shift = 0; n && shift < key_bits; shift += 8u) {
    u32* const index = shift + 8u >= key_bits ? out_index : nullptr;
    hipLaunchKernelGGL(voxel_hist_kernel, dim3(tiles), dim3(VOX_B), 0, s, pairs[cur], n, n_dev, shift, hist);
    launch_exclusive_scan_u32(hist, hist, nullptr, scan_tmp, 256 * (size_t)tiles, s);
    hipLaunchKernelGGL(voxel_scatter_kernel, dim3(tiles), dim3(VOX_B), 0, s, pairs[cur], pairs[cur ^ 1], n, n_dev, shift, hist, index);
    if (index) return nullptr;
    cur ^= 1;
  }
  return pairs[cur];
}

// Returns the buffer that holds the sorted pairs (buffers: launch_radix_sort_pairs).
const u64* launch_voxel_sort(const float* xyz, u32 n, const VoxelGrid* grid, u32 key_bits, u64* const pairs[2], u32* hist, u32* scan_tmp,
                             hipStream_t s) {
  hipLaunchKernelGGL(voxel_keys_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, xyz, n, grid, pairs[0]);
  return launch_radix_sort_pairs(pairs, n, nullptr, key_bits, hist, scan_tmp, nullptr, s);
}

// heads | rank: n_finite words each; the voxel count lands in grid->n_voxels; centroids: cap_points x 3 floats
void launch_voxel_centroids(const float* xyz, const u64* sorted, u32 n_finite, u32* heads, u32* rank, VoxelGrid* grid, u32* scan_tmp,
                            float* centroids, u32 cap_points, hipStream_t s) {
  const dim3 g((n_finite + 255u) / 256u);
  hipLaunchKernelGGL(voxel_heads_kernel, g, dim3(256), 0, s, sorted, n_finite, heads);
  launch_exclusive_scan_u32(heads, rank, &grid->n_voxels, scan_tmp, (size_t)n_finite, s);
  hipLaunchKernelGGL(voxel_centroid_kernel, g, dim3(256), 0, s, xyz, sorted, heads, rank, n_finite, cap_points, centroids);
}

}  // namespace esvo
