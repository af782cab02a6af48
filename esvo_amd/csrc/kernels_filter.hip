// kernels_filter.hip — the event filter of the ingest path (include/esvo_hip.h, esvo_ts_filter_configure): hot-pixel mask,
// per-pixel refractory period, nearest-neighbour support, judged in stream order.
//
// The rule is sequential, but what it reads is local: an event's verdict depends on the history of its own pixel (mask, refractory
// chain) and on the `last` stamps of its 8 neighbours, and whether an event of a neighbour updated `last` depends on that
// neighbour's own history alone.  So a tile of 8x8 pixels that sees, in stream order, every event of its 10x10 patch (the tile and
// a one-pixel halo) reaches the sequential verdict for each of its own 64 pixels: it recomputes the chains of the halo pixels
// (their mask and refractory test need nothing outside the patch; their support test is skipped, it decides no update of `last`)
// and never asks another tile.  Three kernels over a packet of column events (u64 stamps, u16 x, u16 y):
//   flt_bin      thread / event, consecutive elements per lane: events outside the image get their verdict here; every other index
//                goes to the list of its own tile and of each neighbouring tile whose halo holds it (<= 4 lists, one atomic each;
//                lists of fixed capacity, the count keeps running beyond it);
//   flt_walk     one wave / tile: the patch of `last` and of the mask in LDS; the tile's list is sorted into index order (bitonic,
//                in LDS) and walked entry by entry -- lanes 0..8 read the 3x3 neighbourhood, a ballot answers the support test;
//                a tile whose count exceeds the capacity reads the PACKET instead, 64 consecutive events per step, and walks those
//                a ballot finds inside its patch: the same entries in the same order, so the same answers, at O(n / 64) steps
//                for at most 4 n / capacity such tiles.  The tile's 64 `last` values go to the OTHER image of a pair (a tile's halo
//                is another tile's own pixels: nobody may read what this launch writes);
//   flt_compact  thread / event: the kept events to their exclusive rank (scan.hip over bit 0 of the codes) in the twin staging,
//                polarity normalised to 0 / 1; the five verdict counts to the header in front of the twin's stamps, so that counts
//                and kept stamps come down with one copy -- and with them whether the packet was in order and its stamps valid,
//                for packets whose unfiltered stamps never reach the host (device columns, decoded words).
// Per event the code byte is verdict << 1 | kept.
//
// The burst stage (esvo_ts_burst_configure: trail / STC with polarity, between the mask and the refractory test) is a fourth kernel,
// launched between flt_bin and flt_walk only while the stage is on:
//   flt_burst    one wave / tile over the tile's OWN-pixel entries (the stage's rule needs no halo): an event's burst verdict depends
//                on the previous two raw events of its own pixel and on nothing else, so the entries, sorted by (pixel in tile,
//                packet index) in LDS (bitonic, 64-bit keys), are judged all at once -- entry i reads entry i - 1 for `linked` and
//                entry i - 2 for the `linked` bit of its predecessor, the first one or two entries of a pixel read the state the
//                packet found, the last entry of a pixel writes the state it leaves.  Every own entry gets a code here: MASKED,
//                ESVO_FILTER_BURST for the dropped ones, FLT_CODE_PENDING for those the walk still has to judge.  A tile whose
//                count exceeds the capacity reads the packet, 64 events per step, collects its own events in the same LDS array and
//                judges a batch whenever the array is nearly full, the state carried in LDS from batch to batch: the same rule on
//                the same events in the same order.  The state is a pair of images as `last` is.
// flt_walk<true> then leaves out every entry whose code says ESVO_FILTER_BURST, own pixels and halo alike (a burst-dropped event
// never reaches `last`); flt_walk<false>, the stage off, is the kernel as it was.
#include "common.hpp"

namespace esvo {

namespace {
constexpr int FLT_TILE = 8, FLT_PATCH = FLT_TILE + 2, FLT_CELLS = FLT_PATCH * FLT_PATCH;

__device__ inline uint8_t flt_code(u32 verdict) { return (uint8_t)((verdict << 1) | (verdict == ESVO_FILTER_KEPT ? 1u : 0u)); }

constexpr u32 FLT_CODE_BURST = (u32)ESVO_FILTER_BURST << 1;  // flt_code(ESVO_FILTER_BURST)
constexpr u32 FLT_CODE_PENDING = 0xfeu;  // passed the burst stage, the walk's to judge (verdict 7: nothing counts it, so the counts would not add up)
constexpr u64 BST_NONE = ~0ull;          // padding of the burst kernel's key array: behind every entry

// lane j's 64-bit value, j uniform
__device__ inline u64 lane_u64(u64 v, int j) {
  return ((u64)(u32)__builtin_amdgcn_readlane((int)(v >> 32), j) << 32) | (u64)(u32)__builtin_amdgcn_readlane((int)(v & 0xffffffffull), j);
}

__global__ void __launch_bounds__(256) flt_bin_kernel(FilterArgs a) {
  if (blockIdx.x == 0 && threadIdx.x < FLT_HDR_WORDS) a.hdr[threadIdx.x] = threadIdx.x == FLT_H_FIRST_BAD ? 0xffffffffu : 0u;  // (the compaction, two launches on, fills them)
  const int tiles_x = (a.W + FLT_TILE - 1) / FLT_TILE, tiles_y = (a.H + FLT_TILE - 1) / FLT_TILE;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
    const int x = a.x[i], y = a.y[i];
    if (x >= a.W || y >= a.H) { a.code[i] = flt_code(ESVO_FILTER_OUTSIDE); continue; }
    const int tx = x / FLT_TILE, ty = y / FLT_TILE, rx = x % FLT_TILE, ry = y % FLT_TILE;
    // the neighbouring tile columns / rows whose halo holds the pixel: -1, +1 or none (0)
    const int nx = rx == 0 && tx > 0 ? -1 : (rx == FLT_TILE - 1 && tx + 1 < tiles_x ? 1 : 0);
    const int ny = ry == 0 && ty > 0 ? -1 : (ry == FLT_TILE - 1 && ty + 1 < tiles_y ? 1 : 0);
    for (int k = 0; k < 4; ++k) {
      const int dx = (k & 1) ? nx : 0, dy = (k & 2) ? ny : 0;
      if (((k & 1) && !nx) || ((k & 2) && !ny)) continue;
      const u32 tile = (u32)(ty + dy) * (u32)tiles_x + (u32)(tx + dx);
      const u32 pos = atomicAdd(&a.tcount[tile], 1u);
      if (pos < a.tcap) a.tlist[(size_t)tile * a.tcap + pos] = i;
    }
  }
}

// `linked` of the burst stage: the event (t, p) continues the burst of the event (T, P) judged before it at the same pixel
__device__ inline bool bst_linked(u64 T, u32 P, u64 t, u32 p, u64 burst_ns) { return T != 0ull && p == P && (T > t || t - T <= burst_ns); }

__global__ void __launch_bounds__(64) flt_burst_kernel(FilterArgs a, BurstArgs b) {
  __shared__ u64 s_key[FLT_TILE_CAP_MAX];  // pixel of the tile << 32 | packet index
  __shared__ u64 s_t[FLT_TILE_CAP_MAX];    // the sorted entries' stamps and polarities
  __shared__ uint8_t s_p[FLT_TILE_CAP_MAX];
  __shared__ u64 s_st[2][FLT_TILE * FLT_TILE];  // the tile's state, [0] in front of the batch being judged, [1] behind it
  __shared__ uint8_t s_fl[2][FLT_TILE * FLT_TILE];
  const int lane = threadIdx.x;
  const u32 tile = blockIdx.x;
  const int tiles_x = (a.W + FLT_TILE - 1) / FLT_TILE;
  const int tx0 = (int)(tile % (u32)tiles_x) * FLT_TILE, ty0 = (int)(tile / (u32)tiles_x) * FLT_TILE;
  const u32 cnt = a.tcount[tile];  // (own and halo entries: the walk, which runs behind this kernel, clears it)
  const int ox = tx0 + lane % FLT_TILE, oy = ty0 + lane / FLT_TILE;
  const bool o_in = ox < a.W && oy < a.H;
  const size_t o_px = (size_t)oy * a.W + ox;
  s_st[0][lane] = o_in ? b.stamp_in[o_px] : 0ull;
  s_fl[0][lane] = o_in ? b.flags_in[o_px] : (uint8_t)0;
  __syncthreads();
  // One batch: the m entries of s_key (m uniform, 1 .. FLT_TILE_CAP_MAX), any order.
  const auto judge = [&](u32 m) {
    u32 N = 64;  // padded to a power of two
    while (N < m) N <<= 1;
    for (u32 k = m + lane; k < N; k += 64) s_key[k] = BST_NONE;
    __syncthreads();
    for (u32 k = 2; k <= N; k <<= 1)
      for (u32 j = k >> 1; j > 0; j >>= 1) {
        for (u32 q = lane; q < N / 2; q += 64) {
          const u32 lo = 2u * q - (q & (j - 1u)), hi = lo + j;
          const u64 va = s_key[lo], vb = s_key[hi];
          if ((va > vb) == ((lo & k) == 0u)) { s_key[lo] = vb; s_key[hi] = va; }
        }
        __syncthreads();
      }
    for (u32 k = lane; k < m; k += 64) {
      const u32 idx = (u32)s_key[k];
      s_t[k] = a.t[idx];
      s_p[k] = (uint8_t)columns_polarity(b.p, idx, b.p_type);
    }
    s_st[1][lane] = s_st[0][lane]; s_fl[1][lane] = s_fl[0][lane];
    __syncthreads();
    for (u32 k = lane; k < m; k += 64) {
      const u64 key = s_key[k];
      const u32 pix = (u32)(key >> 32), idx = (u32)key;
      const u64 t = s_t[k];
      const u32 p = s_p[k];
      const u32 k1 = k >= 1u ? k - 1u : 0u, k2 = k >= 2u ? k - 2u : 0u;
      const bool has1 = k >= 1u && (u32)(s_key[k1] >> 32) == pix, has2 = k >= 2u && (u32)(s_key[k2] >> 32) == pix;  // (sorted: has2 implies has1)
      const u64 T0 = s_st[0][pix];
      const u32 F0 = s_fl[0][pix];
      const u64 T1 = has1 ? s_t[k1] : T0;
      const u32 P1 = has1 ? (u32)s_p[k1] : (F0 & 1u);
      const bool linked = bst_linked(T1, P1, t, p, b.burst_ns);
      const u64 T2 = has2 ? s_t[k2] : T0;
      const u32 P2 = has2 ? (u32)s_p[k2] : (F0 & 1u);
      const bool K = has1 ? bst_linked(T2, P2, T1, P1, b.burst_ns) : ((F0 >> 1) & 1u) != 0u;  // `linked` of the event before
      const bool pass = b.mode == ESVO_BURST_TRAIL ? !linked : (b.mode == ESVO_BURST_STC_CUT_TRAIL ? linked && !K : linked);
      a.code[idx] = (uint8_t)(pass ? FLT_CODE_PENDING : FLT_CODE_BURST);
      const bool newest = k + 1u >= m || (u32)(s_key[k + 1u] >> 32) != pix;  // (k + 1 < m: an entry)
      if (newest) { s_st[1][pix] = t; s_fl[1][pix] = (uint8_t)(p | (linked ? 2u : 0u)); }
    }
    __syncthreads();
    s_st[0][lane] = s_st[1][lane]; s_fl[0][lane] = s_fl[1][lane];
    __syncthreads();
  };
  // the lane's event (have: there is one) into the batch if it lies at an unmasked pixel of the tile; -> the batch's new length (uniform)
  const auto collect = [&](u32 m, bool have, u32 idx) -> u32 {
    const int ex = have ? (int)a.x[idx] : -1, ey = have ? (int)a.y[idx] : -1;
    const bool own = have && ex < a.W && ey < a.H && ex >= tx0 && ex < tx0 + FLT_TILE && ey >= ty0 && ey < ty0 + FLT_TILE;
    const bool masked = own && a.mask && a.mask[(size_t)ey * a.W + ex];
    if (masked) a.code[idx] = flt_code(ESVO_FILTER_MASKED);  // (the walk says so again: every own entry has a code of this packet before it runs)
    const bool valid = own && !masked;
    const u64 ball = __ballot(valid);
    if (valid) s_key[m + (u32)__popcll(ball & ((1ull << lane) - 1ull))] = ((u64)(u32)((ey - ty0) * FLT_TILE + (ex - tx0)) << 32) | (u64)idx;
    return m + (u32)__popcll(ball);
  };
  if (cnt != 0u) {
    u32 m = 0;
    if (cnt <= a.tcap) {
      for (u32 base = 0; base < cnt; base += 64) {
        const bool have = base + lane < cnt;
        m = collect(m, have, have ? a.tlist[(size_t)tile * a.tcap + base + lane] : 0u);
      }
    } else {
      for (u32 base = 0; base < a.n; base += 64) {
        m = collect(m, base + lane < a.n, base + lane);
        if (m + 64u > FLT_TILE_CAP_MAX) { __syncthreads(); judge(m); m = 0; }
      }
    }
    __syncthreads();
    if (m) judge(m);
  }
  if (o_in) { b.stamp_out[o_px] = s_st[0][lane]; b.flags_out[o_px] = s_fl[0][lane]; }
}

// BURST: the burst stage ran in front (flt_burst_kernel): entries it dropped are left out
template <bool BURST>
__global__ void __launch_bounds__(64) flt_walk_kernel(FilterArgs a) {
  __shared__ u64 s_last[FLT_CELLS];
  __shared__ uint8_t s_mask[FLT_CELLS];
  __shared__ u32 s_list[FLT_TILE_CAP_MAX];
  const int lane = threadIdx.x;
  const u32 tile = blockIdx.x;
  const int tiles_x = (a.W + FLT_TILE - 1) / FLT_TILE;
  const int x0 = (int)(tile % (u32)tiles_x) * FLT_TILE - 1, y0 = (int)(tile / (u32)tiles_x) * FLT_TILE - 1;  // the patch's origin
  const u32 cnt = a.tcount[tile];
  // the lane's own pixel of the tile
  const int ox = x0 + 1 + lane % FLT_TILE, oy = y0 + 1 + lane / FLT_TILE;
  const bool o_in = ox < a.W && oy < a.H;
  const size_t o_px = (size_t)oy * a.W + ox;
  if (cnt == 0) {  // nothing of the packet reaches the patch: the tile's stamps as they are
    if (o_in) a.last_out[o_px] = a.last_in[o_px];
    return;
  }
  for (int c = lane; c < FLT_CELLS; c += 64) {
    const int px = x0 + c % FLT_PATCH, py = y0 + c / FLT_PATCH;
    const bool in = px >= 0 && px < a.W && py >= 0 && py < a.H;
    s_last[c] = in ? a.last_in[(size_t)py * a.W + px] : 0ull;  // (outside the image: no event ever lands there, 0 never supports)
    s_mask[c] = in && a.mask ? a.mask[(size_t)py * a.W + px] : (uint8_t)0;
  }
  __syncthreads();
  // lanes 0..8 stand for the 3x3 neighbourhood of the entry being judged (lane 4: the pixel itself)
  const int ndx = lane % 3 - 1, ndy = (lane / 3) % 3 - 1;
  // One batch: the entries the lanes named in `todo` hold (index, x, y, stamp), walked in lane order.  Everything that decides is
  // uniform across the wave; the lane that holds an entry keeps its code.
  const auto walk = [&](u64 todo, u32 idx, int ex, int ey, u64 et) {
    u32 my_code = 0xffffffffu;
    todo = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(todo >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(todo & 0xffffffffull));
    while (todo) {
      const int j = __builtin_ctzll(todo);  // (uniform: readlane below takes it as a scalar)
      todo &= todo - 1ull;
      const int cx = __builtin_amdgcn_readlane(ex, j) - x0, cy = __builtin_amdgcn_readlane(ey, j) - y0;  // 0..9
      const u64 t = lane_u64(et, j);
      const int c = cy * FLT_PATCH + cx;
      const int qx = cx + ndx, qy = cy + ndy;
      const bool q_in = lane < 9 && qx >= 0 && qx < FLT_PATCH && qy >= 0 && qy < FLT_PATCH;
      const u64 L = q_in ? s_last[qy * FLT_PATCH + qx] : 0ull;
      const u64 Lc = lane_u64(L, 4);
      u32 verdict;
      if (s_mask[c]) verdict = ESVO_FILTER_MASKED;
      else if (a.refractory_ns && Lc && (Lc > t || t - Lc < a.refractory_ns)) verdict = ESVO_FILTER_REFRACTORY;
      else {
        const bool sup = lane < 9 && lane != 4 && L && (L > t || t - L <= a.support_ns);
        const bool any = __ballot(sup) != 0ull;
        verdict = a.support_ns && !any ? ESVO_FILTER_UNSUPPORTED : ESVO_FILTER_KEPT;
        __syncthreads();  // (one wave: orders the reads above before the write)
        if (lane == 0) s_last[c] = t;
        __syncthreads();
      }
      const bool own = cx >= 1 && cx <= FLT_TILE && cy >= 1 && cy <= FLT_TILE;  // the halo's events are another tile's to answer
      if (lane == j && own) my_code = flt_code(verdict);
    }
    if (my_code != 0xffffffffu) a.code[idx] = (uint8_t)my_code;
  };
  if (cnt <= a.tcap) {
    u32 N = 64;  // the list padded to a power of two
    while (N < cnt) N <<= 1;
    for (u32 k = lane; k < N; k += 64) s_list[k] = k < cnt ? a.tlist[(size_t)tile * a.tcap + k] : 0xffffffffu;
    __syncthreads();
    for (u32 k = 2; k <= N; k <<= 1)
      for (u32 j = k >> 1; j > 0; j >>= 1) {
        for (u32 q = lane; q < N / 2; q += 64) {
          const u32 lo = 2u * q - (q & (j - 1u)), hi = lo + j;
          const u32 va = s_list[lo], vb = s_list[hi];
          if ((va > vb) == ((lo & k) == 0u)) { s_list[lo] = vb; s_list[hi] = va; }
        }
        __syncthreads();
      }
    for (u32 base = 0; base < cnt; base += 64) {
      const u32 m = min(64u, cnt - base);
      const bool have = (u32)lane < m;
      const u32 idx = have ? s_list[base + lane] : 0u;
      u64 todo = m == 64u ? ~0ull : (1ull << m) - 1ull;
      if constexpr (BURST) todo = __ballot(have && a.code[idx] != FLT_CODE_BURST);
      walk(todo, idx, have ? (int)a.x[idx] : 0, have ? (int)a.y[idx] : 0, have ? a.t[idx] : 0ull);
    }
  } else {
    for (u32 base = 0; base < a.n; base += 64) {
      const u32 idx = base + lane;
      const bool have = idx < a.n;
      const int ex = have ? (int)a.x[idx] : 0, ey = have ? (int)a.y[idx] : 0;
      bool mine = have && ex < a.W && ey < a.H && ex >= x0 && ex < x0 + FLT_PATCH && ey >= y0 && ey < y0 + FLT_PATCH;
      if constexpr (BURST) mine = mine && a.code[idx] != FLT_CODE_BURST;
      const u64 todo = __ballot(mine);
      if (!todo) continue;
      walk(todo, idx, ex, ey, mine ? a.t[idx] : 0ull);
    }
  }
  __syncthreads();
  if (o_in) a.last_out[o_px] = s_last[(lane / FLT_TILE + 1) * FLT_PATCH + lane % FLT_TILE + 1];
  if (lane == 0) a.tcount[tile] = 0u;  // (only this workgroup reads it: the list is free for the next packet)
}

__global__ void __launch_bounds__(256) flt_compact_kernel(FilterArgs a, const u32* __restrict__ prefix, const void* __restrict__ p, int p_type,
                                                          u64* __restrict__ out_t, uint16_t* __restrict__ out_x, uint16_t* __restrict__ out_y,
                                                          uint8_t* __restrict__ out_p) {
  __shared__ u32 s_cnt[9];  // per verdict 0..7; [8]: the packet is not in order
  if (threadIdx.x < 9) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.n) {
    const u32 c = a.code[i];
    atomicAdd(&s_cnt[(c >> 1) & 7u], 1u);
    // the packet's order and the validity of its stamps, for packets whose stamps never reach the host: decided here, read with the counts
    const u64 t = a.t[i], before = i ? a.t[i - 1] : a.newest;
    if (t < before) s_cnt[8] = 1u;
    if (t == COL_BAD_STAMP) atomicMin(&a.hdr[FLT_H_FIRST_BAD], i);
    if (c & 1u) {
      const u32 pos = prefix[i];
      out_t[pos] = a.t[i]; out_x[pos] = a.x[i]; out_y[pos] = a.y[i];
      out_p[pos] = (uint8_t)columns_polarity(p, i, p_type);
    }
  }
  __syncthreads();
  if (threadIdx.x < 5 && s_cnt[threadIdx.x]) atomicAdd(&a.hdr[FLT_H_VERDICT0 + threadIdx.x], s_cnt[threadIdx.x]);
  if (threadIdx.x == ESVO_FILTER_BURST && s_cnt[ESVO_FILTER_BURST]) atomicAdd(&a.hdr[FLT_H_BURST], s_cnt[ESVO_FILTER_BURST]);
  if (threadIdx.x == 8 && s_cnt[8]) atomicOr(&a.hdr[FLT_H_UNSORTED], 1u);
}
}  // namespace

size_t filter_tiles(int W, int H) { return (size_t)((W + FLT_TILE - 1) / FLT_TILE) * ((H + FLT_TILE - 1) / FLT_TILE); }

// bin -> (burst ->) walk -> scan -> compact on `s`.  scan_tmp: a.n + scan_scratch_elems(a.n) words (the prefix, the scan's sums);
// a.hdr[FLT_H_VERDICT0 + v] receives the count of verdict v (v = 0: the kept events, the twin's length), a.hdr[FLT_H_BURST] that of
// ESVO_FILTER_BURST.
void launch_event_filter(const FilterArgs& a, const BurstArgs& b, u32* scan_tmp, const void* p, int p_type, u64* out_t, uint16_t* out_x,
                         uint16_t* out_y, uint8_t* out_p, hipStream_t s) {
  if (a.n == 0) return;
  const u32 blocks = (a.n + 255u) / 256u;
  hipLaunchKernelGGL(flt_bin_kernel, dim3(min(blocks, 2048u)), dim3(256), 0, s, a);
  const dim3 tiles((u32)filter_tiles(a.W, a.H));
  if (b.mode != ESVO_BURST_OFF) {
    hipLaunchKernelGGL(flt_burst_kernel, tiles, dim3(64), 0, s, a, b);
    hipLaunchKernelGGL(flt_walk_kernel<true>, tiles, dim3(64), 0, s, a);
  } else {
    hipLaunchKernelGGL(flt_walk_kernel<false>, tiles, dim3(64), 0, s, a);
  }
  launch_exclusive_scan_code_bit0(a.code, scan_tmp, nullptr, scan_tmp + a.n, a.n, nullptr, s);
  hipLaunchKernelGGL(flt_compact_kernel, dim3(blocks), dim3(256), 0, s, a, scan_tmp, p, p_type, out_t, out_x, out_y, out_p);
}

}  // namespace esvo
