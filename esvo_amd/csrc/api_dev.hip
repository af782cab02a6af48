// api_dev.hip — test entry points of the shared device primitives: the scans, the fused scan + compaction, the two copy kernels
// of scan.hip and the inline functions of fdiv.hpp.  tests/test_gpu_primitives.py drives them at the sizes where those kernels
// switch paths, which no tick of a fixture can be made to hit.
//
// esvo_debug_* entry points: NOT part of the documented ABI (include/esvo_hip.h does not declare them, ESVO_HIP_ABI_VERSION does not
// count them).  They need no handle and nothing of the product path calls them.  Every call takes host arrays, runs exactly ONE of
// the launch_* functions (or one small kernel around the fdiv.hpp inlines) on a stream of its own, waits for it and copies the results
// back.  Every device (or pinned) buffer the kernel may write is allocated at exactly the size given -- what the production caller
// passes -- between two guard regions of GUARD_WORDS words holding a fixed pattern.  Written buffers are in/out: the caller's bytes
// are what the kernel finds there, so the caller chooses the prefill and can tell "not written" from "written as zero".
// Return value: a negative esvo_status_t, or the number of guard words that no longer hold the pattern (0 when all is well).
// The exceptions are at the end, take a handle, launch nothing and copy something out: esvo_debug_fuse_cell_counts one buffer of the
// last fusion (tests/test_gpu_fuse_cases.py), esvo_debug_bm_owner_count the owner count of the last shared block-matching launch
// (tests/test_gpu_bm_dedupe.py), esvo_debug_ts_ring a camera's event ring and the host's stamp mirror
// (tests/test_gpu_event_columns.py); esvo_debug_live_allocations and esvo_debug_devmem_selftest take no handle and read / walk
// the ledger of devmem.hpp (tests/test_gpu_lifecycle.py).
#include <vector>

#include "context.hpp"
#include "fdiv.hpp"

namespace {
using esvo::u32;

constexpr size_t GUARD_WORDS = 64;
constexpr size_t GUARD_BYTES = GUARD_WORDS * sizeof(u32);  // 256: the payload behind it keeps the alignment of any record
constexpr u32 GUARD_PATTERN = 0xA55AC33Cu;

// one guarded buffer: [guard | payload | guard], in device memory or in pinned host memory
struct GBuf {
  uint8_t* base = nullptr;
  size_t bytes = 0;
  bool pinned = false;
  GBuf() = default;
  GBuf(const GBuf&) = delete;
  GBuf& operator=(const GBuf&) = delete;
  ~GBuf() {
    if (!base) return;
    if (pinned) hipHostFree(base);
    else hipFree(base);
  }
  // payload of `n` bytes (a multiple of 4) taken from `init` (nullptr: the guard pattern)
  hipError_t make(size_t n, const void* init, bool pin = false) {
    bytes = n;
    pinned = pin;
    std::vector<u32> img(2 * GUARD_WORDS + n / 4, GUARD_PATTERN);
    if (init && n) std::memcpy(img.data() + GUARD_WORDS, init, n);
    hipError_t e = pin ? hipHostMalloc(reinterpret_cast<void**>(&base), img.size() * 4, hipHostMallocDefault)
                       : hipMalloc(reinterpret_cast<void**>(&base), img.size() * 4);
    if (e != hipSuccess) { base = nullptr; return e; }
    if (pin) { std::memcpy(base, img.data(), img.size() * 4); return hipSuccess; }
    return hipMemcpy(base, img.data(), img.size() * 4, hipMemcpyHostToDevice);
  }
  template <class T> T* ptr() const { return reinterpret_cast<T*>(base + GUARD_BYTES); }
  // payload back to `dst` (nullable: the guards alone are read); the guard words that changed are added to *bad
  hipError_t finish(void* dst, long long* bad) const {
    u32 g[2 * GUARD_WORDS];
    const uint8_t* const tail = base + GUARD_BYTES + bytes;
    if (pinned) {
      std::memcpy(g, base, GUARD_BYTES);
      std::memcpy(g + GUARD_WORDS, tail, GUARD_BYTES);
      if (dst && bytes) std::memcpy(dst, base + GUARD_BYTES, bytes);
    } else {
      hipError_t e = hipMemcpy(g, base, GUARD_BYTES, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(g + GUARD_WORDS, tail, GUARD_BYTES, hipMemcpyDeviceToHost);
      if (e == hipSuccess && dst && bytes) e = hipMemcpy(dst, base + GUARD_BYTES, bytes, hipMemcpyDeviceToHost);
      if (e != hipSuccess) return e;
    }
    for (size_t i = 0; i < 2 * GUARD_WORDS; ++i) *bad += (g[i] != GUARD_PATTERN);
    return hipSuccess;
  }
};

template <bool Pinned>
int devmem_selftest() {
  using B = esvo::Buf<u32, Pinned>;
  const size_t a0 = esvo::g_live_allocs.load(), b0 = esvo::g_live_bytes.load();
  const auto at = [&](size_t allocs, size_t bytes) { return esvo::g_live_allocs.load() == a0 + allocs && esvo::g_live_bytes.load() == b0 + bytes; };
  { B e; if (e || e.cap()) return 1; }                                          // an empty buffer and its destructor
  if (!at(0, 0)) return 2;
  {
    B b;
    if (b.alloc(100) != hipSuccess || !b || b.cap() != 100 || !at(1, 400)) return 3;
    if ((Pinned ? (std::memset(b, 0x5a, 400), hipSuccess) : hipMemset(b, 0x5a, 400)) != hipSuccess) return 4;  // the memory is there
    u32* const p = b;
    if (b.grow(50) != hipSuccess || b != p || b.cap() != 100 || !at(1, 400)) return 5;   // smaller: nothing happens
    if (b.grow(300) != hipSuccess || !b || b.cap() != 300 || !at(1, 1200)) return 6;     // larger: exactly what was asked for
    u32* const q = b;
    B c(std::move(b));                                                                    // move construction: no free
    if (b || b.cap() || c != q || c.cap() != 300 || !at(1, 1200)) return 7;
    B d;
    if (d.alloc(10) != hipSuccess || !at(2, 1240)) return 8;
    d = std::move(c);                                                                     // move assignment: one free, the target's
    if (c || c.cap() || d != q || d.cap() != 300 || !at(1, 1200)) return 9;
    if (d.release() != hipSuccess || d || d.cap() || !at(0, 0)) return 10;
    if (d.release() != hipSuccess || !at(0, 0)) return 11;                                // twice: nothing more
    if (d.alloc(0) != hipSuccess || d.cap() != 1 || !at(1, 4)) return 12;                 // at least one element
  }                                                                                       // ... freed by its destructor
  return at(0, 0) ? 0 : 13;
}

struct OwnStream {
  hipStream_t s = nullptr;
  ~OwnStream() { if (s) hipStreamDestroy(s); }
};

// what every call does around its one launch
#define DEV_BEGIN()              \
  esvo_context* h = nullptr;     \
  long long bad = 0;             \
  OwnStream st;                  \
  HIPCHK(hipStreamCreate(&st.s))
#define DEV_RUN_DONE()           \
  HIPCHK(hipGetLastError());     \
  HIPCHK(hipStreamSynchronize(st.s))
#define DEV_RETURN() return (int)std::min<long long>(bad, 0x7fffffff)

__global__ void __launch_bounds__(256) debug_fdiv_kernel(const double* __restrict__ a, const double* __restrict__ b, size_t n,
                                                         double* __restrict__ q_by, double* __restrict__ q_fast,
                                                         double* __restrict__ q_refined, u32* __restrict__ fast,
                                                         u32* __restrict__ ok_a) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const esvo::Recip R = esvo::make_recip(b[i]);
    q_by[i] = esvo::div_by(a[i], R);
    q_fast[i] = esvo::div_fast(a[i], R);  // computed whether or not its precondition holds: the caller reads it where it does
    esvo::Recip V;  // a divisor the caller vouches for (kernels_bm.hip, kernels_lm.hip): recip_refined, no window test
    V.b = b[i];
    V.y = esvo::recip_refined(b[i]);
    q_refined[i] = esvo::div_fast(a[i], V);
    fast[i] = R.fast ? 1u : 0u;
    ok_a[i] = esvo::fdiv_ok(a[i]) ? 1u : 0u;
  }
}
__global__ void __launch_bounds__(256) debug_fdiv_b4_kernel(const double* __restrict__ b, const double* __restrict__ a1,
                                                            const double* __restrict__ a2, const double* __restrict__ a3,
                                                            const double* __restrict__ a4, size_t n, u32* __restrict__ ok,
                                                            double* __restrict__ q) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    ok[i] = esvo::fdiv_ok_b4(b[i], a1[i], a2[i], a3[i], a4[i]) ? 1u : 0u;
    const esvo::Recip R = esvo::make_recip(b[i]);
    q[4 * i + 0] = esvo::div_fast(a1[i], R);
    q[4 * i + 1] = esvo::div_fast(a2[i], R);
    q[4 * i + 2] = esvo::div_fast(a3[i], R);
    q[4 * i + 3] = esvo::div_fast(a4[i], R);
  }
}
__global__ void __launch_bounds__(256) debug_recip_kernel(const double* __restrict__ b, size_t n, double* __restrict__ y_make,
                                                          double* __restrict__ y_refined) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    y_make[i] = esvo::make_recip(b[i]).y;
    y_refined[i] = esvo::recip_refined(b[i]);
  }
}
__global__ void __launch_bounds__(256) debug_sqrt_kernel(const double* __restrict__ x, size_t n, double* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = esvo::sqrt_moderate(x[i]);
}
inline unsigned fdiv_blocks(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 4096); }
}  // namespace

extern "C" {

// out[0] scan_is_small(n), [1] scan_compact_is_small(n), [2] scan_tiles(n), [3] scan_scratch_elems(n)
int esvo_debug_scan_predicates(size_t n, size_t out[4]) {
  if (!out) return ESVO_ERR_INVALID_ARG;
  out[0] = esvo::scan_is_small(n) ? 1 : 0;
  out[1] = esvo::scan_compact_is_small(n) ? 1 : 0;
  out[2] = esvo::scan_tiles(n);
  out[3] = esvo::scan_scratch_elems(n);
  return ESVO_OK;
}

// launch_exclusive_scan_u32.  out (in/out, n words): what the device's output buffer holds before and after; in_place != 0: the
// kernel reads and writes ONE buffer (d_out == d_in) that starts as `in`.  total: nullable, in/out, 1 word.
int esvo_debug_scan_u32(const uint32_t* in, size_t n, uint32_t* out, int in_place, uint32_t* total) {
  if ((n && (!in || !out))) return ESVO_ERR_INVALID_ARG;
  DEV_BEGIN();
  GBuf d_in, d_out, d_total, d_tmp;
  if (!in_place) HIPCHK(d_in.make(n * 4, in));
  HIPCHK(d_out.make(n * 4, in_place ? in : out));
  if (total) HIPCHK(d_total.make(4, total));
  HIPCHK(d_tmp.make(esvo::scan_scratch_elems(n) * 4, nullptr));
  esvo::launch_exclusive_scan_u32(in_place ? d_out.ptr<u32>() : d_in.ptr<u32>(), d_out.ptr<u32>(), total ? d_total.ptr<u32>() : nullptr,
                                  d_tmp.ptr<u32>(), n, st.s);
  DEV_RUN_DONE();
  if (!in_place) HIPCHK(d_in.finish(nullptr, &bad));
  HIPCHK(d_out.finish(out, &bad));
  if (total) HIPCHK(d_total.finish(total, &bad));
  HIPCHK(d_tmp.finish(nullptr, &bad));
  DEV_RETURN();
}

// launch_exclusive_scan_code_bit0 (tile_sums == NULL), or launch_scan_down_code_bit0 on the caller's tile sums (scan_tiles(n) words;
// n above the single-workgroup bound only, which is that launcher's contract).  zero: nullable, in/out, zero_words >= n words.
int esvo_debug_scan_code_bit0(const uint8_t* codes, size_t n, const uint32_t* tile_sums, uint32_t* out, uint32_t* total, uint32_t* zero,
                              size_t zero_words) {
  if ((n && (!codes || !out)) || (zero && zero_words < n)) return ESVO_ERR_INVALID_ARG;
  if (tile_sums && esvo::scan_is_small(n)) return ESVO_ERR_INVALID_ARG;
  DEV_BEGIN();
  GBuf d_in, d_out, d_total, d_tmp, d_zero;
  std::vector<uint8_t> padded((n + 3) / 4 * 4, 0xff);  // (the input buffer is never written: its size only has to hold the codes)
  if (n) std::memcpy(padded.data(), codes, n);
  HIPCHK(d_in.make(padded.size(), padded.data()));
  HIPCHK(d_out.make(n * 4, out));
  if (total) HIPCHK(d_total.make(4, total));
  std::vector<u32> tmp(esvo::scan_scratch_elems(n), GUARD_PATTERN);
  if (tile_sums) std::memcpy(tmp.data(), tile_sums, sizeof(u32) * esvo::scan_tiles(n));
  HIPCHK(d_tmp.make(tmp.size() * 4, tmp.data()));
  if (zero) HIPCHK(d_zero.make(zero_words * 4, zero));
  u32* const p_total = total ? d_total.ptr<u32>() : nullptr;
  u32* const p_zero = zero ? d_zero.ptr<u32>() : nullptr;
  if (tile_sums) esvo::launch_scan_down_code_bit0(d_in.ptr<uint8_t>(), d_out.ptr<u32>(), p_total, d_tmp.ptr<u32>(), n, p_zero, st.s);
  else esvo::launch_exclusive_scan_code_bit0(d_in.ptr<uint8_t>(), d_out.ptr<u32>(), p_total, d_tmp.ptr<u32>(), n, p_zero, st.s);
  DEV_RUN_DONE();
  HIPCHK(d_in.finish(nullptr, &bad));
  HIPCHK(d_out.finish(out, &bad));
  if (total) HIPCHK(d_total.finish(total, &bad));
  HIPCHK(d_tmp.finish(nullptr, &bad));
  if (zero) HIPCHK(d_zero.finish(zero, &bad));
  DEV_RETURN();
}

// launch_scan_compact_matches_small: flags (n words, 0 / 1), slots (n records); prefix (n words), total (1 word): in/out;
// out (n records) and slot_of (n words): nullable, in/out
int esvo_debug_compact_matches(const uint32_t* flags, size_t n, const esvo_match_t* slots, uint32_t* prefix, uint32_t* total,
                               esvo_match_t* out, uint32_t* slot_of) {
  if (!flags || !slots || !prefix || !total || !esvo::scan_compact_is_small(n)) return ESVO_ERR_INVALID_ARG;
  DEV_BEGIN();
  GBuf d_flags, d_slots, d_prefix, d_total, d_out, d_slot_of;
  HIPCHK(d_flags.make(n * 4, flags));
  HIPCHK(d_slots.make(n * sizeof(esvo_match_t), slots));
  HIPCHK(d_prefix.make(n * 4, prefix));
  HIPCHK(d_total.make(4, total));
  if (out) HIPCHK(d_out.make(n * sizeof(esvo_match_t), out));
  if (slot_of) HIPCHK(d_slot_of.make(n * 4, slot_of));
  esvo::launch_scan_compact_matches_small(d_flags.ptr<u32>(), d_prefix.ptr<u32>(), d_total.ptr<u32>(), n, d_slots.ptr<esvo_match_t>(),
                                          out ? d_out.ptr<esvo_match_t>() : nullptr, slot_of ? d_slot_of.ptr<u32>() : nullptr, st.s);
  DEV_RUN_DONE();
  HIPCHK(d_flags.finish(nullptr, &bad));
  HIPCHK(d_slots.finish(nullptr, &bad));
  HIPCHK(d_prefix.finish(prefix, &bad));
  HIPCHK(d_total.finish(total, &bad));
  if (out) HIPCHK(d_out.finish(out, &bad));
  if (slot_of) HIPCHK(d_slot_of.finish(slot_of, &bad));
  DEV_RETURN();
}

// launch_scan_compact_points_small.  row (in/out, row_n words; nullable): the device counter row -- the total is its word
// total_index, as in the tick (the row is the kernel's row_src); row == NULL: `total` (in/out, 1 word) stands alone.
// row_host (in/out, row_n words; nullable, needs row): the pinned host row the kernel writes the finished counter row to.
// out: nullable, in/out, n records.
int esvo_debug_compact_points(const uint32_t* flags, size_t n, const esvo_depth_point_t* slots, uint32_t* prefix, uint32_t* total,
                              esvo_depth_point_t* out, uint32_t* row, uint32_t row_n, uint32_t total_index, uint32_t* row_host) {
  if (!flags || !slots || !prefix || !esvo::scan_compact_is_small(n)) return ESVO_ERR_INVALID_ARG;
  if (row ? (total_index >= row_n || row_n > 1024u) : (!total || row_host)) return ESVO_ERR_INVALID_ARG;
  DEV_BEGIN();
  GBuf d_flags, d_slots, d_prefix, d_total, d_out, d_row_host;
  HIPCHK(d_flags.make(n * 4, flags));
  HIPCHK(d_slots.make(n * sizeof(esvo_depth_point_t), slots));
  HIPCHK(d_prefix.make(n * 4, prefix));
  HIPCHK(d_total.make(row ? row_n * 4 : 4, row ? row : total));
  if (out) HIPCHK(d_out.make(n * sizeof(esvo_depth_point_t), out));
  if (row_host) HIPCHK(d_row_host.make(row_n * 4, row_host, /*pin=*/true));
  esvo::launch_scan_compact_points_small(d_flags.ptr<u32>(), d_prefix.ptr<u32>(), d_total.ptr<u32>() + (row ? total_index : 0u), n,
                                         d_slots.ptr<esvo_depth_point_t>(), out ? d_out.ptr<esvo_depth_point_t>() : nullptr, st.s,
                                         row ? d_total.ptr<u32>() : nullptr, row_host ? d_row_host.ptr<u32>() : nullptr,
                                         row_host ? row_n : 0u);
  DEV_RUN_DONE();
  HIPCHK(d_flags.finish(nullptr, &bad));
  HIPCHK(d_slots.finish(nullptr, &bad));
  HIPCHK(d_prefix.finish(prefix, &bad));
  HIPCHK(d_total.finish(row ? row : total, &bad));
  if (out) HIPCHK(d_out.finish(out, &bad));
  if (row_host) HIPCHK(d_row_host.finish(row_host, &bad));
  DEV_RETURN();
}

// launch_lm_pixel_order (kernels_lm.hip): the processing order of a narrow LM launch bounded by max_matches whose compacted list
// holds the n records of `matches` (the count goes to the device, as in a tick); slot s holds match stride_item(s, n, num_threads).
// left / right: the width x height observation images (read by the SSD variant only).  order: in/out, max_matches words.
// *variant (nullable) receives lm_order_variant(): 0 the key is the pixel alone, 1 the patch-SSD octave lies above it.
int esvo_debug_lm_order(const esvo_match_t* matches, size_t n, size_t max_matches, int width, int height, int num_threads, int updown,
                        const uint8_t* left, const uint8_t* right, uint32_t* order, int* variant) {
  if (variant) *variant = esvo::lm_order_variant();
  if (!max_matches || n > max_matches || max_matches > 4000000u || (n && !matches) || !order || !left || !right) return ESVO_ERR_INVALID_ARG;
  if (width < 1 || height < 1 || (size_t)width * height > 4000000u || num_threads < 1) return ESVO_ERR_INVALID_ARG;
  DEV_BEGIN();
  GBuf d_m, d_n, d_l, d_r, d_rows[2], d_hist, d_tmp, d_order;
  const u32 n32 = (u32)n, cap = (u32)max_matches;
  const size_t npx = (size_t)width * height, img_bytes = (npx + 3) / 4 * 4;
  std::vector<uint8_t> img(img_bytes, 0);
  HIPCHK(d_m.make(std::max<size_t>(n, 1) * sizeof(esvo_match_t), nullptr));
  if (n) HIPCHK(hipMemcpy(d_m.ptr<void>(), matches, n * sizeof(esvo_match_t), hipMemcpyHostToDevice));
  HIPCHK(d_n.make(4, &n32));
  std::memcpy(img.data(), left, npx);
  HIPCHK(d_l.make(img_bytes, img.data()));
  std::memcpy(img.data(), right, npx);
  HIPCHK(d_r.make(img_bytes, img.data()));
  for (int k = 0; k < 2; ++k) HIPCHK(d_rows[k].make(max_matches * 8, nullptr));
  HIPCHK(d_hist.make(esvo::voxel_hist_words(max_matches) * 4, nullptr));
  HIPCHK(d_tmp.make(esvo::scan_scratch_elems(esvo::voxel_hist_words(max_matches)) * 4, nullptr));
  HIPCHK(d_order.make(max_matches * 4, order));
  esvo::DevParams dp;
  std::memset(&dp, 0, sizeof(dp));
  dp.W = width; dp.H = height; dp.num_threads = num_threads; dp.updown = updown;
  esvo::u64* const rows[2] = {d_rows[0].ptr<esvo::u64>(), d_rows[1].ptr<esvo::u64>()};
  esvo::launch_lm_pixel_order(d_m.ptr<esvo_match_t>(), d_n.ptr<u32>(), cap, 0, d_l.ptr<uint8_t>(), d_r.ptr<uint8_t>(), dp, rows,
                              d_hist.ptr<u32>(), d_tmp.ptr<u32>(), d_order.ptr<u32>(), st.s);
  DEV_RUN_DONE();
  HIPCHK(d_m.finish(nullptr, &bad));
  HIPCHK(d_n.finish(nullptr, &bad));
  HIPCHK(d_l.finish(nullptr, &bad));
  HIPCHK(d_r.finish(nullptr, &bad));
  for (int k = 0; k < 2; ++k) HIPCHK(d_rows[k].finish(nullptr, &bad));
  HIPCHK(d_hist.finish(nullptr, &bad));
  HIPCHK(d_tmp.finish(nullptr, &bad));
  HIPCHK(d_order.finish(order, &bad));
  DEV_RETURN();
}

// launch_upload_words: src (bytes, a multiple of 4) goes through a pinned buffer; dst: in/out, bytes; zero: nullable, in/out,
// zero_words words of which the launch clears the first n_zero (<= 256)
int esvo_debug_upload_words(const void* src, size_t bytes, void* dst, uint32_t* zero, uint32_t zero_words, uint32_t n_zero) {
  if (bytes % 4 || (bytes && (!src || !dst)) || n_zero > 256u || (zero ? n_zero > zero_words : n_zero != 0)) return ESVO_ERR_INVALID_ARG;
  DEV_BEGIN();
  GBuf h_src, d_dst, d_zero;
  HIPCHK(h_src.make(bytes, src, /*pin=*/true));
  HIPCHK(d_dst.make(bytes, dst));
  if (zero) HIPCHK(d_zero.make((size_t)zero_words * 4, zero));
  esvo::launch_upload_words(h_src.ptr<void>(), d_dst.ptr<void>(), bytes, st.s, zero ? d_zero.ptr<u32>() : nullptr, n_zero);
  DEV_RUN_DONE();
  HIPCHK(h_src.finish(nullptr, &bad));
  HIPCHK(d_dst.finish(dst, &bad));
  if (zero) HIPCHK(d_zero.finish(zero, &bad));
  DEV_RETURN();
}

// launch_back_prologue: three copies in one launch -- src (pinned, bytes: a multiple of 4) -> dst; a_src -> a_dst and b_src -> b_dst
// (multiples of 8 bytes).  Gather mode (a_flags != NULL): a_src holds a_slots depth-point records, a_flags / a_prefix a_slots words
// each, and a_dst (a_dst_bytes) receives the kept records in order with their position in `seq`.  dst, a_dst, b_dst: in/out.
int esvo_debug_back_prologue(const void* src, size_t bytes, void* dst, const void* a_src, size_t a_bytes, void* a_dst, size_t a_dst_bytes,
                             const void* b_src, size_t b_bytes, void* b_dst, const uint32_t* a_flags, const uint32_t* a_prefix,
                             uint32_t a_slots) {
  if (bytes % 4 || a_bytes % 8 || b_bytes % 8 || a_dst_bytes % 8) return ESVO_ERR_INVALID_ARG;
  if ((bytes && (!src || !dst)) || (a_bytes && !a_src) || (a_dst_bytes && !a_dst) || (b_bytes && (!b_src || !b_dst))) return ESVO_ERR_INVALID_ARG;
  if (a_flags ? (!a_prefix || a_bytes != (size_t)a_slots * sizeof(esvo_depth_point_t)) : (a_dst_bytes != a_bytes)) return ESVO_ERR_INVALID_ARG;
  if (a_flags) {  // the kernel trusts flags and prefix: a position outside a_dst is refused here
    for (u32 i = 0; i < a_slots; ++i)
      if (a_flags[i] && ((size_t)a_prefix[i] + 1) * sizeof(esvo_depth_point_t) > a_dst_bytes) return ESVO_ERR_INVALID_ARG;
  }
  DEV_BEGIN();
  GBuf h_src, d_dst, d_a_src, d_a_dst, d_b_src, d_b_dst, d_flags, d_prefix;
  HIPCHK(h_src.make(bytes, src, /*pin=*/true));
  HIPCHK(d_dst.make(bytes, dst));
  HIPCHK(d_a_src.make(a_bytes, a_src));
  HIPCHK(d_a_dst.make(a_dst_bytes, a_dst));
  HIPCHK(d_b_src.make(b_bytes, b_src));
  HIPCHK(d_b_dst.make(b_bytes, b_dst));
  if (a_flags) {
    HIPCHK(d_flags.make((size_t)a_slots * 4, a_flags));
    HIPCHK(d_prefix.make((size_t)a_slots * 4, a_prefix));
  }
  esvo::launch_back_prologue(h_src.ptr<void>(), d_dst.ptr<void>(), bytes, d_a_src.ptr<void>(), d_a_dst.ptr<void>(), a_bytes,
                             d_b_src.ptr<void>(), d_b_dst.ptr<void>(), b_bytes, st.s, a_flags ? d_flags.ptr<u32>() : nullptr,
                             a_flags ? d_prefix.ptr<u32>() : nullptr, a_flags ? a_slots : 0u);
  DEV_RUN_DONE();
  HIPCHK(h_src.finish(nullptr, &bad));
  HIPCHK(d_dst.finish(dst, &bad));
  HIPCHK(d_a_src.finish(nullptr, &bad));
  HIPCHK(d_a_dst.finish(a_dst, &bad));
  HIPCHK(d_b_src.finish(nullptr, &bad));
  HIPCHK(d_b_dst.finish(b_dst, &bad));
  if (a_flags) {
    HIPCHK(d_flags.finish(nullptr, &bad));
    HIPCHK(d_prefix.finish(nullptr, &bad));
  }
  DEV_RETURN();
}

// fdiv.hpp on n pairs: q_by = div_by(a, make_recip(b)); q_fast = div_fast(a, make_recip(b)) and q_refined = div_fast(a, {b,
// recip_refined(b)}) -- both computed on every pair, meaningful where fast[i] && ok_a[i] --; fast = make_recip(b).fast,
// ok_a = fdiv_ok(a) (one word each).  All outputs in/out.
int esvo_debug_fdiv(const double* a, const double* b, size_t n, double* q_by, double* q_fast, double* q_refined, uint32_t* fast,
                    uint32_t* ok_a) {
  if (n && (!a || !b || !q_by || !q_fast || !q_refined || !fast || !ok_a)) return ESVO_ERR_INVALID_ARG;
  DEV_BEGIN();
  GBuf d_a, d_b, d_by, d_fast_q, d_ref_q, d_fast, d_ok;
  HIPCHK(d_a.make(n * 8, a));
  HIPCHK(d_b.make(n * 8, b));
  HIPCHK(d_by.make(n * 8, q_by));
  HIPCHK(d_fast_q.make(n * 8, q_fast));
  HIPCHK(d_ref_q.make(n * 8, q_refined));
  HIPCHK(d_fast.make(n * 4, fast));
  HIPCHK(d_ok.make(n * 4, ok_a));
  if (n)
    hipLaunchKernelGGL(debug_fdiv_kernel, dim3(fdiv_blocks(n)), dim3(256), 0, st.s, d_a.ptr<double>(), d_b.ptr<double>(), n,
                       d_by.ptr<double>(), d_fast_q.ptr<double>(), d_ref_q.ptr<double>(), d_fast.ptr<u32>(), d_ok.ptr<u32>());
  DEV_RUN_DONE();
  HIPCHK(d_by.finish(q_by, &bad));
  HIPCHK(d_fast_q.finish(q_fast, &bad));
  HIPCHK(d_ref_q.finish(q_refined, &bad));
  HIPCHK(d_fast.finish(fast, &bad));
  HIPCHK(d_ok.finish(ok_a, &bad));
  DEV_RETURN();
}

// fdiv_ok_b4(b, a1, a2, a3, a4) -> ok (one word each) and the four div_fast quotients by make_recip(b) -> q[4 i + k] (computed on
// every tuple, meaningful where the window holds).  Outputs in/out.
int esvo_debug_fdiv_b4(const double* b, const double* a1, const double* a2, const double* a3, const double* a4, size_t n, uint32_t* ok,
                       double* q) {
  if (n && (!b || !a1 || !a2 || !a3 || !a4 || !ok || !q)) return ESVO_ERR_INVALID_ARG;
  DEV_BEGIN();
  GBuf d_in[5], d_ok, d_q;
  const double* in[5] = {b, a1, a2, a3, a4};
  for (int k = 0; k < 5; ++k) HIPCHK(d_in[k].make(n * 8, in[k]));
  HIPCHK(d_ok.make(n * 4, ok));
  HIPCHK(d_q.make(n * 32, q));
  if (n)
    hipLaunchKernelGGL(debug_fdiv_b4_kernel, dim3(fdiv_blocks(n)), dim3(256), 0, st.s, d_in[0].ptr<double>(), d_in[1].ptr<double>(),
                       d_in[2].ptr<double>(), d_in[3].ptr<double>(), d_in[4].ptr<double>(), n, d_ok.ptr<u32>(), d_q.ptr<double>());
  DEV_RUN_DONE();
  HIPCHK(d_ok.finish(ok, &bad));
  HIPCHK(d_q.finish(q, &bad));
  DEV_RETURN();
}

// the refined reciprocals themselves: y_make = make_recip(b).y, y_refined = recip_refined(b) (computed on every divisor, meaningful
// inside the window).  Through a quotient a missing refinement step hides behind div_fast's own correction; here it cannot.
int esvo_debug_recip(const double* b, size_t n, double* y_make, double* y_refined) {
  if (n && (!b || !y_make || !y_refined)) return ESVO_ERR_INVALID_ARG;
  DEV_BEGIN();
  GBuf d_b, d_m, d_r;
  HIPCHK(d_b.make(n * 8, b));
  HIPCHK(d_m.make(n * 8, y_make));
  HIPCHK(d_r.make(n * 8, y_refined));
  if (n)
    hipLaunchKernelGGL(debug_recip_kernel, dim3(fdiv_blocks(n)), dim3(256), 0, st.s, d_b.ptr<double>(), n, d_m.ptr<double>(),
                       d_r.ptr<double>());
  DEV_RUN_DONE();
  HIPCHK(d_m.finish(y_make, &bad));
  HIPCHK(d_r.finish(y_refined, &bad));
  DEV_RETURN();
}

// sqrt_moderate(x) on n operands (the caller keeps them inside the function's range); out: in/out
int esvo_debug_sqrt_moderate(const double* x, size_t n, double* out) {
  if (n && (!x || !out)) return ESVO_ERR_INVALID_ARG;
  DEV_BEGIN();
  GBuf d_x, d_out;
  HIPCHK(d_x.make(n * 8, x));
  HIPCHK(d_out.make(n * 8, out));
  if (n) hipLaunchKernelGGL(debug_sqrt_kernel, dim3(fdiv_blocks(n)), dim3(256), 0, st.s, d_x.ptr<double>(), n, d_out.ptr<double>());
  DEV_RUN_DONE();
  HIPCHK(d_out.finish(out, &bad));
  DEV_RETURN();
}

// The one entry here that takes a handle, and the one that launches nothing: the per-cell record counts tile_lists_kernel wrote
// at the handle's last fusion (d_cell_count, width x height words, row-major; cells outside the handle's band keep what an
// earlier fusion left there).  A pending tick is completed and the back stream drained first, as any read of the map does.
int esvo_debug_fuse_cell_counts(esvo_handle h, uint32_t* out, size_t n) {
  if (!h || !out) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (n != (size_t)h->W * (size_t)h->H) FAIL(ESVO_ERR_INVALID_ARG, "esvo_debug_fuse_cell_counts: width x height words are expected");
  HIPCHK(hipSetDevice(h->device));
  int rc = flush_pending_tick(h);
  if (rc) return rc;
  rc = drain_lm_and_back(h);
  if (rc) return rc;
  HIPCHK(hipMemcpy(out, h->d_cell_count, sizeof(u32) * n, hipMemcpyDeviceToHost));
  return ESVO_OK;
}

// Block matching once per distinct raw pixel (context.hpp, d_bm_dedupe): how many searches the newest shared launch ran -- the
// owner count, read where it lies on the device; *shared = 0 when the handle has never taken the path (then *n_owners = 0).
int esvo_debug_bm_owner_count(esvo_handle h, uint32_t* n_owners, int* shared) {
  if (!h || !n_owners || !shared) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  int rc = flush_pending_tick(h);
  if (rc) return rc;
  *n_owners = 0;
  *shared = h->d_bm_dedupe ? 1 : 0;
  if (!h->d_bm_dedupe) return ESVO_OK;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(n_owners, h->d_bm_dedupe + (size_t)h->W * h->H, sizeof(u32), hipMemcpyDeviceToHost));
  return ESVO_OK;
}

// The event ring of a camera as the ingest calls left it: the records of the absolute indices [first_abs, first_abs + n) (out, n
// records), the host's stamp mirror for them (stamps, n words) and ring_base / ring_next (bounds); each pointer may be NULL.  The
// range must lie inside [ring_base, ring_next).  Launches nothing; waits for the camera's pusher and drains the ingest stream first.
// (A render shows a staged stamp through a 30 ms decay rounded to u8: the nanoseconds are invisible there -- tests/test_gpu_event_columns.py.)
int esvo_debug_ts_ring(esvo_handle h, int cam, uint64_t first_abs, size_t n, esvo_event_t* out, uint64_t* stamps, uint64_t bounds[2]) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream_i));
  {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    const u64 base = h->ring_base[cam], next = h->ring_next[cam];
    if (bounds) { bounds[0] = base; bounds[1] = next; }
    if (n && (first_abs < base || first_abs > next || n > next - first_abs))
      FAIL(ESVO_ERR_INVALID_ARG, "esvo_debug_ts_ring: the range must lie inside [ring_base, ring_next)");
    if (stamps)
      for (size_t i = 0; i < n; ++i) stamps[i] = h->ts_host[cam][(size_t)(first_abs - base) + i];
  }
  if (out)
    for (const RingSpan& s : ring_spans(h->ring_cap, first_abs, n))
      HIPCHK(hipMemcpy(out + s.at, h->d_ring[cam] + s.slot, sizeof(esvo_event_t) * s.count, hipMemcpyDeviceToHost));
  return ESVO_OK;
}

// esvo_ts_push_evt3 decodes packets of fewer than n_words words on the host (0: every packet on the device).  The tests of the
// device decode's small shapes move the threshold; *previous (nullable) receives the old one.
int esvo_debug_evt3_device_min(esvo_handle h, size_t n_words, size_t* previous) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp0(h->mu_push[0]), lp1(h->mu_push[1]);
  if (previous) *previous = h->evt3_device_min;
  h->evt3_device_min = n_words;
  return ESVO_OK;
}

// The same for esvo_ts_push_evt2, in BYTES of words and for every EVT 2.x format at once; *previous (nullable) receives the old bound
// of EVT 2.0.
int esvo_debug_evt2_device_min(esvo_handle h, size_t n_bytes, size_t* previous) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp0(h->mu_push[0]), lp1(h->mu_push[1]);
  if (previous) *previous = h->evt2_device_min[0];
  h->evt2_device_min[0] = h->evt2_device_min[1] = n_bytes;
  return ESVO_OK;
}

// The ledger of devmem.hpp: live allocations and live bytes of every DevBuf / PinBuf of the process (tests/test_gpu_lifecycle.py
// asserts on its deltas around its own handles).  The guarded buffers above and esvo_ts_alloc_pinned are not in it.
void esvo_debug_live_allocations(size_t out[2]) {
  out[0] = esvo::g_live_allocs.load();
  out[1] = esvo::g_live_bytes.load();
}

// The owning type itself, a few hundred bytes at a time, each step checked against the ledger: returns 0, or the number of the
// first step whose pointer, capacity or ledger delta is not what devmem.hpp promises.  pinned: PinBuf instead of DevBuf.
int esvo_debug_devmem_selftest(int pinned) { return pinned ? devmem_selftest<true>() : devmem_selftest<false>(); }

}  // extern "C"
