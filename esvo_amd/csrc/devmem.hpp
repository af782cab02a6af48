// devmem.hpp — the one place that allocates and frees GPU and pinned host memory: DevBuf<T> / PinBuf<T>, and DevEvent.
//
// A buffer owns one pointer and its capacity in elements, frees it in its destructor and converts to T*, so launch sites read
// as with a raw pointer.  There is no growth policy in here: callers compute the capacities they ask for.  Two process-wide
// counters (live allocations, live bytes) move only where this type allocates and frees (esvo_debug_live_allocations).
#pragma once
#include <atomic>
#include <cstddef>
#include <hip/hip_runtime.h>

namespace esvo {

inline std::atomic<size_t> g_live_allocs{0}, g_live_bytes{0};  // (atomics: the ingest and tracker threads allocate as well)

template <typename T, bool Pinned>
class Buf {
  T* p_ = nullptr;
  size_t cap_ = 0;  // elements

 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {  // frees what this one held; the source ends empty
    if (this != &o) { (void)release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~Buf() { (void)release(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }  // (for a reinterpret_cast, which takes no conversion)
  T* operator->() const { return p_; }
  size_t cap() const { return cap_; }

  // frees now; an empty buffer stays empty (the buffer is empty afterwards even where the runtime reports an error)
  hipError_t release() {
    if (!p_) return hipSuccess;
    const hipError_t e = Pinned ? hipHostFree(p_) : hipFree(p_);
    g_live_allocs -= 1; g_live_bytes -= cap_ * sizeof(T);
    p_ = nullptr; cap_ = 0;
    return e;
  }
  // n elements, at least one; whatever the buffer held is freed first.  On failure the buffer is empty.
  hipError_t alloc(size_t n) {
    hipError_t e = release();
    if (e != hipSuccess) return e;
    if (!n) n = 1;
    void* q = nullptr;
    e = Pinned ? hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, n * sizeof(T));
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(q); cap_ = n;
    g_live_allocs += 1; g_live_bytes += n * sizeof(T);
    return hipSuccess;
  }
  // nothing when the capacity suffices; otherwise exactly n elements and the contents are gone
  hipError_t grow(size_t n) { return n <= cap_ ? hipSuccess : alloc(n); }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinBuf = Buf<T, true>;

// an event with one owner; one that was never created destroys to nothing
class DevEvent {
  hipEvent_t e_ = nullptr;

 public:
  DevEvent() = default;
  DevEvent(const DevEvent&) = delete;
  DevEvent& operator=(const DevEvent&) = delete;
  ~DevEvent() { if (e_) (void)hipEventDestroy(e_); }
  operator hipEvent_t() const { return e_; }
  hipError_t create(unsigned flags = hipEventDefault) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
};

// The stage events of one tick half, owned as a set and indexed by the set's own enum.  A set whose create() failed midway
// frees what it got with its owner, like any DevEvent.
template <int N> struct EventSet {
  DevEvent e[N];
  hipError_t create() { hipError_t r = hipSuccess; for (DevEvent& x : e) if (r == hipSuccess) r = x.create(); return r; }
};
enum { FE_T0, FE_BM0, FE_BM1, FE_S1, FE_LM0, FE_LM1, FE_S2, FE_CNT, FE_STG, FE_A1, FE_N };  // a front stage, in stream order up to FE_CNT
enum { BE_FU0, BE_FU1, BE_CL1, BE_RG1, BE_N };                                             // a back stage
enum { TE_SC0, TE_SC1, TE_R1, TE_N };                                                      // a camera's scatter and render
using FrontEvents = EventSet<FE_N>; using BackEvents = EventSet<BE_N>; using TsEvents = EventSet<TE_N>;

}  // namespace esvo
