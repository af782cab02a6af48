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

// an event with one owner (the evt[] table of the handle is not one: the communicator lends events into it)
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

}  // namespace esvo
