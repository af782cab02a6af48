// ring_spans.hpp — a range of absolute event indices as the contiguous pieces it occupies in an event ring.
#pragma once
#include <cstdint>

namespace esvo {

struct RingSpan {
  uint64_t slot, count;  // ring[slot, slot + count)
  uint64_t at;           // where the piece starts inside the range: the offset into a linear buffer beside the ring
};
struct RingSpans {
  RingSpan s[2];
  int n;
  constexpr const RingSpan* begin() const { return s; }
  constexpr const RingSpan* end() const { return s + n; }
};

// The absolute indices [first, first + count), count <= ring_cap, of a ring of ring_cap slots: no piece (count 0), one, or -- where
// the range passes the last slot -- two.  (A first slot will do for `first`: only first % ring_cap matters.)
constexpr RingSpans ring_spans(uint64_t ring_cap, uint64_t first, uint64_t count) {
  const uint64_t slot = first % ring_cap;
  const uint64_t head = count < ring_cap - slot ? count : ring_cap - slot;
  return RingSpans{{{slot, head, 0}, {0, count - head, head}}, count == 0 ? 0 : head == count ? 1 : 2};
}

namespace ring_spans_checks {
constexpr bool same(const RingSpan& a, uint64_t slot, uint64_t count, uint64_t at) { return a.slot == slot && a.count == count && a.at == at; }
static_assert(ring_spans(8, 5, 0).n == 0 && ring_spans(8, 16, 0).n == 0, "count 0: no piece");
static_assert(ring_spans(8, 13, 3).n == 1 && same(ring_spans(8, 13, 3).s[0], 5, 3, 0), "a range that ends at the last slot is one piece");
static_assert(ring_spans(8, 13, 4).n == 2 && same(ring_spans(8, 13, 4).s[0], 5, 3, 0) && same(ring_spans(8, 13, 4).s[1], 0, 1, 3),
              "one longer: the second piece holds one event");
static_assert(ring_spans(8, 16, 8).n == 1 && same(ring_spans(8, 16, 8).s[0], 0, 8, 0), "the whole ring from slot 0 is one piece");
static_assert(ring_spans(8, 19, 8).n == 2 && same(ring_spans(8, 19, 8).s[0], 3, 5, 0) && same(ring_spans(8, 19, 8).s[1], 0, 3, 5),
              "the whole ring from any other slot is two");
static_assert(ring_spans(8, 7, 1).n == 1 && same(ring_spans(8, 7, 1).s[0], 7, 1, 0) && ring_spans(8, 7, 2).s[1].count == 1, "the last slot alone");
}  // namespace ring_spans_checks

}  // namespace esvo
