// ingest.hpp — internal to api_ingest.hip (the bodies that are no templates), api_words.hip, api_filter.hip, api_survey.hip: what a packet source of the event ingest needs
#pragma once
#include "context.hpp"

namespace esvo_host {
inline u64 event_stamp(u32 sec, u32 nsec) { return (u64)sec * 1000000000ull + nsec; }
inline u64 event_stamp(const esvo_event_t& e) { return event_stamp(e.sec, e.nsec); }
// a record as the ring holds it: polarity 0 / 1 (bit 7 of the byte is the library's: EV_LATE, common.hpp), the padding zero
inline esvo_event_t event_normalised(esvo_event_t e) {
  e.polarity = e.polarity ? 1 : 0;
  e._pad[0] = e._pad[1] = e._pad[2] = 0;
  return e;
}
// the two refusals every path shares, each asked where its path always asked it; room: the ring must not overwrite events not yet scattered into the SAE (mu_ring held)
inline constexpr char RING_FULL[] = "event ring full: render (scatter) before staging more events";
inline constexpr char BLOCK_TOO_LARGE[] = "event block larger than the event ring";
inline bool ring_has_room(const esvo_context* h, int cam, size_t n) { return h->ring_next[cam] + n - h->scattered[cam] <= h->ring_cap; }
// ---- ingest protocol (INGEST group: may run on another thread than the renders and ticks of the same handle) ----------
// Staging runs on its own stream.  A pusher (one per camera at a time, mu_push) works in three steps:
//   begin   (mu_ring) order + capacity checks, then it RESERVES [ring_next, ring_next + n): from here on selections are
//           validated against ring_reserved, so no new kernel can be pointed at the slots about to be overwritten;
//   drain   the slots hold events older than ring_cap; kernels already enqueued read at most the max_ev events before the
//           last selection point and the not yet completed scatter ranges, so only a (nearly) full ring needs the front
//           stream drained -- done WITHOUT holding mu_ring;
//   copy + commit  host-to-device on the ingest stream (no lock), then (mu_ring) the stamps and ring_next are published.
struct PushTicket { u64 slot = 0, seq = 0; bool drain = false; };
int push_begin(esvo_context* h, int cam, size_t n, u64 t_first, PushTicket& tk);
void push_abort(esvo_context* h, int cam);
int push_drain(esvo_context* h, int cam, const PushTicket& tk);
// what ends every push (caller holds mu_ring): n more events staged, the reservation given back, the stamp mirror cut to ring_cap; returns the stamps dropped
inline size_t commit_tail(esvo_context* h, int cam, size_t n) {
  h->ring_next[cam] += n;
  h->ring_reserved[cam] = h->ring_next[cam];
  size_t evicted = 0;
  for (auto& tsq = h->ts_host[cam]; tsq.size() > h->ring_cap; ++evicted) { tsq.pop_front(); h->ring_base[cam]++; }
  h->stats.events_staged[cam] += n;
  return evicted;
}
// also_locked(evicted): what else has to change in the same critical section (routed band mode); evicted: stamps dropped from the mirror
struct StampArray { const u64* p; u64 operator()(size_t i) const { return p[i]; } };  // stamps that lie in an array: one insert into the mirror
inline void append_stamps(std::deque<u64>& q, size_t n, StampArray a) { q.insert(q.end(), a.p, a.p + n); }
template <typename StampFn> void append_stamps(std::deque<u64>& q, size_t n, StampFn stamp) { for (size_t i = 0; i < n; ++i) q.push_back(stamp(i)); }
// (n and the stamp functor BY VALUE, the functor holding one pointer: read through a reference to the source this loop cost records a sixth of the call)
template <typename StampFn, typename Also>
void push_commit(esvo_context* h, int cam, size_t n, StampFn stamp, bool copy_in_flight, Also also_locked) {
  std::lock_guard<std::mutex> lr(h->mu_ring);
  if (copy_in_flight) h->ingest_pending[cam] = true;
  append_stamps(h->ts_host[cam], n, stamp);
  also_locked(commit_tail(h, cam, n));
}
// a packet's stamps ascend (ties included); n >= 1, the functor by value as above
template <typename StampFn>
bool stamps_in_order(size_t n, StampFn stamp) {
  u64 last = stamp(0);
  for (size_t i = 1; i < n; ++i) { const u64 t = stamp(i); if (t < last) return false; last = t; }
  return true;
}
// a linear host array into the ring slots from `slot` on (ring: d_ring[cam] or the array beside it), on the ingest stream
template <typename T>
hipError_t copy_into_ring(esvo_context* h, T* ring, u64 slot, const T* src, size_t n) {
  for (const RingSpan& s : ring_spans(h->ring_cap, slot, n)) {
    const hipError_t e = hipMemcpyAsync(ring + s.slot, src + s.at, sizeof(T) * s.count, hipMemcpyHostToDevice, h->stream_i);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// The sequence itself (caller holds mu_push[cam]) for src.n events in order: src.stamp_fn(), a small functor i -> stamp; src.enqueue(ticket)
// puts the records into the reserved ring slots, on the ingest stream; src.in_flight: the copy stays in flight behind evt_ingest (the async
// call: the caller keeps the source alive until esvo_ts_push_wait, front-stream readers queue behind it, ingest_fence), else it is awaited.
template <typename Src, typename Also>
int push_staged(esvo_context* h, int cam, Src& src, Also also_locked) {
  if (src.n) {
    PushTicket tk;
    { int rc = push_begin(h, cam, src.n, src.stamp_fn()(0), tk); if (rc) return rc; }
    int rc = push_drain(h, cam, tk);
    if (!rc) rc = src.enqueue(tk);
    if (!rc) rc = [&]() -> int { HIPCHK(src.in_flight ? hipEventRecord(h->evt_ingest[cam], h->stream_i) : hipStreamSynchronize(h->stream_i)); return ESVO_OK; }();
    if (rc) { push_abort(h, cam); return rc; }  // (every failure behind begin gives the reservation back)
  }
  push_commit(h, cam, src.n, src.stamp_fn(), src.in_flight, also_locked);
  return ESVO_OK;
}
// ---- routed band mode (esvo_shard_set_routing): the packet is filtered on the host -----------------------------------------------
// Of the n events of a packet the rank keeps those its Time Surfaces need (raw row inside the camera's source rows) and, for the
// left camera, those it block-matches (floor(y_rect) inside the band): keep_px / sband_*.  Only they are copied to the device
// ring; each kept left event carries its index in the GLOBAL left sequence (d_ring_gidx), because the reference's event selection
// (esvo_Mapping.cpp:562-574) and its thread-stride order are defined on the whole stream -- whose stamps stay on the host
// (glob_ts).  Synchronous (the staging buffer is the library's): esvo_ts_push_events_async behaves like esvo_ts_push_events.
// Caller holds mu_push[cam]; the packet is sorted; get(i): its normalised records.
template <typename GetEv>
int push_routed(esvo_context* h, int cam, size_t n, GetEv get) {
  u64 g0 = 0;
  {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    if (h->last_stamp[cam] && event_stamp(get(0)) < h->last_stamp[cam])
      FAIL(ESVO_ERR_INVALID_ARG, "events must be sorted by time stamp (SURVEY Appendix A-1)");
    g0 = h->glob_base + h->glob_ts.size();
  }
  if (n > h->route_cap[cam]) {  // (idle: every routed push ends with a wait for its copies)
    const size_t cap = std::max<size_t>(n, (size_t)1 << 16);
    (void)h->h_route_ev[cam].release(); h->route_cap[cam] = 0;
    if (cam == 0) (void)h->h_route_gidx.release();
    HIPCHK(h->h_route_ev[cam].alloc(cap));
    if (cam == 0) HIPCHK(h->h_route_gidx.alloc(cap));
    h->route_cap[cam] = cap;
  }
  esvo_event_t* kept = h->h_route_ev[cam];
  std::vector<u64> kept_ts, kept_gl, all_ts;
  std::vector<uint8_t> kept_own;
  kept_ts.reserve(n / 2 + 16);
  if (cam == 0) { kept_gl.reserve(n / 2 + 16); all_ts.resize(n); }
  size_t m = 0;
  const int W = h->W, H = h->H, sy0 = h->sband_y0[cam], sy1 = h->sband_y1[cam];
  const uint8_t* keep_px = h->keep_px.data();
  u64 last = 0;
  for (size_t i = 0; i < n; ++i) {
    const esvo_event_t e = get(i);
    const u64 t = event_stamp(e);
    last = t;
    if (cam == 0) all_ts[i] = t;
    bool keep = false;
    if ((int)e.x < W && (int)e.y < H) keep = cam == 0 ? keep_px[(size_t)e.y * W + e.x] != 0 : ((int)e.y >= sy0 && (int)e.y < sy1);
    if (!keep) continue;
    kept[m] = e;
    if (cam == 0) { h->h_route_gidx[m] = (u32)(g0 + i); kept_gl.push_back(g0 + i); kept_own.push_back((keep_px[(size_t)e.y * W + e.x] >> 1) & 1); }
    kept_ts.push_back(t);
    ++m;
  }
  struct Kept {
    esvo_context* h; int cam; const esvo_event_t* ev; const u64* ts; size_t n; bool in_flight;
    StampArray stamp_fn() const { return {ts}; }
    int enqueue(const PushTicket& tk) {
      HIPCHK(copy_into_ring(h, h->d_ring[cam].get(), tk.slot, ev, n));
      if (cam == 0) HIPCHK(copy_into_ring(h, h->d_ring_gidx.get(), tk.slot, h->h_route_gidx.get(), n));
      return ESVO_OK;
    }
  } src{h, cam, kept, kept_ts.data(), m, false};
  return push_staged(h, cam, src, [&](size_t evicted) {
    h->last_stamp[cam] = last;
    if (cam != 0) return;
    for (size_t i = 0; i < m; ++i) { h->kept_g.push_back(kept_gl[i]); h->own_before.push_back(h->own_total); h->own_total += kept_own[i]; }
    for (size_t i = 0; i < evicted; ++i) { h->kept_g.pop_front(); h->own_before.pop_front(); }
    h->glob_ts.insert(h->glob_ts.end(), all_ts.begin(), all_ts.end());   // (one splice: the tick thread's selection takes this lock too)
    if (h->glob_ts.size() > h->ring_cap) {
      const size_t drop = h->glob_ts.size() - h->ring_cap;
      h->glob_ts.erase(h->glob_ts.begin(), h->glob_ts.begin() + (std::ptrdiff_t)drop);
      h->glob_base += drop;
    }
  });
}
// out-of-order input (api_ingest.hip): ev, the packet's n normalised records in arrival order.  Takes mu_api and mu_push[cam] itself.
int push_unsorted(esvo_context* h, int cam, size_t n, const esvo_event_t* ev);

// ---- the column staging block: `cap` events as columns in one allocation of 13 * cap bytes (d_col, the filter's twin): stamps, then x, y, polarity bytes ----
struct FilterPacket { const u64* d_t; const uint16_t *d_x, *d_y; const void* d_p; int p_type; size_t n; };
struct ColumnBlock {
  u64* t; uint16_t *x, *y; uint8_t* p; size_t cap;
  FilterPacket packet(size_t n) const { return {t, x, y, p, ESVO_P_U8, n}; }  // its first n events as a kernel reads them
};
inline ColumnBlock column_block(uint8_t* d, size_t cap) {
  return {reinterpret_cast<u64*>(d), reinterpret_cast<uint16_t*>(d + 8 * cap), reinterpret_cast<uint16_t*>(d + 10 * cap), d + 12 * cap, cap};
}
// n events of host columns into a block, on the ingest stream and not waited for (p null: that column is left alone)
int upload_columns(esvo_context* h, const ColumnBlock& b, const u64* stamps, const void* x, const void* y, const void* p, size_t n);
// the camera's column staging for n events (caller holds its mu_push; idle: every column push ends with a wait for the ingest stream)
int columns_staging(esvo_context* h, int cam, size_t n);
// [base, base + bytes) lies where its label says (host memory, or plain device memory of the handle's GPU), judged by its first and last byte; what: the refusal's subject
int require_memory_place(esvo_context* h, const void* base, size_t bytes, bool on_device, const std::string& what);

// ---- the event filter (esvo_ts_filter_configure; api_filter.hip) -------------------------------------------------------------------
// runs the camera's filter over a device-resident column packet on the ingest stream and waits: *kept events lie in the twin
// staging (twin: its columns as a packet), their stamps in *kept_stamps (pinned), the packet's counts in *counts.  Caller holds
// mu_push[cam]; nothing of the handle's state has changed until filter_commit.
// newest: the newest staged stamp; *unsorted: the packet is not in order behind it; *first_bad: its first invalid stamp (0xffffffff: none)
// *burst_dropped: the events the burst stage dropped (esvo_ts_burst_configure; 0 while it is off): counts->events_in + *burst_dropped = in.n
int filter_run(esvo_context* h, int cam, const FilterPacket& in, u64 newest, FilterPacket* twin, const u64** kept_stamps, esvo_event_filter_counts_t* counts,
               u64* burst_dropped, bool* unsorted, u32* first_bad);
void filter_commit(esvo_context* h, int cam, const esvo_event_filter_counts_t& counts, u64 burst_dropped);
// api_survey.hip: the hook of push_filtered while a camera's survey is open; caller holds mu_push[cam]
int survey_admit(esvo_context* h, int cam, size_t n);  // ESVO_ERR_CAPACITY where n more events would take a counter beyond 2^32 - 1
// counts the packet on the ingest stream, behind the verdicts that accepted it; wait: nothing else of the push waits for the stream
int survey_count(esvo_context* h, int cam, const FilterPacket& in, bool wait);
void survey_commit(esvo_context* h, int cam, size_t n);
// count-only mode: the whole push.  check_stamps: the packet's stamps never reached the host; *first_bad: its first invalid one
// (0xffffffff: none, and the packet is counted)
int survey_count_only(esvo_context* h, int cam, const FilterPacket& in, bool check_stamps, u32* first_bad);
// With a filter on, every source becomes a device-resident column packet (src.columns(): the camera's column staging, or device
// columns where they lie), the filter leaves the kept events in its twin staging and their stamps on the host, and the twin is
// packed into the ring as a column packet is.  Order and ring room are judged first, on the unfiltered packet; the filter's state
// changes only behind a push that succeeded.  Caller holds mu_push[cam].
struct KeptPacket {
  static constexpr bool in_flight = false;
  esvo_context* h; int cam; FilterPacket k; const u64* stamps; size_t n;
  StampArray stamp_fn() const { return {stamps}; }
  int enqueue(const PushTicket& tk) {
    launch_ts_pack_columns(k.d_x, k.d_y, k.d_t, k.d_p, k.p_type, n, h->d_ring[cam], tk.slot, h->ring_cap, h->stream_i);
    HIPCHK(hipGetLastError());
    return ESVO_OK;
  }
};
template <typename Src>
int push_filtered(esvo_context* h, int cam, Src& src) {
  const char* const out_of_order = "event filter: out-of-order packet (not sorted by time stamp, or older than the newest staged event)";
  const bool host_stamps = src.stamps_on_host();  // (else the filter's last kernel looks at stamps and order: they never come down)
  const bool survey = h->srv[cam].on;  // (esvo_ts_survey_begin; api_survey.hip)
  if (survey) {
    { int rc = survey_admit(h, cam, src.n); if (rc) return rc; }
    if (h->srv[cam].count_only) {  // the packet is decoded and counted: nothing is staged, no order and no ring room is asked for
      FilterPacket raw{};
      { int rc = src.columns(raw); if (rc) return rc; }
      u32 bad = 0xffffffffu;
      { int rc = survey_count_only(h, cam, raw, !src.stamps_on_host(), &bad); if (rc) return rc; }
      if (bad != 0xffffffffu) FAIL(ESVO_ERR_INVALID_ARG, src.bad_stamp_message(bad));
      return ESVO_OK;
    }
  }
  u64 newest = 0;
  {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    newest = h->ts_host[cam].empty() ? 0 : h->ts_host[cam].back();
    if (!ring_has_room(h, cam, src.n)) FAIL(ESVO_ERR_CAPACITY, RING_FULL);  // on the UNFILTERED count: a refusal must come before the filter's state moves
  }
  if (host_stamps && (!src.sorted() || src.stamp_fn()(0) < newest)) FAIL(ESVO_ERR_UNSUPPORTED, out_of_order);
  FilterPacket in{}, twin{};
  { int rc = src.columns(in); if (rc) return rc; }
  const u64* kept_stamps = nullptr;
  esvo_event_filter_counts_t counts{};
  bool unsorted = false;
  u32 first_bad = 0xffffffffu;
  u64 burst_dropped = 0;
  { int rc = filter_run(h, cam, in, newest, &twin, &kept_stamps, &counts, &burst_dropped, &unsorted, &first_bad); if (rc) return rc; }
  if (first_bad != 0xffffffffu) FAIL(ESVO_ERR_INVALID_ARG, src.bad_stamp_message(first_bad));
  if (unsorted) FAIL(ESVO_ERR_UNSUPPORTED, out_of_order);
  // the survey counts the raw packet behind the last refusal, on the stream the staging below waits for (it stages nothing: nobody waits)
  if (survey) { int rc = survey_count(h, cam, in, twin.n == 0); if (rc) return rc; }
  KeptPacket kept{h, cam, twin, kept_stamps, twin.n};
  { int rc = push_staged(h, cam, kept, [](size_t) {}); if (rc) return rc; }
  filter_commit(h, cam, counts, burst_dropped);
  if (survey) survey_commit(h, cam, src.n);
  return ESVO_OK;
}
// records on the host (get(i): normalised) split into columns by a plain loop and uploaded into the camera's column staging
template <typename GetEv>
int records_to_columns(esvo_context* h, int cam, size_t n, GetEv get, FilterPacket& out) {
  { int rc = columns_staging(h, cam, n); if (rc) return rc; }
  u64* const stamps = h->h_col_stamps[cam];
  std::vector<uint16_t> xy(2 * n);
  std::vector<uint8_t> p(n);
  for (size_t i = 0; i < n; ++i) {
    const esvo_event_t e = get(i);
    stamps[i] = event_stamp(e); xy[i] = e.x; xy[n + i] = e.y; p[i] = e.polarity;
  }
  const ColumnBlock b = column_block(h->d_col[cam], h->col_cap[cam]);
  { int rc = upload_columns(h, b, stamps, xy.data(), xy.data() + n, p.data(), n); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream_i));  // (pageable sources that end with this call)
  out = b.packet(n);
  return ESVO_OK;
}

// ---- one staging driver for every packet format --------------------------------------------------------------------------------
// A packet source supplies, beside what push_staged asks for,
//   sorted()       the packet is in order in itself
//   materialise()  makes record(i) valid: the normalised esvo_event_t, which only the paths that filter or sort on the host read; records():
//                  all of them as an array, for the sort alone (the routed path reads record(i): a record source is not copied for it)
//   prepare()      staging memory of its own, before anything is reserved
//   columns()      the packet as device-resident columns (the event filter's input); stamps_on_host(): false where they exist there only
// lp: mu_push[cam] where the source needed its staging for the stamps already; else it is taken here.
template <typename Derived>
struct PacketDefaults {
  static constexpr bool in_flight = false;
  bool sorted() const {  // (the column source answers from the walk that made its stamps: a second pass over a tick's stamps costs a tenth of the call)
    return stamps_in_order(static_cast<const Derived&>(*this).n, static_cast<const Derived&>(*this).stamp_fn());
  }
  int materialise() { return ESVO_OK; }
  std::vector<esvo_event_t> held;  // records() of a source that holds no such array itself
  const esvo_event_t* records() { auto& d = static_cast<Derived&>(*this); held.resize(d.n); for (size_t i = 0; i < d.n; ++i) held[i] = d.record(i); return held.data(); }
  int prepare() { return ESVO_OK; }
  bool stamps_on_host() const { return true; }  // stamp_fn() and sorted() can be asked (else the event filter decides on the device)
  std::string bad_stamp_message(size_t i) const { return "event " + std::to_string(i) + " has no valid time stamp"; }
};
template <typename Src>
int push_packet(esvo_context* h, int cam, Src& src, std::unique_lock<std::mutex> lp = {}) {
  const auto record = [&](size_t i) { return src.record(i); };
  if (h->flt[cam].on.load(std::memory_order_relaxed)) {  // the event filter (esvo_ts_filter_configure): every packet of the camera
    if (!lp.owns_lock()) {
      lp = std::unique_lock<std::mutex>(h->mu_push[cam]);
      HIPCHK(hipSetDevice(h->device));
    }
    if (h->flt[cam].on) return push_filtered(h, cam, src);
  }
  // sorted, and not older than what is staged: the fast path; anything else is sorted in as the reference's callbacks do
  bool in_order = src.sorted();
  if (in_order) {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    const u64 newest = h->routed ? h->last_stamp[cam] : (h->ts_host[cam].empty() ? 0 : h->ts_host[cam].back());
    in_order = src.stamp_fn()(0) >= newest;
  }
  if (!in_order) {
    { int rc = src.materialise(); if (rc) return rc; }
    if (lp.owns_lock()) lp.unlock();  // (push_unsorted takes mu_api before mu_push: the order esvo_reset takes them in)
    return push_unsorted(h, cam, src.n, src.records());
  }
  if (!lp.owns_lock()) {
    lp = std::unique_lock<std::mutex>(h->mu_push[cam]);
    HIPCHK(hipSetDevice(h->device));
  }
  if (h->routed) {
    { int rc = src.materialise(); if (rc) return rc; }
    return push_routed(h, cam, src.n, record);
  }
  { int rc = src.prepare(); if (rc) return rc; }
  return push_staged(h, cam, src, [](size_t) {});
}

struct RecordPacket : PacketDefaults<RecordPacket> {  // esvo_event_t records in host memory, copied as they are
  esvo_context* h; int cam; const esvo_event_t* ev; size_t n; bool in_flight;
  auto stamp_fn() const { return [ev = ev](size_t i) { return event_stamp(ev[i]); }; }
  esvo_event_t record(size_t i) const { return event_normalised(ev[i]); }
  int columns(FilterPacket& out) { return records_to_columns(h, cam, n, [this](size_t i) { return record(i); }, out); }
  int enqueue(const PushTicket& tk) {
    HIPCHK(copy_into_ring(h, h->d_ring[cam].get(), tk.slot, ev, n));
    return ESVO_OK;
  }
};

inline std::string columns_bad_element(size_t i) { return "event columns: element " + std::to_string(i) + " has no valid time stamp ((t + t_offset) * unit outside [0, 2^32 * 10^9))"; }
// the record of element i of host columns, its stamp known and valid
inline esvo_event_t columns_event(const void* x, const void* y, const void* p, int p_type, u64 stamp, size_t i) {
  const uint4 w = columns_record(static_cast<const uint16_t*>(x)[i], static_cast<const uint16_t*>(y)[i], stamp, columns_polarity(p, i, p_type));
  esvo_event_t e;
  std::memcpy(&e, &w, sizeof(w));
  return e;
}
// Columns whose valid stamps lie in h_col_stamps: host columns go to the device as they are, beside their stamps (d_col), device
// columns are read where they lie; a kernel packs the records into the ring.
struct ColumnsPacket : PacketDefaults<ColumnsPacket> {
  esvo_context* h; int cam; const esvo_event_columns_t* c; size_t n; const u64* stamps; bool in_itself;
  bool sorted() const { return in_itself; }
  std::vector<esvo_event_t>* E;  // the slow paths take records: what esvo_ts_push_events does with them, nothing of it twice
  bool host_stamps = true;       // false: a device-resident packet under the event filter, whose stamps stay on the device
  bool stamps_on_host() const { return host_stamps; }
  std::string bad_stamp_message(size_t i) const { return columns_bad_element(i); }
  StampArray stamp_fn() const { return {stamps}; }
  esvo_event_t record(size_t i) const { return (*E)[i]; }
  const esvo_event_t* records() const { return E->data(); }
  int materialise() {
    const void *x = c->x, *y = c->y, *p = c->p;
    std::vector<uint16_t> hx, hy;
    std::vector<uint8_t> hp;
    if (c->memory == ESVO_MEM_DEVICE) {  // down first
      hx.resize(n); hy.resize(n); hp.resize(c->p ? n : 0);
      HIPCHK(hipMemcpyAsync(hx.data(), c->x, 2 * n, hipMemcpyDeviceToHost, h->stream_i));
      HIPCHK(hipMemcpyAsync(hy.data(), c->y, 2 * n, hipMemcpyDeviceToHost, h->stream_i));
      if (c->p) HIPCHK(hipMemcpyAsync(hp.data(), c->p, n, hipMemcpyDeviceToHost, h->stream_i));
      HIPCHK(hipStreamSynchronize(h->stream_i));
      x = hx.data(); y = hy.data(); p = c->p ? hp.data() : nullptr;
    }
    E->resize(n);
    for (size_t i = 0; i < n; ++i) (*E)[i] = columns_event(x, y, p, c->p_type, stamps[i], i);
    return ESVO_OK;
  }
  int columns(FilterPacket& out) {
    const ColumnBlock b = column_block(h->d_col[cam], h->col_cap[cam]);
    out = FilterPacket{b.t, static_cast<const uint16_t*>(c->x), static_cast<const uint16_t*>(c->y), c->p, c->p_type, n};
    if (c->memory == ESVO_MEM_HOST) {
      { int rc = upload_columns(h, b, stamps, c->x, c->y, c->p, n); if (rc) return rc; }
      out.d_x = b.x; out.d_y = b.y; out.d_p = c->p ? b.p : nullptr;
    }
    return ESVO_OK;
  }
  int enqueue(const PushTicket& tk) {
    FilterPacket k{};
    { int rc = columns(k); if (rc) return rc; }
    launch_ts_pack_columns(k.d_x, k.d_y, k.d_t, k.d_p, k.p_type, n, h->d_ring[cam], tk.slot, h->ring_cap, h->stream_i);
    HIPCHK(hipGetLastError());
    return ESVO_OK;
  }
};
}  // namespace esvo_host
