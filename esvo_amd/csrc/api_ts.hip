// api_ts.hip — event ingest and Time-Surface render (see context.hpp).
#include "context.hpp"

namespace esvo_host {

// Time-Surface kernel timings of the last render of a camera (-1: both); the caller knows their events are complete
void collect_ts_timing(esvo_context* h, int only) {
  for (int cam = 0; cam < 2; ++cam) {
    if (!h->ts_timing_pending[cam] || (only >= 0 && cam != only)) continue;
    h->ts_timing_pending[cam] = false;
    const TsEvents& T = h->ts_ev[cam];
    float sc = 0, rd = 0;
    if (hipEventElapsedTime(&sc, T.e[TE_SC0], T.e[TE_SC1]) == hipSuccess &&
        hipEventElapsedTime(&rd, T.e[TE_SC1], T.e[TE_R1]) == hipSuccess) {
      h->stats.ms_ts_scatter = h->stats.ms_kernel[0] = sc;
      h->stats.ms_ts_render = h->stats.ms_kernel[1] = rd;
      h->stats.sum_ms_kernel[0] += sc;
      h->stats.sum_ms_kernel[1] += rd;
      h->stats.sum_ms_kernel[7] += (cam == 0 && h->ts_pair_sample) ? 2 : 1;
    }
    if (cam == 0) h->ts_pair_sample = false;
  }
}

// A copy enqueued by esvo_ts_push_events_async may still be in flight on the ingest stream: whatever the front stream launches
// next that reads the camera's ring (scatter, block matching, the SGM points) waits for it on the DEVICE.  Caller holds mu_ring.
void ingest_fence(esvo_context* h, int cam) {
  if (!h->ingest_pending[cam]) return;
  hipStreamWaitEvent(h->stream, h->evt_ingest[cam], 0);
  h->ingest_pending[cam] = false;
}

// ---- the scatter step (caller holds mu_ring) ---------------------------------------------------------------------------------------
// absolute index of the first staged event of `cam` with stamp >= t_ns: a render at t_ns takes the events below it (strict, TimeSurface.h:68)
static u64 first_staged_at(const esvo_context* h, int cam, u64 t_ns) {
  const auto& tsq = h->ts_host[cam];
  return h->ring_base[cam] + (u64)(std::lower_bound(tsq.begin(), tsq.end(), t_ns) - tsq.begin());
}
// The SAE keeps ONE stamp per pixel, the reference a queue of 20 (TimeSurface.h:28-96): rendering at a T that precedes events
// already scattered would read pixels as empty where getMostRecentEventBeforeT finds the older event.
static int refuse_decreasing_render(esvo_context* h, int cam, u64 upto, const char* who) {
  if (upto < h->scattered[cam])
    FAIL(ESVO_ERR_STATE, std::string(who) + ": t_ns precedes events of an earlier render (render times must not decrease; esvo_reset to replay)");
  return ESVO_OK;
}
// Kernels on the front stream are about to read the events [scattered, upto) of `cam`: what the pusher's eviction guard (push_begin)
// and the counters need to know of that.  Returns the range's first index (upto: there is nothing to do).
static u64 scatter_claim(esvo_context* h, int cam, u64 upto) {
  const u64 a = h->scattered[cam];
  if (upto <= a) return upto;
  h->scatter_pending_lo[cam] = std::min(h->scatter_pending_lo[cam], a);
  h->scatter_seq++;
  h->stats.events_scattered[cam] += upto - a;
  h->scattered[cam] = upto;
  return a;
}
// ... and each contiguous piece of the ring goes to sink(events, count).  (upto - scattered <= ring_cap: staging refuses more.)
template <typename Sink>
static void scatter_upto(esvo_context* h, int cam, u64 upto, Sink sink) {
  const u64 a = scatter_claim(h, cam, upto);
  for (const RingSpan& s : ring_spans(h->ring_cap, a, upto - a)) sink(h->d_ring[cam] + s.slot, (size_t)s.count);
}
// the sink of the renders that scatter both cameras with one launch: at most two pieces per camera, four segments per launch
struct ScatterSegs {
  esvo_context* h;
  TsScatterSegs g;
  int n_seg = 0;
  void flush() { launch_ts_scatter_segs(g, n_seg, h->W, h->H, h->stream); n_seg = 0; }  // (no segments: a no-op inside the launcher)
  void add(int cam, u64 upto) {
    scatter_upto(h, cam, upto, [&](const esvo_event_t* ev, size_t n) {
      g.ev[n_seg] = ev; g.n[n_seg] = n; g.sae[n_seg] = h->d_sae[cam];
      ++n_seg;
    });
  }
};

// Tick-interleaved multi-GPU operation (esvo_comm_tick on a tick another rank maps): every staged event with ts < t_ns that is
// not in the SAE yet is scattered NOW -- on the front stream, which is idle between this rank's block matching and its next
// own render, i.e. beside the own tick's LM launch -- so that the next own render finds only its own tick's events left to
// scatter.  Same bookkeeping as the scatter of a render; stream order keeps it behind the last render and before the next.
// (A side stream was tried first: it ended up in the hardware queue of the exchange stream, behind that stream's wait for the
//  LM launch, and the next own render behind it -- 1.66 instead of 1.3 ms per round.)
int ts_scatter_ahead(esvo_context* h, uint64_t t_ns) {
  if (h->tsq_len || h->routed) return ESVO_OK;  // (queue mode inserts and derives the SAE at render time)
  std::lock_guard<std::mutex> lr(h->mu_ring);
  ScatterSegs segs{h};
  for (int cam = 0; cam < 2; ++cam) {
    const u64 upto = first_staged_at(h, cam, (u64)t_ns);
    if (upto <= h->scattered[cam]) continue;
    ingest_fence(h, cam);
    segs.add(cam, upto);
  }
  if (!segs.n_seg) return ESVO_OK;
  segs.flush();
  HIPCHK(hipGetLastError());
  return ESVO_OK;
}

// The resident surface of `cam` is about to be overwritten on the front stream (caller holds mu_ts): a tracker thread's
// esvo_track_set_current may still be reading the left one on the tracker stream.
void resident_write_begin(esvo_context* h, int cam) {
  if (cam == 0 && h->trk_read_pending) {
    hipStreamWaitEvent(h->stream, h->evt_trk_read, 0);
    h->trk_read_pending = false;
  }
}

// Queue mode (max_event_queue_len > 0; caller holds mu_ring): every staged event of `cam` that is not in its pixel's queue yet
// goes in -- future ones included, as eventsCallback inserts them on arrival (TimeSurface.cpp:403-425) -- and the SAE word
// of every pixel is derived for THIS render time (getMostRecentEventBeforeT); the render kernels read the SAE as ever.
static TsQueueArgs queue_args(esvo_context* h, int cam) {
  TsQueueArgs g{};
  g.q = h->d_tsq[cam]; g.L = h->tsq_len;
  g.tcount = h->d_tsq_tcount; g.tlist = h->d_tsq_tlist; g.tcap = h->tsq_tcap;
  g.over = h->d_tsq_over; g.over_count = h->d_tsq_over_count; g.over_cap = (u32)esvo_context::TSQ_ROUND;
  return g;
}
void queue_prepare(esvo_context* h, int cam, u64 t_ns) {
  const u64 upto = h->ring_next[cam];
  for (u64 a = scatter_claim(h, cam, upto); a < upto; a += esvo_context::TSQ_ROUND) {  // rounds: the overflow list can hold a whole one
    TsQueueArgs g = queue_args(h, cam);
    int k = 0;
    for (const RingSpan& s : ring_spans(h->ring_cap, a, std::min<u64>(upto - a, esvo_context::TSQ_ROUND))) {
      g.ev[k] = h->d_ring[cam] + s.slot; g.n[k] = (size_t)s.count;
      ++k;
    }
    launch_tsq_insert(g, h->W, h->H, h->stream);
  }
  if (!h->tsq_dup[cam].empty()) {  // what eventsCallback inserted in place of late events: copies of the then-newest event (push_unsorted)
    auto& dup = h->tsq_dup[cam];
    if (dup.size() > h->d_tsq_dup.cap()) {
      hipStreamSynchronize(h->stream);
      (void)h->d_tsq_dup.alloc(std::max<size_t>(dup.size(), 4096));  // (on failure the buffer is empty: the copies are dropped below)
    }
    if (h->d_tsq_dup) {
      for (size_t a0 = 0; a0 < dup.size(); a0 += esvo_context::TSQ_ROUND) {
        const size_t cnt = std::min<size_t>(dup.size() - a0, esvo_context::TSQ_ROUND);
        hipMemcpyAsync(h->d_tsq_dup, dup.data() + a0, sizeof(esvo_event_t) * cnt, hipMemcpyHostToDevice, h->stream);
        hipStreamSynchronize(h->stream);  // (pageable source; the rare path)
        TsQueueArgs g = queue_args(h, cam);
        g.ev[0] = h->d_tsq_dup; g.n[0] = cnt;
        launch_tsq_insert(g, h->W, h->H, h->stream);
      }
    }
    dup.clear();
  }
  launch_tsq_view(h->d_tsq[cam], h->tsq_len, h->W, h->H, t_ns, h->d_sae[cam], h->stream);
}

// Both cameras' surfaces at t_ns with one launch per kernel (scatter segments, decay, median + remap): what two
// esvo_ts_render calls do, in four launches less.  obs_out[cam] (may be null) receives a second copy of the surface.
int ts_render_pair(esvo_context* h, uint64_t t_ns, uint8_t* const obs_out[2]) {
  // stage timings of a render that runs alone are sampled (context.hpp, lat_ticks): each event costs the queue ~5 us
  const bool timed = esvo_stage_timed(h);
  {
    std::lock_guard<std::mutex> lr(h->mu_ring);  // what a pusher on another thread reads and writes (context.hpp)
    ingest_fence(h, 0);
    ingest_fence(h, 1);
    u64 upto[2] = {0, 0};
    for (int cam = 0; cam < 2 && !h->tsq_len; ++cam) {
      upto[cam] = first_staged_at(h, cam, (u64)t_ns);
      { int rc = refuse_decreasing_render(h, cam, upto[cam], "esvo_ts_render"); if (rc) return rc; }
    }
    for (int cam = 0; cam < 2; ++cam)
      if (h->ts_timing_pending[cam] && hipEventQuery(h->ts_ev[cam].e[TE_R1]) == hipSuccess) collect_ts_timing(h, cam);
    if (timed) hipEventRecord(h->ts_ev[0].e[TE_SC0], h->stream);
    ScatterSegs segs{h};
    if (h->tsq_len) { queue_prepare(h, 0, (u64)t_ns); queue_prepare(h, 1, (u64)t_ns); }
    else { segs.add(0, upto[0]); segs.add(1, upto[1]); }
    segs.flush();  // (always: the timing events stand around it)
    if (timed) hipEventRecord(h->ts_ev[0].e[TE_SC1], h->stream);
  }
  TsPair c;
  for (int cam = 0; cam < 2; ++cam) {
    c.sae[cam] = h->d_sae[cam]; c.fixmap[cam] = h->d_fixmap[cam]; c.out[cam] = h->d_ts[cam];
    c.out2[cam] = obs_out ? obs_out[cam] : nullptr;
  }
  c.raw[0] = h->d_raw; c.raw[1] = h->d_raw1;
  {
    std::lock_guard<std::mutex> lt(h->mu_ts);
    resident_write_begin(h, 0);
    // (a routed band handle renders the rows of its band + halo only: h->rband_*, whole tiles)
    launch_ts_render_pair(c, h->W, h->H, (u64)t_ns, h->prm.decay_ms / 1000.0, h->prm.ignore_polarity, h->prm.median_blur_kernel_size,
                          h->stream, h->routed ? h->rband_y0 : 0, h->routed ? h->rband_y1 : -1);
    if (timed || h->trk_used.load()) hipEventRecord(h->ts_ev[0].e[TE_R1], h->stream);  // (also what esvo_track_set_current waits for)
    HIPCHK(hipGetLastError());
    h->ts_valid[0] = h->ts_valid[1] = true;
    for (int cam = 0; cam < 2; ++cam) { int rch = hist_store(h, cam, t_ns, h->d_ts[cam], false); if (rch) return rch; }  // (history off: nothing)
  }
  h->ts_timing_pending[0] = timed;
  h->ts_pair_sample = timed;
  h->stats.ts_frames[0]++;
  h->stats.ts_frames[1]++;
  return ESVO_OK;
}

}  // namespace esvo_host

// ---- Time Surface ---------------------------------------------------------------------------------
namespace {
u64 event_stamp(u32 sec, u32 nsec) { return (u64)sec * 1000000000ull + nsec; }
u64 event_stamp(const esvo_event_t& e) { return event_stamp(e.sec, e.nsec); }
// a record as the ring holds it: polarity 0 / 1 (bit 7 of the byte is the library's: EV_LATE, common.hpp), the padding zero
esvo_event_t event_normalised(esvo_event_t e) {
  e.polarity = e.polarity ? 1 : 0;
  e._pad[0] = e._pad[1] = e._pad[2] = 0;
  return e;
}
// ---- ingest protocol (INGEST group: may run on another thread than the renders and ticks of the same handle) ----------
// Staging runs on its own stream.  A pusher (one per camera at a time, mu_push) works in three steps:
//   begin   (mu_ring) order + capacity checks, then it RESERVES [ring_next, ring_next + n): from here on selections are
//           validated against ring_reserved, so no new kernel can be pointed at the slots about to be overwritten;
//   drain   the slots hold events older than ring_cap; kernels already enqueued read at most the max_ev events before the
//           last selection point and the not yet completed scatter ranges, so only a (nearly) full ring needs the front
//           stream drained -- done WITHOUT holding mu_ring;
//   copy + commit  host-to-device on the ingest stream (no lock), then (mu_ring) the stamps and ring_next are published.
struct PushTicket { u64 slot = 0, seq = 0; bool drain = false; };
int push_begin(esvo_context* h, int cam, size_t n, u64 t_first, PushTicket& tk) {
  std::lock_guard<std::mutex> lr(h->mu_ring);
  const auto& tsq = h->ts_host[cam];
  if (!tsq.empty() && t_first < tsq.back()) FAIL(ESVO_ERR_INVALID_ARG, "events must be sorted by time stamp (SURVEY Appendix A-1)");
  // the ring must not overwrite events that are not yet scattered into the SAE
  if (h->ring_next[cam] + n - h->scattered[cam] > h->ring_cap)
    FAIL(ESVO_ERR_CAPACITY, "event ring full: render (scatter) before staging more events");
  tk.slot = h->ring_next[cam] % h->ring_cap;
  h->ring_reserved[cam] = h->ring_next[cam] + n;
  if (h->ring_reserved[cam] > h->ring_cap) {
    const u64 evict_end = h->ring_reserved[cam] - h->ring_cap;  // first absolute index that survives
    u64 oldest_read = h->scatter_pending_lo[cam];               // scatter kernels enqueued since the last drain
    if (cam == 0) {  // the selections of the (up to) two ticks whose front stages may not have completed: each reads at most
                     // max_ev events up to its selection point
      const u64 sel_lo = std::min(h->sh_first, h->sh_first_prev);
      oldest_read = std::min(oldest_read, sel_lo > (u64)h->max_ev ? sel_lo - (u64)h->max_ev : 0);
    }
    oldest_read = std::min(oldest_read, h->em_guard_lo[cam]);  // an event-matching tick's gather (api_em.hip)
    tk.drain = evict_end > oldest_read;
    tk.seq = h->scatter_seq;
  }
  return ESVO_OK;
}
void push_abort(esvo_context* h, int cam) {
  std::lock_guard<std::mutex> lr(h->mu_ring);
  h->ring_reserved[cam] = h->ring_next[cam];
}
int push_drain(esvo_context* h, int cam, const PushTicket& tk) {
  if (!tk.drain) return ESVO_OK;
  if (hipStreamSynchronize(h->stream) != hipSuccess) FAIL(ESVO_ERR_HIP, "draining the front stream failed");
  std::lock_guard<std::mutex> lr(h->mu_ring);
  if (h->scatter_seq == tk.seq) h->scatter_pending_lo[0] = h->scatter_pending_lo[1] = ~0ull;  // nothing enqueued meanwhile
  return ESVO_OK;
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
  auto& tsq = h->ts_host[cam];
  append_stamps(tsq, n, stamp);
  h->ring_next[cam] += n;
  h->ring_reserved[cam] = h->ring_next[cam];
  size_t evicted = 0;
  for (; tsq.size() > h->ring_cap; ++evicted) { tsq.pop_front(); h->ring_base[cam]++; }
  h->stats.events_staged[cam] += n;
  also_locked(evicted);
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

// ---- out-of-order input ---------------------------------------------------------------------------------------------------
// The reference sorts on arrival: both nodes insertion-sort every event into their queue (TimeSurface.cpp:412-420,
// esvo_Mapping.cpp:692-702: `while (EQ[i].ts > e.ts)` -- strict, so equal stamps keep their arrival order: a STABLE sort).
//   mapper side   the ring holds the events in that sorted order; a packet that reaches back into already staged events is merged
//                 into the ring's tail on the device (ts_merge_kernel).  (esvo_Mapping::eventsCallback also RESETS the whole mapper
//                 when a message's FIRST stamp lies before its queue's newest, :678-687: that decision stays with the caller --
//                 stats.late_events tells it -- the library never throws a map away on its own.)
//   Time Surface  eventsCallback then inserts events_.back() -- the NEWEST event, not the one that just arrived (:421-422, SURVEY
//                 Appendix A-1).  For an event that is late on arrival (stamp < the newest stamp seen before it) that is a second
//                 copy of the newest event and the late event itself never enters the per-pixel queues: the late event is marked
//                 (EV_LATE, common.hpp) and skipped by the scatter; the second copy is a no-op for the one-stamp-per-pixel SAE and,
//                 in queue mode, is inserted with the next batch (tsq_dup).
// The rare path: it takes the mapper group's lock and drains the front stream before it moves anything.
template <typename GetEv>
int push_unsorted(esvo_context* h, int cam, size_t n, GetEv get) {
  std::lock_guard<std::recursive_mutex> la(h->mu_api);  // (before mu_push: the order esvo_reset takes them in)
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  if (h->routed) FAIL(ESVO_ERR_UNSUPPORTED, "out-of-order packets on a row-routed band handle: sort them first (or use ESVO_ROUTE_BROADCAST)");
  std::vector<esvo_event_t> S(n);
  std::vector<u64> t(n);
  std::vector<u32> order(n);
  u64 newest = 0;
  esvo_event_t newest_ev{};
  size_t K = 0, pos_rel = 0;
  // nothing enqueued may still read the ring's tail (block matching of a pending tick, a scatter) while it moves
  if (hipStreamSynchronize(h->stream) != hipSuccess || hipStreamSynchronize(h->stream_i) != hipSuccess) FAIL(ESVO_ERR_HIP, "draining the streams failed");
  u64 last_idx = 0;
  bool any = false, have_newest_ev = false;
  {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    if (!h->ts_host[cam].empty()) { newest = h->ts_host[cam].back(); last_idx = h->ring_next[cam] - 1; any = true; }
  }
  if (any && h->tsq_len) {  // queue mode: the record of the newest staged event (the ring's last: sorted), whose copies stand in for late events
    HIPCHK(hipMemcpy(&newest_ev, h->d_ring[cam] + last_idx % h->ring_cap, sizeof(esvo_event_t), hipMemcpyDeviceToHost));
    have_newest_ev = true;
  }
  // late on arrival: below the running maximum of everything that arrived before (a tie is NOT late: it becomes back())
  size_t n_late = 0;
  std::vector<esvo_event_t> dups;
  for (size_t i = 0; i < n; ++i) {
    esvo_event_t e = get(i);
    t[i] = event_stamp(e);
    order[i] = (u32)i;
    if (t[i] < newest) {
      e.polarity |= (uint8_t)EV_LATE;   // the library's mark: the byte and the padding magic together (common.hpp, ev_is_late)
      e._pad[0] = (uint8_t)(EV_LATE_PAD & 0xffu); e._pad[1] = (uint8_t)((EV_LATE_PAD >> 8) & 0xffu); e._pad[2] = (uint8_t)((EV_LATE_PAD >> 16) & 0xffu);
      ++n_late;
      if (h->tsq_len && have_newest_ev) dups.push_back(newest_ev);
    } else {
      newest = t[i];
      newest_ev = e;
      have_newest_ev = true;
    }
    S[i] = e;
  }
  std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return t[a] < t[b]; });
  std::vector<esvo_event_t> P(n);
  std::vector<u64> tp(n);
  for (size_t j = 0; j < n; ++j) { P[j] = S[order[j]]; tp[j] = t[order[j]]; }
  // the staged events the packet reaches back into: those with a stamp ABOVE the packet's smallest (equal ones arrived earlier: they stay in front)
  std::vector<u64> ts_tail;
  u64 pos_abs = 0, ring_next = 0;
  {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    const auto& tsq = h->ts_host[cam];
    pos_rel = std::upper_bound(tsq.begin(), tsq.end(), tp[0]) - tsq.begin();
    K = tsq.size() - pos_rel;
    pos_abs = h->ring_base[cam] + pos_rel;
    ring_next = h->ring_next[cam];
    if (h->ring_next[cam] + n - h->scattered[cam] > h->ring_cap) FAIL(ESVO_ERR_CAPACITY, "event ring full: render (scatter) before staging more events");
    if (K > ((size_t)1 << 22)) FAIL(ESVO_ERR_CAPACITY, "packet reaches back over more than 4 M staged events");
    // the merged tail (K staged + n new events) is written back into the ring: positions j and j + ring_cap would share a slot
    if (K + n > h->ring_cap)
      FAIL(ESVO_ERR_CAPACITY, "an out-of-order packet reaches back over more staged events than the event ring holds with it (a clock jump "
                              "or a looped bag: the reference resets its mapper here, esvo_Mapping.cpp:680-687 -- esvo_reset and re-stage)");
    ts_tail.assign(tsq.begin() + pos_rel, tsq.end());
    h->ring_reserved[cam] = ring_next + n;
  }
  const auto room = [](auto& buf, size_t need) {  // a scratch that is too small is replaced by one with half as much again
    return need <= buf.cap() || buf.alloc(std::max<size_t>(need + need / 2, 4096)) == hipSuccess;
  };
  if (!room(h->d_merge_a, K) || !room(h->d_merge_b, n) || !room(h->d_merge_plan, K + n)) {
    (void)hipGetLastError();
    push_abort(h, cam);
    FAIL(ESVO_ERR_CAPACITY, "out of device memory for the out-of-order merge");
  }
  // plan of the merged tail: staged first on equal stamps
  std::vector<u32> plan(K + n);
  std::vector<u64> merged(K + n);
  size_t a = 0, b = 0, n_before_scattered = 0;
  u64 scattered_rel = 0;
  {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    scattered_rel = h->scattered[cam] > pos_abs ? h->scattered[cam] - pos_abs : 0;  // staged events of the tail already in the SAE
  }
  for (size_t j = 0; j < K + n; ++j) {
    if (b >= n || (a < K && ts_tail[a] <= tp[b])) { plan[j] = (u32)a; merged[j] = ts_tail[a]; ++a; }
    else {
      plan[j] = 0x80000000u | (u32)b; merged[j] = tp[b];
      if (a < scattered_rel) ++n_before_scattered;  // lands among events that are scattered already: it is late (never scattered)
      ++b;
    }
  }
  hipError_t e = hipSuccess;
  const u64 slot0 = pos_abs % h->ring_cap;
  for (const RingSpan& s : ring_spans(h->ring_cap, pos_abs, K))  // a copy of the tail (it may wrap)
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_merge_a + s.at, h->d_ring[cam] + s.slot, sizeof(esvo_event_t) * s.count, hipMemcpyDeviceToDevice, h->stream_i);
  if (e == hipSuccess) e = hipMemcpyAsync(h->d_merge_b, P.data(), sizeof(esvo_event_t) * n, hipMemcpyHostToDevice, h->stream_i);
  if (e == hipSuccess) e = hipMemcpyAsync(h->d_merge_plan, plan.data(), sizeof(u32) * (K + n), hipMemcpyHostToDevice, h->stream_i);
  if (e == hipSuccess) {
    launch_ts_merge(h->d_merge_a, h->d_merge_b, h->d_merge_plan, K + n, h->d_ring[cam], slot0, h->ring_cap, h->stream_i);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream_i);
  if (e != hipSuccess) { push_abort(h, cam); FAIL(ESVO_ERR_HIP, std::string("out-of-order merge failed: ") + hipGetErrorString(e)); }
  std::lock_guard<std::mutex> lr(h->mu_ring);
  auto& tsq = h->ts_host[cam];
  tsq.erase(tsq.begin() + pos_rel, tsq.end());
  for (u64 v : merged) tsq.push_back(v);
  h->ring_next[cam] += n;
  h->ring_reserved[cam] = h->ring_next[cam];
  if (h->scattered[cam] > pos_abs) h->scattered[cam] += n_before_scattered;
  while (tsq.size() > h->ring_cap) { tsq.pop_front(); h->ring_base[cam]++; }
  h->stats.events_staged[cam] += n;
  h->stats.late_events[cam] += n_late;
  for (const esvo_event_t& d : dups) h->tsq_dup[cam].push_back(d);
  return ESVO_OK;
}

// ---- the event filter (esvo_ts_filter_configure; api_filter.hip) -------------------------------------------------------------------
// With a filter on, every source becomes a device-resident column packet (src.columns(): the camera's column staging, or device
// columns where they lie), the filter leaves the kept events in its twin staging and their stamps on the host, and the twin is
// packed into the ring as a column packet is.  Order and ring room are judged first, on the unfiltered packet; the filter's state
// changes only behind a push that succeeded.  Caller holds mu_push[cam].
int columns_staging(esvo_context* h, int cam, size_t n);
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
    if (h->ring_next[cam] + src.n - h->scattered[cam] > h->ring_cap)  // on the UNFILTERED count: a refusal must come before the filter's state moves
      FAIL(ESVO_ERR_CAPACITY, "event ring full: render (scatter) before staging more events");
  }
  if (host_stamps && (!src.sorted() || src.stamp_fn()(0) < newest)) FAIL(ESVO_ERR_UNSUPPORTED, out_of_order);
  FilterPacket in{}, twin{};
  { int rc = src.columns(in); if (rc) return rc; }
  const u64* kept_stamps = nullptr;
  esvo_event_filter_counts_t counts{};
  bool unsorted = false;
  u32 first_bad = 0xffffffffu;
  { int rc = filter_run(h, cam, in, newest, &twin, &kept_stamps, &counts, &unsorted, &first_bad); if (rc) return rc; }
  if (first_bad != 0xffffffffu) FAIL(ESVO_ERR_INVALID_ARG, src.bad_stamp_message(first_bad));
  if (unsorted) FAIL(ESVO_ERR_UNSUPPORTED, out_of_order);
  // the survey counts the raw packet behind the last refusal, on the stream the staging below waits for (it stages nothing: nobody waits)
  if (survey) { int rc = survey_count(h, cam, in, twin.n == 0); if (rc) return rc; }
  KeptPacket kept{h, cam, twin, kept_stamps, twin.n};
  { int rc = push_staged(h, cam, kept, [](size_t) {}); if (rc) return rc; }
  filter_commit(h, cam, counts);
  if (survey) survey_commit(h, cam, src.n);
  return ESVO_OK;
}
// records on the host (get(i): normalised) split into columns by a plain loop and uploaded into the camera's column staging
template <typename GetEv>
int records_to_columns(esvo_context* h, int cam, size_t n, GetEv get, FilterPacket& out) {
  { int rc = columns_staging(h, cam, n); if (rc) return rc; }
  const size_t cap = h->col_cap[cam];
  uint8_t* const d = h->d_col[cam];
  u64* const stamps = h->h_col_stamps[cam];
  std::vector<uint16_t> xy(2 * n);
  std::vector<uint8_t> p(n);
  for (size_t i = 0; i < n; ++i) {
    const esvo_event_t e = get(i);
    stamps[i] = event_stamp(e); xy[i] = e.x; xy[n + i] = e.y; p[i] = e.polarity;
  }
  HIPCHK(hipMemcpyAsync(d, stamps, sizeof(u64) * n, hipMemcpyHostToDevice, h->stream_i));
  HIPCHK(hipMemcpyAsync(d + 8 * cap, xy.data(), 2 * n, hipMemcpyHostToDevice, h->stream_i));
  HIPCHK(hipMemcpyAsync(d + 10 * cap, xy.data() + n, 2 * n, hipMemcpyHostToDevice, h->stream_i));
  HIPCHK(hipMemcpyAsync(d + 12 * cap, p.data(), n, hipMemcpyHostToDevice, h->stream_i));
  HIPCHK(hipStreamSynchronize(h->stream_i));  // (pageable sources that end with this call)
  out = FilterPacket{reinterpret_cast<const u64*>(d), reinterpret_cast<const uint16_t*>(d + 8 * cap), reinterpret_cast<const uint16_t*>(d + 10 * cap),
                     d + 12 * cap, ESVO_P_U8, n};
  return ESVO_OK;
}

// ---- one staging driver for every packet format --------------------------------------------------------------------------------
// A packet source supplies, beside what push_staged asks for,
//   sorted()       the packet is in order in itself
//   materialise()  makes record(i) valid: the normalised esvo_event_t, which only the paths that filter or sort on the host read
//   prepare()      staging memory of its own, before anything is reserved
//   columns()      the packet as device-resident columns (the event filter's input); stamps_on_host(): false where they exist there only
// lp: mu_push[cam] where the source needed its staging for the stamps already; else it is taken here.
template <typename Derived>
struct PacketDefaults {
  static constexpr bool in_flight = false;
  bool sorted() const {  // (the column source answers from the walk that made its stamps: a second pass over a tick's stamps costs a tenth of the call)
    const size_t n = static_cast<const Derived&>(*this).n;
    const auto stamp = static_cast<const Derived&>(*this).stamp_fn();
    bool in_order = true;
    u64 last = stamp(0);
    for (size_t i = 1; i < n && in_order; ++i) {
      const u64 t = stamp(i);
      in_order = t >= last;
      last = t;
    }
    return in_order;
  }
  int materialise() { return ESVO_OK; }
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
    return push_unsorted(h, cam, src.n, record);
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

u32 rd32(const uint8_t* p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }
// The 13-byte records of a dvs_msgs/EventArray {u16 x, u16 y, u32 sec, u32 nsec, u8 polarity}: they go to the device as they are and
// are widened to esvo_event_t in the ring by a kernel; the host only walks the time stamps (order check + selection index).
struct WirePacket : PacketDefaults<WirePacket> {
  esvo_context* h; int cam; const uint8_t* rec; size_t n;
  auto stamp_fn() const { return [rec = rec](size_t i) { return event_stamp(rd32(rec + i * 13 + 4), rd32(rec + i * 13 + 8)); }; }
  esvo_event_t record(size_t i) const {  // widened on the host
    const uint8_t* r = rec + i * 13;
    esvo_event_t e{};
    e.x = (uint16_t)(r[0] | (r[1] << 8));
    e.y = (uint16_t)(r[2] | (r[3] << 8));
    e.sec = rd32(r + 4);
    e.nsec = rd32(r + 8);
    e.polarity = r[12];
    return event_normalised(e);
  }
  int columns(FilterPacket& out) { return records_to_columns(h, cam, n, [this](size_t i) { return record(i); }, out); }
  int prepare() {
    if (n * 13 > h->d_wire[cam].cap())  // this camera's staging buffer: its pusher is the only user (mu_push)
      HIPCHK(h->d_wire[cam].alloc(std::max<size_t>(n * 13, (size_t)1 << 20)));
    return ESVO_OK;
  }
  int enqueue(const PushTicket& tk) {
    HIPCHK(hipMemcpyAsync(h->d_wire[cam], rec, n * 13, hipMemcpyHostToDevice, h->stream_i));
    launch_ts_unpack_wire(h->d_wire[cam], n, h->d_ring[cam], tk.slot, h->ring_cap, h->stream_i);
    HIPCHK(hipGetLastError());
    return ESVO_OK;
  }
};
}  // namespace

extern "C" {

static int push_events_impl(esvo_handle h, int cam, const esvo_event_t* ev, size_t n, bool wait) {
  if (!h || cam < 0 || cam > 1 || (n && !ev)) return ESVO_ERR_INVALID_ARG;
  if (n == 0) return ESVO_OK;
  if (n > h->ring_cap) FAIL(ESVO_ERR_CAPACITY, "event block larger than the event ring");
  RecordPacket src{{}, h, cam, ev, n, !wait};
  return push_packet(h, cam, src);
}
int esvo_ts_push_events(esvo_handle h, int cam, const esvo_event_t* ev, size_t n) { return push_events_impl(h, cam, ev, n, true); }
int esvo_ts_push_events_async(esvo_handle h, int cam, const esvo_event_t* ev, size_t n) { return push_events_impl(h, cam, ev, n, false); }
int esvo_ts_push_wait(esvo_handle h, int cam) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream_i));
  return ESVO_OK;
}
int esvo_host_alloc(size_t bytes, void** out) {
  esvo_context* h = nullptr;
  if (!out || !bytes) return ESVO_ERR_INVALID_ARG;
  HIPCHK(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return ESVO_OK;
}
int esvo_host_free(void* p) {
  esvo_context* h = nullptr;
  if (p) HIPCHK(hipHostFree(p));
  return ESVO_OK;
}
// A serialised dvs_msgs/EventArray (ROS1 wire format): std_msgs/Header {u32 seq, u32 sec, u32 nsec, string frame_id},
// u32 height, u32 width, Event[] {u32 count, count x 13 B}: the header is checked here, the records are the packet
// (WirePacket).
int esvo_ts_push_event_array(esvo_handle h, int cam, const uint8_t* msg, size_t n_bytes, size_t* n_events) {
  if (!h || cam < 0 || cam > 1 || !msg) return ESVO_ERR_INVALID_ARG;
  if (n_bytes < 16) FAIL(ESVO_ERR_INVALID_ARG, "EventArray message shorter than its header");
  const size_t id_len = rd32(msg + 12);
  size_t off = 16 + id_len;
  if (off < 16 || off + 12 > n_bytes) FAIL(ESVO_ERR_INVALID_ARG, "EventArray message truncated (frame_id / height / width / count)");
  const u32 height = rd32(msg + off), width = rd32(msg + off + 4), n = rd32(msg + off + 8);
  off += 12;
  if (n_events) *n_events = n;
  if ((size_t)n * 13 != n_bytes - off) FAIL(ESVO_ERR_INVALID_ARG, "EventArray message length does not match its event count");
  if ((height && (int)height != h->H) || (width && (int)width != h->W)) FAIL(ESVO_ERR_INVALID_ARG, "EventArray sensor size differs from the handle's");
  if (n == 0) return ESVO_OK;
  if (n > h->ring_cap) FAIL(ESVO_ERR_CAPACITY, "event block larger than the event ring");
  WirePacket src{{}, h, cam, msg + off, n};
  return push_packet(h, cam, src);
}

// ---- column ingest: x / y / t / p arrays in host or device memory (include/esvo_hip.h, esvo_ts_push_event_columns) ----------------
extern "C++" {
namespace {
size_t col_t_size(int t_type) { return t_type == ESVO_T_US_U32 ? 4 : 8; }
const char* columns_arg_error(const esvo_event_columns_t* c, size_t n) {
  if (c->t_type != ESVO_T_NS_I64 && c->t_type != ESVO_T_US_I64 && c->t_type != ESVO_T_US_U32) return "event columns: unknown t_type";
  if (c->p_type != ESVO_P_U8 && c->p_type != ESVO_P_I8) return "event columns: unknown p_type";
  if (c->memory != ESVO_MEM_HOST && c->memory != ESVO_MEM_DEVICE) return "event columns: unknown memory";
  if (n && (!c->x || !c->y || !c->t)) return "event columns: x, y and t must not be NULL";
  if ((uintptr_t)c->x % 2 || (uintptr_t)c->y % 2 || (uintptr_t)c->t % col_t_size(c->t_type))
    return "event columns: a column base is not aligned for its element type";
  return nullptr;
}
std::string columns_bad_element(size_t i) { return "event columns: element " + std::to_string(i) + " has no valid time stamp ((t + t_offset) * unit outside [0, 2^32 * 10^9))"; }
// the record of element i of host columns, its stamp known and valid
esvo_event_t columns_event(const void* x, const void* y, const void* p, int p_type, u64 stamp, size_t i) {
  const uint4 w = columns_record(static_cast<const uint16_t*>(x)[i], static_cast<const uint16_t*>(y)[i], stamp, columns_polarity(p, i, p_type));
  esvo_event_t e;
  std::memcpy(&e, &w, sizeof(w));
  return e;
}
// What the runtime knows of a pointer: 0 host memory (pageable, pinned or registered), 1 plain device memory of `device`,
// 2 anything else (managed memory, another GPU's).  Launches nothing, copies nothing.
int column_memory_kind(const void* p, int device) {
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return 0; }  // unknown to the runtime: pageable
  if (a.isManaged || a.type == hipMemoryTypeManaged) return 2;
  if (a.type == hipMemoryTypeUnregistered || a.type == hipMemoryTypeHost) return 0;
  return a.type == hipMemoryTypeDevice && a.device == device ? 1 : 2;
}
// the camera's column staging for n events (caller holds its mu_push; idle: every column push ends with a wait for the ingest stream)
int columns_staging(esvo_context* h, int cam, size_t n) {
  if (n <= h->col_cap[cam]) return ESVO_OK;
  const size_t cap = (std::max<size_t>(n + n / 2, 256) + 255) / 256 * 256;
  h->col_cap[cam] = 0;
  (void)h->d_col[cam].release(); (void)h->h_col_stamps[cam].release();
  HIPCHK(h->d_col[cam].alloc(cap * 13));
  HIPCHK(h->h_col_stamps[cam].alloc(cap));
  h->col_cap[cam] = cap;
  return ESVO_OK;
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
    const size_t cap = h->col_cap[cam];
    uint8_t* const d = h->d_col[cam];
    u64* const d_stamps = reinterpret_cast<u64*>(d);
    const uint16_t* kx = static_cast<const uint16_t*>(c->x);
    const uint16_t* ky = static_cast<const uint16_t*>(c->y);
    const void* kp = c->p;
    if (c->memory == ESVO_MEM_HOST) {
      HIPCHK(hipMemcpyAsync(d_stamps, stamps, sizeof(u64) * n, hipMemcpyHostToDevice, h->stream_i));
      HIPCHK(hipMemcpyAsync(d + 8 * cap, c->x, 2 * n, hipMemcpyHostToDevice, h->stream_i));
      HIPCHK(hipMemcpyAsync(d + 10 * cap, c->y, 2 * n, hipMemcpyHostToDevice, h->stream_i));
      if (c->p) HIPCHK(hipMemcpyAsync(d + 12 * cap, c->p, n, hipMemcpyHostToDevice, h->stream_i));
      kx = reinterpret_cast<const uint16_t*>(d + 8 * cap);
      ky = reinterpret_cast<const uint16_t*>(d + 10 * cap);
      if (c->p) kp = d + 12 * cap;
    }
    out = FilterPacket{d_stamps, kx, ky, kp, c->p_type, n};
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
}  // namespace
}  // extern "C++"

int esvo_event_columns_to_events(const esvo_event_columns_t* c, size_t n, esvo_event_t* out, size_t* first_bad) {
  esvo_context* h = nullptr;
  if (first_bad) *first_bad = n;
  if (!c || (n && !out)) return ESVO_ERR_INVALID_ARG;
  if (const char* msg = columns_arg_error(c, n)) FAIL(ESVO_ERR_INVALID_ARG, msg);
  if (c->memory != ESVO_MEM_HOST) FAIL(ESVO_ERR_INVALID_ARG, "esvo_event_columns_to_events: host memory only");
  for (size_t i = 0; i < n; ++i) {
    const u64 s = columns_stamp_ns(c->t, i, c->t_type, c->t_offset);
    if (s == COL_BAD_STAMP) {
      if (first_bad) *first_bad = i;
      FAIL(ESVO_ERR_INVALID_ARG, columns_bad_element(i));
    }
    out[i] = columns_event(c->x, c->y, c->p, c->p_type, s, i);
  }
  return ESVO_OK;
}
void esvo_event_columns_sizes(size_t out[4]) {
  out[0] = sizeof(esvo_event_columns_t);
  out[1] = out[2] = out[3] = 0;
}

int esvo_ts_push_event_columns(esvo_handle h, int cam, const esvo_event_columns_t* c, size_t n) {
  if (!h || cam < 0 || cam > 1 || !c) return ESVO_ERR_INVALID_ARG;
  if (n == 0) return ESVO_OK;
  if (const char* msg = columns_arg_error(c, n)) FAIL(ESVO_ERR_INVALID_ARG, msg);
  if (n > h->ring_cap) FAIL(ESVO_ERR_CAPACITY, "event block larger than the event ring");
  const bool on_device = c->memory == ESVO_MEM_DEVICE;
  std::unique_lock<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  {  // where the columns lie, first and last byte of each, before anything is launched or copied
    const void* base[4] = {c->x, c->y, c->t, c->p};
    const size_t bytes[4] = {2 * n, 2 * n, col_t_size(c->t_type) * n, n};
    for (int k = 0; k < 4; ++k) {
      if (!base[k]) continue;
      const int want = on_device ? 1 : 0;
      if (column_memory_kind(base[k], h->device) != want || column_memory_kind(static_cast<const uint8_t*>(base[k]) + bytes[k] - 1, h->device) != want)
        FAIL(ESVO_ERR_INVALID_ARG, on_device ? "event columns labelled ESVO_MEM_DEVICE must be plain device memory of the handle's GPU (not host, managed or another GPU's)"
                                             : "event columns labelled ESVO_MEM_HOST must be host memory (a device or managed pointer was given)");
    }
  }
  { int rc = columns_staging(h, cam, n); if (rc) return rc; }
  u64* const stamps = h->h_col_stamps[cam];
  if (on_device && h->flt[cam].on) {  // under the event filter validity and order are judged by its last kernel: the stamps stay on the device
    launch_ts_columns_stamps(c->t, c->t_type, c->t_offset, n, reinterpret_cast<u64*>(h->d_col[cam].get()), h->stream_i);
    HIPCHK(hipGetLastError());
    std::vector<esvo_event_t> none;
    ColumnsPacket judged{{}, h, cam, c, n, stamps, true, &none};
    judged.host_stamps = false;
    return push_packet(h, cam, judged, std::move(lp));
  }
  if (on_device) {  // t -> stamps on the device, down once
    u64* const d_stamps = reinterpret_cast<u64*>(h->d_col[cam].get());
    launch_ts_columns_stamps(c->t, c->t_type, c->t_offset, n, d_stamps, h->stream_i);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(stamps, d_stamps, sizeof(u64) * n, hipMemcpyDeviceToHost, h->stream_i));
    HIPCHK(hipStreamSynchronize(h->stream_i));
  }
  bool in_order = true;
  u64 last = 0;
  for (size_t i = 0; i < n; ++i) {  // the stamps (host columns: computed here), their validity, their order
    const u64 s = on_device ? stamps[i] : columns_stamp_ns(c->t, i, c->t_type, c->t_offset);
    if (s == COL_BAD_STAMP) FAIL(ESVO_ERR_INVALID_ARG, columns_bad_element(i));
    stamps[i] = s;
    in_order = in_order && s >= last;
    last = s;
  }
  std::vector<esvo_event_t> E;
  ColumnsPacket src{{}, h, cam, c, n, stamps, in_order, &E};
  return push_packet(h, cam, src, std::move(lp));
}

// ---- EVT 3.0 ingest: Prophesee's 16-bit word stream in host or device memory (include/esvo_hip.h, esvo_ts_push_evt3) -------------
extern "C++" {
namespace {
enum { EVT3_DEC_OK, EVT3_DEC_BAD_STAMP, EVT3_DEC_FULL };
// The word state machine as written in the header, every rule through common.hpp's functions.  emit(record) -> false: no room.
// c.events counts the events emitted so far: at EVT3_DEC_BAD_STAMP the index of the bad one.
template <class Emit>
int evt3_decode_host(esvo_evt3_state_t& s, const uint16_t* words, size_t n_words, int64_t t_offset_us, esvo_evt3_counts_t& c, Emit emit) {
  for (size_t i = 0; i < n_words; ++i) {
    const u32 w = words[i], t = evt3_type(w), m = evt3_mask(w);
    ++c.words;
    if (m) {
      if (!evt3_emits(w, s.flags)) c.dropped_events += (u64)__builtin_popcount(m);
      else {
        const u64 stamp = evt3_stamp_ns(evt3_t_us(s.loops, s.time_high, s.time_low), t_offset_us);
        if (stamp == COL_BAD_STAMP) return EVT3_DEC_BAD_STAMP;
        const u32 x0 = t == EVT3_ADDR_X ? (w & 0x7FFu) : (u32)s.base_x;
        const u32 pol = t == EVT3_ADDR_X ? ((w >> 11) & 1u) : ((s.flags & EVT3_VECT_POL) ? 1u : 0u);
        for (u32 mm = m; mm; mm &= mm - 1u) {
          const uint4 r = columns_record((uint16_t)((x0 + (u32)__builtin_ctz(mm)) & 0xFFFFu), s.y, stamp, pol);
          esvo_event_t e;
          std::memcpy(&e, &r, sizeof(r));
          if (!emit(e)) return EVT3_DEC_FULL;
          ++c.events;
        }
      }
    }
    switch (t) {
      case EVT3_ADDR_Y: s.y = (uint16_t)(w & 0x7FFu); s.flags |= EVT3_HAVE_Y; break;
      case EVT3_ADDR_X: break;
      case EVT3_VECT_BASE_X:
        s.base_x = (uint16_t)(w & 0x7FFu);
        s.flags = (s.flags & ~(u32)EVT3_VECT_POL) | (((w >> 11) & 1u) ? (u32)EVT3_VECT_POL : 0u) | EVT3_HAVE_BASE;
        break;
      case EVT3_VECT_12: case EVT3_VECT_8: s.base_x = (uint16_t)((s.base_x + evt3_base_advance(w)) & 0xFFFFu); break;
      case EVT3_TIME_LOW: s.time_low = (uint16_t)(w & 0xFFFu); break;
      case EVT3_TIME_HIGH:
        if (evt3_time_loop((s.flags & EVT3_HAVE_TH) != 0, s.time_high, w & 0xFFFu)) { ++s.loops; ++c.time_loops; }
        s.time_high = (uint16_t)(w & 0xFFFu); s.flags |= EVT3_HAVE_TH;
        break;
      case EVT3_EXT_TRIGGER: ++c.ext_triggers; break;
      default: ++c.ignored_words;
    }
  }
  return EVT3_DEC_OK;
}
// The same for EVT 2.0 / 2.1: every word through evt2_word as a 64-bit word of the EVT 2.1 layout.
template <class Emit>
int evt2_decode_host(esvo_evt2_state_t& s, const u32* words, size_t n_words, int format, int64_t t_offset_us, esvo_evt2_counts_t& c, Emit emit) {
  for (size_t i = 0; i < n_words; ++i) {
    const u64 W = evt2_word(words, i, format);
    const u32 t = evt2_type(W), m = evt2_mask(W);
    ++c.words;
    if (m) {
      if (!evt2_emits(s.flags)) c.dropped_events += (u64)__builtin_popcount(m);
      else {
        const u64 stamp = evt2_stamp_ns(s.loops, s.time_high, W, t_offset_us);
        if (stamp == COL_BAD_STAMP) return EVT3_DEC_BAD_STAMP;
        for (u32 mm = m; mm; mm &= mm - 1u) {
          const uint4 r = columns_record((uint16_t)((evt2_x0(W) + (u32)__builtin_ctz(mm)) & 0xFFFFu), (uint16_t)evt2_y(W), stamp, t);
          esvo_event_t e;
          std::memcpy(&e, &r, sizeof(r));
          if (!emit(e)) return EVT3_DEC_FULL;
          ++c.events;
        }
      }
    } else if (t == EVT2_TIME_HIGH) {
      const u32 v = evt2_time_high(W);
      if (evt2_time_loop(evt2_emits(s.flags), s.time_high, v)) { ++s.loops; ++c.time_loops; }
      s.time_high = v; s.flags |= EVT2_HAVE_TH;
    } else if (t == EVT2_EXT_TRIGGER) ++c.ext_triggers;
    else if (evt2_counts_as_ignored(t)) ++c.ignored_words;
  }
  return EVT3_DEC_OK;
}
std::string words_bad_event(const char* name, size_t i) {
  return std::string(name) + " words: event " + std::to_string(i) + " has no valid time stamp ((t_us + t_offset_us) * 1000 outside [0, 2^32 * 10^9))";
}
void evt3_add(esvo_evt3_counts_t& a, const esvo_evt3_counts_t& b) {
  a.words += b.words; a.events += b.events; a.dropped_events += b.dropped_events; a.ignored_words += b.ignored_words;
  a.ext_triggers += b.ext_triggers; a.time_loops += b.time_loops;
}
// What a word format gives the one push path below (push_words): its names and sizes, where the handle keeps its state, its host
// decoder, its device decode and the end state in the header the decode leaves.
struct Evt3Format {
  using State = esvo_evt3_state_t;
  const char* name() const { return "EVT3"; }
  size_t word_bytes() const { return 2; }
  size_t alignment() const { return 2; }
  const char* size_error() const { return "EVT3 words: an odd number of bytes"; }
  const char* alignment_error() const { return "EVT3 words: the base is not 2-byte aligned"; }
  State& state(esvo_context* h, int cam) const { return h->evt3_state[cam]; }
  esvo_evt3_counts_t& totals(esvo_context* h, int cam) const { return h->evt3_totals[cam]; }
  bool decoded_on_host(const esvo_context* h, size_t n_words) const { return n_words < h->evt3_device_min || n_words > EVT3_DEVICE_MAX_WORDS; }
  size_t events_guess(size_t n_words) const { return 2 * n_words; }
  template <class Emit>
  int decode_host(State& s, const void* w, size_t n_words, int64_t t_offset_us, esvo_evt3_counts_t& c, Emit emit) const {
    return evt3_decode_host(s, static_cast<const uint16_t*>(w), n_words, t_offset_us, c, emit);
  }
  size_t tiles(size_t n_words, const void* d_words) const { return evt3_tiles(n_words, d_words); }
  void launch(const void* d_words, size_t n_words, const State& st0, int64_t t_offset_us, u32* tiles, u32* hdr, uint8_t* d, size_t cap, hipStream_t s) const {
    launch_evt3_decode(static_cast<const uint16_t*>(d_words), n_words, st0, t_offset_us, tiles, hdr, reinterpret_cast<u64*>(d),
                       reinterpret_cast<uint16_t*>(d + 8 * cap), reinterpret_cast<uint16_t*>(d + 10 * cap), d + 12 * cap, cap, s);
  }
  void end_state(const u32* hdr, State& st1) const {
    st1.flags = hdr[EVT3_H_FLAGS]; st1.y = (uint16_t)(hdr[EVT3_H_Y_BASE] & 0xffffu); st1.base_x = (uint16_t)(hdr[EVT3_H_Y_BASE] >> 16);
    st1.time_high = (uint16_t)(hdr[EVT3_H_TIME] & 0xffffu); st1.time_low = (uint16_t)(hdr[EVT3_H_TIME] >> 16); st1.loops = hdr[EVT3_H_LOOPS_END];
  }
};
struct Evt2Format {
  using State = esvo_evt2_state_t;
  int format;  // ESVO_EVT_2_0, ESVO_EVT_2_1 or ESVO_EVT_2_1_LEGACY
  const char* name() const { return "EVT2"; }
  size_t word_bytes() const { return evt2_word_bytes(format); }
  size_t alignment() const { return 4; }
  const char* size_error() const { return format == ESVO_EVT_2_0 ? "EVT2 words: n_bytes is not a multiple of 4 (EVT 2.0)" : "EVT2 words: n_bytes is not a multiple of 8 (EVT 2.1)"; }
  const char* alignment_error() const { return "EVT2 words: the base is not 4-byte aligned"; }
  State& state(esvo_context* h, int cam) const { return h->evt2_state[cam]; }
  esvo_evt2_counts_t& totals(esvo_context* h, int cam) const { return h->evt2_totals[cam]; }
  bool decoded_on_host(const esvo_context* h, size_t n_words) const {
    return n_words * word_bytes() < h->evt2_device_min[format == ESVO_EVT_2_0 ? 0 : 1] || n_words > EVT2_DEVICE_MAX_WORDS;
  }
  size_t events_guess(size_t n_words) const { return format == ESVO_EVT_2_0 ? n_words : 2 * n_words; }
  template <class Emit>
  int decode_host(State& s, const void* w, size_t n_words, int64_t t_offset_us, esvo_evt2_counts_t& c, Emit emit) const {
    return evt2_decode_host(s, static_cast<const u32*>(w), n_words, format, t_offset_us, c, emit);
  }
  size_t tiles(size_t n_words, const void*) const { return evt2_tiles(n_words); }
  void launch(const void* d_words, size_t n_words, const State& st0, int64_t t_offset_us, u32* tiles, u32* hdr, uint8_t* d, size_t cap, hipStream_t s) const {
    launch_evt2_decode(static_cast<const u32*>(d_words), n_words, format, st0, t_offset_us, tiles, hdr, reinterpret_cast<u64*>(d),
                       reinterpret_cast<uint16_t*>(d + 8 * cap), reinterpret_cast<uint16_t*>(d + 10 * cap), d + 12 * cap, cap, s);
  }
  void end_state(const u32* hdr, State& st1) const { st1.flags = hdr[EVT3_H_FLAGS]; st1.time_high = hdr[EVT3_H_TIME]; st1.loops = hdr[EVT3_H_LOOPS_END]; }
};
// A packet the device decoded into the camera's column staging: a device-resident ColumnsPacket, whose slow paths take the records
// of the host decoder (the words come down first where they lie on the device).
template <class F>
struct WordsPacket : ColumnsPacket {
  F f; const void* words; size_t n_words; bool on_device; typename F::State st0; int64_t t_offset_us;
  int materialise() {
    esvo_context* const h = this->h;
    std::vector<u64> hw;  // (8-byte units: aligned for every word size)
    const void* w = words;
    if (on_device) {
      const size_t n_bytes = n_words * f.word_bytes();
      hw.resize((n_bytes + 7) / 8);
      HIPCHK(hipMemcpyAsync(hw.data(), words, n_bytes, hipMemcpyDeviceToHost, h->stream_i));
      HIPCHK(hipStreamSynchronize(h->stream_i));
      w = hw.data();
    }
    std::vector<esvo_event_t>* const E = this->E;
    E->clear(); E->reserve(this->n);
    typename F::State s = st0;
    esvo_evt3_counts_t c{};
    if (f.decode_host(s, w, n_words, t_offset_us, c, [&](const esvo_event_t& e) { E->push_back(e); return true; }) != EVT3_DEC_OK || E->size() != this->n)
      FAIL(ESVO_ERR_STATE, std::string(f.name()) + ": the host decode disagrees with the device decode");
    return ESVO_OK;
  }
};
// esvo_ts_push_evt3 / esvo_ts_push_evt2 behind their own argument checks
template <class F>
int push_words(esvo_handle h, int cam, const F& f, const void* words_v, size_t n_bytes, int memory, int64_t t_offset_us, size_t* n_events) {
  const std::string name = f.name();
  if (memory != ESVO_MEM_HOST && memory != ESVO_MEM_DEVICE) FAIL(ESVO_ERR_INVALID_ARG, name + " words: unknown memory");
  if (n_bytes % f.word_bytes()) FAIL(ESVO_ERR_INVALID_ARG, f.size_error());
  if (n_bytes && !words_v) FAIL(ESVO_ERR_INVALID_ARG, name + " words: NULL");
  if ((uintptr_t)words_v % f.alignment()) FAIL(ESVO_ERR_INVALID_ARG, f.alignment_error());
  const size_t n_words = n_bytes / f.word_bytes();
  if (n_words > 0x7fffffffull) FAIL(ESVO_ERR_INVALID_ARG, name + " words: more than 2^31 - 1 words in one call");
  if (n_words == 0) return ESVO_OK;
  const bool on_device = memory == ESVO_MEM_DEVICE;
  std::unique_lock<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  {  // where the words lie, first and last byte, before anything is launched or copied
    const int want = on_device ? 1 : 0;
    if (column_memory_kind(words_v, h->device) != want || column_memory_kind(static_cast<const uint8_t*>(words_v) + n_bytes - 1, h->device) != want)
      FAIL(ESVO_ERR_INVALID_ARG, name + (on_device ? " words labelled ESVO_MEM_DEVICE must be plain device memory of the handle's GPU (not host, managed or another GPU's)"
                                                   : " words labelled ESVO_MEM_HOST must be host memory (a device or managed pointer was given)"));
  }
  const typename F::State st0 = f.state(h, cam);
  typename F::State st1 = st0;
  esvo_evt3_counts_t cnt{};
  const auto commit = [&]() {  // (under mu_push[cam])
    f.state(h, cam) = st1;
    evt3_add(f.totals(h, cam), cnt);
    if (n_events) *n_events = (size_t)cnt.events;
  };
  int rc = ESVO_OK;
  if (h->routed || f.decoded_on_host(h, n_words)) {
    // decoded on the host: the record paths.  (Small packets: three launches and a read-back cost more than the walk.)
    std::vector<u64> hw;
    const void* w = words_v;
    if (on_device) {
      hw.resize((n_bytes + 7) / 8);
      HIPCHK(hipMemcpyAsync(hw.data(), words_v, n_bytes, hipMemcpyDeviceToHost, h->stream_i));
      HIPCHK(hipStreamSynchronize(h->stream_i));
      w = hw.data();
    }
    std::vector<esvo_event_t> E;
    const size_t room = (size_t)h->ring_cap;
    const int drc = f.decode_host(st1, w, n_words, t_offset_us, cnt, [&](const esvo_event_t& e) {
      if (E.size() >= room) return false;
      E.push_back(e);
      return true;
    });
    if (drc == EVT3_DEC_BAD_STAMP) FAIL(ESVO_ERR_INVALID_ARG, words_bad_event(f.name(), (size_t)cnt.events));
    if (drc == EVT3_DEC_FULL) FAIL(ESVO_ERR_CAPACITY, "event block larger than the event ring");
    if (E.empty()) { commit(); return ESVO_OK; }
    RecordPacket src{{}, h, cam, E.data(), E.size(), false};
    rc = push_packet(h, cam, src, std::move(lp));
  } else {
    const void* d_words = words_v;
    if (!on_device) {  // (d_evt3_words counts in 2-byte units whatever the word size)
      const size_t n_half = n_bytes / 2;
      if (n_half > h->d_evt3_words[cam].cap()) HIPCHK(h->d_evt3_words[cam].alloc(std::max<size_t>(n_half + n_half / 2, (size_t)1 << 16)));
      d_words = h->d_evt3_words[cam].get();
    }
    const size_t n_tiles = f.tiles(n_words, d_words);
    if (n_tiles * EVT3_TILE_WORDS > h->d_evt3_tiles[cam].cap()) HIPCHK(h->d_evt3_tiles[cam].alloc(std::max<size_t>(2 * n_tiles, 64) * EVT3_TILE_WORDS));
    if (!h->d_evt3_hdr[cam]) { HIPCHK(h->d_evt3_hdr[cam].alloc(EVT3_HDR_WORDS)); HIPCHK(h->h_evt3_hdr[cam].alloc(EVT3_HDR_WORDS)); }
    { int rcs = columns_staging(h, cam, std::min<size_t>(f.events_guess(n_words), (size_t)h->ring_cap)); if (rcs) return rcs; }  // (a guess: the header tells)
    u32* const hdr = h->h_evt3_hdr[cam];
    const auto decode = [&]() -> int {  // the three launches and the header's way down
      f.launch(d_words, n_words, st0, t_offset_us, h->d_evt3_tiles[cam], h->d_evt3_hdr[cam], h->d_col[cam], h->col_cap[cam], h->stream_i);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(hdr, h->d_evt3_hdr[cam], sizeof(u32) * EVT3_HDR_WORDS, hipMemcpyDeviceToHost, h->stream_i));
      HIPCHK(hipStreamSynchronize(h->stream_i));
      return ESVO_OK;
    };
    if (!on_device) HIPCHK(hipMemcpyAsync(h->d_evt3_words[cam], words_v, n_bytes, hipMemcpyHostToDevice, h->stream_i));
    { int rcd = decode(); if (rcd) return rcd; }
    const size_t n = hdr[EVT3_H_EVENTS];
    if (hdr[EVT3_H_FIRST_BAD] != 0xffffffffu) FAIL(ESVO_ERR_INVALID_ARG, words_bad_event(f.name(), hdr[EVT3_H_FIRST_BAD]));
    if (n > h->ring_cap) FAIL(ESVO_ERR_CAPACITY, "event block larger than the event ring");
    if (n > h->col_cap[cam]) {  // the guess was too small: once more into staging that holds them
      { int rcs = columns_staging(h, cam, n); if (rcs) return rcs; }
      { int rcd = decode(); if (rcd) return rcd; }
    }
    f.end_state(hdr, st1);
    cnt.words = n_words; cnt.events = n; cnt.dropped_events = hdr[EVT3_H_DROPPED]; cnt.ignored_words = hdr[EVT3_H_IGNORED];
    cnt.ext_triggers = hdr[EVT3_H_EXT]; cnt.time_loops = hdr[EVT3_H_LOOPS];
    if (n == 0) { commit(); return ESVO_OK; }
    const size_t cap = h->col_cap[cam];
    uint8_t* const d = h->d_col[cam];
    u64* const stamps = h->h_col_stamps[cam];
    const bool judged_on_device = h->flt[cam].on;  // under the event filter the order is judged by its last kernel: one read-back, the kept stamps
    bool in_order = true;
    if (!judged_on_device) {
      HIPCHK(hipMemcpyAsync(stamps, d, sizeof(u64) * n, hipMemcpyDeviceToHost, h->stream_i));
      HIPCHK(hipStreamSynchronize(h->stream_i));
      for (size_t i = 1; i < n && in_order; ++i) in_order = stamps[i] >= stamps[i - 1];
    }
    esvo_event_columns_t c{};
    c.x = d + 8 * cap; c.y = d + 10 * cap; c.p = d + 12 * cap; c.t = d;
    c.t_type = ESVO_T_NS_I64; c.p_type = ESVO_P_U8; c.memory = ESVO_MEM_DEVICE;
    std::vector<esvo_event_t> E;
    WordsPacket<F> src{{{}, h, cam, &c, n, stamps, in_order, &E}, f, words_v, n_words, on_device, st0, t_offset_us};
    src.host_stamps = !judged_on_device;
    rc = push_packet(h, cam, src, std::move(lp));
  }
  if (rc) return rc;
  std::lock_guard<std::mutex> lp2(h->mu_push[cam]);  // (push_packet gave the lock back)
  commit();
  return ESVO_OK;
}
// The header of a Prophesee .raw file: ASCII lines each starting with '%', ended by the first line that does not or by "% end".
// named(line, is_format_line) is called for every "% evt " and "% format " line, before the line's fields are read, and ends the
// walk with its code unless that is ESVO_OK.
template <class Named>
int raw_header_walk(const uint8_t* file, size_t n_bytes, size_t* data_offset, int* width, int* height, Named named) {
  if (data_offset) *data_offset = 0;
  if (width) *width = 0;
  if (height) *height = 0;
  if ((n_bytes && !file) || !data_offset) return ESVO_ERR_INVALID_ARG;
  const auto number_after = [](const std::string& line, const char* key) {  // the decimal number behind `key`, or 0
    const size_t at = line.find(key);
    return at == std::string::npos ? 0 : std::atoi(line.c_str() + at + std::strlen(key));
  };
  size_t off = 0;
  while (off < n_bytes && file[off] == '%') {
    size_t eol = off;
    while (eol < n_bytes && file[eol] != '\n') ++eol;
    std::string line(reinterpret_cast<const char*>(file) + off, eol - off);
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
    off = eol < n_bytes ? eol + 1 : n_bytes;
    if (line == "% end") break;
    if (line.rfind("% evt ", 0) == 0) { const int rc = named(line, false); if (rc) return rc; }
    if (line.rfind("% format ", 0) == 0) {
      { const int rc = named(line, true); if (rc) return rc; }
      if (width && number_after(line, "width=")) *width = number_after(line, "width=");
      if (height && number_after(line, "height=")) *height = number_after(line, "height=");
    }
    if (line.rfind("% geometry ", 0) == 0) {
      const size_t xat = line.find('x', 11);
      if (width) *width = std::atoi(line.c_str() + 11);
      if (height && xat != std::string::npos) *height = std::atoi(line.c_str() + xat + 1);
    }
  }
  *data_offset = off;
  return ESVO_OK;
}
int raw_unsupported(const std::string& msg) {
  esvo_context* h = nullptr;
  FAIL(ESVO_ERR_UNSUPPORTED, msg);
}
}  // namespace
}  // extern "C++"

int esvo_evt3_to_events(esvo_evt3_state_t* st, const uint16_t* words, size_t n_words, int64_t t_offset_us, esvo_event_t* out, size_t cap,
                        size_t* n_out, esvo_evt3_counts_t* counts) {
  esvo_context* h = nullptr;
  if (n_out) *n_out = 0;
  if (!st || (n_words && !words) || (uintptr_t)words % 2) return ESVO_ERR_INVALID_ARG;
  esvo_evt3_state_t s = *st;
  esvo_evt3_counts_t c{};
  const int rc = evt3_decode_host(s, words, n_words, t_offset_us, c, [&](const esvo_event_t& e) {
    if (!out) return true;
    if (c.events >= cap) return false;
    out[c.events] = e;
    return true;
  });
  if (n_out) *n_out = (size_t)c.events;
  if (rc == EVT3_DEC_BAD_STAMP) FAIL(ESVO_ERR_INVALID_ARG, words_bad_event("EVT3", (size_t)c.events));
  if (rc == EVT3_DEC_FULL) FAIL(ESVO_ERR_CAPACITY, "esvo_evt3_to_events: the words hold more events than `out` has room for");
  *st = s;
  if (counts) *counts = c;
  return ESVO_OK;
}
void esvo_evt3_sizes(size_t out[4]) {
  out[0] = sizeof(esvo_evt3_state_t); out[1] = sizeof(esvo_evt3_counts_t);
  out[2] = out[3] = 0;
}
int esvo_evt3_raw_header(const uint8_t* file, size_t n_bytes, size_t* data_offset, int* width, int* height) {
  return raw_header_walk(file, n_bytes, data_offset, width, height, [](const std::string& line, bool format_line) {
    if (!format_line && line.substr(6) != "3.0") return raw_unsupported("Prophesee .raw: '" + line + "' -- only EVT 3.0 is decoded");
    if (format_line && line.compare(9, 4, "EVT3") != 0) return raw_unsupported("Prophesee .raw: '" + line + "' -- only EVT3 is decoded");
    return (int)ESVO_OK;
  });
}
int esvo_raw_header(const uint8_t* file, size_t n_bytes, size_t* data_offset, int* width, int* height, int* format) {
  int named_format = 0;
  bool legacy = false;
  if (format) *format = 0;
  const int rc = raw_header_walk(file, n_bytes, data_offset, width, height, [&](const std::string& line, bool format_line) {
    std::string name = line.substr(format_line ? 9 : 6);
    if (format_line) {
      name = name.substr(0, name.find(';'));
      if (line.find("endianness=legacy") != std::string::npos) legacy = true;
    }
    if (name == (format_line ? "EVT2" : "2.0")) named_format = ESVO_EVT_2_0;
    else if (name == (format_line ? "EVT21" : "2.1")) named_format = ESVO_EVT_2_1;
    else if (name == (format_line ? "EVT3" : "3.0")) named_format = ESVO_EVT_3_0;
    else return raw_unsupported("Prophesee .raw: '" + line + "' -- EVT 2.0, EVT 2.1 and EVT 3.0 are decoded");
    return (int)ESVO_OK;
  });
  if (rc) return rc;
  if (format) *format = named_format == ESVO_EVT_2_1 && legacy ? (int)ESVO_EVT_2_1_LEGACY : named_format;
  return ESVO_OK;
}

int esvo_evt2_to_events(esvo_evt2_state_t* st, const void* words, size_t n_bytes, int format, int64_t t_offset_us, esvo_event_t* out, size_t cap,
                        size_t* n_out, esvo_evt2_counts_t* counts) {
  esvo_context* h = nullptr;
  if (n_out) *n_out = 0;
  if (!st || !evt2_format_known(format) || (n_bytes && !words) || (uintptr_t)words % 4 || n_bytes % evt2_word_bytes(format)) return ESVO_ERR_INVALID_ARG;
  esvo_evt2_state_t s = *st;
  esvo_evt2_counts_t c{};
  const int rc = evt2_decode_host(s, static_cast<const u32*>(words), n_bytes / evt2_word_bytes(format), format, t_offset_us, c, [&](const esvo_event_t& e) {
    if (!out) return true;
    if (c.events >= cap) return false;
    out[c.events] = e;
    return true;
  });
  if (n_out) *n_out = (size_t)c.events;
  if (rc == EVT3_DEC_BAD_STAMP) FAIL(ESVO_ERR_INVALID_ARG, words_bad_event("EVT2", (size_t)c.events));
  if (rc == EVT3_DEC_FULL) FAIL(ESVO_ERR_CAPACITY, "esvo_evt2_to_events: the words hold more events than `out` has room for");
  *st = s;
  if (counts) *counts = c;
  return ESVO_OK;
}
void esvo_evt2_sizes(size_t out[4]) {
  out[0] = sizeof(esvo_evt2_state_t); out[1] = sizeof(esvo_evt2_counts_t);
  out[2] = out[3] = 0;
}
int esvo_ts_evt2_state(esvo_handle h, int cam, esvo_evt2_state_t* get, const esvo_evt2_state_t* set) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  if (get) *get = h->evt2_state[cam];
  if (set) {
    esvo_evt2_state_t s = *set;
    s.flags &= 0x1u; s.time_high &= 0x0FFFFFFFu; s.reserved = 0;  // what a stream can leave
    h->evt2_state[cam] = s;
  }
  return ESVO_OK;
}
int esvo_ts_evt2_stats(esvo_handle h, int cam, esvo_evt2_counts_t* totals) {
  if (!h || cam < 0 || cam > 1 || !totals) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  *totals = h->evt2_totals[cam];
  return ESVO_OK;
}
int esvo_ts_push_evt2(esvo_handle h, int cam, const void* words, size_t n_bytes, int format, int memory, int64_t t_offset_us, size_t* n_events) {
  if (n_events) *n_events = 0;
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  if (!evt2_format_known(format)) FAIL(ESVO_ERR_INVALID_ARG, "EVT2 words: unknown format (ESVO_EVT_2_0, ESVO_EVT_2_1 or ESVO_EVT_2_1_LEGACY; EVT 3.0 words go to esvo_ts_push_evt3)");
  return push_words(h, cam, Evt2Format{format}, words, n_bytes, memory, t_offset_us, n_events);
}

int esvo_ts_evt3_state(esvo_handle h, int cam, esvo_evt3_state_t* get, const esvo_evt3_state_t* set) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  if (get) *get = h->evt3_state[cam];
  if (set) {
    esvo_evt3_state_t s = *set;
    s.flags &= 0xFu; s.y &= 0x7FFu; s.time_high &= 0xFFFu; s.time_low &= 0xFFFu; s.reserved = 0;  // what a stream can leave
    h->evt3_state[cam] = s;
  }
  return ESVO_OK;
}
int esvo_ts_evt3_stats(esvo_handle h, int cam, esvo_evt3_counts_t* totals) {
  if (!h || cam < 0 || cam > 1 || !totals) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  *totals = h->evt3_totals[cam];
  return ESVO_OK;
}

int esvo_ts_push_evt3(esvo_handle h, int cam, const void* words_v, size_t n_bytes, int memory, int64_t t_offset_us, size_t* n_events) {
  if (n_events) *n_events = 0;
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  return push_words(h, cam, Evt3Format{}, words_v, n_bytes, memory, t_offset_us, n_events);
}

namespace {
// FORWARD mode, first use for a camera: the contribution lists of TimeSurface.cpp:85-116.  A source pixel s with rectified
// position (u, v), u, v >= 0, u_i + 1 < W, v_i + 1 < H adds to the four pixels around (u, v); every destination pixel gets the
// list of (source, corner) pairs that reach it, in raster order of the sources (a stable counting sort).
int build_forward_lists(esvo_context* h, int cam) {
  if (h->d_fwd_off[cam]) return ESVO_OK;
  const std::vector<float>& lut = h->h_rect_lut[cam];
  const size_t npx = (size_t)h->W * h->H;
  if (lut.size() != 2 * npx) FAIL(ESVO_ERR_STATE, "esvo_ts_render_forward: this camera's rect_lut was not given to esvo_create");
  if (npx >= (1u << 30)) FAIL(ESVO_ERR_UNSUPPORTED, "image too large for the packed contribution records");
  const size_t W = (size_t)h->W, H = (size_t)h->H;
  std::vector<u32> off(npx + 1, 0);
  auto corners = [&](size_t s, size_t dst[4]) -> bool {
    const double u = (double)lut[2 * s], v = (double)lut[2 * s + 1];
    if (!(u >= 0 && v >= 0)) return false;
    const double fu = std::floor(u), fv = std::floor(v);
    if (!(fu < 4e9 && fv < 4e9)) return false;
    const size_t u_i = (size_t)fu, v_i = (size_t)fv;
    if (!(u_i + 1 < W && v_i + 1 < H)) return false;
    dst[0] = v_i * W + u_i; dst[1] = v_i * W + u_i + 1; dst[2] = (v_i + 1) * W + u_i; dst[3] = (v_i + 1) * W + u_i + 1;
    return true;
  };
  size_t dst[4];
  for (size_t s = 0; s < npx; ++s)
    if (corners(s, dst))
      for (int c = 0; c < 4; ++c) off[dst[c] + 1]++;
  for (size_t i = 0; i < npx; ++i) off[i + 1] += off[i];
  std::vector<u32> src(std::max<size_t>(off[npx], 1)), fill(off.begin(), off.end() - 1);
  for (size_t s = 0; s < npx; ++s)
    if (corners(s, dst))
      for (int c = 0; c < 4; ++c) src[fill[dst[c]]++] = (u32)s | ((u32)c << 30);
  HIPCHK(h->d_fwd_off[cam].alloc(npx + 1));
  HIPCHK(h->d_fwd_src[cam].alloc(src.size()));
  HIPCHK(h->d_fwd_lut[cam].alloc(npx));
  if (!h->d_fwd_val) HIPCHK(h->d_fwd_val.alloc(npx));
  HIPCHK(hipMemcpy(h->d_fwd_off[cam], off.data(), sizeof(u32) * (npx + 1), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_fwd_src[cam], src.data(), sizeof(u32) * src.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_fwd_lut[cam], lut.data(), sizeof(float2) * npx, hipMemcpyHostToDevice));
  return ESVO_OK;
}
}  // namespace

int esvo_ts_render_forward(esvo_handle h, int cam, uint64_t t_ns, uint8_t* out_mono8) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  if (h->routed) FAIL(ESVO_ERR_UNSUPPORTED, "FORWARD mode on a routed band handle (the splat needs every raw row): use ESVO_ROUTE_BROADCAST");
  { int rc = build_forward_lists(h, cam); if (rc) return rc; }
  {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    ingest_fence(h, cam);
    const u64 upto = first_staged_at(h, cam, (u64)t_ns);
    if (h->tsq_len) queue_prepare(h, cam, (u64)t_ns);
    else {  // events with ts < T that are not in the SAE yet (as esvo_ts_render)
      { int rc = refuse_decreasing_render(h, cam, upto, "esvo_ts_render_forward"); if (rc) return rc; }
      scatter_upto(h, cam, upto, [&](const esvo_event_t* ev, size_t n) { launch_ts_scatter(ev, n, h->d_sae[cam], h->W, h->H, h->stream); });
    }
  }
  {
    std::lock_guard<std::mutex> lt(h->mu_ts);
    resident_write_begin(h, cam);
    launch_ts_render_forward(h->d_sae[cam], h->d_fwd_off[cam], h->d_fwd_src[cam], h->d_fwd_lut[cam], h->d_fwd_val, cam ? h->d_raw1 : h->d_raw,
                             h->d_ts[cam], h->W, h->H, (u64)t_ns, h->prm.decay_ms / 1000.0, h->prm.ignore_polarity,
                             h->prm.median_blur_kernel_size, h->stream);
    if (cam == 0) hipEventRecord(h->ts_ev[0].e[TE_R1], h->stream);  // what esvo_track_set_current waits for
    HIPCHK(hipGetLastError());
    h->ts_valid[cam] = true;
    { int rch = hist_store(h, cam, t_ns, h->d_ts[cam], false); if (rch) return rch; }  // the Time-Surface history (off: nothing)
  }
  if (cam == 0) h->ts_timing_pending[0] = false;  // TE_R1 no longer belongs to a timed scatter / render pair
  h->stats.ts_frames[cam]++;
  if (out_mono8) {
    HIPCHK(hipMemcpyAsync(out_mono8, h->d_ts[cam], (size_t)h->W * h->H, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return ESVO_OK;
}

int esvo_ts_render(esvo_handle h, int cam, uint64_t t_ns, uint8_t* out_mono8) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  const TsEvents& T = h->ts_ev[cam];
  const bool timed = esvo_stage_timed(h);  // sampled for renders that run alone (context.hpp, lat_ticks)
  {
    std::lock_guard<std::mutex> lr(h->mu_ring);
    ingest_fence(h, cam);
    const u64 upto = first_staged_at(h, cam, (u64)t_ns);  // events below it that are not in the SAE yet are scattered
    if (!h->tsq_len) { int rc = refuse_decreasing_render(h, cam, upto, "esvo_ts_render"); if (rc) return rc; }
    if (h->ts_timing_pending[cam] && hipEventQuery(T.e[TE_R1]) == hipSuccess) collect_ts_timing(h, cam);
    if (timed) hipEventRecord(T.e[TE_SC0], h->stream);
    if (h->tsq_len) queue_prepare(h, cam, (u64)t_ns);
    else scatter_upto(h, cam, upto, [&](const esvo_event_t* ev, size_t n) { launch_ts_scatter(ev, n, h->d_sae[cam], h->W, h->H, h->stream); });
    if (timed) hipEventRecord(T.e[TE_SC1], h->stream);
  }
  {
    std::lock_guard<std::mutex> lt(h->mu_ts);
    resident_write_begin(h, cam);
    launch_ts_render(h->d_sae[cam], h->d_fixmap[cam], h->d_raw, h->d_ts[cam], h->W, h->H, (u64)t_ns, h->prm.decay_ms / 1000.0,
                     h->prm.ignore_polarity, h->prm.median_blur_kernel_size, h->stream, h->routed ? h->rband_y0 : 0,
                     h->routed ? h->rband_y1 : -1);
    if (timed || (cam == 0 && h->trk_used.load())) hipEventRecord(T.e[TE_R1], h->stream);
    HIPCHK(hipGetLastError());
    h->ts_valid[cam] = true;
    { int rch = hist_store(h, cam, t_ns, h->d_ts[cam], false); if (rch) return rch; }  // the Time-Surface history (off: nothing)
  }
  h->ts_timing_pending[cam] = timed;
  h->stats.ts_frames[cam]++;
  if (out_mono8) {
    HIPCHK(hipMemcpyAsync(out_mono8, h->d_ts[cam], (size_t)h->W * h->H, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    collect_ts_timing(h);
  }
  return ESVO_OK;
}

}  // extern "C"
