// api_ts.hip — Time-Surface render: the scatter of staged events, queue mode and the render calls (see context.hpp; the events arrive through api_ingest.hip).
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
extern "C" {

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
