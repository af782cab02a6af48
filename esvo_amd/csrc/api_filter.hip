// api_filter.hip — the event filter of the ingest path (include/esvo_hip.h, esvo_ts_filter_configure) and its burst stage
// (esvo_ts_burst_configure): their configuration and state, the launch sequence over a column packet (kernels_filter.hip) and the
// rule itself on the host (esvo_event_filter_host, esvo_event_burst_filter_host).
// The push calls reach it through push_packet (ingest.hpp).
#include "ingest.hpp"

namespace esvo_host {

static void add_counts(esvo_event_filter_counts_t& a, const esvo_event_filter_counts_t& b) {
  a.events_in += b.events_in; a.kept += b.kept; a.outside += b.outside; a.masked += b.masked; a.refractory += b.refractory;
  a.unsupported += b.unsupported;
}

// the filter's staging for packets of n events
static int filter_staging(esvo_context* h, int cam, size_t n) {
  auto& F = h->flt[cam];
  if (n <= F.cap) return ESVO_OK;
  const size_t cap = (std::max<size_t>(n + n / 2, 256) + 255) / 256 * 256;
  F.cap = 0;
  HIPCHK(F.d_twin.alloc(sizeof(u32) * FLT_HDR_WORDS + cap * 13));
  HIPCHK(F.d_code.alloc(cap));
  HIPCHK(F.d_scan.alloc(cap + scan_scratch_elems(cap)));
  HIPCHK(F.h_twin.alloc(FLT_HDR_WORDS / 2 + cap));
  F.cap = cap;
  return ESVO_OK;
}

int filter_run(esvo_context* h, int cam, const FilterPacket& in, u64 newest, FilterPacket* twin, const u64** kept_stamps, esvo_event_filter_counts_t* counts,
               u64* burst_dropped, bool* unsorted, u32* first_bad) {
  auto& F = h->flt[cam];
  auto& B = h->bst[cam];
  if (in.n > 0x7fffffffull) FAIL(ESVO_ERR_UNSUPPORTED, "event filter: more than 2^31 - 1 events in one packet");
  { int rc = filter_staging(h, cam, in.n); if (rc) return rc; }
  const size_t npx = (size_t)h->W * h->H;
  const ColumnBlock b = column_block(F.d_twin.get() + sizeof(u32) * FLT_HDR_WORDS, F.cap);  // the twin staging behind its header
  FilterArgs a{};
  a.t = in.d_t; a.x = in.d_x; a.y = in.d_y; a.n = (u32)in.n;
  a.W = h->W; a.H = h->H;
  a.refractory_ns = F.refractory_ns; a.support_ns = F.support_ns; a.newest = newest;
  a.mask = F.has_mask ? F.d_mask.get() : nullptr;
  a.last_in = F.d_last + (size_t)F.cur * npx; a.last_out = F.d_last + (size_t)(F.cur ^ 1) * npx;
  a.tcount = F.d_tcount; a.tlist = F.d_tlist; a.tcap = h->flt_tcap;
  a.code = F.d_code; a.hdr = reinterpret_cast<u32*>(F.d_twin.get());
  BurstArgs ba{};
  ba.mode = B.mode;
  if (B.mode != ESVO_BURST_OFF) {
    ba.burst_ns = B.burst_ns; ba.p = in.d_p; ba.p_type = in.p_type;
    ba.stamp_in = B.d_stamp + (size_t)B.cur * npx; ba.stamp_out = B.d_stamp + (size_t)(B.cur ^ 1) * npx;
    ba.flags_in = B.d_flags + (size_t)B.cur * npx; ba.flags_out = B.d_flags + (size_t)(B.cur ^ 1) * npx;
  }
  launch_event_filter(a, ba, F.d_scan, in.d_p, in.p_type, b.t, b.x, b.y, b.p, h->stream_i);
  HIPCHK(hipGetLastError());
  // the verdict counts and the kept stamps (at most n of them) with one copy
  HIPCHK(hipMemcpyAsync(F.h_twin, F.d_twin, sizeof(u32) * FLT_HDR_WORDS + sizeof(u64) * in.n, hipMemcpyDeviceToHost, h->stream_i));
  HIPCHK(hipStreamSynchronize(h->stream_i));
  const u32* hdr = reinterpret_cast<const u32*>(F.h_twin.get()) + FLT_H_VERDICT0;
  *unsorted = reinterpret_cast<const u32*>(F.h_twin.get())[FLT_H_UNSORTED] != 0u;
  *first_bad = reinterpret_cast<const u32*>(F.h_twin.get())[FLT_H_FIRST_BAD];
  *burst_dropped = reinterpret_cast<const u32*>(F.h_twin.get())[FLT_H_BURST];
  if (*burst_dropped > in.n || (B.mode == ESVO_BURST_OFF && *burst_dropped)) FAIL(ESVO_ERR_STATE, "event filter: the verdict counts do not add up to the packet");
  // (the events the burst stage dropped stand in none of the filter's counts)
  *counts = esvo_event_filter_counts_t{in.n - *burst_dropped, hdr[ESVO_FILTER_KEPT], hdr[ESVO_FILTER_OUTSIDE], hdr[ESVO_FILTER_MASKED],
                                       hdr[ESVO_FILTER_REFRACTORY], hdr[ESVO_FILTER_UNSUPPORTED]};
  if (counts->kept + counts->outside + counts->masked + counts->refractory + counts->unsupported != counts->events_in)
    FAIL(ESVO_ERR_STATE, "event filter: the verdict counts do not add up to the packet");
  *twin = b.packet((size_t)counts->kept);
  *kept_stamps = F.h_twin.get() + FLT_HDR_WORDS / 2;
  return ESVO_OK;
}
void filter_commit(esvo_context* h, int cam, const esvo_event_filter_counts_t& counts, u64 burst_dropped) {
  h->flt[cam].cur ^= 1;
  add_counts(h->flt_totals[cam], counts);
  if (h->bst[cam].mode != ESVO_BURST_OFF) {  // the stage judged what passed the bounds and the mask
    h->bst[cam].cur ^= 1;
    auto& t = h->bst_totals[cam];
    t.passed += counts.kept + counts.refractory + counts.unsupported; t.dropped += burst_dropped;
    t.judged = t.passed + t.dropped;
  }
}
int filter_zero_state(esvo_context* h, hipStream_t st) {
  for (auto& F : h->flt)
    if (F.on) {
      HIPCHK(hipMemsetAsync(F.d_last, 0, sizeof(u64) * 2 * (size_t)h->W * h->H, st));
      HIPCHK(hipMemsetAsync(F.d_tcount, 0, sizeof(u32) * filter_tiles(h->W, h->H), st));
    }
  for (auto& B : h->bst)
    if (B.mode != ESVO_BURST_OFF) {
      HIPCHK(hipMemsetAsync(B.d_stamp, 0, sizeof(u64) * 2 * (size_t)h->W * h->H, st));
      HIPCHK(hipMemsetAsync(B.d_flags, 0, 2 * (size_t)h->W * h->H, st));
    }
  return ESVO_OK;
}

}  // namespace esvo_host

extern "C" {

int esvo_ts_filter_configure(esvo_handle h, int cam, const esvo_event_filter_t* f) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  if (f && (f->reserved[0] || f->reserved[1] || f->reserved[2] || f->reserved[3])) FAIL(ESVO_ERR_INVALID_ARG, "esvo_event_filter_t: reserved words must be 0");
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  auto& F = h->flt[cam];
  if (f && h->routed) FAIL(ESVO_ERR_UNSUPPORTED, "event filter on a row-routed band handle: packets are filtered by row on the host there (use ESVO_ROUTE_BROADCAST)");
  HIPCHK(hipStreamSynchronize(h->stream_i));
  const auto release = [&]() {
    F.on = false; F.cap = 0; F.cur = 0; F.has_mask = false;
    (void)F.d_last.release(); (void)F.d_mask.release(); (void)F.d_twin.release(); (void)F.d_code.release(); (void)F.d_tcount.release();
    (void)F.d_tlist.release(); (void)F.d_scan.release(); (void)F.h_twin.release();
  };
  if (!f && h->srv[cam].on) FAIL(ESVO_ERR_STATE, "esvo_ts_filter_configure: an event survey of this camera is open (esvo_ts_survey_end first)");
  if (!f && h->bst[cam].mode != ESVO_BURST_OFF) FAIL(ESVO_ERR_STATE, "esvo_ts_filter_configure: the burst stage of this camera's filter is on (esvo_ts_burst_configure with mode ESVO_BURST_OFF first)");
  if (!f) { release(); return ESVO_OK; }
  const size_t npx = (size_t)h->W * h->H, tiles = filter_tiles(h->W, h->H);
  hipError_t e = hipSuccess;
  if (!F.on) {
    e = F.d_last.alloc(2 * npx);
    if (e == hipSuccess) e = F.d_tcount.alloc(tiles);
    if (e == hipSuccess) e = F.d_tlist.alloc(tiles * h->flt_tcap);
  }
  if (e == hipSuccess && f->mask && !F.d_mask) e = F.d_mask.alloc(npx);
  if (e == hipSuccess) e = hipMemset(F.d_last, 0, sizeof(u64) * 2 * npx);
  if (e == hipSuccess) e = hipMemset(F.d_tcount, 0, sizeof(u32) * tiles);
  if (e == hipSuccess && f->mask) e = hipMemcpy(F.d_mask, f->mask, npx, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    release();
    FAIL(ESVO_ERR_HIP, std::string("esvo_ts_filter_configure: ") + hipGetErrorString(e));
  }
  F.refractory_ns = f->refractory_ns; F.support_ns = f->support_ns; F.has_mask = f->mask != nullptr; F.cur = 0;
  F.on = true;
  return ESVO_OK;
}

int esvo_ts_filter_stats(esvo_handle h, int cam, esvo_event_filter_counts_t* totals) {
  if (!h || cam < 0 || cam > 1 || !totals) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  *totals = h->flt_totals[cam];
  return ESVO_OK;
}

int esvo_ts_filter_state(esvo_handle h, int cam, uint64_t* get_last, const uint64_t* set_last) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  auto& F = h->flt[cam];
  if (!F.on) FAIL(ESVO_ERR_STATE, "esvo_ts_filter_state: no event filter is configured for this camera");
  const size_t npx = (size_t)h->W * h->H;
  u64* const cur = F.d_last + (size_t)F.cur * npx;
  HIPCHK(hipStreamSynchronize(h->stream_i));
  if (get_last) HIPCHK(hipMemcpy(get_last, cur, sizeof(u64) * npx, hipMemcpyDeviceToHost));
  if (set_last) HIPCHK(hipMemcpy(cur, set_last, sizeof(u64) * npx, hipMemcpyHostToDevice));
  return ESVO_OK;
}

int esvo_ts_burst_configure(esvo_handle h, int cam, const esvo_event_burst_t* b) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  if (b && (b->reserved[0] || b->reserved[1] || b->reserved[2])) FAIL(ESVO_ERR_INVALID_ARG, "esvo_event_burst_t: reserved words must be 0");
  if (b && b->mode > ESVO_BURST_STC_KEEP_TRAIL) FAIL(ESVO_ERR_INVALID_ARG, "esvo_event_burst_t: unknown mode");
  if (b && b->mode != ESVO_BURST_OFF && b->burst_ns == 0) FAIL(ESVO_ERR_INVALID_ARG, "esvo_event_burst_t: burst_ns must be above 0");
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  auto& B = h->bst[cam];
  HIPCHK(hipStreamSynchronize(h->stream_i));
  const auto release = [&]() { B.mode = ESVO_BURST_OFF; B.burst_ns = 0; B.cur = 0; (void)B.d_stamp.release(); (void)B.d_flags.release(); };
  if (!b || b->mode == ESVO_BURST_OFF) { release(); return ESVO_OK; }
  if (!h->flt[cam].on) FAIL(ESVO_ERR_STATE, "esvo_ts_burst_configure: no event filter is configured for this camera (esvo_ts_filter_configure; both periods 0 and no mask pass everything)");
  const size_t npx = (size_t)h->W * h->H;
  hipError_t e = hipSuccess;
  if (!B.d_stamp) e = B.d_stamp.alloc(2 * npx);
  if (e == hipSuccess && !B.d_flags) e = B.d_flags.alloc(2 * npx);
  if (e == hipSuccess) e = hipMemset(B.d_stamp, 0, sizeof(u64) * 2 * npx);
  if (e == hipSuccess) e = hipMemset(B.d_flags, 0, 2 * npx);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    release();
    FAIL(ESVO_ERR_HIP, std::string("esvo_ts_burst_configure: ") + hipGetErrorString(e));
  }
  B.mode = b->mode; B.burst_ns = b->burst_ns; B.cur = 0;
  return ESVO_OK;
}

int esvo_ts_burst_stats(esvo_handle h, int cam, esvo_event_burst_counts_t* totals) {
  if (!h || cam < 0 || cam > 1 || !totals) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  *totals = h->bst_totals[cam];
  return ESVO_OK;
}

int esvo_ts_burst_state(esvo_handle h, int cam, uint64_t* get_stamp, uint8_t* get_flags, const uint64_t* set_stamp, const uint8_t* set_flags) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  if ((set_stamp == nullptr) != (set_flags == nullptr)) FAIL(ESVO_ERR_INVALID_ARG, "esvo_ts_burst_state: set_stamp and set_flags go together");
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  auto& B = h->bst[cam];
  if (B.mode == ESVO_BURST_OFF) FAIL(ESVO_ERR_STATE, "esvo_ts_burst_state: the burst stage of this camera is off");
  const size_t npx = (size_t)h->W * h->H;
  if (set_flags)
    for (size_t i = 0; i < npx; ++i)
      if (set_flags[i] > 3) FAIL(ESVO_ERR_INVALID_ARG, "esvo_ts_burst_state: flag byte " + std::to_string(i) + " is above 3");
  u64* const st = B.d_stamp + (size_t)B.cur * npx;
  uint8_t* const fl = B.d_flags + (size_t)B.cur * npx;
  HIPCHK(hipStreamSynchronize(h->stream_i));
  if (get_stamp) HIPCHK(hipMemcpy(get_stamp, st, sizeof(u64) * npx, hipMemcpyDeviceToHost));
  if (get_flags) HIPCHK(hipMemcpy(get_flags, fl, npx, hipMemcpyDeviceToHost));
  if (set_stamp) {
    HIPCHK(hipMemcpy(st, set_stamp, sizeof(u64) * npx, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(fl, set_flags, npx, hipMemcpyHostToDevice));
  }
  return ESVO_OK;
}

// both host entry points: the filter's rule, with the burst stage in it where b names a mode
static int filter_host(const char* who, const esvo_event_burst_t* b, const esvo_event_filter_t* f, int width, int height, uint64_t* bstamp, uint8_t* bflags,
                       uint64_t* last, const esvo_event_t* ev, size_t n, uint8_t* verdict, esvo_event_t* out, size_t cap, size_t* n_out,
                       esvo_event_burst_counts_t* add_burst, esvo_event_filter_counts_t* add) {
  esvo_context* h = nullptr;
  if (n_out) *n_out = 0;
  if (!f || !last || width <= 0 || height <= 0 || (n && !ev)) return ESVO_ERR_INVALID_ARG;
  if (f->reserved[0] || f->reserved[1] || f->reserved[2] || f->reserved[3]) FAIL(ESVO_ERR_INVALID_ARG, "esvo_event_filter_t: reserved words must be 0");
  if (b && (b->reserved[0] || b->reserved[1] || b->reserved[2])) FAIL(ESVO_ERR_INVALID_ARG, "esvo_event_burst_t: reserved words must be 0");
  if (b && b->mode > ESVO_BURST_STC_KEEP_TRAIL) FAIL(ESVO_ERR_INVALID_ARG, "esvo_event_burst_t: unknown mode");
  const u32 mode = b ? b->mode : (u32)ESVO_BURST_OFF;
  if (mode != ESVO_BURST_OFF && b->burst_ns == 0) FAIL(ESVO_ERR_INVALID_ARG, "esvo_event_burst_t: burst_ns must be above 0");
  if (mode != ESVO_BURST_OFF && (!bstamp || !bflags)) FAIL(ESVO_ERR_INVALID_ARG, std::string(who) + ": bstamp and bflags are required while the stage is on");
  const size_t W = (size_t)width, H = (size_t)height;
  // the state advances only on success: the pixels a packet rewrites, with what they held
  std::vector<std::pair<size_t, u64>> undo;
  struct BurstUndo { size_t px; u64 stamp; uint8_t flags; };
  std::vector<BurstUndo> bundo;
  std::vector<uint8_t> v(n);
  esvo_event_filter_counts_t c{};
  esvo_event_burst_counts_t bc{};
  size_t kept = 0;
  bool full = false;
  for (size_t i = 0; i < n && !full; ++i) {
    const esvo_event_t& e = ev[i];
    const u64 t = (u64)e.sec * 1000000000ull + e.nsec;
    const size_t x = e.x, y = e.y, px = y * W + x;
    uint8_t r = ESVO_FILTER_KEPT;
    if (x >= W || y >= H) r = ESVO_FILTER_OUTSIDE;
    else if (f->mask && f->mask[px]) r = ESVO_FILTER_MASKED;
    else if (mode != ESVO_BURST_OFF) {
      const u64 T = bstamp[px];
      const u32 p = e.polarity ? 1u : 0u, P = bflags[px] & 1u, K = (bflags[px] >> 1) & 1u;
      const bool linked = T != 0 && p == P && (T > t || t - T <= b->burst_ns);
      const bool pass = mode == ESVO_BURST_TRAIL ? !linked : (mode == ESVO_BURST_STC_CUT_TRAIL ? linked && !K : linked);
      bundo.push_back({px, T, bflags[px]});
      bstamp[px] = t; bflags[px] = (uint8_t)(p | (linked ? 2u : 0u));
      ++bc.judged;
      if (pass) ++bc.passed; else { ++bc.dropped; r = ESVO_FILTER_BURST; }
    }
    if (r != ESVO_FILTER_KEPT) {  // judged above
    } else if (f->refractory_ns && last[px] && (last[px] > t || t - last[px] < f->refractory_ns)) {
      r = ESVO_FILTER_REFRACTORY;
    } else {
      bool sup = false;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if (!dx && !dy) continue;
          const long qx = (long)x + dx, qy = (long)y + dy;
          if (qx < 0 || qy < 0 || qx >= (long)W || qy >= (long)H) continue;
          const u64 L = last[(size_t)qy * W + (size_t)qx];
          sup = sup || (L && (L > t || t - L <= f->support_ns));
        }
      undo.emplace_back(px, last[px]);
      last[px] = t;
      r = f->support_ns && !sup ? ESVO_FILTER_UNSUPPORTED : ESVO_FILTER_KEPT;
    }
    v[i] = r;
    switch (r) {
      case ESVO_FILTER_OUTSIDE: ++c.outside; break;
      case ESVO_FILTER_MASKED: ++c.masked; break;
      case ESVO_FILTER_REFRACTORY: ++c.refractory; break;
      case ESVO_FILTER_UNSUPPORTED: ++c.unsupported; break;
      case ESVO_FILTER_BURST: break;  // (in none of the filter's counts)
      default:
        if (out) {
          if (kept >= cap) { full = true; break; }
          esvo_event_t k = e;
          k.polarity = k.polarity ? 1 : 0; k._pad[0] = k._pad[1] = k._pad[2] = 0;  // as the ring holds it
          out[kept] = k;
        }
        ++kept; ++c.kept;
    }
  }
  if (full) {
    for (size_t k = undo.size(); k-- > 0;) last[undo[k].first] = undo[k].second;
    for (size_t k = bundo.size(); k-- > 0;) { bstamp[bundo[k].px] = bundo[k].stamp; bflags[bundo[k].px] = bundo[k].flags; }
    if (n_out) *n_out = kept;
    FAIL(ESVO_ERR_CAPACITY, std::string(who) + ": more events are kept than `out` has room for");
  }
  c.events_in = n - bc.dropped;
  if (verdict) std::memcpy(verdict, v.data(), n);
  if (n_out) *n_out = kept;
  if (add) add_counts(*add, c);
  if (add_burst) { add_burst->judged += bc.judged; add_burst->passed += bc.passed; add_burst->dropped += bc.dropped; }
  return ESVO_OK;
}

int esvo_event_filter_host(const esvo_event_filter_t* f, int width, int height, uint64_t* last, const esvo_event_t* ev, size_t n,
                           uint8_t* verdict, esvo_event_t* out, size_t cap, size_t* n_out, esvo_event_filter_counts_t* add) {
  return filter_host("esvo_event_filter_host", nullptr, f, width, height, nullptr, nullptr, last, ev, n, verdict, out, cap, n_out, nullptr, add);
}

int esvo_event_burst_filter_host(const esvo_event_burst_t* b, const esvo_event_filter_t* f, int width, int height,
                                 uint64_t* bstamp, uint8_t* bflags, uint64_t* last, const esvo_event_t* ev, size_t n,
                                 uint8_t* verdict, esvo_event_t* out, size_t cap, size_t* n_out,
                                 esvo_event_burst_counts_t* add_burst, esvo_event_filter_counts_t* add_filter) {
  return filter_host("esvo_event_burst_filter_host", b, f, width, height, bstamp, bflags, last, ev, n, verdict, out, cap, n_out, add_burst, add_filter);
}

void esvo_event_burst_sizes(size_t out[4]) {
  out[0] = sizeof(esvo_event_burst_t); out[1] = sizeof(esvo_event_burst_counts_t);
  out[2] = out[3] = 0;
}

void esvo_event_filter_sizes(size_t out[4]) {
  out[0] = sizeof(esvo_event_filter_t); out[1] = sizeof(esvo_event_filter_counts_t);
  out[2] = out[3] = 0;
}

}  // extern "C"
