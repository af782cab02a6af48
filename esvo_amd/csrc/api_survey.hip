// api_survey.hip — the event survey of the ingest path (include/esvo_hip.h, esvo_ts_survey_begin): its state, the hook push_filtered
// (ingest.hpp) calls while a survey is open, the mask call and its installation into the camera's filter, and both rules on the host
// (esvo_event_survey_host, esvo_hot_pixel_mask_host).  The kernels are in kernels_survey.hip.
#include "ingest.hpp"

namespace {
constexpr u64 SRV_MAX_EVENTS = 0xffffffffull;  // events_in + outside of a survey: no counter can wrap below it

const char* rule_error(const esvo_hot_pixel_rule_t* r) {
  if (r->reserved[0] || r->reserved[1] || r->reserved[2] || r->reserved[3]) return "esvo_hot_pixel_rule_t: reserved words must be 0";
  if (r->min_count == 0) return "esvo_hot_pixel_rule_t: min_count must be >= 1";
  if (r->rank_permille > 1000) return "esvo_hot_pixel_rule_t: rank_permille must be 0..1000";
  if (r->factor == 0 && r->max_rate_hz == 0) return "esvo_hot_pixel_rule_t: both tests are off (factor and max_rate_hz are 0)";
  return nullptr;
}
// k of the rule: floor(rank_permille * (npx - 1) / 1000)
u64 rule_rank(const esvo_hot_pixel_rule_t* r, u64 npx) { return (u64)r->rank_permille * (npx - 1) / 1000ull; }
// R of the rule; *on: the rate test applies (it is asked for and the survey has a duration)
u32 rule_rate_count(const esvo_hot_pixel_rule_t* r, u64 t_first, u64 t_last, bool* on) {
  *on = r->max_rate_hz != 0 && t_last > t_first;
  if (!*on) return 0u;
  const unsigned __int128 v = (unsigned __int128)r->max_rate_hz * (unsigned __int128)(t_last - t_first) / 1000000000ull;
  return v > (unsigned __int128)0xffffffffull ? 0xffffffffu : (u32)v;
}
const char* state_error(const uint32_t* counts, size_t npx) {
  for (size_t i = 0; i < npx; ++i)
    if ((u64)counts[i] + counts[npx + i] > SRV_MAX_EVENTS) return "event survey: the two planes of a pixel add up beyond 2^32 - 1";
  return nullptr;
}
}  // namespace

namespace esvo_host {

static SurveyArgs survey_args(esvo_context* h, int cam, const FilterPacket& in) {
  auto& S = h->srv[cam];
  SurveyArgs a{};
  a.t = in.d_t; a.x = in.d_x; a.y = in.d_y; a.p = in.d_p; a.p_type = in.p_type; a.n = (u32)in.n;
  a.W = h->W; a.H = h->H;
  a.counts = S.d_counts; a.stats = S.d_stats;
  return a;
}
static int survey_zero(esvo_context* h, int cam, hipStream_t st) {
  auto& S = h->srv[cam];
  HIPCHK(hipMemsetAsync(S.d_counts, 0, sizeof(u32) * 2 * (size_t)h->W * h->H, st));
  HIPCHK(hipMemsetAsync(S.d_stats, 0, sizeof(u64) * SRV_STAT_WORDS, st));
  HIPCHK(hipMemsetAsync(S.d_stats + SRV_S_T_FIRST, 0xff, sizeof(u64), st));  // (~0: no counted event yet)
  return ESVO_OK;
}

int survey_admit(esvo_context* h, int cam, size_t n) {
  if (h->srv_events[cam] + n > SRV_MAX_EVENTS)
    FAIL(ESVO_ERR_CAPACITY, "event survey: the packet would take events_in + outside beyond 2^32 - 1 (take the mask, then esvo_ts_survey_end / _begin)");
  return ESVO_OK;
}
int survey_count(esvo_context* h, int cam, const FilterPacket& in, bool wait) {
  launch_survey_count(survey_args(h, cam, in), h->stream_i);
  HIPCHK(hipGetLastError());
  if (wait) HIPCHK(hipStreamSynchronize(h->stream_i));
  return ESVO_OK;
}
void survey_commit(esvo_context* h, int cam, size_t n) {
  h->srv_events[cam] += n;
  h->srv_packets[cam] += 1;
}
int survey_count_only(esvo_context* h, int cam, const FilterPacket& in, bool check_stamps, u32* first_bad) {
  auto& S = h->srv[cam];
  *first_bad = 0xffffffffu;
  if (in.n > 0x7fffffffull) FAIL(ESVO_ERR_UNSUPPORTED, "event survey: more than 2^31 - 1 events in one packet");
  if (check_stamps) {  // device columns: validity is the one thing a count-only push still has to learn before it counts
    launch_survey_first_bad(in.d_t, (u32)in.n, S.d_sel, h->stream_i);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(first_bad, S.d_sel + SRV_SEL_FIRST_BAD, sizeof(u32), hipMemcpyDeviceToHost, h->stream_i));
    HIPCHK(hipStreamSynchronize(h->stream_i));
    if (*first_bad != 0xffffffffu) return ESVO_OK;
  }
  { int rc = survey_count(h, cam, in, true); if (rc) return rc; }  // (waits: the columns may be the caller's)
  survey_commit(h, cam, in.n);
  return ESVO_OK;
}
int survey_zero_state(esvo_context* h, hipStream_t st) {
  for (int cam = 0; cam < 2; ++cam)
    if (h->srv[cam].on) { int rc = survey_zero(h, cam, st); if (rc) return rc; }
  return ESVO_OK;
}

}  // namespace esvo_host

extern "C" {

int esvo_ts_survey_begin(esvo_handle h, int cam, const esvo_event_survey_t* s) {
  if (!h || cam < 0 || cam > 1 || !s) return ESVO_ERR_INVALID_ARG;
  if (s->reserved[0] || s->reserved[1] || s->reserved[2]) FAIL(ESVO_ERR_INVALID_ARG, "esvo_event_survey_t: reserved words must be 0");
  if (s->flags & ~(uint32_t)ESVO_SURVEY_COUNT_ONLY) FAIL(ESVO_ERR_INVALID_ARG, "esvo_event_survey_t: unknown flags");
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  auto& S = h->srv[cam];
  if (!h->flt[cam].on) FAIL(ESVO_ERR_STATE, "esvo_ts_survey_begin: no event filter is configured for this camera (esvo_ts_filter_configure; both periods 0 and no mask pass everything)");
  if (S.on) FAIL(ESVO_ERR_STATE, "esvo_ts_survey_begin: a survey of this camera is open already");
  const size_t npx = (size_t)h->W * h->H;
  if (npx >= ((size_t)1 << 31)) FAIL(ESVO_ERR_UNSUPPORTED, "event survey: more than 2^31 - 1 pixels");
  hipError_t e = S.d_counts.alloc(2 * npx);
  if (e == hipSuccess) e = S.d_stats.alloc(SRV_STAT_WORDS);
  if (e == hipSuccess) e = S.d_sel.alloc(SRV_SEL_WORDS);
  if (e == hipSuccess) e = S.d_report.alloc(SRV_REPORT_WORDS);
  if (e == hipSuccess) e = S.d_mask.alloc(npx);
  int rc = ESVO_OK;
  if (e == hipSuccess) {
    rc = survey_zero(h, cam, h->stream_i);
    if (!rc && hipStreamSynchronize(h->stream_i) != hipSuccess) rc = ESVO_ERR_HIP;
  }
  if (e != hipSuccess || rc) {
    (void)hipGetLastError();
    (void)S.d_counts.release(); (void)S.d_stats.release(); (void)S.d_sel.release(); (void)S.d_report.release(); (void)S.d_mask.release();
    if (e != hipSuccess) FAIL(ESVO_ERR_HIP, std::string("esvo_ts_survey_begin: ") + hipGetErrorString(e));
    return rc;
  }
  h->srv_events[cam] = h->srv_packets[cam] = 0;
  S.count_only = (s->flags & ESVO_SURVEY_COUNT_ONLY) != 0;
  S.on = true;
  return ESVO_OK;
}

int esvo_ts_survey_end(esvo_handle h, int cam) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  auto& S = h->srv[cam];
  if (!S.on) FAIL(ESVO_ERR_STATE, "esvo_ts_survey_end: no survey of this camera is open");
  HIPCHK(hipStreamSynchronize(h->stream_i));
  S.on = false; S.count_only = false;
  (void)S.d_counts.release(); (void)S.d_stats.release(); (void)S.d_sel.release(); (void)S.d_report.release(); (void)S.d_mask.release();
  h->srv_events[cam] = h->srv_packets[cam] = 0;
  return ESVO_OK;
}

// the stats as the ABI names them, from the device's words and the host's packet count; caller holds mu_push[cam], the stream idle
static int survey_read_stats(esvo_context* h, int cam, esvo_event_survey_stats_t* out) {
  u64 w[SRV_STAT_WORDS];
  HIPCHK(hipMemcpy(w, h->srv[cam].d_stats, sizeof(w), hipMemcpyDeviceToHost));
  const bool any = w[SRV_S_IN] != 0;
  *out = esvo_event_survey_stats_t{w[SRV_S_IN], w[SRV_S_OUTSIDE], h->srv_packets[cam], any ? w[SRV_S_T_FIRST] : 0, any ? w[SRV_S_T_LAST] : 0};
  return ESVO_OK;
}

int esvo_ts_survey_stats(esvo_handle h, int cam, esvo_event_survey_stats_t* out) {
  if (!h || cam < 0 || cam > 1 || !out) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  if (!h->srv[cam].on) FAIL(ESVO_ERR_STATE, "esvo_ts_survey_stats: no survey of this camera is open");
  HIPCHK(hipStreamSynchronize(h->stream_i));
  return survey_read_stats(h, cam, out);
}

int esvo_ts_survey_state(esvo_handle h, int cam, uint32_t* get, const uint32_t* set, const esvo_event_survey_stats_t* stats_set) {
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  if (stats_set && !set) FAIL(ESVO_ERR_INVALID_ARG, "esvo_ts_survey_state: stats_set goes with set only");
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  auto& S = h->srv[cam];
  if (!S.on) FAIL(ESVO_ERR_STATE, "esvo_ts_survey_state: no survey of this camera is open");
  const size_t npx = (size_t)h->W * h->H;
  if (set) if (const char* msg = state_error(set, npx)) FAIL(ESVO_ERR_INVALID_ARG, msg);
  if (stats_set && (stats_set->events_in > SRV_MAX_EVENTS || stats_set->outside > SRV_MAX_EVENTS || stats_set->events_in + stats_set->outside > SRV_MAX_EVENTS))
    FAIL(ESVO_ERR_INVALID_ARG, "esvo_ts_survey_state: stats_set's events_in + outside lie beyond 2^32 - 1");
  HIPCHK(hipStreamSynchronize(h->stream_i));
  if (get) HIPCHK(hipMemcpy(get, S.d_counts, sizeof(u32) * 2 * npx, hipMemcpyDeviceToHost));
  if (set) HIPCHK(hipMemcpy(S.d_counts, set, sizeof(u32) * 2 * npx, hipMemcpyHostToDevice));
  if (stats_set) {
    const bool any = stats_set->events_in != 0;
    const u64 w[SRV_STAT_WORDS] = {stats_set->events_in, stats_set->outside, any ? stats_set->t_first : ~0ull, any ? stats_set->t_last : 0ull};
    HIPCHK(hipMemcpy(S.d_stats, w, sizeof(w), hipMemcpyHostToDevice));
    h->srv_events[cam] = stats_set->events_in + stats_set->outside;
    h->srv_packets[cam] = stats_set->packets;
  }
  return ESVO_OK;
}

int esvo_ts_survey_mask(esvo_handle h, int cam, const esvo_hot_pixel_rule_t* rule, uint8_t* mask_out, int install, esvo_hot_pixel_report_t* report) {
  if (!h || cam < 0 || cam > 1 || !rule) return ESVO_ERR_INVALID_ARG;
  if (const char* msg = rule_error(rule)) FAIL(ESVO_ERR_INVALID_ARG, msg);
  if (install != ESVO_MASK_KEEP && install != ESVO_MASK_REPLACE && install != ESVO_MASK_UNION) FAIL(ESVO_ERR_INVALID_ARG, "esvo_ts_survey_mask: unknown install");
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  auto& S = h->srv[cam];
  auto& F = h->flt[cam];
  if (!S.on) FAIL(ESVO_ERR_STATE, "esvo_ts_survey_mask: no survey of this camera is open");
  if (install != ESVO_MASK_KEEP && !F.on) FAIL(ESVO_ERR_STATE, "esvo_ts_survey_mask: no event filter is configured to install the mask into");
  const size_t npx = (size_t)h->W * h->H;
  HIPCHK(hipStreamSynchronize(h->stream_i));
  esvo_event_survey_stats_t st{};
  { int rc = survey_read_stats(h, cam, &st); if (rc) return rc; }  // (32 bytes: R is the host's to compute)
  bool rate_on = false;
  const u32 R = rule_rate_count(rule, st.t_first, st.t_last, &rate_on);
  if (install != ESVO_MASK_KEEP && !F.d_mask) HIPCHK(F.d_mask.alloc(npx));  // (before anything is launched: the filter stays as it is on failure)
  launch_survey_mask(S.d_counts, (u32)npx, (u32)rule_rank(rule, npx), rule->min_count, rule->factor, rate_on, R, S.d_sel, S.d_mask, S.d_report, h->stream_i);
  HIPCHK(hipGetLastError());
  if (install == ESVO_MASK_UNION && F.has_mask) {
    launch_survey_mask_or(F.d_mask, S.d_mask, (u32)npx, h->stream_i);
    HIPCHK(hipGetLastError());
  } else if (install != ESVO_MASK_KEEP) {
    HIPCHK(hipMemcpyAsync(F.d_mask, S.d_mask, npx, hipMemcpyDeviceToDevice, h->stream_i));
  }
  u64 rep[SRV_REPORT_WORDS] = {};
  if (report) HIPCHK(hipMemcpyAsync(rep, S.d_report, sizeof(rep), hipMemcpyDeviceToHost, h->stream_i));
  if (mask_out) HIPCHK(hipMemcpyAsync(mask_out, S.d_mask, npx, hipMemcpyDeviceToHost, h->stream_i));
  HIPCHK(hipStreamSynchronize(h->stream_i));
  if (install != ESVO_MASK_KEEP) F.has_mask = true;
  if (report) {
    *report = esvo_hot_pixel_report_t{};
    report->baseline = (u32)rep[SRV_R_BASELINE]; report->rate_count = R; report->n_hot = (u32)rep[SRV_R_HOT];
    report->max_count = (u32)(rep[SRV_R_MAX] >> 32); report->max_pixel = 0xffffffffu - (u32)(rep[SRV_R_MAX] & 0xffffffffull);
    report->events_hot = rep[SRV_R_EVENTS];
  }
  return ESVO_OK;
}

int esvo_event_survey_host(int width, int height, uint32_t* counts, esvo_event_survey_stats_t* stats, const esvo_event_t* ev, size_t n) {
  esvo_context* h = nullptr;
  if (width <= 0 || height <= 0 || !counts || !stats || (n && !ev)) return ESVO_ERR_INVALID_ARG;
  if (n == 0) return ESVO_OK;
  if (stats->events_in + stats->outside + n > SRV_MAX_EVENTS) FAIL(ESVO_ERR_CAPACITY, "esvo_event_survey_host: the events would take events_in + outside beyond 2^32 - 1");
  const size_t W = (size_t)width, H = (size_t)height, npx = W * H;
  for (size_t i = 0; i < n; ++i) {
    const esvo_event_t& e = ev[i];
    if (e.x >= W || e.y >= H) { ++stats->outside; continue; }
    const u64 t = (u64)e.sec * 1000000000ull + e.nsec;
    if (stats->events_in == 0) stats->t_first = stats->t_last = t;
    stats->t_first = std::min<u64>(stats->t_first, t); stats->t_last = std::max<u64>(stats->t_last, t);
    ++counts[(e.polarity ? npx : 0) + (size_t)e.y * W + e.x];
    ++stats->events_in;
  }
  ++stats->packets;
  return ESVO_OK;
}

int esvo_hot_pixel_mask_host(const esvo_hot_pixel_rule_t* rule, int width, int height, const uint32_t* counts, const esvo_event_survey_stats_t* stats,
                             uint8_t* mask, esvo_hot_pixel_report_t* report) {
  esvo_context* h = nullptr;
  if (!rule || width <= 0 || height <= 0 || !counts || !stats) return ESVO_ERR_INVALID_ARG;
  if (const char* msg = rule_error(rule)) FAIL(ESVO_ERR_INVALID_ARG, msg);
  const size_t npx = (size_t)width * (size_t)height;
  if (const char* msg = state_error(counts, npx)) FAIL(ESVO_ERR_INVALID_ARG, msg);
  std::vector<u32> c(npx);
  for (size_t i = 0; i < npx; ++i) c[i] = counts[i] + counts[npx + i];
  std::vector<u32> order(c);
  const size_t k = (size_t)rule_rank(rule, npx);
  std::nth_element(order.begin(), order.begin() + (std::ptrdiff_t)k, order.end());
  const u32 B = order[k];
  bool rate_on = false;
  const u32 R = rule_rate_count(rule, stats->events_in ? stats->t_first : 0, stats->events_in ? stats->t_last : 0, &rate_on);
  esvo_hot_pixel_report_t rep{};
  rep.baseline = B; rep.rate_count = R;
  for (size_t i = 0; i < npx; ++i) {
    const bool hot = c[i] >= rule->min_count && ((rule->factor != 0 && (u64)c[i] > (u64)rule->factor * B) || (rate_on && c[i] > R));
    if (mask) mask[i] = hot ? 1 : 0;
    if (hot) { ++rep.n_hot; rep.events_hot += c[i]; }
    if (c[i] > rep.max_count) { rep.max_count = c[i]; rep.max_pixel = (u32)i; }
  }
  if (report) *report = rep;
  return ESVO_OK;
}

void esvo_event_survey_sizes(size_t out[4]) {
  out[0] = sizeof(esvo_event_survey_t); out[1] = sizeof(esvo_event_survey_stats_t);
  out[2] = sizeof(esvo_hot_pixel_rule_t); out[3] = sizeof(esvo_hot_pixel_report_t);
}

}  // extern "C"
