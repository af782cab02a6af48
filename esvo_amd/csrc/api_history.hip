// api_history.hip — the Time-Surface history: the nodes' TS_history_ on the device (see context.hpp).
//
// Both nodes keep the last TS_HISTORY_LENGTH stereo pairs by stamp (esvo_Mapping.cpp:757-761, esvo_Tracking.cpp:241-247); the
// tracker registers against the newest, the mapper observes the second newest that has a pose (esvo_Mapping.cpp:497-534).  Here
// the pairs stay in HBM: every frame that becomes a camera's resident frame is copied into a slot on the front stream, behind
// its render, and the mapper's and the tracker's calls read the slot of a stamp as they read the resident frame.  No arithmetic:
// what this file owns is the lifetime of the slots and the order of their writes and reads.
//   writes   front stream, enqueued under mu_ts (renders, esvo_ts_history_put): stream order among themselves
//   mapper   front stream (esvo_map_set_observation_at, esvo_ts_history_get): stream order, no event
//   tracker  tracker stream behind evt_hist (recorded behind the newest store); it leaves evt_trk_read behind its read, which
//            the next store of a left frame waits for (resident_write_begin)
#include "context.hpp"

namespace esvo_host {

namespace {
uint8_t* hist_frame(esvo_context* h, u32 slot, int cam) { return h->d_hist + ((size_t)2 * slot + (size_t)cam) * h->hist_stride; }

// the entry of a stamp (null: not retained); caller holds mu_ts
esvo_context::HistEntry* hist_find(esvo_context* h, u64 t_ns) {
  auto it = std::lower_bound(h->hist.begin(), h->hist.end(), t_ns, [](const esvo_context::HistEntry& e, u64 t) { return e.t_ns < t; });
  return it != h->hist.end() && it->t_ns == t_ns ? &*it : nullptr;
}

std::string hist_missing(esvo_context* h, const char* call, u64 t_ns, bool pair) {
  std::string m = std::string(call) + ": stamp " + std::to_string(t_ns) + (pair ? " is not retained as a complete pair" : " is not retained");
  if (h->hist.empty()) return m + " (the history is empty)";
  return m + " (retained: " + std::to_string(h->hist.size()) + " stamps, " + std::to_string(h->hist.front().t_ns) + " .. " +
         std::to_string(h->hist.back().t_ns) + ")";
}
}  // namespace

void hist_clear(esvo_context* h) {
  h->hist.clear();
  h->hist_free.clear();
  for (size_t s = h->hist_len; s-- > 0;) h->hist_free.push_back((u32)s);
}

// The frame of `cam` at t_ns goes into the history (src: W * H bytes, device or host memory), on the front stream.  The entry is
// inserted in stamp order, then the smallest stamp goes while there are more than hist_len (esvo_Mapping.cpp:757-761): a stamp
// below every retained one on a full history is not retained.  A stamp that is retained already keeps its slot and the frame is
// overwritten.  Caller holds mu_ts; history off: nothing.
int hist_store(esvo_context* h, int cam, uint64_t t_ns, const uint8_t* src, bool from_host) {
  if (!h->hist_len) return ESVO_OK;
  esvo_context::HistEntry* e = hist_find(h, (u64)t_ns);
  if (!e) {
    if (h->hist.size() == h->hist_len) {
      if ((u64)t_ns < h->hist.front().t_ns) return ESVO_OK;
      h->hist_free.push_back(h->hist.front().slot);
      h->hist.erase(h->hist.begin());
    }
    const u32 slot = h->hist_free.back();
    h->hist_free.pop_back();
    auto at = std::lower_bound(h->hist.begin(), h->hist.end(), (u64)t_ns, [](const esvo_context::HistEntry& x, u64 t) { return x.t_ns < t; });
    e = &*h->hist.insert(at, esvo_context::HistEntry{(u64)t_ns, slot, 0});
  }
  e->cams |= (uint8_t)(1u << cam);
  resident_write_begin(h, cam);  // a tracker read of the slot's former frame may be in flight
  HIPCHK(hipMemcpyAsync(hist_frame(h, e->slot, cam), src, (size_t)h->W * h->H, from_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                        h->stream));
  if (h->trk_used.load()) HIPCHK(hipEventRecord(h->evt_hist, h->stream));  // (what esvo_track_set_current_at waits for)
  return ESVO_OK;
}

}  // namespace esvo_host

extern "C" {

int esvo_ts_history_configure(esvo_handle h, size_t length) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  if (length && (h->sharded || h->routed || h->comm))
    FAIL(ESVO_ERR_UNSUPPORTED, "the Time-Surface history is not available on band-sharded or tick-interleaved handles");
  if (length > ((size_t)1 << 20)) FAIL(ESVO_ERR_CAPACITY, "Time-Surface history of more than 2^20 pairs");
  std::lock_guard<std::mutex> ltk(h->mu_track);  // (the order esvo_reset takes them in)
  std::lock_guard<std::mutex> lts(h->mu_ts);
  HIPCHK(hipSetDevice(h->device));
  // no store and no read of a slot may be in flight when the slots go
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream_t));
  h->trk_read_pending = false;
  (void)h->d_hist.release();
  h->hist_len = 0;
  h->hist_stride = 0;
  hist_clear(h);
  if (!length) return ESVO_OK;
  const size_t stride = ((size_t)h->W * h->H + 255) / 256 * 256;
  HIPCHK(h->evt_hist.create(hipEventDisableTiming));
  if (h->d_hist.alloc(length * 2 * stride) != hipSuccess) {
    (void)hipGetLastError();
    FAIL(ESVO_ERR_CAPACITY, "out of device memory for the Time-Surface history");
  }
  h->hist_len = length;
  h->hist_stride = stride;
  hist_clear(h);
  return ESVO_OK;
}

int esvo_ts_history_list(esvo_handle h, uint64_t* t_ns, uint8_t* cams, size_t cap, size_t* n) {
  if (!h || !n) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lts(h->mu_ts);
  if (!h->hist_len) FAIL(ESVO_ERR_STATE, "the Time-Surface history is off: esvo_ts_history_configure first");
  *n = h->hist.size();
  if (!t_ns && !cams) return ESVO_OK;
  if (cap < h->hist.size()) FAIL(ESVO_ERR_CAPACITY, "esvo_ts_history_list: the arrays are shorter than the history");
  for (size_t i = 0; i < h->hist.size(); ++i) {
    if (t_ns) t_ns[i] = h->hist[i].t_ns;
    if (cams) cams[i] = h->hist[i].cams;
  }
  return ESVO_OK;
}

int esvo_ts_history_get(esvo_handle h, uint64_t t_ns, int cam, uint8_t* out_mono8) {
  if (!h || !out_mono8 || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  const uint8_t* src = nullptr;
  {
    std::lock_guard<std::mutex> lts(h->mu_ts);
    if (!h->hist_len) FAIL(ESVO_ERR_STATE, "the Time-Surface history is off: esvo_ts_history_configure first");
    const esvo_context::HistEntry* e = hist_find(h, (u64)t_ns);
    if (!e || !(e->cams & (1u << cam))) FAIL(ESVO_ERR_STATE, hist_missing(h, "esvo_ts_history_get", (u64)t_ns, false));
    src = hist_frame(h, e->slot, cam);
  }
  // (the slot cannot be written meanwhile: stores are mapper-group calls, and this one holds the group's lock)
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(out_mono8, src, (size_t)h->W * h->H, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return ESVO_OK;
}

int esvo_ts_history_put(esvo_handle h, uint64_t t_ns, int cam, const uint8_t* mono8) {
  if (!h || !mono8 || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  HIPCHK(hipSetDevice(h->device));
  {
    std::lock_guard<std::mutex> lts(h->mu_ts);
    if (!h->hist_len) FAIL(ESVO_ERR_STATE, "the Time-Surface history is off: esvo_ts_history_configure first");
    int rc = hist_store(h, cam, t_ns, mono8, true);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(h->stream));  // `mono8` is borrowed for the duration of the call only
  return ESVO_OK;
}

int esvo_map_set_observation_at(esvo_handle h, uint64_t t_ns, const double T_world_cam[16]) {
  if (!h || !T_world_cam) return ESVO_ERR_INVALID_ARG;
  API_LOCK(h);
  const uint8_t* src[2] = {nullptr, nullptr};
  {
    std::lock_guard<std::mutex> lts(h->mu_ts);
    if (!h->hist_len) FAIL(ESVO_ERR_STATE, "the Time-Surface history is off: esvo_ts_history_configure first");
    const esvo_context::HistEntry* e = hist_find(h, (u64)t_ns);
    if (!e || e->cams != 3) FAIL(ESVO_ERR_STATE, hist_missing(h, "esvo_map_set_observation_at", (u64)t_ns, true));
    src[0] = hist_frame(h, e->slot, 0);
    src[1] = hist_frame(h, e->slot, 1);
  }
  HIPCHK(hipSetDevice(h->device));
  // = esvo_map_set_observation with the host images of the two frames: the blur (createMatchProblem's GaussianBlurTS(5) when
  // SmoothTimeSurface, EventBM.cpp:68-72) reads the slot directly, the un-smoothed pair is one device-to-device copy each
  begin_observation(h);
  hipError_t err = hipSuccess;
  for (int cam = 0; cam < 2 && err == hipSuccess; ++cam) {
    if (h->prm.smooth_time_surface) { launch_gaussian5(src[cam], h->d_obs[cam], h->W, h->H, h->stream); err = hipGetLastError(); }
    else err = hipMemcpyAsync(h->d_obs[cam], src[cam], (size_t)h->W * h->H, hipMemcpyDeviceToDevice, h->stream);
  }
  if (err != hipSuccess) {
    revert_observation(h);
    FAIL(ESVO_ERR_HIP, std::string("esvo_map_set_observation_at: ") + hipGetErrorString(err));
  }
  std::memcpy(h->T_world_obs, T_world_cam, sizeof(double) * 16);
  h->obs_t_ns = t_ns;
  h->obs_set = true;
  return ESVO_OK;
}

int esvo_track_set_current_at(esvo_handle h, uint64_t t_ns, int kernel_size) {
  if (!h) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> _trk_lock(h->mu_track);
  if (kernel_size != 0 && kernel_size != 5)
    FAIL(ESVO_ERR_UNSUPPORTED, "tracker kernelSize must be 0 or 5 (the shipped configs); other sizes take OpenCV's float kernel path");
  HIPCHK(hipSetDevice(h->device));
  const size_t npx = (size_t)h->W * h->H;
  if (!h->d_trk_neg) {
    HIPCHK(h->d_trk_blur.alloc(npx));
    HIPCHK(h->d_trk_neg.alloc(npx));
    HIPCHK(h->d_trk_du.alloc(npx));
    HIPCHK(h->d_trk_dv.alloc(npx));
  }
  {
    std::lock_guard<std::mutex> lt(h->mu_ts);
    if (!h->hist_len) FAIL(ESVO_ERR_STATE, "the Time-Surface history is off: esvo_ts_history_configure first");
    const esvo_context::HistEntry* e = hist_find(h, (u64)t_ns);
    if (!e || !(e->cams & 1u)) FAIL(ESVO_ERR_STATE, hist_missing(h, "esvo_track_set_current_at", (u64)t_ns, false));
    const uint8_t* src = hist_frame(h, e->slot, 0);
    // As esvo_track_set_current on the resident frame: stores record evt_hist only once the tracker has shown up (trk_used), and
    // they are enqueued under mu_ts, held here -- the first call drains the front stream instead, every later store has recorded
    // the event.  The read is marked so that the next store of a left frame queues behind it.
    if (!h->trk_used.exchange(true)) HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamWaitEvent(h->stream_t, h->evt_hist, 0));
    if (kernel_size == 5) launch_gaussian5(src, h->d_trk_blur, h->W, h->H, h->stream_t);
    else HIPCHK(hipMemcpyAsync(h->d_trk_blur, src, npx, hipMemcpyDeviceToDevice, h->stream_t));
    HIPCHK(hipEventRecord(h->evt_trk_read, h->stream_t));
    h->trk_read_pending = true;
  }
  launch_track_images(h->d_trk_blur, h->d_trk_neg, h->d_trk_du, h->d_trk_dv, h->W, h->H, h->stream_t);
  HIPCHK(hipGetLastError());
  h->trk_cur = true;
  return ESVO_OK;
}

// dataTransferring's choice of TS_obs_ (esvo_Mapping.cpp:497-534; esvo_MVStereo.cpp:559-576): nothing below eleven pairs; from
// the second newest ("in case that the tf is behind the most current TS", :503) down to the oldest, the first pair with a pose;
// while the system initialises, the second newest with the identity.
int esvo_ts_history_select(const uint64_t* t_ns, size_t n, int initialization, esvo_em_pose_fn pose_fn, void* user, size_t* index,
                           double T_world_cam[16]) {
  esvo_context* h = nullptr;
  if ((n && !t_ns) || !index || !T_world_cam || (!initialization && !pose_fn)) return ESVO_ERR_INVALID_ARG;
  for (size_t i = 1; i < n; ++i)
    if (t_ns[i] <= t_ns[i - 1]) FAIL(ESVO_ERR_INVALID_ARG, "esvo_ts_history_select: stamps must ascend");
  if (n <= 10) return ESVO_AGAIN;
  for (size_t i = n - 1; i-- > 0;) {
    if (initialization) {
      for (int k = 0; k < 16; ++k) T_world_cam[k] = (k % 5 == 0) ? 1.0 : 0.0;
      *index = i;
      return ESVO_OK;
    }
    double T[16];
    if (pose_fn(user, t_ns[i], T) == 1) {
      std::memcpy(T_world_cam, T, sizeof(T));
      *index = i;
      return ESVO_OK;
    }
  }
  return ESVO_AGAIN;
}

int esvo_ts_history_select_observation(esvo_handle h, int initialization, esvo_em_pose_fn pose_fn, void* user, uint64_t* t_ns,
                                       double T_world_cam[16]) {
  if (!h || !t_ns || !T_world_cam || (!initialization && !pose_fn)) return ESVO_ERR_INVALID_ARG;
  std::vector<uint64_t> pairs;
  {
    std::lock_guard<std::mutex> lts(h->mu_ts);
    if (!h->hist_len) FAIL(ESVO_ERR_STATE, "the Time-Surface history is off: esvo_ts_history_configure first");
    for (const esvo_context::HistEntry& e : h->hist)
      if (e.cams == 3) pairs.push_back(e.t_ns);
  }
  // (the pose lookup is the caller's code: it runs without any of the handle's locks)
  size_t index = 0;
  const int rc = esvo_ts_history_select(pairs.data(), pairs.size(), initialization, pose_fn, user, &index, T_world_cam);
  if (rc == ESVO_OK) *t_ns = pairs[index];
  return rc;
}

}  // extern "C"
