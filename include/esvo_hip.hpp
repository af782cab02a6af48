// esvo_hip.hpp — C++ host layer over the C-ABI (esvo_hip.h), mirroring the reference's own
// class interface for the hot path so that ESVO's node code (and tests written like it) keeps
// its shape:
//
//   esvo_time_surface::TimeSurface::eventsCallback / createTimeSurfaceAtTime
//                                     (esvo_time_surface/src/TimeSurface.cpp:403-425, :52-152)
//   esvo_core::core::EventBM::resetParameters / createMatchProblem / match_all_HyperThread
//                                     (esvo_core/src/core/EventBM.cpp:34-78, :269-315)
//   esvo_core::core::EventMatcher::resetParameters / createMatchProblem / match_all_HyperThread
//                                     (esvo_core/src/core/EventMatcher.cpp:33-58, :184-246)
//   esvo_core::core::DepthProblemSolver::solve / pointCulling
//                                     (esvo_core/src/core/DepthProblemSolver.cpp:28-78, :216-244)
//   esvo_core::core::DepthFusion (window push + update loop) / DepthMap::clean /
//   DepthRegularization::apply        (esvo_core/src/esvo_Mapping.cpp:341-395)
//   esvo_core::core::RegProblemLM::setProblem / operator() / df   (the tracker's evaluation side,
//                                     esvo_core/src/core/RegProblemLM.cpp:26-269)
//
// Header only, C++14, no ROS / Eigen / OpenCV types: poses are row-major 4x4 doubles, images are
// mono8 pointers, events are esvo_event_t (layout-identical to dvs_msgs::Event).  Every method
// throws esvo_hip::Error carrying esvo_last_error() — the reference's failure mode for these calls
// is exit(-1) or a silent return.  All compute happens in libesvo_hip.so on the GPU.
#ifndef ESVO_HIP_HPP
#define ESVO_HIP_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "esvo_hip.h"

namespace esvo_hip {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

using Event = esvo_event_t;
using EventMatchPair = esvo_match_t;   // x_left, invDepth, cost, disp, pose index (EventMatchPair.h:16-38)
using DepthPoint = esvo_depth_point_t; // every field of DepthPoint.h:70-88

// std::map<ros::Time, Transformation> st_map_ (esvo_Mapping.cpp:585-599), flattened
struct StampTransformationMap {
  std::vector<uint64_t> stamps_ns;
  std::vector<double> T_world_virtual;  // 16 per stamp, row-major
  size_t size() const { return stamps_ns.size(); }
  void emplace(uint64_t t_ns, const double T[16]) {
    stamps_ns.push_back(t_ns);
    T_world_virtual.insert(T_world_virtual.end(), T, T + 16);
  }
  void clear() { stamps_ns.clear(); T_world_virtual.clear(); }
};

// StampedTimeSurfaceObs (TimeSurfaceObservation.h:27-157): mono8 pair + pose.  left/right may be
// null: the pair rendered last on the device is used.
struct StampedTimeSurfaceObs {
  uint64_t t_ns = 0;
  const uint8_t* TS_left = nullptr;
  const uint8_t* TS_right = nullptr;
  double T_world_cam[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
};

// One GPU context shared by the TimeSurface nodes and the mapper (RAII over esvo_handle).
class Context {
 public:
  Context(const esvo_params_t& params, const esvo_calib_t& left, const esvo_calib_t& right, int device = 0)
      : params_(params), width_(left.width), height_(left.height) {
    int rc = esvo_create(&params_, &left, &right, device, &h_);
    if (rc != ESVO_OK) throw Error(rc, std::string("esvo_create: ") + esvo_last_error(nullptr));
  }
  ~Context() { if (h_) esvo_destroy(h_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  esvo_handle handle() const { return h_; }
  const esvo_params_t& params() const { return params_; }
  int width() const { return width_; }
  int height() const { return height_; }
  void check(int rc, const char* what) const {
    if (rc != ESVO_OK) throw Error(rc, std::string(what) + ": " + esvo_last_error(h_));
  }
  void setParams(const esvo_params_t& p) { check(esvo_set_params(h_, &p), "esvo_set_params"); params_ = p; }
  void reset() { check(esvo_reset(h_), "esvo_reset"); }  // esvo_Mapping::reset, esvo_Mapping.cpp:764-804
  // the scale-loop guard of the LM refinement: the limit travels in the parameters (setParams), the counts come back here
  void setLmScalePassLimit(int32_t limit) { esvo_params_t p = params_; p.lm_scale_pass_limit = limit; setParams(p); }
  esvo_lm_stats_t lmStats() const {
    esvo_lm_stats_t st{};
    check(esvo_map_lm_stats(h_, &st), "esvo_map_lm_stats");
    return st;
  }

 private:
  esvo_params_t params_;
  int width_, height_;
  esvo_handle h_ = nullptr;
};
using ContextPtr = std::shared_ptr<Context>;

// esvo_time_surface::TimeSurface for one camera
class TimeSurface {
 public:
  TimeSurface(ContextPtr ctx, int cam) : ctx_(std::move(ctx)), cam_(cam) {}
  // TimeSurface::eventsCallback: events of one EventArray message, time sorted
  void eventsCallback(const Event* events, size_t n) {
    ctx_->check(esvo_ts_push_events(ctx_->handle(), cam_, events, n), "esvo_ts_push_events");
  }
  // the same from x / y / t / p columns in host or device memory (DSEC's layout, a GPU producer's tensors): esvo_ts_push_event_columns
  void eventColumns(const esvo_event_columns_t& columns, size_t n) {
    ctx_->check(esvo_ts_push_event_columns(ctx_->handle(), cam_, &columns, n), "esvo_ts_push_event_columns");
  }
  // the same from Prophesee EVT 3.0 words in host or device memory (a Metavision raw-data callback, a .raw file's data): esvo_ts_push_evt3.
  // The camera's decoder state carries over from call to call; returns the number of events the words emitted.
  size_t evt3Words(const void* words, size_t n_bytes, int memory = ESVO_MEM_HOST, int64_t t_offset_us = 0) {
    size_t n_events = 0;
    ctx_->check(esvo_ts_push_evt3(ctx_->handle(), cam_, words, n_bytes, memory, t_offset_us, &n_events), "esvo_ts_push_evt3");
    return n_events;
  }
  // the same from EVT 2.0 / 2.1 words (format: ESVO_EVT_2_0, ESVO_EVT_2_1 or ESVO_EVT_2_1_LEGACY): esvo_ts_push_evt2
  size_t evt2Words(const void* words, size_t n_bytes, int format, int memory = ESVO_MEM_HOST, int64_t t_offset_us = 0) {
    size_t n_events = 0;
    ctx_->check(esvo_ts_push_evt2(ctx_->handle(), cam_, words, n_bytes, format, memory, t_offset_us, &n_events), "esvo_ts_push_evt2");
    return n_events;
  }
  // the camera's event filter (esvo_ts_filter_configure): hot-pixel mask ([H * W], non-zero = masked, copied; null: none), refractory
  // period and neighbour support in ns (0: that test is off); from then on every call above stages only the events it keeps
  void setEventFilter(uint64_t refractory_ns, uint64_t support_ns, const uint8_t* mask = nullptr) {
    esvo_event_filter_t f{};
    f.refractory_ns = refractory_ns; f.support_ns = support_ns; f.mask = mask;
    ctx_->check(esvo_ts_filter_configure(ctx_->handle(), cam_, &f), "esvo_ts_filter_configure");
  }
  void clearEventFilter() { ctx_->check(esvo_ts_filter_configure(ctx_->handle(), cam_, nullptr), "esvo_ts_filter_configure"); }
  esvo_event_filter_counts_t eventFilterStats() {
    esvo_event_filter_counts_t c{};
    ctx_->check(esvo_ts_filter_stats(ctx_->handle(), cam_, &c), "esvo_ts_filter_stats");
    return c;
  }
  // get_last / set_last: [H * W] ns stamps, either may be null (esvo_ts_filter_state)
  void eventFilterState(uint64_t* get_last, const uint64_t* set_last = nullptr) {
    ctx_->check(esvo_ts_filter_state(ctx_->handle(), cam_, get_last, set_last), "esvo_ts_filter_state");
  }
  // the burst stage of the camera's filter (esvo_ts_burst_configure): mode ESVO_BURST_TRAIL keeps the first event of every same-polarity
  // burst of a pixel, ESVO_BURST_STC_CUT_TRAIL the second, ESVO_BURST_STC_KEEP_TRAIL all but the first; burst_ns: the largest gap inside
  // a burst.  The filter must be set (setEventFilter(0, 0) passes everything: the stage alone)
  void setBurstFilter(uint32_t mode, uint64_t burst_ns) {
    esvo_event_burst_t b{};
    b.mode = mode; b.burst_ns = burst_ns;
    ctx_->check(esvo_ts_burst_configure(ctx_->handle(), cam_, &b), "esvo_ts_burst_configure");
  }
  void clearBurstFilter() { ctx_->check(esvo_ts_burst_configure(ctx_->handle(), cam_, nullptr), "esvo_ts_burst_configure"); }
  esvo_event_burst_counts_t burstFilterStats() {
    esvo_event_burst_counts_t c{};
    ctx_->check(esvo_ts_burst_stats(ctx_->handle(), cam_, &c), "esvo_ts_burst_stats");
    return c;
  }
  // get_* / set_*: [H * W] ns stamps and flag bytes (bit 0 polarity, bit 1 linked); the get pair may be null, the set pair goes together
  void burstFilterState(uint64_t* get_stamp, uint8_t* get_flags, const uint64_t* set_stamp = nullptr, const uint8_t* set_flags = nullptr) {
    ctx_->check(esvo_ts_burst_state(ctx_->handle(), cam_, get_stamp, get_flags, set_stamp, set_flags), "esvo_ts_burst_state");
  }
  // the camera's event survey (esvo_ts_survey_begin): per-pixel counts of every packet the calls above accept, kept on the device; the
  // filter must be set (setEventFilter(0, 0) passes everything).  count_only: packets are decoded and counted, nothing is staged
  void beginSurvey(bool count_only = false) {
    esvo_event_survey_t s{};
    s.flags = count_only ? ESVO_SURVEY_COUNT_ONLY : 0;
    ctx_->check(esvo_ts_survey_begin(ctx_->handle(), cam_, &s), "esvo_ts_survey_begin");
  }
  void endSurvey() { ctx_->check(esvo_ts_survey_end(ctx_->handle(), cam_), "esvo_ts_survey_end"); }
  esvo_event_survey_stats_t surveyStats() {
    esvo_event_survey_stats_t s{};
    ctx_->check(esvo_ts_survey_stats(ctx_->handle(), cam_, &s), "esvo_ts_survey_stats");
    return s;
  }
  // the hot-pixel rule on the survey's counts (esvo_ts_survey_mask): mask_out ([H * W], 0 / 1) may be null; install: ESVO_MASK_KEEP,
  // ESVO_MASK_REPLACE or ESVO_MASK_UNION puts the mask into the camera's filter, device to device
  esvo_hot_pixel_report_t learnHotPixelMask(const esvo_hot_pixel_rule_t& rule, uint8_t* mask_out = nullptr, int install = ESVO_MASK_REPLACE) {
    esvo_hot_pixel_report_t r{};
    ctx_->check(esvo_ts_survey_mask(ctx_->handle(), cam_, &rule, mask_out, install, &r), "esvo_ts_survey_mask");
    return r;
  }
  // TimeSurface::createTimeSurfaceAtTime: the rectified mono8 Time Surface at the sync time
  void createTimeSurfaceAtTime(uint64_t external_sync_time_ns, uint8_t* out_mono8 /*nullable*/) {
    ctx_->check(esvo_ts_render(ctx_->handle(), cam_, external_sync_time_ns, out_mono8), "esvo_ts_render");
  }

 private:
  ContextPtr ctx_;
  int cam_;
};

// TS_history_ of the mapper and tracker nodes (std::map<ros::Time, TimeSurfaceObservation>, TS_HISTORY_LENGTH pairs) kept on
// the device: every frame createTimeSurfaceAtTime renders is retained under its stamp; DepthFusion::setObservationAt and
// RegProblemLM::setCurrentAt pick theirs by stamp.  One per Context.
class TimeSurfaceHistory {
 public:
  // pose(t_ns, T_world_cam) -> whether a pose is known at that stamp (getPoseAt)
  using PoseLookup = std::function<bool(uint64_t, double*)>;
  explicit TimeSurfaceHistory(ContextPtr ctx) : ctx_(std::move(ctx)) {}
  // TS_HISTORY_LENGTH pairs are retained from here on; 0 switches the history off.  Empties it.
  void configure(size_t TS_HISTORY_LENGTH) {
    ctx_->check(esvo_ts_history_configure(ctx_->handle(), TS_HISTORY_LENGTH), "esvo_ts_history_configure");
  }
  // the retained stamps, ascending; cams (nullable): bit 0 left present, bit 1 right present
  std::vector<uint64_t> stamps(std::vector<uint8_t>* cams = nullptr) const {
    size_t n = 0;
    ctx_->check(esvo_ts_history_list(ctx_->handle(), nullptr, nullptr, 0, &n), "esvo_ts_history_list");
    std::vector<uint64_t> t(n);
    std::vector<uint8_t> c(n);
    if (n) ctx_->check(esvo_ts_history_list(ctx_->handle(), t.data(), c.data(), n, &n), "esvo_ts_history_list");
    t.resize(n); c.resize(n);
    if (cams) *cams = c;
    return t;
  }
  void get(uint64_t t_ns, int cam, std::vector<uint8_t>& mono8) const {
    mono8.resize((size_t)ctx_->width() * ctx_->height());
    ctx_->check(esvo_ts_history_get(ctx_->handle(), t_ns, cam, mono8.data()), "esvo_ts_history_get");
  }
  // timeSurfaceCallback's emplace for a Time-Surface node in another process (esvo_Mapping.cpp:737-761)
  void put(uint64_t t_ns, int cam, const uint8_t* mono8) {
    ctx_->check(esvo_ts_history_put(ctx_->handle(), t_ns, cam, mono8), "esvo_ts_history_put");
  }
  // dataTransferring's choice of TS_obs_ (esvo_Mapping.cpp:497-534) among the retained complete pairs: false where the node
  // returns false; otherwise obs.t_ns and obs.T_world_cam are filled in (TS_left / TS_right stay null: the frames are on the
  // device, DepthFusion::setObservationAt takes them).  initialization: ESVO_System_Status_ == "INITIALIZATION".
  bool selectObservation(bool initialization, const PoseLookup& pose, StampedTimeSurfaceObs& obs) const {
    struct Tramp {
      static int call(void* user, uint64_t t_ns, double T[16]) { return (*static_cast<const PoseLookup*>(user))(t_ns, T) ? 1 : 0; }
    };
    const bool have = static_cast<bool>(pose);
    if (!initialization && !have) throw Error(ESVO_ERR_INVALID_ARG, "selectObservation: no pose lookup");
    uint64_t t = 0;
    double T[16];
    const int rc = esvo_ts_history_select_observation(ctx_->handle(), initialization ? 1 : 0, have ? &Tramp::call : nullptr,
                                                      const_cast<PoseLookup*>(&pose), &t, T);
    if (rc == ESVO_AGAIN) return false;
    ctx_->check(rc, "esvo_ts_history_select_observation");
    obs.t_ns = t;
    obs.TS_left = obs.TS_right = nullptr;
    std::copy(T, T + 16, obs.T_world_cam);
    return true;
  }

 private:
  ContextPtr ctx_;
};

// esvo_core::core::EventBM
class EventBM {
 public:
  explicit EventBM(ContextPtr ctx) : ctx_(std::move(ctx)) {}
  void resetParameters(size_t patch_size_X, size_t patch_size_Y, size_t min_disparity, size_t max_disparity, size_t step,
                       double ZNCC_Threshold, bool bUpDownConfiguration) {
    esvo_params_t p = ctx_->params();
    p.patch_size_x = (int32_t)patch_size_X; p.patch_size_y = (int32_t)patch_size_Y;
    p.bm_min_disparity = (int32_t)min_disparity; p.bm_max_disparity = (int32_t)max_disparity;
    p.bm_step = (int32_t)step; p.bm_zncc_threshold = ZNCC_Threshold; p.bm_updown = bUpDownConfiguration;
    ctx_->setParams(p);
  }
  void createMatchProblem(const StampedTimeSurfaceObs* pStampedTsObs, const StampTransformationMap* pSt_map,
                          const std::vector<Event>* pvEvents) {
    obs_ = pStampedTsObs; st_map_ = pSt_map; events_ = pvEvents;
    ctx_->check(esvo_map_set_observation(ctx_->handle(), obs_->t_ns, obs_->TS_left, obs_->TS_right, obs_->T_world_cam),
                "esvo_map_set_observation");
  }
  void match_all_HyperThread(std::vector<EventMatchPair>& vEMP) {
    vEMP.resize(events_->size());
    size_t n = 0;
    ctx_->check(esvo_map_match(ctx_->handle(), events_->data(), events_->size(), st_map_->stamps_ns.data(),
                               st_map_->T_world_virtual.data(), st_map_->size(), vEMP.data(), vEMP.size(), &n),
                "esvo_map_match");
    vEMP.resize(n);
  }

 private:
  ContextPtr ctx_;
  const StampedTimeSurfaceObs* obs_ = nullptr;
  const StampTransformationMap* st_map_ = nullptr;
  const std::vector<Event>* events_ = nullptr;
};

// esvo_core::core::EventSlice (EventMatcher.h:17-28): indices into the left event vector instead of iterators; the slice
// covers numEvents events from begin, transf is its row-major T_world pose
struct EventSlice {
  size_t begin = 0, numEvents = 0;
  uint64_t t_median_ns = 0;
  double transf[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
};

// esvo_core::core::EventMatcher (EventMatcher.cpp), the [26] matcher of esvo_MVStereo modes 0 and 2, over esvo_map_match_em.
// patch_size_X / patch_size_Y and NUM_THREAD_MAPPING are the handle's esvo_params_t (patch_size_x/_y, num_threads);
// patch_intensity_threshold and patch_valid_ratio are kept, as the reference keeps them, and never read.
class EventMatcher {
 public:
  explicit EventMatcher(ContextPtr ctx, double Time_THRESHOLD = 10e-5, double EPIPOLAR_THRESHOLD = 0.5, double TS_NCC_THRESHOLD = 0.1,
                        size_t patch_intensity_threshold = 125, double patch_valid_ratio = 0.1)
      : ctx_(std::move(ctx)) {
    resetParameters(Time_THRESHOLD, EPIPOLAR_THRESHOLD, TS_NCC_THRESHOLD, patch_intensity_threshold, patch_valid_ratio);
  }
  void resetParameters(double Time_THRESHOLD, double EPIPOLAR_THRESHOLD, double TS_NCC_THRESHOLD, size_t patch_intensity_threshold,
                       double patch_valid_ratio) {
    em_.time_threshold = Time_THRESHOLD;
    em_.epipolar_threshold = EPIPOLAR_THRESHOLD;
    em_.ncc_threshold = TS_NCC_THRESHOLD;
    em_.patch_intensity_threshold = (int32_t)patch_intensity_threshold;
    em_.patch_valid_ratio = patch_valid_ratio;
  }
  const esvo_em_params_t& params() const { return em_; }
  // vEventPtr_left: the events the slices index (vEventsPtr_left_); vEventPtr_cand: the right selection (vEventsPtr_right_)
  void createMatchProblem(const StampedTimeSurfaceObs* pTS_obs, const std::vector<EventSlice>* vEventSlice_ptr,
                          const std::vector<Event>* vEventPtr_left, const std::vector<Event>* vEventPtr_cand) {
    slices_ = vEventSlice_ptr; left_ = vEventPtr_left; cand_ = vEventPtr_cand;
    ctx_->check(esvo_map_set_observation(ctx_->handle(), pTS_obs->t_ns, pTS_obs->TS_left, pTS_obs->TS_right, pTS_obs->T_world_cam),
                "esvo_map_set_observation");
  }
  void match_all_HyperThread(std::vector<EventMatchPair>& vEMP) {
    const size_t ns = slices_->size();
    std::vector<uint32_t> begin(ns), count(ns);
    std::vector<double> T(16 * ns);
    size_t total = 0;
    for (size_t s = 0; s < ns; ++s) {
      begin[s] = (uint32_t)(*slices_)[s].begin;
      count[s] = (uint32_t)(*slices_)[s].numEvents;
      std::copy((*slices_)[s].transf, (*slices_)[s].transf + 16, T.begin() + 16 * s);
      total += count[s];
    }
    vEMP.resize(total);
    size_t n = 0;
    ctx_->check(esvo_map_match_em(ctx_->handle(), &em_, left_->data(), left_->size(), begin.data(), count.data(), T.data(), ns,
                                  cand_->data(), cand_->size(), vEMP.data(), vEMP.size(), &n),
                "esvo_map_match_em");
    vEMP.resize(n);
  }

 private:
  ContextPtr ctx_;
  esvo_em_params_t em_{1e-3, 10e-5, 0.5, 0.1, 3000, 125, 0.1};
  const std::vector<EventSlice>* slices_ = nullptr;
  const std::vector<Event>* left_ = nullptr;
  const std::vector<Event>* cand_ = nullptr;
};

// esvo_core::core::DepthProblemSolver (NUMERICAL problem type, Tdist norm)
class DepthProblemSolver {
 public:
  explicit DepthProblemSolver(ContextPtr ctx) : ctx_(std::move(ctx)) {}
  void solve(const std::vector<EventMatchPair>* pvEMP, const StampedTimeSurfaceObs* /*the observation set by EventBM*/,
             std::vector<DepthPoint>& vdp) {
    vdp.resize(pvEMP->size());
    size_t n = 0;
    ctx_->check(esvo_map_refine(ctx_->handle(), pvEMP->data(), pvEMP->size(), /*cull*/ 0, vdp.data(), vdp.size(), &n),
                "esvo_map_refine");
    vdp.resize(n);
  }
  // DepthProblemSolver::pointCulling (DepthProblemSolver.cpp:216-244): a stable host-side filter
  static void pointCulling(std::vector<DepthPoint>& vdp, double std_variance_threshold, double cost_threshold,
                           double invDepth_min_range, double invDepth_max_range) {
    std::vector<DepthPoint> kept;
    kept.reserve(vdp.size());
    for (const DepthPoint& d : vdp)
      if (d.variance <= std::pow(std_variance_threshold, 2) && d.residual <= cost_threshold && d.inv_depth > -1e-6 &&
          d.inv_depth >= invDepth_min_range && d.inv_depth <= invDepth_max_range)
        kept.push_back(d);
    vdp.swap(kept);
  }

 private:
  ContextPtr ctx_;
};

// The fusion stage of MappingAtTime (esvo_Mapping.cpp:341-395): dqvDepthPoints_.push_back(vdp) + window
// policy, then DepthFusion::update over the window (newest -> oldest) on a fresh DepthFrame,
// DepthMap::clean and DepthRegularization::apply.
class DepthFusion {
 public:
  explicit DepthFusion(ContextPtr ctx) : ctx_(std::move(ctx)) {}
  void pushFrame(const std::vector<DepthPoint>& vdp, const StampTransformationMap& st_map) {
    ctx_->check(esvo_map_push_frame(ctx_->handle(), vdp.data(), vdp.size(), st_map.T_world_virtual.data(), st_map.size()),
                "esvo_map_push_frame");
  }
  // esvo_MVStereo's PURE_BLOCK_MATCHING branch (esvo_MVStereo.cpp:411-423): vEMP2vDP, the window of maxNumFusionFrames_ frames
  // and DepthFusion::naive_propagation of every frame -- on the matches of EventBM::match_all_HyperThread
  void naivePropagation(const std::vector<EventMatchPair>& vEMP, const StampTransformationMap& st_map) {
    ctx_->check(esvo_map_fuse_matches_naive(ctx_->handle(), vEMP.data(), vEMP.size(), st_map.T_world_virtual.data(), st_map.size()),
                "esvo_map_fuse_matches_naive");
  }
  // esvo_MVStereo's PURE_SEMI_GLOBAL_MATCHING branch behind sgbm_->compute (esvo_MVStereo.cpp:320-361): createEdgeMask + the
  // DepthPoint loop on vEventsPtr_left_SGM_, the window of maxNumFusionFrames_ frames and naive_propagation of every frame, at the
  // observation set last.  dispMap: the W*H disparity x 16 image (CV_16S), or nullptr for the device's last SGM result.
  // Returns the number of points of the new frame.
  size_t pushDisparityFrame(const int16_t* dispMap, const std::vector<Event>& vEventsSGM) {
    size_t n = 0;
    ctx_->check(esvo_map_push_disparity_frame(ctx_->handle(), dispMap, vEventsSGM.data(), vEventsSGM.size(), &n),
                "esvo_map_push_disparity_frame");
    return n;
  }
  // TS_obs_ = the retained pair of that stamp (TimeSurfaceHistory; esvo_Mapping.cpp:512-519): what EventBM::createMatchProblem
  // does with the host images of the pair, without the images leaving the device
  void setObservationAt(uint64_t t_ns, const double T_world_cam[16]) {
    ctx_->check(esvo_map_set_observation_at(ctx_->handle(), t_ns, T_world_cam), "esvo_map_set_observation_at");
  }
  // returns numFusionCount
  size_t update() {
    size_t n = 0;
    ctx_->check(esvo_map_fuse(ctx_->handle(), &n), "esvo_map_fuse");
    return n;
  }
  // DepthMap iteration (SmartGrid::begin()/end()) in the reference's list order
  void getDepthMap(std::vector<DepthPoint>& out) {
    out.resize((size_t)ctx_->width() * ctx_->height());
    size_t n = 0;
    ctx_->check(esvo_map_get_depth_points(ctx_->handle(), out.data(), out.size(), &n), "esvo_map_get_depth_points");
    out.resize(n);
  }
  // publishPointCloud's payload (esvo_Mapping.cpp:925-932): float32 xyz in the world frame
  void getPointCloud(std::vector<float>& xyz) {
    xyz.resize((size_t)ctx_->width() * ctx_->height() * 3);
    size_t n = 0;
    ctx_->check(esvo_map_get_pointcloud_xyz(ctx_->handle(), xyz.data(), xyz.size() / 3, &n), "esvo_map_get_pointcloud_xyz");
    xyz.resize(n * 3);
  }
  // the same cloud built and KEPT on the device (esvo_map_cloud_build): returns its point count; RegProblemLM::setProblemFromMap
  // registers against it, getDevicePointCloud copies it out (12 B per point)
  size_t buildPointCloud() {
    size_t n = 0;
    ctx_->check(esvo_map_cloud_build(ctx_->handle(), &n), "esvo_map_cloud_build");
    return n;
  }
  void getDevicePointCloud(std::vector<float>& xyz) {
    size_t n = 0;
    ctx_->check(esvo_map_cloud_get(ctx_->handle(), nullptr, 0, &n), "esvo_map_cloud_get");
    xyz.resize(n * 3);
    ctx_->check(esvo_map_cloud_get(ctx_->handle(), xyz.data(), n, &n), "esvo_map_cloud_get");
  }

 private:
  ContextPtr ctx_;
};

// pc_global_ of the mapper node (publishPointCloud's global-cloud branch, esvo_Mapping.cpp:955-977), accumulated on the device:
// construct once (the node's `if (bVisualizeGlobalPC_) reserve`, :148-153), call update(t) where the node enters the branch,
// get() for the message.  nearCloud is pc_near_ (:925-932) by itself.
class GlobalPointCloud {
 public:
  GlobalPointCloud(ContextPtr ctx, double visualize_range = 2.5, double visualizeGPC_interval = 3, size_t numAddedPC_threshold = 1000,
                   size_t capacity_points = 0, float leaf = 0.3f)
      : ctx_(std::move(ctx)) {
    esvo_gpc_params_t p{};
    p.visualize_range = visualize_range;
    p.interval_s = visualizeGPC_interval;
    p.num_added_per_refresh = numAddedPC_threshold;
    p.capacity_points = capacity_points;
    p.leaf = leaf;
    ctx_->check(esvo_map_gpc_configure(ctx_->handle(), &p), "esvo_map_gpc_configure");
  }
  // true when the interval let the refresh through (t_last_pub_pc_ = t.toSec() then)
  bool update(uint64_t t_ns) {
    int refreshed = 0;
    ctx_->check(esvo_map_gpc_update(ctx_->handle(), t_ns, &refreshed), "esvo_map_gpc_update");
    return refreshed != 0;
  }
  void get(std::vector<float>& xyz) {
    size_t n = 0;
    ctx_->check(esvo_map_gpc_get(ctx_->handle(), nullptr, 0, &n), "esvo_map_gpc_get");
    xyz.resize(n * 3);
    ctx_->check(esvo_map_gpc_get(ctx_->handle(), xyz.data(), n, &n), "esvo_map_gpc_get");
  }
  size_t size() {
    size_t n = 0;
    ctx_->check(esvo_map_gpc_get(ctx_->handle(), nullptr, 0, &n), "esvo_map_gpc_get");
    return n;
  }
  esvo_gpc_stats_t stats() {
    esvo_gpc_stats_t st{};
    ctx_->check(esvo_map_gpc_stats(ctx_->handle(), &st), "esvo_map_gpc_stats");
    return st;
  }
  void nearCloud(double visualize_range, std::vector<float>& xyz) {
    xyz.resize((size_t)ctx_->width() * ctx_->height() * 3);
    size_t n = 0;
    ctx_->check(esvo_map_cloud_near(ctx_->handle(), visualize_range, xyz.data(), xyz.size() / 3, &n), "esvo_map_cloud_near");
    xyz.resize(n * 3);
  }

 private:
  ContextPtr ctx_;
};

// esvo_Mapping::createDenoisingMask + extractDenoisedEvents (esvo_Mapping.cpp:1046-1072) for the stage-wise
// path (esvo_map_tick applies them itself when params.denoising is set): binary map of the selected events
// at their RAW pixels -> 3x3 median (BORDER_REPLICATE) -> keep the events whose pixel is 255, in order.
inline void extractDenoisedEvents(const std::vector<Event>& vCloseEvents, std::vector<Event>& vEdgeEvents, int width, int height,
                                  size_t maxNum) {
  std::vector<uint8_t> map((size_t)width * height, 0);
  for (const Event& e : vCloseEvents)
    if (e.x < width && e.y < height) map[(size_t)e.y * width + e.x] = 1;
  vEdgeEvents.clear();
  for (const Event& e : vCloseEvents) {
    if (vEdgeEvents.size() >= maxNum) break;
    if (e.x >= width || e.y >= height) continue;
    int cnt = 0;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = std::min(std::max((int)e.y + dy, 0), height - 1), xx = std::min(std::max((int)e.x + dx, 0), width - 1);
        cnt += map[(size_t)yy * width + xx];
      }
    if (cnt >= 5) vEdgeEvents.push_back(e);
  }
}

// esvo_Mapping::MappingAtTime on device-resident events / Time Surfaces (the fused path)
inline void MappingAtTime(Context& ctx, const StampedTimeSurfaceObs& obs, const StampTransformationMap& st_map) {
  ctx.check(esvo_map_set_observation(ctx.handle(), obs.t_ns, obs.TS_left, obs.TS_right, obs.T_world_cam),
            "esvo_map_set_observation");
  ctx.check(esvo_map_tick(ctx.handle(), obs.t_ns, st_map.stamps_ns.data(), st_map.T_world_virtual.data(), st_map.size()),
            "esvo_map_tick");
}

// esvo_MVStereo::MappingAtTime in MVStereoMode 1, PURE_BLOCK_MATCHING (esvo_MVStereo.cpp:383-432): block matching, vEMP2vDP and
// naive_propagation of the window instead of refinement and fusion
inline void MappingAtTimePureBlockMatching(Context& ctx, const StampedTimeSurfaceObs& obs, const StampTransformationMap& st_map) {
  ctx.check(esvo_map_set_observation(ctx.handle(), obs.t_ns, obs.TS_left, obs.TS_right, obs.T_world_cam),
            "esvo_map_set_observation");
  ctx.check(esvo_map_tick_bm_only(ctx.handle(), obs.t_ns, st_map.stamps_ns.data(), st_map.T_world_virtual.data(), st_map.size()),
            "esvo_map_tick_bm_only");
}

// esvo_MVStereo::MappingAtTime in MVStereoMode 4, PURE_SEMI_GLOBAL_MATCHING (esvo_MVStereo.cpp:311-376): StereoSGBM on the
// observation's Time-Surface pair (obs.TS_left / TS_right: host images, or nullptr for the device-resident frames), the mode's
// DepthPoints on the staged events and naive_propagation of the window.  Returns the number of points of the new frame.
inline size_t MappingAtTimeSemiGlobalMatching(Context& ctx, const StampedTimeSurfaceObs& obs) {
  ctx.check(esvo_map_set_observation(ctx.handle(), obs.t_ns, obs.TS_left, obs.TS_right, obs.T_world_cam),
            "esvo_map_set_observation");
  size_t n = 0;
  ctx.check(esvo_map_tick_sgm(ctx.handle(), obs.TS_left, obs.TS_right, &n, nullptr), "esvo_map_tick_sgm");
  return n;
}

// ---- the tracker's optimiser: host C++ over the device's normal equations ----------------------------------------------------
// The pieces of a step (ESVO_HD) are compiled for the device as well: track_solve_kernel (esvo_track_solve, on_device = 1) runs
// the same expressions in the same order inside one launch, and returns the host loop's bits.
#if defined(__HIPCC__)
#define ESVO_HD __host__ __device__
#define ESVO_UNROLL _Pragma("unroll")
#else
#define ESVO_HD
#define ESVO_UNROLL
#endif
// tools::cayley2rot (esvo_core/src/tools/cayley.cpp), row-major
ESVO_HD inline void cayley2rot(const double c[3], double R[9]) {
  const double c0 = c[0], c1 = c[1], c2 = c[2];
  const double s = 1.0 + ((c0 * c0 + c1 * c1) + c2 * c2);
  const double M[9] = {1 + c0 * c0 - c1 * c1 - c2 * c2, 2 * (c0 * c1 - c2), 2 * (c0 * c2 + c1),
                       2 * (c0 * c1 + c2), 1 - c0 * c0 + c1 * c1 - c2 * c2, 2 * (c1 * c2 - c0),
                       2 * (c0 * c2 - c1), 2 * (c1 * c2 + c0), 1 - c0 * c0 - c1 * c1 + c2 * c2};
  for (int i = 0; i < 9; ++i) R[i] = M[i] / s;
}
// U V^T of the SVD of a (nearly orthonormal) 3x3 matrix = its orthogonal polar factor -- what addMotionUpdate's JacobiSVD
// re-orthonormalisation (RegProblemLM.cpp:355-357) returns; Newton's iteration X <- (X + X^-T) / 2 converges quadratically
ESVO_HD inline void orthonormalize3(double X[9]) {
  for (int it = 0; it < 20; ++it) {
    const double* a = X;
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double c10 = a[2] * a[7] - a[1] * a[8], c11 = a[0] * a[8] - a[2] * a[6], c12 = a[1] * a[6] - a[0] * a[7];
    const double c20 = a[1] * a[5] - a[2] * a[4], c21 = a[2] * a[3] - a[0] * a[5], c22 = a[0] * a[4] - a[1] * a[3];
    const double det = (a[0] * c00 + a[1] * c01) + a[2] * c02;
    const double invT[9] = {c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det};  // X^-T
    double d = 0;
    for (int i = 0; i < 9; ++i) { const double n = 0.5 * (X[i] + invT[i]); d = std::max(d, std::fabs(n - X[i])); X[i] = n; }
    if (d < 1e-16) break;
  }
}
// solves A x = rhs (6 x 6, row-major) by Gaussian elimination with partial pivoting; false if singular.  Every index is a
// loop counter (the pivot row is found and swapped by comparing counters, not by indexing with it), so that the device
// compiler, with the loops unrolled, keeps the 6 x 7 tableau in registers.
ESVO_HD inline bool solve6(const double A_in[36], const double rhs[6], double x[6]) {
  double A[6][7];
  ESVO_UNROLL
  for (int i = 0; i < 6; ++i) {
    ESVO_UNROLL
    for (int j = 0; j < 6; ++j) A[i][j] = A_in[i * 6 + j];
    A[i][6] = rhs[i];
  }
  ESVO_UNROLL
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    double pv = A[c][c];  // A[piv][c]
    ESVO_UNROLL
    for (int r = c + 1; r < 6; ++r) if (std::fabs(A[r][c]) > std::fabs(pv)) { piv = r; pv = A[r][c]; }
    if (pv == 0.0 || !std::isfinite(pv)) return false;
    ESVO_UNROLL
    for (int r = c + 1; r < 6; ++r)
      if (r == piv) {
        ESVO_UNROLL
        for (int j = 0; j < 7; ++j) { const double v = A[r][j]; A[r][j] = A[c][j]; A[c][j] = v; }
      }
    ESVO_UNROLL
    for (int r = c + 1; r < 6; ++r) {
      const double f = A[r][c] / A[c][c];
      ESVO_UNROLL
      for (int j = c; j < 7; ++j) A[r][j] -= f * A[c][j];
    }
  }
  ESVO_UNROLL
  for (int i = 5; i >= 0; --i) {
    double s = A[i][6];
    ESVO_UNROLL
    for (int j = i + 1; j < 6; ++j) s -= A[i][j] * x[j];
    x[i] = s / A[i][i];
  }
  return true;
}
// one trial of an iteration: (H + lam diag(H) + 1e-9 I) dx = -b, then addMotionUpdate's pose Rn = orth(cayley2rot(dx_c) R),
// tn = dx_t + cayley2rot(dx_c) t; false if the damped system is singular
ESVO_HD inline bool gn_trial_step(const double H[36], const double b[6], double lam, const double R[9], const double t[3], double dx[6],
                                  double Rn[9], double tn[3]) {
  double A[36], rhs[6];
  for (int i = 0; i < 36; ++i) A[i] = H[i];
  for (int i = 0; i < 6; ++i) { A[i * 6 + i] = (H[i * 6 + i] + lam * H[i * 6 + i]) + 1e-9; rhs[i] = -b[i]; }
  if (!solve6(A, rhs, dx)) return false;
  double dR[9];
  cayley2rot(dx, dR);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      Rn[r * 3 + c] = (dR[r * 3 + 0] * R[0 * 3 + c] + dR[r * 3 + 1] * R[1 * 3 + c]) + dR[r * 3 + 2] * R[2 * 3 + c];
  orthonormalize3(Rn);
  for (int r = 0; r < 3; ++r) tn[r] = dx[3 + r] + ((dR[r * 3 + 0] * t[0] + dR[r * 3 + 1] * t[1]) + dR[r * 3 + 2] * t[2]);
  return true;
}
// the reduction the linear model predicts for the step: |f|^2 - |f + J dx|^2 = -(2 b.dx + dx.H dx)
ESVO_HD inline double gn_predicted_reduction(const double H[36], const double b[6], const double dx[6]) {
  double pred = 0;
  for (int i = 0; i < 6; ++i) {
    double hd = 0;
    for (int j = 0; j < 6; ++j) hd += H[i * 6 + j] * dx[j];
    pred -= dx[i] * (2.0 * b[i] + hd);
  }
  return pred;
}
ESVO_HD inline bool gn_accept(double pred, double cost, double cost_t) { return pred > 0 && (cost - cost_t) >= 1e-4 * pred; }
ESVO_HD inline double gn_step_norm(const double dx[6]) {
  double nrm = 0;
  for (int i = 0; i < 6; ++i) nrm += dx[i] * dx[i];
  return std::sqrt(nrm);
}
struct Registration { double R[9]; double t[3]; double rms = 0; int iterations = 0; bool ok = true; };
// What a registration did, for a caller who asks (esvo_track_solve): one esvo_track_iter_t per outer iteration (at most `cap`;
// `offset` is the caller's to fill -- the batch schedule lives in its normal_eq) and the reason it stopped
// (esvo_track_solve_info_t::stop).  A recorder only: no value it stores feeds back into the loop.
struct RegistrationTrace {
  esvo_track_iter_t* rec = nullptr;
  size_t cap = 0;
  int stop = 0;
  void put(int it, double cost, double lambda, double step_norm, size_t n, int pick, int trials) {
    if (!rec || (size_t)it >= cap) return;
    esvo_track_iter_t& r = rec[it];
    r.cost = cost; r.lambda = lambda; r.step_norm = step_norm; r.n = (uint32_t)n; r.offset = 0; r.pick = pick; r.trials = trials;
  }
};
// Levenberg-damped Gauss-Newton on x = (Cayley parameters, translation), linearised at x = 0 in every iteration exactly as
// RegProblemSolverLM::solve_analytical does (RegProblemSolverLM.cpp:160-183: x.fill(0), minimizeInit, ONE minimizeOneStep,
// addMotionUpdate):
//   (H + lambda diag(H) + 1e-9 I) dx = -b,   R' = orth(cayley2rot(dx_c) R),   t' = dx_t + cayley2rot(dx_c) t
// Like Eigen's minimizeOneStep, a trial step is ACCEPTED only if it pays: the cost is evaluated at the trial pose (same
// batch) and the step taken iff actual reduction / predicted reduction >= 1e-4, with
//   predicted = |f|^2 - |f + J dx|^2 = -(2 b.dx + dx.H dx);
// otherwise the damping is raised tenfold and the step recomputed (up to 6 times) -- the driver never moves to a pose with
// a higher cost.  After an accepted step the damping is lowered tenfold (never below `damping`) and carried into the next
// iteration (Marquardt's schedule; Eigen's minimizeInit restarts its trust region at every outer iteration and spends functor
// evaluations shrinking it again -- on the Time Surface's piecewise-constant image the useful damping is 1 .. 10, three
// rejections away from 1e-3, every time).
// The trials lambda, 10 lambda, 100 lambda of an iteration are SPECULATIVE: all three poses go to `normal_eq` in one call
// (one kernel launch, one workgroup per pose, one read-back on the device) and the first acceptable one in that order is
// taken -- the result is that of trying them one after the other, at the latency of one evaluation.
// It stops after max_iterations, when an accepted step is shorter than 1e-6, or when no damping up to 1e5 x the current one
// yields an acceptable step (the state in which Eigen's trust radius has shrunk below xtol |x|: its status 2 / 3, on which
// the reference's loop breaks, :181-182).  Stated deviation (DESIGN.md "Deviations"): the step is Levenberg's diagonal
// damping, not MINPACK's lmpar trust-region solve, so single steps differ from Eigen's while the fixed point is the same
// (bounded against the reference's loop on recorded cases: tests/test_track_normal.py, tests/golden/ref_track_solve.npz).
// `normal_eq(it, k, R[k][9], t[k][3], H[k][36], b[k][6], cost[k], &n)` evaluates H = J^T J, b = J^T f, cost = |f|^2 at k poses
// (1 <= k <= 3) on the batch of outer iteration `it`: esvo_track_normal_equations_batch on the device, or the CPU oracle's
// restatement in the tests.  same_batch: the batch does not depend on `it`, so the evaluation at an accepted trial pose IS
// the next iteration's linearisation.  trace (optional): a recorder of what each iteration did (RegistrationTrace).
constexpr int kRegisterTrials = 3;
template <class NormalEq>
Registration gauss_newton_register(NormalEq&& normal_eq, const double R0[9], const double t0[3], int max_iterations = 12,
                                   double damping = 1e-3, bool same_batch = true, RegistrationTrace* trace = nullptr) {
  constexpr int K = kRegisterTrials;
  Registration g;
  RegistrationTrace none;
  RegistrationTrace& tr = trace ? *trace : none;
  tr.stop = 0;
  for (int i = 0; i < 9; ++i) g.R[i] = R0[i];
  for (int i = 0; i < 3; ++i) g.t[i] = t0[i];
  double H[36], b[6], cost = 0, lambda = damping;
  size_t n = 0;
  bool have = false;
  for (int it = 0; it < max_iterations; ++it) {
    if (!have && !normal_eq(it, 1, g.R, g.t, H, b, &cost, &n)) { g.ok = false; tr.stop = 3; return g; }
    have = false;
    g.iterations = it + 1;
    g.rms = n ? std::sqrt(cost / (double)n) : 0.0;
    const double cost_it = cost;
    const size_t n_it = n;
    double dx[K][6], Rn[K][9], tn[K][3], Ht[K][36], bt[K][6], cost_t[K];
    size_t nt = 0;
    int pick = -1, pick_at = -1, tried = 0;
    double lam_tried = lambda;  // the damping of the last system set up: the singular one, or the third of the round
    for (int round = 0; round < 2 && pick < 0; ++round) {  // dampings lambda 10^0..2, then lambda 10^3..5
      int k_eff = 0;
      double lam = lambda;
      for (int k = 0; k < K; ++k, lam *= 10.0) {
        lam_tried = lam;
        if (!gn_trial_step(H, b, lam, g.R, g.t, dx[k], Rn[k], tn[k])) break;
        k_eff = k + 1;
      }
      if (k_eff == 0 || !normal_eq(it, k_eff, &Rn[0][0], &tn[0][0], &Ht[0][0], &bt[0][0], cost_t, &nt)) {
        g.ok = false; tr.stop = 3; tr.put(it, cost_it, lam_tried, 0.0, n_it, -1, tried);
        return g;
      }
      lam = lambda;
      for (int k = 0; k < k_eff && pick < 0; ++k, lam *= 10.0) {
        const double pred = gn_predicted_reduction(H, b, dx[k]);
        ++tried;
        if (gn_accept(pred, cost, cost_t[k])) { pick = k; pick_at = round * K + k; lambda = lam; }
      }
      if (pick < 0) {
        if (k_eff < K) {  // a singular damped system among the trials, none before it acceptable
          g.ok = false; tr.stop = 3; tr.put(it, cost_it, lam_tried, 0.0, n_it, -1, tried);
          return g;
        }
        lambda = lam;  // = lambda x 10 x 10 x 10, the product a one-by-one loop arrives at
      }
    }
    if (pick < 0) {  // no step pays any more: (R, t) stays the last accepted pose
      tr.stop = 2; tr.put(it, cost_it, lam_tried, 0.0, n_it, -1, tried);
      break;
    }
    for (int i = 0; i < 9; ++i) g.R[i] = Rn[pick][i];
    for (int i = 0; i < 3; ++i) g.t[i] = tn[pick][i];
    const double lam_pick = lambda;
    lambda = lambda / 10.0 > damping ? lambda / 10.0 : damping;
    if (same_batch) {
      for (int i = 0; i < 36; ++i) H[i] = Ht[pick][i];
      for (int i = 0; i < 6; ++i) b[i] = bt[pick][i];
      cost = cost_t[pick]; n = nt; have = true;
      g.rms = n ? std::sqrt(cost / (double)n) : 0.0;
    }
    const double step = gn_step_norm(dx[pick]);
    tr.put(it, cost_it, lam_pick, step, n_it, pick_at, tried);
    if (step < 1e-6) { tr.stop = 1; break; }
  }
  return g;
}

// The stochastic swaps of RegProblemLM::setProblem (RegProblemLM.cpp:45-49) without the cloud: for i < n_take the reference swaps
// vPointXYZPtr_[i] with vPointXYZPtr_[i + rand() % (size - i)]; draws[i] is that rand() (it stays with the caller), and
// order[i] is the index -- in the cloud as it was before the swaps -- of the point that ends up at position i.  Only the
// positions the swaps touch are remembered (a sparse map over the identity): O(n_take) time and memory whatever n_cloud is.
// n_take > n_cloud is clamped (:39-40); order has room for min(n_take, n_cloud) indices.  Returns how many it wrote.
inline size_t stochastic_order(size_t n_cloud, size_t n_take, const uint32_t* draws, uint32_t* order) {
  if (n_take > n_cloud) n_take = n_cloud;
  std::unordered_map<size_t, uint32_t> moved;  // position -> what it holds, where that is not the position itself
  moved.reserve(2 * n_take);
  auto at = [&](size_t p) { const auto it = moved.find(p); return it == moved.end() ? (uint32_t)p : it->second; };
  for (size_t i = 0; i < n_take; ++i) {
    const size_t j = i + (size_t)draws[i] % (n_cloud - i);
    const uint32_t vi = at(i), vj = at(j);
    order[i] = vj;      // position i is final: every later swap touches positions > i only
    moved[j] = vi;
    moved.erase(i);
  }
  return n_take;
}

// esvo_core::core::RegProblemLM's evaluation side (esvo_core/src/core/RegProblemLM.cpp): the per-point loops of
// setProblem (:44-56), operator() (:91-136) and df (:178-269) on the device.  The 6-DoF LM driver, the Cayley update and
// the SVD re-orthonormalisation (getWarpingTransformation / addMotionUpdate, :328-364) stay with the caller, who passes
// the resulting 4x4 warp (for operator()) or R_, t_ (for df) in row-major doubles.
struct RegProblemConfig {       // the fields of RegProblemConfig the evaluation reads (cfg/tracking/*.yaml)
  int kernelSize = 5;
  bool huber = true;            // LSnorm: "Huber" | "l2"
  double huber_threshold = 50.0;
  size_t BATCH_SIZE = 300;
  size_t MAX_REGISTRATION_POINTS = 2000;
};
class RegProblemLM {
 public:
  RegProblemLM(ContextPtr ctx, const RegProblemConfig& cfg) : ctx_(std::move(ctx)), cfg_(cfg) {}
  // setProblem: ref's point cloud (already in the stochastic order of :48-49) + the current frame's left Time Surface
  // (nullptr = the device-resident one of the last createTimeSurfaceAtTime of the left camera)
  void setProblem(const float* ref_xyz_world, size_t n_points, const double T_world_ref[16], const uint8_t* cur_TS_left) {
    numPoints_ = std::min(n_points, cfg_.MAX_REGISTRATION_POINTS);
    ctx_->check(esvo_track_set_reference(ctx_->handle(), ref_xyz_world, numPoints_, T_world_ref), "esvo_track_set_reference");
    ctx_->check(esvo_track_set_current(ctx_->handle(), cur_TS_left, cfg_.kernelSize), "esvo_track_set_current");
    numBatches_ = std::max(numPoints_ / cfg_.BATCH_SIZE, (size_t)1);
    setStochasticSampling(0, numPoints_);
  }
  // setProblem on the mapper's device-resident cloud (DepthFusion::buildPointCloud, same Context): what the tracking node's
  // refDataTransferring + setProblem do with /esvo_mapping/pointcloud_local (esvo_Tracking.cpp:203-234, RegProblemLM.cpp:38-55)
  // without the cloud leaving the device.  draws[i]: the rand() of swap i (:49), n_draws >= min(cloud, MAX_REGISTRATION_POINTS)
  // of them; draws == nullptr: no swaps, the first points in list order.
  void setProblemFromMap(const uint32_t* draws, size_t n_draws, const double T_world_ref[16], size_t MAX_REGISTRATION_POINTS,
                         const uint8_t* cur_TS_left) {
    const float* d_xyz = nullptr;
    size_t n_cloud = 0;
    ctx_->check(esvo_map_cloud_device(ctx_->handle(), &d_xyz, &n_cloud, nullptr), "esvo_map_cloud_device");
    numPoints_ = std::min(n_cloud, MAX_REGISTRATION_POINTS);
    if (draws) {
      if (n_draws < numPoints_) throw Error(ESVO_ERR_INVALID_ARG, "setProblemFromMap: fewer draws than registration points");
      std::vector<uint32_t> order(numPoints_);
      stochastic_order(n_cloud, numPoints_, draws, order.data());
      ctx_->check(esvo_track_set_reference_from_cloud(ctx_->handle(), order.data(), numPoints_, T_world_ref), "esvo_track_set_reference_from_cloud");
    } else {
      ctx_->check(esvo_track_set_reference_from_cloud(ctx_->handle(), nullptr, numPoints_, T_world_ref), "esvo_track_set_reference_from_cloud");
    }
    ctx_->check(esvo_track_set_current(ctx_->handle(), cur_TS_left, cfg_.kernelSize), "esvo_track_set_current");
    numBatches_ = std::max(numPoints_ / cfg_.BATCH_SIZE, (size_t)1);
    setStochasticSampling(0, numPoints_);
  }
  // the current frame = the retained left Time Surface of that stamp (TimeSurfaceHistory; curDataTransferring's
  // TS_history_.rbegin(), esvo_Tracking.cpp:241-247): replaces the frame setProblem / setProblemFromMap set, keeps the reference
  void setCurrentAt(uint64_t t_ns) {
    ctx_->check(esvo_track_set_current_at(ctx_->handle(), t_ns, cfg_.kernelSize), "esvo_track_set_current_at");
  }
  void setStochasticSampling(size_t offset, size_t N) { offset_ = offset; count_ = N; }
  // operator(): fvec for the warp T_left_ref the caller derived from x; returns the number of values
  size_t operator()(const double T_left_ref[16], std::vector<double>& fvec) const {
    fvec.resize(count_);
    size_t n = 0;
    ctx_->check(esvo_track_residuals(ctx_->handle(), T_left_ref, offset_, count_, cfg_.huber ? ESVO_TRACK_HUBER : ESVO_TRACK_L2,
                                     cfg_.huber_threshold, fvec.data(), &n), "esvo_track_residuals");
    fvec.resize(n);
    return n;
  }
  // df at x = 0: fjac is n x 6, column-major (Eigen::MatrixXd layout)
  size_t df(const double R[9], const double t[3], std::vector<double>& fjac) const {
    fjac.resize(6 * count_);
    size_t n = 0;
    ctx_->check(esvo_track_jacobian(ctx_->handle(), R, t, offset_, count_, fjac.data(), &n), "esvo_track_jacobian");
    fjac.resize(6 * n);
    return n;
  }
  // F(0), df(0) and their products J^T J, J^T F, |F|^2 on the current batch in one device call
  size_t normalEquations(const double R[9], const double t[3], double H[36], double b[6], double* cost) const {
    size_t n = 0;
    ctx_->check(esvo_track_normal_equations(ctx_->handle(), R, t, offset_, count_, cfg_.huber ? ESVO_TRACK_HUBER : ESVO_TRACK_L2,
                                            cfg_.huber_threshold, H, b, cost, &n), "esvo_track_normal_equations");
    return n;
  }
  // ... at k poses (R: k x 9, t: k x 3, H: k x 36, b: k x 6, cost: k) in one launch
  size_t normalEquations(int k, const double* R, const double* t, double* H, double* b, double* cost) const {
    size_t n = 0;
    ctx_->check(esvo_track_normal_equations_batch(ctx_->handle(), k, R, t, offset_, count_, cfg_.huber ? ESVO_TRACK_HUBER : ESVO_TRACK_L2,
                                                  cfg_.huber_threshold, H, b, cost, &n), "esvo_track_normal_equations_batch");
    return n;
  }
  // RegProblemSolverLM::solve_analytical's loop (RegProblemSolverLM.cpp:148-215) with gauss_newton_register as the step:
  // the batch advances with the iteration as setStochasticSampling does there (:167-168)
  // on_device: the same loop, the same schedule and the same bits in ONE kernel launch (esvo_track_solve)
  Registration solve(const double R0[9], const double t0[3], int MAX_ITERATION = 12, double damping = 1e-3, bool on_device = false) {
    const bool batches = cfg_.BATCH_SIZE < numPoints_;
    if (on_device) {
      esvo_track_solve_params_t prm = {};
      prm.n_points = numPoints_; prm.batch_size = cfg_.BATCH_SIZE;
      prm.ls_norm = cfg_.huber ? ESVO_TRACK_HUBER : ESVO_TRACK_L2; prm.max_iterations = MAX_ITERATION; prm.on_device = 1;
      prm.huber_threshold = cfg_.huber_threshold; prm.damping = damping;
      Registration g;
      for (int i = 0; i < 9; ++i) g.R[i] = R0[i];
      for (int i = 0; i < 3; ++i) g.t[i] = t0[i];
      esvo_track_solve_info_t info;
      ctx_->check(esvo_track_solve(ctx_->handle(), &prm, g.R, g.t, &info, nullptr, 0), "esvo_track_solve");
      g.rms = info.rms; g.iterations = info.iterations; g.ok = info.ok != 0;
      return g;
    }
    auto ne = [&](int it, int k, const double* R, const double* t, double* H, double* b, double* cost, size_t* n) {
      if (batches) setStochasticSampling(((size_t)it % numBatches_) * cfg_.BATCH_SIZE, cfg_.BATCH_SIZE);
      *n = normalEquations(k, R, t, H, b, cost);
      return true;
    };
    return gauss_newton_register(ne, R0, t0, MAX_ITERATION, damping, !batches);
  }
  // the visualisation block of RegProblemSolverLM (RegProblemSolverLM.cpp:180-209): the bytes of Reproj_Map_Left (bgr8, H x W x 3)
  // for the registered motion (R, t); invDepth_*_range are the tracker's 1 / z_max_ and 1 / z_min_.  Returns the number of
  // points whose centre pixel is inside the image.
  size_t reprojectionMap(const double R[9], const double t[3], double invDepth_min_range, double invDepth_max_range, uint8_t* bgr,
                         size_t numVisualization = 2000) const {
    size_t n_inside = 0;
    ctx_->check(esvo_track_reprojection_map(ctx_->handle(), R, t, numVisualization, invDepth_min_range, invDepth_max_range, bgr, &n_inside),
                "esvo_track_reprojection_map");
    return n_inside;
  }
  size_t numBatches_ = 1, numPoints_ = 0;

 private:
  ContextPtr ctx_;
  RegProblemConfig cfg_;
  size_t offset_ = 0, count_ = 0;
};

}  // namespace esvo_hip
#endif  // ESVO_HIP_HPP
