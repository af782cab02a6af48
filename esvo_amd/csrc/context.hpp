// context.hpp — the state behind an esvo_handle and what the api_*.hip translation units share.
//
// One esvo_context owns every device buffer of one GPU: SAE + staged event rings (Time Surface), the observation pair,
// per-tick BM/LM scratch, the fusion window ring and the dense DepthMap.  It owns them through DevBuf / PinBuf members
// (devmem.hpp): a member that is a buffer is freed with the handle, a raw pointer member owns nothing (the views are listed
// together below) -- esvo_destroy has no list to keep.  Events are DevEvent members in the same way; only the streams stay raw
// handles, created and destroyed by esvo_create / esvo_destroy.  Two ticks are in flight: what one index of that machinery selects
// -- buffers, flags, stage events -- sits in one slot struct (front[fpar], back[par], pose[pose_buf]).  Each entry point replays, on
// the handle's HIP streams, the call sequence of the reference seam it replaces (cited in include/esvo_hip.h); nothing
// computes on the CPU except bookkeeping (time-stamp binary searches, window policy, output ordering).
//   api_core.hip   lifecycle, parameters, self-tests           api_ts.hip     Time-Surface render: scatter, queue mode
//   api_map.hip    mapper: stage launches, the tick pipeline   api_window.hip fusion window, back stage, map export
//   api_modes.hip  synchronous MVStereo modes 1 and 4, SGM     api_shard.hip  band mode: routed front, phases, configuration
//   api_out.hip    DepthMap / cloud / image outputs, stats     api_comm.hip   tick-interleaved multi-GPU exchange
//   api_em.hip     event-to-event matching (modes 0 and 2)     api_gpc.hip    the global point cloud
//   api_track.hip  tracker residual / Jacobian evaluation      api_bag.hip, api_dev.hip  bag reader, development hooks
//   api_history.hip  Time-Surface history: frames by stamp, the mapper's and the tracker's pick
//   api_ingest.hip, api_words.hip   event ingest (ingest.hpp: what the two share): records, EventArray messages, columns; EVT 2 / EVT 3 words
//   api_filter.hip, api_survey.hip  the ingest path's event filter; per-pixel counts of the pushed stream and the mask learnt from them
#pragma once
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "devmem.hpp"
#include "ring_spans.hpp"

using namespace esvo;

struct FrameRec {
  u32 off;    // offset in the window ring
  u32 count;  // points
  u32 slot;   // pose-table slot (NO_SLOT for empty frames)
  u32 run;    // 1, or the number of consecutive EMPTY frames this record stands for: a frame without points adds
              // nothing to the fusion but counts as a frame of the window (esvo_Mapping.cpp:341-368,385), and a
              // sparse stretch under CONST_POINTS may queue any number of them
};
enum : u32 { NO_SLOT = 0xffffffffu };

// ---- SESSION STATE: the bookkeeping of what a handle has been fed since esvo_create or the last esvo_reset.  The rule: a member
// declared inside one of the *Session structs below is put back to its initial value by esvo_reset, by assignment of a fresh struct,
// and is never named there; a member declared anywhere else survives a reset.  One struct per lock that guards its members (esvo_reset
// holds them all); esvo_context derives from them, so a use site reads h->ring_base[cam] as ever.
struct IngestSession {  // under mu_ring: the event rings
  std::deque<u64> ts_host[2];   // time stamps of staged events [ring_base, ring_base + size)
  u64 ring_base[2] = {0, 0};    // absolute index of ts_host[cam].front()
  u64 ring_next[2] = {0, 0};    // absolute index of the next event to stage
  u64 ring_reserved[2] = {0, 0};  // >= ring_next: end of the block a pusher is copying right now (its slots are being
                                  // overwritten: selections are validated against THIS, not against ring_next)
  u64 scattered[2] = {0, 0};    // absolute index of the first event not yet in the SAE
  u64 scatter_pending_lo[2] = {~0ull, ~0ull};  // oldest event a possibly still running scatter kernel reads
  bool ingest_pending[2] = {false, false};     // esvo_context::evt_ingest of that camera stands for a copy nobody has awaited
  u64 sh_first = 0;             // the newest selection's first event
  u64 sh_first_prev = 0;        // the selection before it (two ticks may be in flight)
  // routed band mode: event selection stays GLOBAL (dataTransferring walks the whole left stream): every left stamp is kept on the
  // host, each kept event remembers its index in that sequence
  std::deque<u64> glob_ts;      // stamps of ALL left events [glob_base, glob_base + size)
  u64 glob_base = 0;
  std::deque<u64> kept_g;       // global index of each kept left event, aligned with ts_host[0]
  std::deque<u64> own_before;   // how many OWN events (floor(y_rect) in the band) were kept before this one: the count of a
  u64 own_total = 0;            //   selection's own events bounds its LM launch (the ring also holds the raster's halo events)
  u64 last_stamp[2] = {0, 0};   // newest stamp seen per camera (kept or not): the order check of the push calls
  // queue mode, out-of-order packets (api_ingest.hip, push_unsorted): the copies of the then-newest event that take a late event's place
  // in the per-pixel queues, inserted with the next batch
  std::vector<esvo_event_t> tsq_dup[2];
  // EVT 3.0 ingest (esvo_ts_push_evt3): the decoder state a camera's stream is in, and the totals of its successful calls -- under
  // that camera's mu_push, not mu_ring
  esvo_evt3_state_t evt3_state[2] = {};
  esvo_evt3_counts_t evt3_totals[2] = {};
  // the same of EVT 2.0 / 2.1 ingest (esvo_ts_push_evt2): one state serves the three formats
  esvo_evt2_state_t evt2_state[2] = {};
  esvo_evt2_counts_t evt2_totals[2] = {};
  // the event filter (esvo_ts_filter_configure): the totals of a camera's successful pushes, under its mu_push.  (The `last` image
  // is device memory: esvo_reset zeroes it beside the other session buffers, EventFilter below.)
  esvo_event_filter_counts_t flt_totals[2] = {};
  // the filter's burst stage (esvo_ts_burst_configure): the same of its totals (the state images: EventBurst below)
  esvo_event_burst_counts_t bst_totals[2] = {};
  // the event survey (esvo_ts_survey_begin), under the camera's mu_push: what the host knows of an open survey without a read-back --
  // events of its accepted packets (events_in + outside of its stats: the bound that keeps every counter below 2^32) and the packets.
  // (The counts are device memory: esvo_reset zeroes them beside the other session buffers, EventSurvey below.)
  u64 srv_events[2] = {0, 0}, srv_packets[2] = {0, 0};
};
struct TsSession {  // under mu_ts (the right camera's flag: mapper group only)
  bool ts_valid[2] = {false, false};  // d_ts[cam] holds a render
  bool trk_read_pending = false;      // evt_trk_read stands for a tracker read of d_ts[0] the next render has to wait for
};
struct SchedSession {  // mapper group (mu_api): what the scheduling policies have learnt -- results do not depend on any of it
  float ema_lm_ms = 0.f, ema_back_ms = 0.f;  // the second LM queue (esvo_context::lm_queues): smoothed stage timings, the decision
  bool lm_two_on = false;
  // the pipeline's way back from its slow operating point (api_map.hip, pipeline_resync)
  struct Resync { double last_ms = 0; float period_ema = 0, period_before = 0; u32 streak = 0, cooldown = 0, check_in = 0; bool lm_wait_back = false; } resync;
  // pair layout of the LM kernel (esvo_context::lm_pair_forced): the last four launch times per layout, their count, the decisions
  float lm_pair_ms[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  u32 lm_pair_n[2] = {0u, 0u};
  u32 lm_pair_decisions = 0;
  int lm_pair_current = -1;     // the layout the policy settled on (-1: still exploring)
};
struct MapSession {  // mapper group (mu_api): observation, window, DepthMap, what is still to be collected
  bool obs_set = false;
  u32 n_pose = 0;
  std::deque<FrameRec> frames;  // the fusion window, oldest first
  size_t n_window_frames = 0;   // frames of the window as the reference counts them (empty ones included)
  u32 map_id_bound = 0;         // creation ids of d_map_cur are below this: what the fusion that built it numbered (run_fuse:
                                // points x records per point; esvo_map_init_sgm: 4 x points).  Recorded where the ids are
                                // assigned: the window may shrink afterwards without a fusion (esvo_map_push_frame).
  u64 committed_t_ns = 0;       // stamp of the newest tick whose back stage is enqueued (0: none)
  bool stats_pending = false;   // the last tick's counters / timings have not been read back yet
  bool back_pending[2] = {false, false};  // back-stage timings / counters of that parity not collected yet
  bool ts_timing_pending[2] = {false, false};
  bool ts_pair_sample = false;  // the pending sample of camera 0 covers both cameras (pair render)
  bool halo_error = false;      // routed band mode, sticky until a reset: ticks are refused with ESVO_ERR_HALO
  bool dn_pending = false;      // Denoising on a routed handle: phase 0 returned ESVO_AGAIN, the mask bits are being exchanged
  bool sgm_disp_valid = false;  // the per-tick SGM mode (esvo_map_tick_sgm / esvo_map_push_disparity_frame): d_sgm_disp holds an image
  esvo_sgm_stats_t sgm_stats = {};
  esvo_lm_stats_t lm_stats = {};  // the scale-loop guard (esvo_map_lm_stats): the last launch's counts and the running totals
};
struct CloudSession {  // under mu_cloud: the device-resident point cloud (esvo_context::d_cloud_xyz)
  int cloud_cur = -1;           // the buffer that holds the snapshot (-1: none -- before the first build, after a reset)
  size_t cloud_n = 0;
  u64 cloud_t_ns = 0;           // committed_t_ns at the build
  bool cloud_read_pending[2] = {false, false};
};

// A tick's state between its phases.  Unsharded ticks are finished lazily: esvo_map_tick(k) enqueues the front
// stage of tick k and only then completes tick k-1 (point count -> window policy -> back stage), so the host
// never waits on the front stream while it still has work to enqueue there.
struct TickState {
  u32 n = 0, off = 0, points = 0, n_pose = 0;
  u32 n_loc = 0;                    // routed band mode: events of the selection in this rank's ring (n stays the global count)
  u32 n_own = 0;                    //   ... of which the rank owns (block-matches and refines) this many
  u32 g_first = 0;                  //   global index (low 32 bits) of the selection's newest event
  u32 max_kept = 0;                 // sharded: largest kept count among the ranks (block length of exchange 2)
  int pose_buf = 0;
  u64 t_ns = 0;
  double T_world_obs[16];
  hipStream_t lm_stream = nullptr;  // where the tick's LM launch was enqueued
  hipStream_t cnt_stream = nullptr; // where its frame (point compaction) and counters follow: the same, or the idle second LM queue
  int obs_par = 0;                  // which observation pair it reads
  int lm_pair = -1;                 // LM layout of the tick: 1 pair, 0 wide, -1 not a candidate (policy feedback)
  bool lat = false;                 // enqueued in latency mode: LM in the front queue, polled waits
  bool timed = true;                // its stage-timing events were recorded
  bool lm_two = false;              // its LM launch alternates between the two LM queues
  bool host_row_sent = false;        // latency mode: its point compaction left the counter row in the pinned host row (no copy follows)
  bool gather = false;              // latency mode: its frame is still in the solver slots (flags + prefix): the back stage's first launch compacts it
  bool timed_lm = true;             // ... at least the two around the LM launch (the layout policy's feedback)
  bool lm_guard = false;            // its LM launch ran the scale-loop guard: the fold follows, the counter row holds CNT_LM_*
};

// ---- THE SLOTS: what one index of the two-ticks-in-flight machinery selects.  They sit outside the *Session structs, so all of it
// survives esvo_reset (whose drains complete every event): the halves are symmetric, work resumes on whichever is current.
// The observation pair, the map pair, the cloud pair and the streams are other domains with swap points of their own: handle members.
struct FrontSlot {  // front[fpar]: what a front stage (block matching, LM, frame assembly) writes while the other parity's LM stage may still run
  DevBuf<esvo_match_t> d_matches;
  DevBuf<u32> d_counters;         // the front stage's counter row (common.hpp: CNT_*)
  DevBuf<DevPoint> d_pt_slots, d_stage;  // LM output by slot (+ keep flags, their scan, its scratch); a lazily completed tick's frame until its count is known
  DevBuf<u32> d_pt_flags, d_pt_prefix, d_scan_tmp_l;
  DevBuf<u32> d_lm_pix_order;     // the narrow LM launch's processing order (esvo_context::d_lm_sort_rows); allocated when the handle can see such launches
  DevBuf<u32> d_lm_guard;         // the scale-loop guard's striped counts (common.hpp: LmGuard); allocated by the first guarded launch
  TickState tk;                   // read only while tick_pending, which flush_pending_tick clears
  bool gather_guard = false;      // a back stage's first launch reads the solver slots until FE_STG: complete after a reset's drains
  FrontEvents own_ev, *ev = &own_ev;  // ev: the set in use: its own, or one the communicator lends per own tick (api_comm.hip, OwnTick)
  u32* h_counters = nullptr; u64* d_clk = nullptr;  // views: this parity's row / block of the handle's h_counters / d_clk
};
struct BackSlot {  // back[par]: a back stage (fusion, clean, regulariser) and what the host reads of it two ticks later
  BackEvents ev;                  // BE_RG1 is also "back stage of this parity done"
  bool timed = true;              // the stage recorded its stage events: describes ev, which survives a reset
  u32 *h_cnt = nullptr, *h_fr_table = nullptr, *d_fr_table = nullptr;  // views: its row of h_cnt_b, its halves of the frame tables
};
// pose[pose_buf]: a tick's pose table, [T | toSec]; released: the back stage has copied it into its frame's slot (the next upload waits)
struct PoseBuf { DevBuf<double> d_T; DevEvent released; };

struct esvo_context : IngestSession, TsSession, SchedSession, MapSession, CloudSession {
  esvo_params_t prm;
  DevParams dp;
  int W = 0, H = 0, device = 0;
  // Two streams, two ticks in flight: the front stage (TS, block matching, LM, frame assembly) of tick k+1 runs on
  // `stream` while the back stage (propagate, fuse, clean, regularise) of tick k runs on `stream_b`.  The back
  // stage only reads what the front stage finished (the frame in the window ring, the tick's pose table).
  hipStream_t stream = nullptr;
  hipStream_t stream_b = nullptr;
  // LM stage of a lazy tick (refinement, frame assembly, counters): block matching and the Time Surfaces of the NEXT tick run
  // beside it on `stream`.  What the two stages share exists twice: d_obs2 and the FrontSlot buffers (work in flight keeps its own).
  hipStream_t stream_l = nullptr;
  // A SECOND queue for the LM stage (round 3): the LM stages of consecutive lazy ticks alternate between stream_l and
  // stream_l1 by the tick's parity, so the head of tick k+1's launch fills the chip while the tail of tick k's -- a few
  // long dependent chains -- drains.  Used for launches in the latency-bound (wide) layout; what the stage writes is in FrontSlot.
  hipStream_t stream_l1 = nullptr;
  // Whether the second queue pays depends on what else the tick holds: where the LM launch is much longer than the fusion
  // stage (346x260, no regulariser: 0.37 ms against 0.12) two launches in flight raise the rate by 18 %; where the two are
  // of similar length (DSEC's reference-faithful tick: 0.25 against 0.30 ms) the fusion stage is the bottleneck either way
  // and a second resident LM launch only takes its registers (0.33 -> 0.375 ms).  So the handle decides from its own stage
  // timings (HIP events of the completed ticks, smoothed).  Scheduling only -- results do not depend on it.  ESVO_LM_QUEUES = 1 / 2
  // forces never / always.  Thresholds: on above 1.5 x, off below 1.2 x until round 6; since the back chain lost ~60 us (no markers
  // between its kernels on most ticks, the one-launch prologue, reg_view's counter) the DSEC tick gains from the second queue as well
  // (0.289 -> 0.264 ms per overlapping tick; 346x260 1000 events 0.203 -> 0.191): on above 0.9 x, off below 0.7 x
  // (profiles/r06_lowlat_tick.txt).
  int lm_queues = 0;              // 0 auto, 1 never, 2 always
  // ESVO_TIMELINE=1 (tools/regime_probe.py): when every stage of every tick ran, collected from the HIP events as they complete
  bool tl_on = false;
  DevEvent tl_ref;
  std::vector<std::array<float, 8>> tl_front;
  std::vector<std::array<float, 4>> tl_back;
  // Latency mode (round 6, api_map.hip): a tick that arrives while nothing of the previous one is pending -- the caller reads every
  // tick's result before it hands in the next, as the ROS node does -- has nothing to overlap with.  Its LM launch stays in the
  // front queue (no cross-queue hand-off: ~25 us) and the host polls for its counters and its end instead of sleeping on the
  // completion interrupt (~10-20 us per wake-up), for ticks of at most lat_max_events events.  ESVO_LOWLAT=0 (A/B) switches it off.
  bool lat_mode = true;
  bool lat_last = false;          // the newest tick was enqueued in latency mode (what synchronising calls look at)
  u32 lat_max_events = 40000u;
  // Stage timings are SAMPLED on that path.  Every hipEventRecord between two dependent kernels costs the queue ~5 us (a marker
  // packet the next dispatch waits for: kernels with no event between them follow each other with no gap at all --
  // profiles/r06_lowlat_tick.txt), and a tick recorded fourteen of them for nothing but esvo_stats_t's ms_* fields.  A tick that
  // runs alone records them for its first 8 ticks and for one tick in lat_timed_every afterwards; ms_* / ms_kernel[] hold the latest
  // sample, sum_ms_kernel[] sums the samples, stats.stage_timing_samples counts them.  The LM layout policy (lm_pair_*) lives on LM
  // launch times: the two events around the LM launch are recorded as well whenever the policy is exploring or trying the layout it
  // is not using (TickState::timed_lm).  Ticks that overlap (the throughput path) record all of them as before.
  // Overlapping SMALL ticks (at most lat_max_events events; two in flight, nobody waits) are paced by the host: ~45 runtime calls per
  // tick, a third of them event records.  They sample their stage timings one tick in pipe_timed_every; the throughput path (larger
  // ticks, paced by the LM kernel) keeps recording every tick: sampling one in four measured -0.5 % on one box and +0.3 % on
  // another, a four-way A/B with the one-launch back prologue nothing at all (profiles/r06_throughput_ab.txt).
  u32 pipe_timed_every = 4;       // ESVO_PIPE_TIMED_EVERY (A/B; 1 = every tick)
  u32 lat_timed_every = 31;       // ESVO_LOWLAT_TIMED_EVERY (A/B; 1 = every tick)
  int reg_sparse_forced = -1;     // ESVO_REG_SPARSE (A/B): the regulariser's sparse-map layout never (0) / always (1); -1: by the element count
  bool stage_events_on = true;    // false while a tick whose stage timings are not sampled is being enqueued (api_map.hip)
  std::atomic<bool> trk_used{false};  // esvo_track_set_current has read the resident surface: renders record TE_R1 for it
  // ... and the copies that open its back stage (frame into the ring, pose table into the frame's slot) are not enqueued one by one
  // but handed to run_fuse, whose frame-table upload carries them in the same launch (scan.hip, back_prologue_kernel)
  struct DeferredCopies {
    bool active = false;
    const void* a_src = nullptr; void* a_dst = nullptr; size_t a_bytes = 0; hipEvent_t ev_a = nullptr;  // frame points; event recorded behind it (null: none)
    const u32* a_flags = nullptr; const u32* a_prefix = nullptr; u32 a_slots = 0;          // gather mode: a_src = the solver slots
    const void* b_src = nullptr; void* b_dst = nullptr; size_t b_bytes = 0; hipEvent_t ev_b = nullptr;  // pose table
  } pro;
  DevBuf<uint8_t> d_obs2[2][2];
  int obs_par = 0;
  hipStream_t stream_i = nullptr;  // event ingest (H2D into the ring): staging new events never waits for a running tick
  bool own_stream = false;
  int par = 0;                    // parity of the tick being assembled
  double baseline = 0;
  struct EmState* em = nullptr;  // event-to-event matching (api_em.hip): buffers, last selection and counts; created on first use
  struct GpcState* gpc = nullptr;  // the global point cloud (api_gpc.hip): near-cloud and voxel-filter scratch, pc_global_, its stats

  // ---- threading contract (include/esvo_hip.h, "Threads"): three groups of calls may run concurrently on one handle --
  // INGEST (esvo_ts_push_events / _event_array / _bag: the ROS spinner's eventsCallback), TRACKER (esvo_track_*) and
  // everything else (the MAPPER group: renders, ticks, outputs, parameters).
  std::recursive_mutex mu_api;  // held by every mapper-group call for its duration (they call each other: recursive)
  std::mutex mu_ring;           // IngestSession, scatter_seq, stats.events_staged / _scattered.  Never held across a host wait.
  std::mutex mu_push[2];        // one pusher per camera at a time (held across its host-to-device copy)
  std::mutex mu_track;          // tracker-group calls
  std::mutex mu_ts;             // the resident left Time Surface (d_ts[0], ts_valid[0], TE_R1) between a render and a
                                // tracker read (esvo_track_set_current without a host image); the Time-Surface history's table
  std::mutex mu_cloud;          // the device-resident point cloud between a build (mapper group) and a tracker gather
                                // (esvo_track_set_reference_from_cloud): CloudSession, evt_cloud_built, evt_cloud_read.  Held only while those change or while work that reads
                                // or writes a buffer is ENQUEUED -- never across a host wait, so neither group waits on the host
                                // for the other: the build fills the buffer that is NOT current and publishes it afterwards.
  // Lock order: mu_api (API_LOCK) comes before mu_track, never after it -- esvo_reset takes mu_api, mu_push[0..1], mu_track,
  // mu_ts, mu_ring in that order, and no tracker-group call takes mu_api.  mu_cloud is innermost for both groups (mapper:
  // mu_api -> mu_cloud; tracker: mu_track -> mu_cloud; esvo_reset holds all of them) and nothing is locked under it.

  // ---- VIEWS: raw pointers that own nothing and are never freed.  Each aliases one buffer of a double-buffered set (or a
  // part of one) and is re-pointed by a swap; kernels capture the pointer at launch, so work in flight keeps its own.
  uint8_t* d_obs[2] = {nullptr, nullptr};  // d_obs2[obs_par][cam]: the observation pair of the current parity
  double* d_pose_T = nullptr;              // pose[pose_buf].d_T: the tick's pose table (re-pointed by upload_poses alone)
  double* d_pose_sec = nullptr;            // its tail (d_pose_T + 16 m): toSec() of the stamps
  MapCell* d_map = nullptr;                // the cells of d_map_mem[0]
  MapCell* d_map2 = nullptr;               // the cells of d_map_mem[1]
  MapCell* d_map_cur = nullptr;            // d_map or d_map2: the DepthMap that is current
  void* xchg_send = nullptr;               // the send / receive block of the exchange that is due (d_codes_* or d_pts_*);
  void* xchg_recv = nullptr;               //   one rank: recv aliases send

  // calibration
  DevBuf<float2> d_lut;
  DevBuf<uint8_t> d_mask;
  DevBuf<int2> d_fixmap[2];

  // Time Surface
  DevBuf<u64> d_sae[2];
  DevBuf<uint8_t> d_raw, d_raw1;
  // FORWARD-mode Time Surface (esvo_ts_render_forward): host copy of each camera's rect_lut, and -- built on first use --
  // its device copy, the per-destination contribution lists (CSR: offsets, source index | corner << 30) and a f64 scratch
  std::vector<float> h_rect_lut[2];
  DevBuf<float2> d_fwd_lut[2];
  DevBuf<uint32_t> d_fwd_off[2], d_fwd_src[2];
  DevBuf<double> d_fwd_val;  // the right camera's raw surface when both cameras render in one launch (esvo_map_tick_resident)
  DevBuf<uint8_t> d_ts[2];
  // Time-Surface history (api_history.hip; the nodes' TS_history_): hist_len entries of two frames each, frame (slot, cam) at
  // d_hist + (2 * slot + cam) * hist_stride.  The stride is W * H rounded up to 256 bytes, so every frame starts as an allocation
  // does.  The table (stamp -> slot, ascending stamps), the free slots and evt_hist are guarded by mu_ts; every store is
  // enqueued on the front stream under that lock, every tracker read on the tracker stream behind evt_hist.  0: off.
  struct HistEntry { u64 t_ns; u32 slot; uint8_t cams; };  // cams: bit 0 left present, bit 1 right present
  size_t hist_len = 0, hist_stride = 0;
  DevBuf<uint8_t> d_hist;
  std::vector<HistEntry> hist;
  std::vector<u32> hist_free;
  DevEvent evt_hist;            // the front stream behind the newest store (a later record implies the earlier stores)
  DevBuf<esvo_event_t> d_ring[2];
  DevBuf<uint8_t> d_wire[2];  // staging of serialised 13-byte event records (esvo_ts_push_event_array), per camera
  // staging of column packets (esvo_ts_push_event_columns), per camera and under its mu_push: col_cap events (a multiple of 256),
  // grown on demand.  d_col: [col_cap u64 stamps | col_cap u16 x | col_cap u16 y | col_cap u8 p] -- the last three hold host
  // columns only, device columns are read where they lie.  h_col_stamps: the pinned stamps, computed by the host's walk (host
  // columns) or brought down from d_col (device columns); what push_commit publishes.
  DevBuf<uint8_t> d_col[2];
  PinBuf<u64> h_col_stamps[2];
  size_t col_cap[2] = {0, 0};
  // staging of EVT 3.0 packets (esvo_ts_push_evt3), per camera and under its mu_push, grown on demand: host words on the device, the
  // tile tuples of the scans, the header the decode leaves (device / pinned).  The events land in d_col.
  DevBuf<uint16_t> d_evt3_words[2];
  DevBuf<u32> d_evt3_tiles[2], d_evt3_hdr[2];
  PinBuf<u32> h_evt3_hdr[2];
  // packets of fewer words are decoded on the host: the measured crossover, ~12 800 events at 2.03 words per event
  // (profiles/evt3_ingest_ab.txt); esvo_debug_evt3_device_min moves it for tests
  size_t evt3_device_min = 24576;
  // esvo_ts_push_evt2 shares the EVT 3.0 staging above (d_evt3_words holds the bytes of either).  Its bounds are in BYTES of words,
  // [0] EVT 2.0, [1] EVT 2.1 in either half order: the measured crossovers of host decode + record push and the device decode,
  // ~20 000 events of EVT 2.0 and ~29 000 one-event words of EVT 2.1 (profiles/evt2_ingest_ab.txt);
  // esvo_debug_evt2_device_min moves both
  size_t evt2_device_min[2] = {20480 * 4, 28672 * 8};
  // The event filter of a camera (esvo_ts_filter_configure; api_filter.hip, kernels_filter.hip), under its mu_push; configuration:
  // it survives a reset, which zeroes d_last.  d_last: [2][W * H], a pair -- a packet reads image `cur` and writes the other, and
  // only a push that succeeded makes that one current.  d_twin: [FLT_HDR_WORDS u32 | cap u64 stamps | cap u16 x | cap u16 y | cap u8 p],
  // the kept events of a packet behind the verdict counts; h_twin: the pinned copy of its header and stamps; d_code / d_scan: a
  // verdict code per event, their exclusive scan and its scratch.  The staging grows with the packets (cap: a multiple of 256).
  struct EventFilter {
    std::atomic<bool> on{false};  // (read without a lock by push_packet: a handle without a filter takes no new lock)
    u64 refractory_ns = 0, support_ns = 0;
    bool has_mask = false;
    int cur = 0;
    DevBuf<u64> d_last;
    DevBuf<uint8_t> d_mask, d_twin, d_code;
    DevBuf<u32> d_tcount, d_tlist, d_scan;
    PinBuf<u64> h_twin;
    size_t cap = 0;
  } flt[2];
  // The burst stage of a camera's filter (esvo_ts_burst_configure; api_filter.hip, flt_burst_kernel), under its mu_push; the
  // configuration survives a reset, which zeroes the state.  d_stamp / d_flags: [2][W * H], pairs as d_last is, with an index of
  // their own (a filter reconfiguration restarts the filter's pair and leaves this one alone).
  struct EventBurst {
    u32 mode = 0;  // ESVO_BURST_OFF: no stage, no memory
    u64 burst_ns = 0;
    int cur = 0;
    DevBuf<u64> d_stamp;
    DevBuf<uint8_t> d_flags;
  } bst[2];
  // The event survey of a camera (esvo_ts_survey_begin; api_survey.hip, kernels_survey.hip), under its mu_push; open or not survives a
  // reset, which zeroes the counts.  d_counts: [2][W * H], plane = polarity; d_stats: SRV_STAT_WORDS; d_sel / d_report / d_mask: the
  // radix select's words, the report and the mask bytes of esvo_ts_survey_mask.
  struct EventSurvey {
    std::atomic<bool> on{false};
    bool count_only = false;
    DevBuf<u32> d_counts, d_sel;
    DevBuf<u64> d_stats, d_report;
    DevBuf<uint8_t> d_mask;
  } srv[2];
  u32 flt_tcap = FLT_TILE_CAP_MAX;  // ESVO_FLT_TILE_CAP (tests): entries of a tile's list; beyond it the tile reads the packet
  u64 ring_cap = 0;
  // esvo_ts_push_events_async: the newest enqueued (not awaited) copy of a camera; consumers of the ring on the front stream
  // queue behind it (ingest_fence, api_ts.hip) -- under mu_ring, with IngestSession::ingest_pending
  DevEvent evt_ingest[2];

  // observation
  DevBuf<uint8_t> d_obs_tmp;

  // pose table of the tick
  PoseBuf pose[2];
  int pose_buf = 0;
  std::vector<double> h_pose_T;
  PinBuf<double> h_pin;        // pinned staging: 2 slots x (max_poses x 17 + 16) doubles

  // per-tick scratch
  u32 max_ev = 0;
  DevBuf<esvo_event_t> d_tick_ev;
  DevBuf<esvo_match_t> d_match_slots;
  DevBuf<u32> d_match_flags, d_match_prefix;
  // split LM launch (kernels_lm.hip): F(x0) of every match, its cost, the processing order; allocated when the handle can see
  // launches above the wide layout's bound
  DevBuf<double> d_lm_fvec0, d_lm_fnorm0;
  DevBuf<u32> d_lm_meta, d_lm_order, d_lm_hist;
  // the processing order of the narrow LM launch (kernels_lm.hip): built on the front queue behind the match compaction, read by
  // the LM launch on its own queue while the next tick's front stage runs -- so the order exists per front parity
  // (FrontSlot::d_lm_pix_order); the sort's rows and histogram are the front queue's alone.
  DevBuf<u64> d_lm_sort_rows[2];
  DevBuf<u32> d_lm_sort_hist;
  bool lm_order_on = true;        // ESVO_LM_ORDER=0 (test / A/B only): the launch takes its slots in grid order
  // block matching once per distinct raw pixel (kernels_bm.hip, launch_bm_match_dedupe): one allocation -- the owner table
  // [W * H], the owner count (4 words, the first is used), the owner list [max_ev], the search outcomes [max_ev] -- on the front
  // queue alone, the next tick's block matching is behind its readers.  Allocated when the handle can see launches of
  // bm_dedupe_min events; run_bm takes the path for those.
  DevBuf<u32> d_bm_dedupe;
  bool bm_dedupe_on = true;       // ESVO_BM_DEDUPE=0 (test / A/B only): one search per event
  u32 bm_dedupe_min = esvo::BM_DEDUPE_MIN_EVENTS;  // ESVO_BM_DEDUPE_MIN=<n> (tests): the smallest launch bound that shares
  DevBuf<u64> d_clk;           // in-run shader-clock probe of the LM kernel (LmArgs::clk, common.hpp); read by esvo_get_stats
  bool clk_probe = true;          // ESVO_CLK_PROBE=0 (A/B only) launches the LM kernel without it
  DevBuf<DevPoint> d_pts_tmp;  // stage-wise refine output
  PinBuf<u32> h_counters;      // pinned, a row per front parity (FrontSlot::h_counters)
  DevBuf<u32> d_scan_tmp;
  DevBuf<u32> d_cnt_b;         // the back stage's counter row (common.hpp: CNTB_*)
  PinBuf<u32> h_cnt_b;         // pinned, CNTB_ROWS rows of it (CNTB_ROW_*)
  DevBuf<u32> d_scan_tmp_b;

  // fusion window
  DevBuf<DevPoint> d_win;
  u32 win_cap = 0;
  u32 n_pose_slots = 0;
  std::vector<char> slot_used;
  DevBuf<double> d_frame_pose_T;
  u32 max_poses = 0;
  DevBuf<u32> d_fr_table;      // fr_cum | fr_off | fr_slot
  PinBuf<u32> h_fr_table;      // pinned
  u32 max_frames = 0;             // capacity in NON-EMPTY frames (pose slots, frame tables)

  // DepthMap
  DevBuf<DevPoint> d_prop;
  // fusion front (kernels_fuse.hip): per tile a fixed-capacity list of point ids + one shared overflow list; per cell the
  // (offset, count) of its sorted record list; the touched cells by length class; counters (class sizes, cursors)
  DevBuf<u32> d_tile_count;
  DevBuf<uint2> d_tile_pts, d_over_pts;
  DevBuf<u32> d_cell_count, d_cell_offset, d_cell_list;
  DevBuf<u32> d_fuse_ctr;      // class_count | class_total | rec_cursor | over_count (common.hpp: FUSE_CTR_*)
  u32 fuse_tile_rec = 4096;       // entries of a tile's own region of d_rec_ids (ESVO_FUSE_TILE_REC: tests)
  u32 fuse_slice_cap = 0;         // entries of one (class, slice) segment of d_cell_list
  u32 fuse_tile_cap = 1024;       // ESVO_FUSE_TILE_CAP (tests): entries per tile list
  u32 fuse_pmax_plus1 = 0;        // ESVO_FUSE_PMAX (tests) + 1: candidates up to which a tile takes the bit-row path
  DevBuf<u32> d_rec_ids;       // record ids of cells whose list does not fit LDS (degenerate scenes)
  u32 fuse_lds_cap = 0;           // ESVO_FUSE_LDS_CAP (tests): record ids per tile kept in LDS; 0 = the maximum
  DevBuf<uint8_t> d_map_mem[2];  // each: the cells + their dense flags (common.hpp: map_buffer_bytes); d_map / d_map2 view them
  DevBuf<u32> d_owner_max, d_owner_min;
  DevBuf<u32> d_sel;           // denoising: walk positions of the kept events
  DevBuf<uint8_t> d_evmap;     // denoising: binary event map
  // sharded mode (kernels_shard.hip): dense local lists + the (matched, kept) byte per slot that is exchanged
  DevBuf<u32> d_own_w;         // slot w of the k-th own match
  DevBuf<u32> d_lkeep;         // keep flag of the k-th own match after LM + culling
  DevBuf<uint8_t> d_codes;     // [codes_bytes] one byte per slot (all ranks' slots, after exchange 1)
  size_t codes_bytes = 0;
  // what the caller must all-gather across the ranks before the next phase (esvo_shard_exchange): xchg_block bytes from
  // xchg_send of every rank into xchg_recv, rank-major.  One rank (n_shards == 1): recv aliases send, nothing to exchange.
  DevBuf<uint8_t> d_codes_send;             // exchange 1: [roundup8(ceil(n / N))] the bytes of the own slots r, r + N ...
  DevBuf<uint8_t> d_codes_all;              //             [N][that]
  DevBuf<unsigned long long> d_pts_send;    // exchange 2: [1 + own * 13] count | kept points (final index in seq)
  DevBuf<unsigned long long> d_pts_all;     //             [N][1 + max_kept * 13]
  DevBuf<u32> d_rank_kept;                  // [SHARD_MAX_RANKS] kept count of every rank (from exchange 1)
  static constexpr u32 SHARD_MAX_RANKS = 1024;
  bool sharded = false;
  // ---- routed band mode (esvo_shard_set_routing): events are routed by image row at ingest, the Time Surfaces are
  // rendered for the band + halo only, block matching and refinement belong to the rank that owns floor(y_rect) of the event.
  bool routed = false;
  int ts_halo = 0;                       // rows beyond the band for which the observation pair is valid
  int rband_y0 = 0, rband_y1 = 0;        // rectified rows the Time Surfaces are rendered for (whole tiles of TS_TILE_ROWS)
  int oband_y0 = 0, oband_y1 = 0;        // rows of the observation pair that hold data: what block matching and LM may read
  int sband_y0[2] = {0, 0}, sband_y1[2] = {0, 0};  // RAW rows whose events a camera's SAE needs for rband (remap + median taps)
  std::vector<int> fix_row_lo[2], fix_row_hi[2];   // per rectified row: the raw rows its remap taps reach (from the fixed-point maps)
  std::vector<uint8_t> keep_px;          // left camera, [W * H]: bit 0 the SAE needs the pixel's events, bit 1 floor(y_rect) is in the band
  DevBuf<u32> d_ring_gidx;            // [ring_cap] low 32 bits of the global index of the left ring's events
  PinBuf<esvo_event_t> h_route_ev[2];  // pinned staging of the kept events of one push, per camera
  PinBuf<u32> h_route_gidx;
  size_t route_cap[2] = {0, 0};
  // out-of-order packets (api_ingest.hip, push_unsorted): scratch of the ring merge; queue mode: the device copy of tsq_dup
  DevBuf<esvo_event_t> d_merge_a, d_merge_b;
  DevBuf<u32> d_merge_plan;
  DevBuf<esvo_event_t> d_tsq_dup;
  DevBuf<u32> d_halo_viol;            // [2] matches whose refinement read outside oband, all ranks, summed over the ticks | scratch
  DevBuf<u32> d_dn_flags;             // [2][max_ev] kept flag + exclusive prefix per walk position of the raw selection (lazily)
  // pair layout of the LM kernel (kernels_lm.hip): chosen per tick from the LM launch times the handle measures anyway
  // (HIP events).  The first eight candidate ticks alternate between the layouts, then the faster one is used, with one tick
  // of the other every 64 so that a change of scene is noticed; a layout's figure is the MINIMUM of its last four launches
  // (the first ticks of a handle are slow whatever the layout).  ESVO_LM_PAIR = 0 / 1 forces never / always.  Scheduling
  // only: same bits either way.
  int lm_pair_forced = -1;
  FrontSlot front[2];
  int fpar = 0;                   // parity of the newest front stage
  FrontSlot& front_cur() { return front[fpar]; }
  bool tick_pending = false;      // front_cur().tk has its front stage enqueued but is not committed yet
  BackSlot back[2];
  TsEvents ts_ev[2];              // per camera; TE_R1 of camera 0 is also what esvo_track_set_current waits for (mu_ts)
  DevEvent ev_frame;              // back_after_front: everything enqueued on the front stream so far, for the back stream
  // per-pixel event queues (max_event_queue_len > 0; kernels_ts.hip): key sets of both cameras + the batch's tile lists
  int tsq_len = 0;
  DevBuf<u64> d_tsq[2];
  DevBuf<u32> d_tsq_tcount;
  DevBuf<uint4> d_tsq_tlist, d_tsq_over;
  DevBuf<u32> d_tsq_over_count;
  u32 tsq_tcap = 0;
  static constexpr u64 TSQ_ROUND = 1ull << 20;  // events per insertion round = capacity of the overflow list
  DevBuf<double2> d_reg_ab, d_reg_cd;
  double T_world_frame[16];
  // export
  DevBuf<u32> d_exp_flags, d_exp_prefix;
  DevBuf<esvo_depth_point_t> d_export;
  DevBuf<u32> d_export_cell;
  // The map's point cloud kept on the device (esvo_map_cloud_build; kernels_cloud.hip): a SNAPSHOT in one of two buffers of W*H
  // points (allocated by the first build).  A build fills the buffer that is not current, on the back stream and behind the
  // event of the tracker's last gather out of it (evt_cloud_read), records evt_cloud_built, reads the count -- its one host
  // read -- and only then makes the buffer current, under mu_cloud.  The tracker's gather runs on its own stream behind
  // evt_cloud_built.  Ticks never touch the buffers; esvo_reset empties them (cloud_cur = -1).
  DevBuf<float> d_cloud_xyz[2];
  DevBuf<u32> d_cloud_ids;     // [3][cloud_id_cap] present | prefix | where, by creation id
  size_t cloud_id_cap = 0;
  DevBuf<u32> d_cloud_scan;    // scan scratch for cloud_id_cap ids
  DevBuf<u32> d_cloud_cnt;     // [0] elements [1] cells whose id was outside the bound (must stay 0)
  PinBuf<u32> h_cloud_cnt;     // pinned copy of it
  DevEvent evt_cloud_built[2];
  DevEvent evt_cloud_read[2];   // the tracker stream's newest gather out of that buffer

  // tracker residual / Jacobian evaluation (kernels_track.hip): own stream, own images, synchronous calls
  hipStream_t stream_t = nullptr;
  DevBuf<uint8_t> d_trk_blur, d_trk_neg;
  DevBuf<int16_t> d_trk_du, d_trk_dv;
  DevBuf<float> d_trk_xyz;
  DevBuf<double> d_trk_pts, d_trk_out;
  PinBuf<double> h_trk_ne;     // pinned: the 28 sums of esvo_track_normal_equations
  PinBuf<TrackSolveOut> h_trk_solve;  // pinned: what track_solve_kernel writes (esvo_track_solve, on_device)
  PinBuf<float> h_trk_xyz;     // pinned staging of esvo_track_set_reference's point cloud
  bool trk_xyz_inflight = false;  // an upload out of it has been enqueued and no call has waited for the tracker stream since
  size_t trk_cap = 0;
  DevEvent evt_trk_read;  // the tracker stream has read the resident left Time Surface (mu_ts)
  // the reprojection map (kernels_track_viz.hip): the tracker group's own image, owner words, jet table and counter, allocated
  // on first use under mu_track -- the d_viz_* buffers below are the mapper group's
  DevBuf<uint8_t> d_trk_viz_bgr;
  DevBuf<u32> d_trk_viz_owner;   // all 0 between calls (the paint pass clears what the mark pass set)
  DevBuf<uint8_t> d_trk_viz_jet;
  DevBuf<u32> d_trk_viz_cnt;

  // pinned staging slots for frame pose tables that arrive from the host (push_frame variants): a slot is reused only
  // after the back stream has consumed it
  static constexpr int POSE_POOL = 32;
  PinBuf<double> h_pose_pool;
  DevEvent pool_evt[POSE_POOL];

  // SGM initialisation (kernels_sgm.hip): allocated on first use, released by esvo_destroy
  SgmScratch sgm = {};            // what the launchers take by value: raw pointers into the buffers of the next three lines
  DevBuf<uint8_t> d_sgm_plane[4];  // sobL, rawL, sobR, rawR
  DevBuf<int16_t> d_sgm_vol[6], d_sgm_d1, d_sgm_d1b;
  DevBuf<u32> d_sgm_d2key;
  bool sgm_ok = false;
  DevBuf<uint8_t> d_sgm_img[2];
  DevBuf<int16_t> d_sgm_disp;
  DevBuf<u32> d_sgm_pair;      // [2][4 * max_ev] winner flags / ranks of naive_propagation
  DevBuf<double> d_sgm_T;
  DevEvent evt_sgm[3];  // the per-tick SGM mode: before / behind the SGM chain, behind the point stage

  // debug images (kernels_viz.hip): allocated on first use
  DevBuf<uint8_t> d_viz_bgr, d_viz_jet;
  DevBuf<u32> d_viz_owner;

  struct esvo_comm* comm = nullptr;  // multi-GPU exchange (api_comm.hip), null on single-GPU handles

  esvo_stats_t stats;

  // ---- SURVIVES A RESET although it belongs to the session (everything outside the *Session structs survives; what is fixed at
  // esvo_create, configuration, buffers and events do so by nature).  Left in place above: par / fpar / obs_par / pose_buf, the slots
  // and views they select; pro (active inside one tick_phase2); the tools' timeline; (?) em, which has no reset hook.
  // (?): the code shows no reason -- a reset handle keeps it as it always has, a later change decides.
  u32 lat_ticks = 0;            // ticks enqueued with nothing pending before them (band-sharded ticks: all of them -- every phase of such a
  u32 pipe_seq = 0;             // tick is waited for by an exchange) / overlapping small ticks: they pace the SAMPLING of stage timings, no result
  u64 scatter_seq = 0;          // scatter launches so far, under mu_ring (a pusher that drained the front stream resets scatter_pending_lo
                                // only if no scatter was enqueued meanwhile): compared for equality only
  u64 em_guard_lo[2] = {~0ull, ~0ull};  // oldest ring event an esvo_map_tick_em gather may still read (api_em.hip): lifted before that call returns
  int pin_slot = 0;             // which half of h_pin the next pose table takes: either will do
  int pool_next = 0;            // ... which slot of h_pose_pool (pool_evt[] says when a slot is free again)
  double T_world_obs[16];       // the observation's pose and stamp: every tick checks obs_set before it reads them
  u64 obs_t_ns = 0;
  size_t xchg_block = 0;        // 0 behind a tick's last phase, like xchg_send / xchg_recv; (?) a reset between two phases keeps the three
  size_t trk_n = 0;             // (?) points of the tracker's reference
  bool trk_cur = false;         // (?) esvo_track_set_current has run: the tracker keeps its images
  bool trk_viz_valid = false;   // (?) d_trk_viz_bgr holds the image of a call
};

namespace esvo_host {
// esvo_last_error: the message of the calling THREAD's last failed call (with or without a handle) -- three threads may
// use one handle at the same time, a string inside the handle could be rewritten while another thread reads it
extern thread_local std::string g_create_error;
// api_core.hip
void fill_dev_params(esvo_context* h);
void set_compute_band(esvo_context* h);
void jet256_bgr(uint8_t jet[768]);  // DrawPoint's 256 BGR triples: the mapper's debug images and the tracker's reprojection map
// api_ts.hip
void collect_ts_timing(esvo_context* h, int only = -1);
void ingest_fence(esvo_context* h, int cam);  // caller holds mu_ring
int ts_scatter_ahead(esvo_context* h, uint64_t t_ns);
void resident_write_begin(esvo_context* h, int cam);
int ts_render_pair(esvo_context* h, uint64_t t_ns, uint8_t* const obs_out[2]);
// api_filter.hip, api_survey.hip (their hooks in the push path: ingest.hpp)
int filter_zero_state(esvo_context* h, hipStream_t st);  // esvo_reset: the `last` images of both cameras
int survey_zero_state(esvo_context* h, hipStream_t st);  // esvo_reset: the counts and stats of both cameras
// api_history.hip
int hist_store(esvo_context* h, int cam, uint64_t t_ns, const uint8_t* src, bool from_host);  // caller holds mu_ts
void hist_clear(esvo_context* h);                                                             // caller holds mu_ts
// api_em.hip
void em_release(esvo_context* h);  // frees the event-matching state (esvo_destroy)
// api_gpc.hip
void gpc_release(esvo_context* h);  // frees the global-cloud state (esvo_destroy)
void gpc_reset(esvo_context* h);    // empties the global cloud, keeps t_last_pub (esvo_reset)
// api_map.hip
struct FrontOpts { bool split = false, lat = false, pipe = false; };  // a front stage's scheduling, decided by the call that enqueues it:
// split: LM on its own queue (the lazy tick path); lat: nothing is pending before the tick (latency mode); pipe: it overlaps the previous tick
u64 lower_bound_sec(const esvo_context* h, int cam, double t);
u64 ros_time_from_sec(double t);
int upload_poses(esvo_context* h, const uint64_t* pose_t_ns, const double* pose_T, size_t m, u32* d_zero_row = nullptr);
int select_events(esvo_context* h, uint64_t t_ns, u64* first_out, u32* n_out);
int denoise_select(esvo_context* h, u32 n, u32* n_kept);
inline void switch_front_parity(esvo_context* h) { h->fpar ^= 1; }  // a new front stage takes the other FrontSlot: the previous tick's LM stage may still run on its own
int run_bm(esvo_context* h, const esvo_event_t* d_ev, u64 first, u64 cap, int reverse, u32 n, const u32* sel = nullptr);
int run_order_matches(esvo_context* h, u32 n, bool local, bool by_index = false);
int run_lm(esvo_context* h, u32 max_matches, int cull, bool dense, hipStream_t st = nullptr, int pair = -1, const u32* order = nullptr, bool by_index = false);
int run_order_points(esvo_context* h, u32 max_matches, DevPoint* dst, hipStream_t st = nullptr, u32* host_row = nullptr);
void collect_bm_failures(esvo_context* h, const u32* row, bool accumulate);
int read_counters(esvo_context* h);
bool lm_guard_wanted(const esvo_context* h);  // the scale-loop guard applies to the handle's next refinement launch
void collect_lm_guard(esvo_context* h, const u32* row, bool guarded);  // the launch's CNT_LM_* words -> MapSession::lm_stats
int tick_phase0(esvo_context* h, uint64_t t_ns, const uint64_t* pose_t_ns, const double* pose_T, size_t m, FrontOpts opt = FrontOpts());
int tick_phase1_enqueue(esvo_context* h);
int tick_phase1_collect(esvo_context* h, int fp);
int collect_front_stats(esvo_context* h, TickState& tk, const u32* cnt, const FrontEvents& ev);
int tick_phase2(esvo_context* h, int fp);
int flush_pending_tick(esvo_context* h);  // completes a lazily finished tick (see TickState)
int finalize_tick_stats(esvo_context* h);
void begin_observation(esvo_context* h);
void revert_observation(esvo_context* h);
// api_window.hip
int back_after_front(esvo_context* h);
void collect_back(esvo_context* h, int par);
int window_reserve(esvo_context* h, u32 n, u32* off_out);
int window_probe_after_pops(esvo_context* h, size_t keep_below, u32 n);
int commit_frame(esvo_context* h, u32 off, u32 count, const double* pose_T_host, u32 m, int pose_buf = 0, bool apply_policy = true);
int flush_deferred_copies(esvo_context* h);
int run_fuse(esvo_context* h, int par, const double* T_world_obs, bool naive = false);
int fuse_window_now(esvo_context* h, const double* T_world_obs, bool naive = false, int* par_out = nullptr);
int commit_naive_frame(esvo_context* h, const DevPoint* d_src, u32 count, const double* pose_T_host, u32 m, int pose_buf);
void window_stats(esvo_context* h);
int drain_lm_and_back(esvo_context* h);
int export_map(esvo_context* h, std::vector<esvo_depth_point_t>& out, std::vector<u32>* cells);
// api_shard.hip
int select_events_routed(esvo_context* h, uint64_t t_ns, u32* n_out, u32* g_first_out, u64* loc_first_out, u32* n_loc_out, u32* n_own_out);
int routed_denoise_resume(esvo_context* h);
int shard_front(esvo_context* h, TickState& tk, u32 n, const u32* sel);
int shard_order_points(esvo_context* h, TickState& tk);
int shard_scatter_frame(esvo_context* h, TickState& tk);
// api_comm.hip
void comm_release(esvo_context* h);
void comm_reset(esvo_context* h);
}  // namespace esvo_host
using namespace esvo_host;

#define HIPCHK(call)                                                                              \
  do {                                                                                            \
    hipError_t _e = (call);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      char _b[512];                                                                               \
      snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
      (void)h; g_create_error = _b;                                                               \
      return ESVO_ERR_HIP;                                                                        \
    }                                                                                             \
  } while (0)

// Polled waits (latency mode, api_map.hip): hipEventQuery / hipStreamQuery in a loop for at most `budget_us`, then the blocking
// call.  The blocking calls sleep on the completion interrupt (10-20 us from the signal to the woken thread); a tick the caller
// waits for pays that twice (counters, end of tick).  "Not ready" is an error code the runtime remembers: it is cleared here, or
// the next hipGetLastError() behind a launch would report it.
template <class T>
inline hipError_t esvo_wait(hipError_t (*query)(T), hipError_t (*block)(T), T x, bool poll, double budget_us) {
  if (poll) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t q = query(x);
      if (q == hipSuccess) return q;
      (void)hipGetLastError();
      if (q != hipErrorNotReady) return q;
      if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > budget_us) break;
    }
  }
  return block(x);
}
inline hipError_t esvo_wait_event(hipEvent_t e, bool poll, double budget_us = 3000.0) { return esvo_wait(hipEventQuery, hipEventSynchronize, e, poll, budget_us); }
inline hipError_t esvo_wait_stream(hipStream_t s, bool poll, double budget_us = 3000.0) { return esvo_wait(hipStreamQuery, hipStreamSynchronize, s, poll, budget_us); }

struct StageEventsScope {  // stage-timing events off (or on) for the calls of one scope, back on at its end whatever the exit
  esvo_context* h;
  StageEventsScope(esvo_context* hh, bool on) : h(hh) { h->stage_events_on = on; }
  ~StageEventsScope() { h->stage_events_on = true; }
};
// whether the operations enqueued NOW (renders, a tick's stages) record their stage-timing events (context.hpp, lat_ticks)
inline bool esvo_stage_timed(const esvo_context* h) {
  if (!h->lat_mode || h->tl_on || (h->comm && !h->sharded)) return true;  // (tick-interleaved ranks: every tick)
  if (h->tick_pending) {  // overlapping ticks: the small ones are paced by the HOST's enqueueing (pipe_seq); the large ones: every tick
    if (h->front[h->fpar].tk.n && h->front[h->fpar].tk.n <= h->lat_max_events) return h->pipe_seq % h->pipe_timed_every == 0u;
    return true;
  }
  return h->lat_ticks < 8u || h->lat_ticks % h->lat_timed_every == 0u;
}

#define ESVO_SET_ERR(msg) (esvo_host::g_create_error = (msg))
#define API_LOCK(h) std::lock_guard<std::recursive_mutex> _api_lock((h)->mu_api)

#define FAIL(code, msg)                      \
  do {                                       \
    (void)h; g_create_error = (msg);                    \
    return (code);                           \
  } while (0)
