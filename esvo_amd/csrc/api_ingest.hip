// api_ingest.hip — event ingest (ingest.hpp): the staging protocol's steps, out-of-order packets, the column staging; the push calls for records, EventArray messages and columns
#include "ingest.hpp"

namespace esvo_host {

int push_begin(esvo_context* h, int cam, size_t n, u64 t_first, PushTicket& tk) {
  std::lock_guard<std::mutex> lr(h->mu_ring);
  const auto& tsq = h->ts_host[cam];
  if (!tsq.empty() && t_first < tsq.back()) FAIL(ESVO_ERR_INVALID_ARG, "events must be sorted by time stamp (SURVEY Appendix A-1)");
  if (!ring_has_room(h, cam, n)) FAIL(ESVO_ERR_CAPACITY, RING_FULL);
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
int push_unsorted(esvo_context* h, int cam, size_t n, const esvo_event_t* ev) {
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
    esvo_event_t e = ev[i];
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
    if (!ring_has_room(h, cam, n)) FAIL(ESVO_ERR_CAPACITY, RING_FULL);
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
  if (h->scattered[cam] > pos_abs) h->scattered[cam] += n_before_scattered;
  commit_tail(h, cam, n);
  h->stats.late_events[cam] += n_late;
  for (const esvo_event_t& d : dups) h->tsq_dup[cam].push_back(d);
  return ESVO_OK;
}

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
int upload_columns(esvo_context* h, const ColumnBlock& b, const u64* stamps, const void* x, const void* y, const void* p, size_t n) {
  HIPCHK(hipMemcpyAsync(b.t, stamps, sizeof(u64) * n, hipMemcpyHostToDevice, h->stream_i));
  HIPCHK(hipMemcpyAsync(b.x, x, 2 * n, hipMemcpyHostToDevice, h->stream_i));
  HIPCHK(hipMemcpyAsync(b.y, y, 2 * n, hipMemcpyHostToDevice, h->stream_i));
  if (p) HIPCHK(hipMemcpyAsync(b.p, p, n, hipMemcpyHostToDevice, h->stream_i));
  return ESVO_OK;
}
// What the runtime knows of a pointer: 0 host memory (pageable, pinned or registered), 1 plain device memory of `device`,
// 2 anything else (managed memory, another GPU's).  Launches nothing, copies nothing.
static int column_memory_kind(const void* p, int device) {
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return 0; }  // unknown to the runtime: pageable
  if (a.isManaged || a.type == hipMemoryTypeManaged) return 2;
  if (a.type == hipMemoryTypeUnregistered || a.type == hipMemoryTypeHost) return 0;
  return a.type == hipMemoryTypeDevice && a.device == device ? 1 : 2;
}
int require_memory_place(esvo_context* h, const void* base, size_t bytes, bool on_device, const std::string& what) {
  const int want = on_device ? 1 : 0;
  if (column_memory_kind(base, h->device) != want || column_memory_kind(static_cast<const uint8_t*>(base) + bytes - 1, h->device) != want)
    FAIL(ESVO_ERR_INVALID_ARG, what + (on_device ? " labelled ESVO_MEM_DEVICE must be plain device memory of the handle's GPU (not host, managed or another GPU's)"
                                                 : " labelled ESVO_MEM_HOST must be host memory (a device or managed pointer was given)"));
  return ESVO_OK;
}


static u32 rd32(const uint8_t* p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }
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

// ---- column ingest: x / y / t / p arrays in host or device memory (include/esvo_hip.h, esvo_ts_push_event_columns) ----------------
static size_t col_t_size(int t_type) { return t_type == ESVO_T_US_U32 ? 4 : 8; }
static const char* columns_arg_error(const esvo_event_columns_t* c, size_t n) {
  if (c->t_type != ESVO_T_NS_I64 && c->t_type != ESVO_T_US_I64 && c->t_type != ESVO_T_US_U32) return "event columns: unknown t_type";
  if (c->p_type != ESVO_P_U8 && c->p_type != ESVO_P_I8) return "event columns: unknown p_type";
  if (c->memory != ESVO_MEM_HOST && c->memory != ESVO_MEM_DEVICE) return "event columns: unknown memory";
  if (n && (!c->x || !c->y || !c->t)) return "event columns: x, y and t must not be NULL";
  if ((uintptr_t)c->x % 2 || (uintptr_t)c->y % 2 || (uintptr_t)c->t % col_t_size(c->t_type))
    return "event columns: a column base is not aligned for its element type";
  return nullptr;
}
}  // namespace esvo_host

extern "C" {

static int push_events_impl(esvo_handle h, int cam, const esvo_event_t* ev, size_t n, bool wait) {
  if (!h || cam < 0 || cam > 1 || (n && !ev)) return ESVO_ERR_INVALID_ARG;
  if (n == 0) return ESVO_OK;
  if (n > h->ring_cap) FAIL(ESVO_ERR_CAPACITY, BLOCK_TOO_LARGE);
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
  if (n > h->ring_cap) FAIL(ESVO_ERR_CAPACITY, BLOCK_TOO_LARGE);
  WirePacket src{{}, h, cam, msg + off, n};
  return push_packet(h, cam, src);
}

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
  if (n > h->ring_cap) FAIL(ESVO_ERR_CAPACITY, BLOCK_TOO_LARGE);
  const bool on_device = c->memory == ESVO_MEM_DEVICE;
  std::unique_lock<std::mutex> lp(h->mu_push[cam]);
  HIPCHK(hipSetDevice(h->device));
  const void* base[4] = {c->x, c->y, c->t, c->p};  // where the columns lie, first and last byte of each, before anything is launched or copied
  const size_t bytes[4] = {2 * n, 2 * n, col_t_size(c->t_type) * n, n};
  for (int k = 0; k < 4; ++k)
    if (base[k]) { int rc = require_memory_place(h, base[k], bytes[k], on_device, "event columns"); if (rc) return rc; }
  { int rc = columns_staging(h, cam, n); if (rc) return rc; }
  u64* const stamps = h->h_col_stamps[cam];
  u64* const d_stamps = column_block(h->d_col[cam], h->col_cap[cam]).t;
  if (on_device && h->flt[cam].on) {  // under the event filter validity and order are judged by its last kernel: the stamps stay on the device
    launch_ts_columns_stamps(c->t, c->t_type, c->t_offset, n, d_stamps, h->stream_i);
    HIPCHK(hipGetLastError());
    std::vector<esvo_event_t> none;
    ColumnsPacket judged{{}, h, cam, c, n, stamps, true, &none};
    judged.host_stamps = false;
    return push_packet(h, cam, judged, std::move(lp));
  }
  if (on_device) {  // t -> stamps on the device, down once
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

}  // extern "C"
