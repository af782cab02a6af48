// api_words.hip — event ingest from Prophesee's EVT 3.0 and EVT 2.0 / 2.1 words: both host decoders, the one push path of the two calls (push_words), the .raw header
#include "ingest.hpp"

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
  void launch(const void* d_words, size_t n_words, const State& st0, int64_t t_offset_us, u32* tiles, u32* hdr, const ColumnBlock& b, hipStream_t s) const {
    launch_evt3_decode(static_cast<const uint16_t*>(d_words), n_words, st0, t_offset_us, tiles, hdr, b.t, b.x, b.y, b.p, b.cap, s);
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
  void launch(const void* d_words, size_t n_words, const State& st0, int64_t t_offset_us, u32* tiles, u32* hdr, const ColumnBlock& b, hipStream_t s) const {
    launch_evt2_decode(static_cast<const u32*>(d_words), n_words, format, st0, t_offset_us, tiles, hdr, b.t, b.x, b.y, b.p, b.cap, s);
  }
  void end_state(const u32* hdr, State& st1) const { st1.flags = hdr[EVT3_H_FLAGS]; st1.time_high = hdr[EVT3_H_TIME]; st1.loops = hdr[EVT3_H_LOOPS_END]; }
};
// words where the host can read them: those that lie on the device come down into hw first (8-byte units: aligned for every word size)
int words_on_host(esvo_context* h, const void* words, size_t n_bytes, bool on_device, std::vector<u64>& hw, const void** w) {
  *w = words;
  if (!on_device) return ESVO_OK;
  hw.resize((n_bytes + 7) / 8);
  HIPCHK(hipMemcpyAsync(hw.data(), words, n_bytes, hipMemcpyDeviceToHost, h->stream_i));
  HIPCHK(hipStreamSynchronize(h->stream_i));
  *w = hw.data();
  return ESVO_OK;
}
// A packet the device decoded into the camera's column staging: a device-resident ColumnsPacket, whose slow paths take the records
// of the host decoder (the words come down first where they lie on the device).
template <class F>
struct WordsPacket : ColumnsPacket {
  F f; const void* words; size_t n_words; bool on_device; typename F::State st0; int64_t t_offset_us;
  int materialise() {
    esvo_context* const h = this->h;
    std::vector<u64> hw; const void* w = nullptr;
    { int rc = words_on_host(h, words, n_words * f.word_bytes(), on_device, hw, &w); if (rc) return rc; }
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
  { int rcp = require_memory_place(h, words_v, n_bytes, on_device, name + " words"); if (rcp) return rcp; }  // before anything is launched or copied
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
    std::vector<u64> hw; const void* w = nullptr;
    { int rcw = words_on_host(h, words_v, n_bytes, on_device, hw, &w); if (rcw) return rcw; }
    std::vector<esvo_event_t> E;
    const size_t room = (size_t)h->ring_cap;
    const int drc = f.decode_host(st1, w, n_words, t_offset_us, cnt, [&](const esvo_event_t& e) {
      if (E.size() >= room) return false;
      E.push_back(e);
      return true;
    });
    if (drc == EVT3_DEC_BAD_STAMP) FAIL(ESVO_ERR_INVALID_ARG, words_bad_event(f.name(), (size_t)cnt.events));
    if (drc == EVT3_DEC_FULL) FAIL(ESVO_ERR_CAPACITY, BLOCK_TOO_LARGE);
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
      f.launch(d_words, n_words, st0, t_offset_us, h->d_evt3_tiles[cam], h->d_evt3_hdr[cam], column_block(h->d_col[cam], h->col_cap[cam]), h->stream_i);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(hdr, h->d_evt3_hdr[cam], sizeof(u32) * EVT3_HDR_WORDS, hipMemcpyDeviceToHost, h->stream_i));
      HIPCHK(hipStreamSynchronize(h->stream_i));
      return ESVO_OK;
    };
    if (!on_device) HIPCHK(hipMemcpyAsync(h->d_evt3_words[cam], words_v, n_bytes, hipMemcpyHostToDevice, h->stream_i));
    { int rcd = decode(); if (rcd) return rcd; }
    const size_t n = hdr[EVT3_H_EVENTS];
    if (hdr[EVT3_H_FIRST_BAD] != 0xffffffffu) FAIL(ESVO_ERR_INVALID_ARG, words_bad_event(f.name(), hdr[EVT3_H_FIRST_BAD]));
    if (n > h->ring_cap) FAIL(ESVO_ERR_CAPACITY, BLOCK_TOO_LARGE);
    if (n > h->col_cap[cam]) {  // the guess was too small: once more into staging that holds them
      { int rcs = columns_staging(h, cam, n); if (rcs) return rcs; }
      { int rcd = decode(); if (rcd) return rcd; }
    }
    f.end_state(hdr, st1);
    cnt.words = n_words; cnt.events = n; cnt.dropped_events = hdr[EVT3_H_DROPPED]; cnt.ignored_words = hdr[EVT3_H_IGNORED];
    cnt.ext_triggers = hdr[EVT3_H_EXT]; cnt.time_loops = hdr[EVT3_H_LOOPS];
    if (n == 0) { commit(); return ESVO_OK; }
    const ColumnBlock b = column_block(h->d_col[cam], h->col_cap[cam]);
    u64* const stamps = h->h_col_stamps[cam];
    const bool judged_on_device = h->flt[cam].on;  // under the event filter the order is judged by its last kernel: one read-back, the kept stamps
    bool in_order = true;
    if (!judged_on_device) {
      HIPCHK(hipMemcpyAsync(stamps, b.t, sizeof(u64) * n, hipMemcpyDeviceToHost, h->stream_i));
      HIPCHK(hipStreamSynchronize(h->stream_i));
      in_order = stamps_in_order(n, StampArray{stamps});
    }
    esvo_event_columns_t c{};
    c.x = b.x; c.y = b.y; c.p = b.p; c.t = b.t;
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
// esvo_evt3_to_events / esvo_evt2_to_events behind their own argument checks; full: the call's text where `out` has no room
template <class F>
int words_to_events(const F& f, typename F::State* st, const void* words, size_t n_words, int64_t t_offset_us, esvo_event_t* out, size_t cap, size_t* n_out,
                    esvo_evt3_counts_t* counts, const char* full) {
  esvo_context* h = nullptr;
  typename F::State s = *st;
  esvo_evt3_counts_t c{};
  const int rc = f.decode_host(s, words, n_words, t_offset_us, c, [&](const esvo_event_t& e) {
    if (!out) return true;
    if (c.events >= cap) return false;
    out[c.events] = e;
    return true;
  });
  if (n_out) *n_out = (size_t)c.events;
  if (rc == EVT3_DEC_BAD_STAMP) FAIL(ESVO_ERR_INVALID_ARG, words_bad_event(f.name(), (size_t)c.events));
  if (rc == EVT3_DEC_FULL) FAIL(ESVO_ERR_CAPACITY, full);
  *st = s;
  if (counts) *counts = c;
  return ESVO_OK;
}
// esvo_ts_evt3_stats / esvo_ts_evt2_stats; all: the handle's totals of that format, one per camera
int words_stats(esvo_handle h, int cam, esvo_evt3_counts_t (esvo_context::*all)[2], esvo_evt3_counts_t* totals) {
  if (!h || cam < 0 || cam > 1 || !totals) return ESVO_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lp(h->mu_push[cam]);
  *totals = (h->*all)[cam];
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

extern "C" {

int esvo_evt3_to_events(esvo_evt3_state_t* st, const uint16_t* words, size_t n_words, int64_t t_offset_us, esvo_event_t* out, size_t cap,
                        size_t* n_out, esvo_evt3_counts_t* counts) {
  if (n_out) *n_out = 0;
  if (!st || (n_words && !words) || (uintptr_t)words % 2) return ESVO_ERR_INVALID_ARG;
  return words_to_events(Evt3Format{}, st, words, n_words, t_offset_us, out, cap, n_out, counts,
                         "esvo_evt3_to_events: the words hold more events than `out` has room for");
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
  if (n_out) *n_out = 0;
  if (!st || !evt2_format_known(format) || (n_bytes && !words) || (uintptr_t)words % 4 || n_bytes % evt2_word_bytes(format)) return ESVO_ERR_INVALID_ARG;
  return words_to_events(Evt2Format{format}, st, words, n_bytes / evt2_word_bytes(format), t_offset_us, out, cap, n_out, counts,
                         "esvo_evt2_to_events: the words hold more events than `out` has room for");
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
int esvo_ts_evt2_stats(esvo_handle h, int cam, esvo_evt2_counts_t* totals) { return words_stats(h, cam, &esvo_context::evt2_totals, totals); }
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
int esvo_ts_evt3_stats(esvo_handle h, int cam, esvo_evt3_counts_t* totals) { return words_stats(h, cam, &esvo_context::evt3_totals, totals); }

int esvo_ts_push_evt3(esvo_handle h, int cam, const void* words_v, size_t n_bytes, int memory, int64_t t_offset_us, size_t* n_events) {
  if (n_events) *n_events = 0;
  if (!h || cam < 0 || cam > 1) return ESVO_ERR_INVALID_ARG;
  return push_words(h, cam, Evt3Format{}, words_v, n_bytes, memory, t_offset_us, n_events);
}

}  // extern "C"
