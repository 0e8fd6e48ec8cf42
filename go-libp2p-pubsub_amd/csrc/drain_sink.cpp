// drain_sink.cpp -- the sink (drain_impl.hpp): standing
// queries drained behind every window of a run, through the shared-list pass
// of drain_shared.cpp, into one result per run.  run.cpp calls the sink_*
// hooks; ps_sink_set registers the queries and ps_sink_take lends a result.
#include "drain_impl.hpp"

using namespace psamd;

namespace {

// A device buffer of the sink's result grown with its contents kept: the
// windows before have written there, on s.  (Not the steady state: the next
// run of the same shape finds the room.)
int sink_grow(ps_engine* e, DevBuf& buf, size_t need, hipStream_t s) {
  if (need <= buf.bytes) return PS_OK;
  DevBuf nb;
  HIP_TRY(nb.ensure(std::max(need, 2 * buf.bytes)), "alloc sink result");
  if (buf.bytes) {
    HIP_TRY(hipMemcpyAsync(nb.p, buf.p, buf.bytes, hipMemcpyDeviceToDevice, s), "move sink result");
    HIP_TRY(hipStreamSynchronize(s), "sync");
  }
  buf.swap(nb);
  return PS_OK;
}

constexpr size_t kSinkHdrBytes = 256;  // the cursors in front of list_off; the view's header
static_assert(2 * sizeof(SinkCursor) <= kSinkHdrBytes, "both cursors lie in front of list_off");

}  // namespace

// ---- the sink's run hooks (run.cpp calls them) ---------------

int psamd::sink_precheck(ps_engine* e) {
  auto& D = e->drain;
  auto& K = D.sink;
  if (!K.on) return PS_OK;
  if (K.count == 2) return e->fail(PS_E_STATE, "two sink results untaken: ps_sink_take first");
  if (K.list_cap || K.id_cap) return PS_OK;
  // the engine's id cap for this run at most: a topic's messages once, or once
  // per query where every query takes a private list
  std::vector<uint32_t> per_topic(e->topics.size(), 0);
  uint32_t most = 0;
  for (uint32_t t : K.topic) most = std::max(most, ++per_topic[t]);
  const bool paced = e->pending_nonzero_start;
  if (static_cast<uint64_t>(e->pending.size()) * ((!D.env.share || paced) ? most : 1u) <= kDrainAsyncMaxIds) return PS_OK;
  uint64_t bound = 0;
  for (const RunMsg& m : e->pending) {
    const bool priv = !D.env.share || (paced && e->topics[m.topic].kind == Kind::Children);
    bound += priv ? per_topic[m.topic] : (per_topic[m.topic] ? 1u : 0u);
  }
  if (bound > kDrainAsyncMaxIds) return e->fail(PS_E_RANGE, "the sink's result may exceed 2^30 ids: run smaller batches");
  return PS_OK;
}

int psamd::sink_open(ps_engine* e) {
  auto& K = e->drain.sink;
  if (!K.on) return PS_OK;
  HIP_TRY(hipSetDevice(e->cfg.device), "hipSetDevice");
  auto& R = K.res[(K.head + K.count) & 1];
  // (the slot's last run is complete: its result was taken or discarded)
  if (R.arena.size() > 1) {
    size_t cap = 0;
    for (auto& c : R.arena) {
      cap += c.cap;
      (void)hipHostFree(c.h);
    }
    R.arena.clear();
    uint8_t* h = nullptr;
    R.arena_used = 0;
    HIP_TRY(sink_stage(R, cap, &h), "alloc sink staging");
  }
  if (!R.ev_done) HIP_TRY(hipEventCreateWithFlags(&R.ev_done, hipEventDisableTiming), "sink event");
  R.arena_used = 0;
  R.windows = 0;
  R.list_cap = K.list_cap;
  R.id_cap = K.id_cap;
  R.enqueued = false;
  R.run = ++K.runs;
  K.open = &R;
  K.host_ms = 0;
  return PS_OK;
}

void psamd::sink_abort(ps_engine* e) {
  auto& K = e->drain.sink;
  if (!K.open) return;
  // the slot is given up: what its windows staged must have left the staging
  (void)hipStreamSynchronize(e->stream);
  K.runs_done = std::max(K.runs_done, K.open->run);
  K.open = nullptr;
}

// The window just remembered, drained into the open result: its tables (always
// built here: a later drain of the last window reuses them), the shared-list
// pass that ps_drain_shared_begin runs, then k_sink_commit and k_sink_emit at
// the run's cursor -- the counts never reach the host between windows.  All
// on `stream`; nothing waits.
int psamd::sink_window(ps_engine* e) {
  auto& D = e->drain;
  auto& K = D.sink;
  if (!K.open) return PS_OK;
  auto& R = *K.open;
  const auto t_host0 = hclock::now();
  const size_t n = K.topic.size();
  const uint32_t w = R.windows;
  if (const int rj = twin_join(e)) return rj;
  int rc = drain_ready(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  const uint32_t nt = static_cast<uint32_t>(e->topics.size());

  // the tables and the window's input in a region of the arena that no other
  // window of the run uses (a timed build waits for the stream: nothing of the sink may)
  const SharedLayout L(n, nt);
  size_t used = 0;
  uint8_t* h = nullptr;
  if ((rc = drain_tables_async(e, Staging{nullptr, &R}, L.tail, false, &used, &h))) return rc;

  // the sorted queries: the last window's while the node space and every
  // topic's window shape are the same
  std::vector<uint64_t> key{e->graph_epoch, nt, n};
  for (uint32_t t = 0; t < nt; ++t) {
    key.push_back(static_cast<uint64_t>(D.tab.topics[t].flags) << 32 | D.tab.topics[t].n_pos);
    key.push_back(e->last_cnt[t]);
  }
  if (key != K.sort_key) {
    K.sort_key.clear();
    K.sort_r = SharedSort{};
    K.sort_tail.assign(L.tail, 0);
    if (shared_stage(e, K.topic.data(), K.peer.data(), L, K.sort_tail.data(), &K.sort_r))
      return e->fail(PS_E_RANGE, "too many rows in one sink window");
    K.sort_key = key;
  }
  const SharedSort& S = K.sort_r;
  std::memcpy(h, K.sort_tail.data(), L.tail);

  // this window's caps (the caller's: the run's, for min(list_cap, rows)
  // lists a window), and the run's as far as this window
  const bool own = K.list_cap == 0 && K.id_cap == 0;
  size_t win_lists = std::min<size_t>(K.list_cap, S.n_rows), win_ids = 0;
  uint32_t seg_bound = 0;
  const bool rows_fit = shared_caps(D, S, n, own, &win_lists, &win_ids, &seg_bound);
  if (own) {
    R.list_cap += win_lists;
    R.id_cap += win_ids;
  }
  if (R.id_cap > kDrainAsyncMaxIds) return e->fail(PS_E_RANGE, "the sink's result may exceed 2^30 ids");
  if (!rows_fit || R.list_cap >= 0x7FFFFFFFull || (static_cast<uint64_t>(w) + 1) * n >= (1ull << 32))
    return e->fail(PS_E_RANGE, "too many rows in one sink window");

  // the result on the device: it grows with the windows, contents kept
  if ((rc = sink_grow(e, R.d_wl, (static_cast<size_t>(w) + 1) * n * 4, s)) ||
      (rc = sink_grow(e, R.d_off, kSinkHdrBytes + (R.list_cap + 1) * 8, s)) || (rc = sink_grow(e, R.d_ids, R.id_cap * 4, s)))
    return rc;
  SinkCursor* const cur = R.d_off.as<SinkCursor>();
  if (w == 0) HIP_TRY(hipMemsetAsync(cur, 0, kSinkHdrBytes, s), "clear sink cursor");

  // The window's lists, counted and scanned.  No row to read: a row of PS_NONE,
  // no list, and the cursor moves on by one window.
  auto& B = K.lb;
  HIP_TRY(K.d_lq.ensure(n * 4), "alloc sink lists");
  DrainArgs a{};
  DrainCtl* ctl = nullptr;
  if (S.n_rows == 0) {
    HIP_TRY(B.d_aux.ensure(sizeof(DrainCtl)), "alloc drain control");
    HIP_TRY(B.scratch.d_off.ensure(8), "alloc drain offsets");
    ctl = B.d_aux.as<DrainCtl>();
    if ((rc = drain_err_word(e, s))) return rc;
    if (n) HIP_TRY(hipMemsetAsync(K.d_lq.p, 0xFF, n * 4, s), "clear sink lists");
    HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(DrainCtl), s), "clear drain control");
    HIP_TRY(hipMemsetAsync(B.scratch.d_off.p, 0, 8, s), "clear drain offsets");
  } else {
    const PhaseTimer untimed{D.ev_t, s, false};
    float none[3] = {0, 0, 0};
    if ((rc = shared_pass(e, B, L, h, S, win_lists, seg_bound, K.d_lq.as<uint32_t>(), untimed, none, &a, &ctl))) return rc;
  }
  const uint64_t* const seg_off = B.scratch.d_off.as<uint64_t>();
  SinkCommit c{};
  c.lists = a.queries;  // (not read where the window has no list)
  c.ctl = ctl;
  c.seg_off = seg_off;
  c.win_lq = K.d_lq.as<uint32_t>();
  c.err = D.tab.d_err;
  c.cur = cur;
  c.list_off = reinterpret_cast<uint64_t*>(R.d_off.as<uint8_t>() + kSinkHdrBytes);
  c.win_list = R.d_wl.as<uint32_t>();
  c.w = w;
  c.n = static_cast<uint32_t>(n);
  c.win_list_cap = S.n_rows ? static_cast<uint32_t>(win_lists) : 0;
  c.list_cap = static_cast<uint32_t>(R.list_cap);
  c.id_cap = R.id_cap;
  HIP_TRY(launch_sink_commit(c, s), "k_sink_commit");
  if (S.n_rows)
    HIP_TRY(launch_sink_emit(a, ctl, cur, w, seg_bound, seg_off, R.d_ids.as<uint32_t>(), R.id_cap, s), "k_sink_emit");

  // the last reader of this window's rows on `stream` (run.cpp: drain_fence):
  // the entry of this row set, else one whose row set is gone
  Drain::Sink::Fence* F = nullptr;
  for (auto& f : K.fence)
    if (f.seen == e->rows.seen.p) F = &f;
  for (auto& f : K.fence)
    if (!F && (!f.seen || f.seen != e->rows_other.seen.p)) F = &f;
  if (!F) return e->fail(PS_E_STATE, "sink: no fence entry for the row set");
  if (!F->ev) HIP_TRY(hipEventCreateWithFlags(&F->ev, kStreamEvent), "sink event");
  HIP_TRY(hipEventRecord(F->ev, s), "event");
  F->seen = e->rows.seen.p;
  F->run = R.run;
  K.last_ev = F->ev;
  R.windows = w + 1;
  K.host_ms += ms_since(t_host0);
  return PS_OK;
}

// The run's result leaves behind its last window: the cursor that window
// left (the header), win_list, list_off and the ids, on the copy stream.
int psamd::sink_close(ps_engine* e) {
  auto& D = e->drain;
  auto& K = D.sink;
  if (!K.open) return PS_OK;
  auto& R = *K.open;
  const auto t_host0 = hclock::now();
  const size_t n = K.topic.size();
  R.o_wl = kSinkHdrBytes;
  R.o_off = R.o_wl + align256(static_cast<size_t>(R.windows) * n * 4);
  R.o_ids = R.o_off + align256((R.list_cap + 1) * 8);
  const size_t res_bytes = R.o_ids + R.id_cap * 4;
  HIP_TRY(pinned_ensure(&R.h_res, nullptr, &R.res_cap, res_bytes), "alloc sink view");
  if (R.windows == 0) {  // no window ran: an empty result, written here
    std::memset(R.h_res, 0, kSinkHdrBytes);
    std::memset(R.h_res + R.o_off, 0, 8);
  } else {
    hipStream_t cs = D.copy_stream;
    const uint8_t* const d_off = R.d_off.as<uint8_t>();
    HIP_TRY(hipStreamWaitEvent(cs, K.last_ev, 0), "wait");
    HIP_TRY(hipMemcpyAsync(R.h_res, d_off + (R.windows & 1) * sizeof(SinkCursor), sizeof(SinkCursor), hipMemcpyDeviceToHost, cs),
            "read sink header");
    if (n)
      HIP_TRY(hipMemcpyAsync(R.h_res + R.o_wl, R.d_wl.p, static_cast<size_t>(R.windows) * n * 4, hipMemcpyDeviceToHost, cs),
              "read sink lists");
    HIP_TRY(hipMemcpyAsync(R.h_res + R.o_off, d_off + kSinkHdrBytes, (R.list_cap + 1) * 8, hipMemcpyDeviceToHost, cs),
            "read sink offsets");
    if (R.id_cap)
      HIP_TRY(hipMemcpyAsync(R.h_res + R.o_ids, R.d_ids.p, R.id_cap * 4, hipMemcpyDeviceToHost, cs), "read sink ids");
    HIP_TRY(hipEventRecord(R.ev_done, cs), "event");
    R.enqueued = true;
  }
  K.open = nullptr;
  ++K.count;
  if (D.env.timing)
    std::fprintf(stderr, "psamd sink: queries %zu windows %u list_cap %zu id_cap %zu view_bytes %zu host_us %.1f\n", n,
                 R.windows, R.list_cap, R.id_cap, res_bytes, 1e3 * (K.host_ms + ms_since(t_host0)));
  return PS_OK;
}

extern "C" {

// ---- ps_sink_set / ps_sink_take ----------------------------

int ps_sink_set(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, size_t list_cap, size_t id_cap) {
  if (!e || (n && (!topic || !peer))) return PS_E_INVAL;
  if (e->world > 1) return e->fail(PS_E_STATE, "ps_sink_set on a multi-rank engine");
  if (e->infl_count) return e->fail(PS_E_STATE, "a run in flight: ps_wait first");
  if (const int rq = drain_check_queries(e, topic, peer, n)) return rq;
  if (n >= 0x7FFFFFFFull || list_cap >= 0x7FFFFFFFull) return e->fail(PS_E_RANGE, "too many queries or lists");
  if (id_cap > kDrainAsyncMaxIds) return e->fail(PS_E_RANGE, "a sink result holds 2^30 ids at most");
  auto& D = e->drain;
  auto& K = D.sink;
  // results not yet taken are discarded: whatever still fills them ends first
  if (K.runs) {
    HIP_TRY(hipStreamSynchronize(e->stream), "sync");
    if (D.copy_stream) HIP_TRY(hipStreamSynchronize(D.copy_stream), "sync");
  }
  K.head = K.count = 0;
  K.runs_done = K.runs;
  for (auto& r : K.res) r.enqueued = false;
  K.sort_key.clear();
  K.topic.assign(topic, topic + n);
  K.peer.assign(peer, peer + n);
  K.list_cap = list_cap;
  K.id_cap = id_cap;
  K.on = n > 0;
  return PS_OK;
}

int ps_sink_take(ps_engine* e, const uint32_t** win_list_out, const uint64_t** list_off_out, const uint32_t** msg_out,
                 uint32_t* n_windows_out, uint32_t* n_lists_out, uint64_t* total_out) {
  if (!e || !win_list_out || !list_off_out || !msg_out || !n_windows_out || !n_lists_out || !total_out) return PS_E_INVAL;
  auto& K = e->drain.sink;
  if (K.count == 0) return e->fail(PS_E_NOTREADY, "no sink result outstanding");
  auto& R = K.res[K.head];
  K.head ^= 1;
  --K.count;
  if (R.enqueued) {
    HIP_TRY(hipEventSynchronize(R.ev_done), "wait for the sink result");
    R.enqueued = false;
  }
  K.runs_done = std::max(K.runs_done, R.run);  // (its emits are complete: drain_fence waits for none of them)
  const SinkCursor* hdr = reinterpret_cast<const SinkCursor*>(R.h_res);
  *win_list_out = reinterpret_cast<const uint32_t*>(R.h_res + R.o_wl);
  *list_off_out = reinterpret_cast<const uint64_t*>(R.h_res + R.o_off);
  *msg_out = reinterpret_cast<const uint32_t*>(R.h_res + R.o_ids);
  *n_windows_out = hdr->windows;
  *n_lists_out = hdr->lists;
  *total_out = hdr->ids;
  if (hdr->windows != R.windows) return e->fail(PS_E_STATE, "sink: the result's window count is not the run's");
  return drain_view_status(e, hdr->err, hdr->over);
}

}  // extern "C"
