// drain_sink.cpp -- the sink (drain_impl.hpp): standing
// queries drained behind every window of a run, through the shared-list pass
// of drain_shared.cpp, into one result per run.  run.cpp calls the sink_*
// hooks; ps_sink_set registers the queries and ps_sink_take lends a result.
// And the audience sink (§5.5h): standing topics drained behind every window
// through the audience pass of drain_topics.cpp, ps_sink_set_topics /
// ps_sink_take_topics.  An engine has one sink, of one kind (Sink::kind): the
// hooks dispatch on it, and the slots, the fence and the arena serve both.
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

// The last reader of the window's rows on `stream` (run.cpp: drain_fence),
// recorded behind the window's last kernel: the entry of this row set, else
// one whose row set is gone.  The window then counts.
int sink_fence(ps_engine* e, Drain::Sink::Res& R) {
  auto& K = e->drain.sink;
  hipStream_t s = e->stream;
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
  R.windows += 1;
  return PS_OK;
}

}  // namespace

// ---- the sink's run hooks (run.cpp calls them) ---------------

int psamd::sink_precheck(ps_engine* e) {
  auto& D = e->drain;
  auto& K = D.sink;
  if (!K.on) return PS_OK;
  if (K.count == 2)
    return e->fail(PS_E_STATE, K.kind == Drain::Sink::kTopics ? "two sink results untaken: ps_sink_take_topics first"
                                                              : "two sink results untaken: ps_sink_take first");
  if (K.kind == Drain::Sink::kTopics) {
    // the engine's id cap for this run at most: a named tree topic's messages
    // once; once per non-root node (the peers at most) where every node takes
    // a private list
    if (K.id_cap) return PS_OK;
    const bool paced = e->pending_nonzero_start;
    const uint64_t nodes = e->cfg.n_peers;
    if (static_cast<uint64_t>(e->pending.size()) * ((!D.env.share || paced) ? nodes : 1u) <= kDrainAsyncMaxIds) return PS_OK;
    std::vector<uint8_t> named(e->topics.size(), 0);
    for (uint32_t t : K.topic) named[t] = 1;
    uint64_t bound = 0;
    for (const RunMsg& m : e->pending) {
      if (!named[m.topic]) continue;
      const bool priv = !D.env.share || (paced && e->topics[m.topic].kind == Kind::Children);
      bound += priv ? nodes : 1u;
    }
    if (bound > kDrainAsyncMaxIds) return e->fail(PS_E_RANGE, "the sink's result may exceed 2^30 ids: run smaller batches");
    return PS_OK;
  }
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
  R.exc_cap = K.exc_cap;
  R.n_nodes.clear();
  K.strip_bytes = 0;
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
static int sink_window_queries(ps_engine* e) {
  auto& D = e->drain;
  auto& K = D.sink;
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

  if ((rc = sink_fence(e, R))) return rc;
  K.host_ms += ms_since(t_host0);
  return PS_OK;
}

// The audience sink's window (ps_sink_set_topics): the tables,
// the audience pass that ps_drain_topics_begin runs over the standing topics
// -- its entries and strips read where the last window left them on the
// device while what they are cut from stays, else re-cut into the arena and
// uploaded on `stream`, behind the last window's readers -- into a
// window-local view, then k_audience_sink_commit and k_sink_emit at the run's
// cursor.  All on `stream`; nothing waits.
static int sink_window_topics(ps_engine* e) {
  auto& D = e->drain;
  auto& K = D.sink;
  auto& R = *K.open;
  const auto t_host0 = hclock::now();
  const size_t n = K.topic.size();
  const uint32_t* const topic = K.topic.data();
  const uint32_t w = R.windows;
  if (const int rj = twin_join(e)) return rj;
  int rc = drain_ready(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  size_t used = 0;
  uint8_t* h = nullptr;
  if ((rc = drain_tables_async(e, Staging{nullptr, &R}, 0, false, &used, &h))) return rc;

  // the entries and the strips: the device's while the node space and every
  // standing topic's table shape and node range are the same
  std::vector<uint64_t> key{e->graph_epoch, n};
  for (size_t i = 0; i < n; ++i) {
    const DrainTopic& T = D.tab.topics[topic[i]];
    uint32_t u0 = 0;
    const uint32_t nn = aud_nodes(e, topic[i], &u0);
    key.push_back(static_cast<uint64_t>(T.flags) << 32 | T.n_pos);
    key.push_back(static_cast<uint64_t>(nn) << 32 | e->last_topics[topic[i]].nbase);
    key.push_back(u0);
  }
  const size_t o_strips = align256((n + 1) * sizeof(AudEntry));
  AudShape A;
  if (key == K.strip_key) {
    aud_stage(e, topic, n, nullptr, nullptr, ~0ull, &A);  // (the shape and the window's own caps alone)
  } else {
    K.strip_key.clear();
    size_t o = 0;
    uint64_t strips_max = 0;
    const size_t bytes = aud_stage_bytes(e, topic, n, &o, &strips_max);
    if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one sink window");
    uint8_t* hs = nullptr;
    HIP_TRY(sink_stage(R, bytes, &hs), "alloc sink staging");
    if (!aud_stage(e, topic, n, reinterpret_cast<AudEntry*>(hs), reinterpret_cast<AudStrip*>(hs + o_strips), strips_max, &A))
      return e->fail(PS_E_STATE, "audience: more strips than staged");
    const size_t in_bytes = o_strips + static_cast<size_t>(A.ns) * sizeof(AudStrip);
    HIP_TRY(K.d_strips.ensure(in_bytes), "alloc sink strips");
    HIP_TRY(hipMemcpyAsync(K.d_strips.p, hs, in_bytes, hipMemcpyHostToDevice, s), "upload audience strips");
    K.strip_bytes += in_bytes;
    K.strip_key = key;
  }
  for (size_t i = 0; i < n; ++i) {
    uint32_t u0 = 0;
    R.n_nodes.push_back(aud_nodes(e, topic[i], &u0));
  }

  // this window's caps (the engine's where the caller named none, else the
  // caller's for the run, no more than a window can fill), and the run's as
  // far as this window
  size_t win_exc = K.exc_cap ? std::min<uint64_t>(K.exc_cap, std::max<uint64_t>(A.n_verdicts, 1)) : 0;
  size_t win_lists = K.list_cap ? std::min<uint64_t>(K.list_cap, std::max<uint64_t>(n + A.n_verdicts, 1)) : 0;
  size_t win_ids = K.id_cap;
  uint32_t seg_bound = 0;
  const bool rows_fit = aud_caps(A, n, &win_exc, &win_lists, &win_ids, &seg_bound);
  if (!K.exc_cap) R.exc_cap += win_exc;
  if (!K.list_cap) R.list_cap += win_lists;
  if (!K.id_cap) R.id_cap += win_ids;
  if (R.id_cap > kDrainAsyncMaxIds) return e->fail(PS_E_RANGE, "the sink's result may exceed 2^30 ids");
  if (!rows_fit || R.list_cap >= 0x7FFFFFFFull || R.exc_cap >= 0x7FFFFFFFull ||
      (static_cast<uint64_t>(w) + 1) * n >= (1ull << 32))
    return e->fail(PS_E_RANGE, "too many rows in one sink window");

  // the result on the device: it grows with the windows, contents kept
  const size_t rows = (static_cast<size_t>(w) + 1) * n;
  if ((rc = sink_grow(e, R.d_wl, rows * 4, s)) || (rc = sink_grow(e, R.d_nf, rows * 8, s)) ||
      (rc = sink_grow(e, R.d_eo, (rows + 1) * 8, s)) || (rc = sink_grow(e, R.d_ep, R.exc_cap * 4, s)) ||
      (rc = sink_grow(e, R.d_el, R.exc_cap * 4, s)) ||
      (rc = sink_grow(e, R.d_off, kSinkHdrBytes + (R.list_cap + 1) * 8, s)) || (rc = sink_grow(e, R.d_ids, R.id_cap * 4, s)))
    return rc;
  SinkCursor* const cur = R.d_off.as<SinkCursor>();
  if (w == 0) HIP_TRY(hipMemsetAsync(cur, 0, kSinkHdrBytes, s), "clear sink cursor");

  // the window-local view: topic_list | n_full | exc_off | exc_peer | exc_list
  const size_t v_nf = align256(n * 4), v_eo = v_nf + align256(n * 8), v_ep = v_eo + align256((n + 1) * 8);
  const size_t v_el = v_ep + align256(win_exc * 4);
  HIP_TRY(K.d_view.ensure(v_el + align256(win_exc * 4)), "alloc sink view");
  uint8_t* const dv = K.d_view.as<uint8_t>();
  const AudView view{reinterpret_cast<uint32_t*>(dv), reinterpret_cast<uint64_t*>(dv + v_nf),
                     reinterpret_cast<uint64_t*>(dv + v_eo), reinterpret_cast<uint32_t*>(dv + v_ep),
                     reinterpret_cast<uint32_t*>(dv + v_el)};
  auto& B = K.lb;
  DrainArgs a{};
  DrainCtl* ctl = nullptr;
  if ((rc = drain_err_word(e, s))) return rc;
  if (A.ns == 0) {  // no row to read: a row of PS_NONE, no exception, no list; the cursor moves on by one window
    HIP_TRY(B.d_aux.ensure(align256(sizeof(DrainCtl))), "alloc drain control");
    HIP_TRY(B.scratch.d_off.ensure(8), "alloc drain offsets");
    ctl = B.d_aux.as<DrainCtl>();
    HIP_TRY(hipMemsetAsync(dv, 0, v_ep, s), "clear sink view");
    if (n) HIP_TRY(hipMemsetAsync(dv, 0xFF, n * 4, s), "clear sink lists");
    HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(DrainCtl), s), "clear drain control");
    HIP_TRY(hipMemsetAsync(B.scratch.d_off.p, 0, 8, s), "clear drain offsets");
    seg_bound = 0;
  } else {
    const PhaseTimer untimed{D.ev_t, s, false};
    float none[6] = {0, 0, 0, 0, 0, 0};
    const AudBufs bufs{&B, &K.d_verdict, &K.d_exc, &K.d_full, &K.d_rec};
    const uint8_t* const din = K.d_strips.as<uint8_t>();
    if ((rc = aud_pass(e, bufs, reinterpret_cast<const AudEntry*>(din), reinterpret_cast<const AudStrip*>(din + o_strips),
                       n, A, win_exc, win_lists, seg_bound, view, untimed, none, &a, &ctl)))
      return rc;
  }
  const uint64_t* const seg_off = B.scratch.d_off.as<uint64_t>();
  AudSinkCommit c{};
  c.lists = a.queries;  // (not read where the window has no list)
  c.ctl = ctl;
  c.seg_off = seg_off;
  c.win_topic_list = view.topic_list;
  c.win_n_full = view.n_full;
  c.win_exc_off = view.exc_off;
  c.win_exc_peer = view.exc_peer;
  c.win_exc_list = view.exc_list;
  c.err = D.tab.d_err;
  c.cur = cur;
  c.list_off = reinterpret_cast<uint64_t*>(R.d_off.as<uint8_t>() + kSinkHdrBytes);
  c.topic_list = R.d_wl.as<uint32_t>();
  c.n_full = R.d_nf.as<uint64_t>();
  c.exc_off = R.d_eo.as<uint64_t>();
  c.exc_peer = R.d_ep.as<uint32_t>();
  c.exc_list = R.d_el.as<uint32_t>();
  c.w = w;
  c.n = static_cast<uint32_t>(n);
  c.win_list_cap = A.ns ? static_cast<uint32_t>(win_lists) : 0;
  c.win_exc_cap = A.ns ? static_cast<uint32_t>(win_exc) : 0;
  c.list_cap = static_cast<uint32_t>(R.list_cap);
  c.exc_cap = static_cast<uint32_t>(R.exc_cap);
  c.id_cap = R.id_cap;
  HIP_TRY(launch_audience_sink_commit(c, s), "k_audience_sink_commit");
  if (A.ns) HIP_TRY(launch_sink_emit(a, ctl, cur, w, seg_bound, seg_off, R.d_ids.as<uint32_t>(), R.id_cap, s), "k_sink_emit");
  // classify reads every row of the named topics: the event is recorded
  // whether or not the window has a segment to emit
  if ((rc = sink_fence(e, R))) return rc;
  K.host_ms += ms_since(t_host0);
  return PS_OK;
}

int psamd::sink_window(ps_engine* e) {
  auto& K = e->drain.sink;
  if (!K.open) return PS_OK;
  return K.kind == Drain::Sink::kTopics ? sink_window_topics(e) : sink_window_queries(e);
}

// The audience sink's result: the cursor (the header), the rows, the records,
// list_off and the ids, on the copy stream; the n_nodes rows, which the host
// knows, into the view behind what the copies bring.
static int sink_close_topics(ps_engine* e) {
  auto& D = e->drain;
  auto& K = D.sink;
  auto& R = *K.open;
  const auto t_host0 = hclock::now();
  const size_t n = K.topic.size();
  const size_t rows = static_cast<size_t>(R.windows) * n;
  R.o_wl = kSinkHdrBytes;
  R.o_nf = R.o_wl + align256(rows * 4);
  R.o_eo = R.o_nf + align256(rows * 8);
  R.o_ep = R.o_eo + align256((rows + 1) * 8);
  R.o_el = R.o_ep + align256(R.exc_cap * 4);
  R.o_off = R.o_el + align256(R.exc_cap * 4);
  R.o_ids = R.o_off + align256((R.list_cap + 1) * 8);
  const size_t res_bytes = R.o_ids + R.id_cap * 4;
  R.o_nn = align256(res_bytes);
  HIP_TRY(pinned_ensure(&R.h_res, nullptr, &R.res_cap, R.o_nn + std::max<size_t>(rows, 1) * 8), "alloc sink view");
  if (rows) std::memcpy(R.h_res + R.o_nn, R.n_nodes.data(), rows * 8);
  if (R.windows == 0) {  // no window ran: an empty result, written here
    std::memset(R.h_res, 0, kSinkHdrBytes);
    std::memset(R.h_res + R.o_eo, 0, 8);
    std::memset(R.h_res + R.o_off, 0, 8);
  } else {
    hipStream_t cs = D.copy_stream;
    const uint8_t* const d_off = R.d_off.as<uint8_t>();
    HIP_TRY(hipStreamWaitEvent(cs, K.last_ev, 0), "wait");
    HIP_TRY(hipMemcpyAsync(R.h_res, d_off + (R.windows & 1) * sizeof(SinkCursor), sizeof(SinkCursor), hipMemcpyDeviceToHost, cs),
            "read sink header");
    if (rows) {
      HIP_TRY(hipMemcpyAsync(R.h_res + R.o_wl, R.d_wl.p, rows * 4, hipMemcpyDeviceToHost, cs), "read sink lists");
      HIP_TRY(hipMemcpyAsync(R.h_res + R.o_nf, R.d_nf.p, rows * 8, hipMemcpyDeviceToHost, cs), "read sink totals");
    }
    HIP_TRY(hipMemcpyAsync(R.h_res + R.o_eo, R.d_eo.p, (rows + 1) * 8, hipMemcpyDeviceToHost, cs), "read sink exceptions");
    if (R.exc_cap) {
      HIP_TRY(hipMemcpyAsync(R.h_res + R.o_ep, R.d_ep.p, R.exc_cap * 4, hipMemcpyDeviceToHost, cs), "read sink exceptions");
      HIP_TRY(hipMemcpyAsync(R.h_res + R.o_el, R.d_el.p, R.exc_cap * 4, hipMemcpyDeviceToHost, cs), "read sink exceptions");
    }
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
    std::fprintf(stderr,
                 "psamd sink_topics: topics %zu windows %u exc_cap %zu list_cap %zu id_cap %zu strips %s upload_bytes %zu "
                 "view_bytes %zu host_us %.1f\n",
                 n, R.windows, R.exc_cap, R.list_cap, R.id_cap,
                 R.windows == 0 ? "none" : (K.strip_bytes ? "uploaded" : "kept"), K.strip_bytes, res_bytes,
                 1e3 * (K.host_ms + ms_since(t_host0)));
  return PS_OK;
}

// The run's result leaves behind its last window: the cursor that window
// left (the header), win_list, list_off and the ids, on the copy stream.
int psamd::sink_close(ps_engine* e) {
  auto& D = e->drain;
  auto& K = D.sink;
  if (!K.open) return PS_OK;
  if (K.kind == Drain::Sink::kTopics) return sink_close_topics(e);
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

// One sink per engine, of one kind: either set call replaces whatever sink
// stands (n == 0: clears it).  Results not yet taken are discarded: whatever
// still fills them ends first.
static int sink_replace(ps_engine* e, Drain::Sink::Kind kind, const uint32_t* topic, const uint32_t* peer, size_t n,
                        size_t exc_cap, size_t list_cap, size_t id_cap) {
  auto& D = e->drain;
  auto& K = D.sink;
  if (K.runs) {
    HIP_TRY(hipStreamSynchronize(e->stream), "sync");
    if (D.copy_stream) HIP_TRY(hipStreamSynchronize(D.copy_stream), "sync");
  }
  K.head = K.count = 0;
  K.runs_done = K.runs;
  for (auto& r : K.res) r.enqueued = false;
  K.sort_key.clear();
  K.strip_key.clear();
  K.kind = kind;
  K.topic.assign(topic, topic + n);
  K.peer.assign(peer, peer + (peer ? n : 0));
  K.exc_cap = exc_cap;
  K.list_cap = list_cap;
  K.id_cap = id_cap;
  K.on = n > 0;
  return PS_OK;
}

// the take calls: the oldest untaken result of `kind`, completed
static int sink_take_oldest(ps_engine* e, Drain::Sink::Kind kind, Drain::Sink::Res** out) {
  auto& K = e->drain.sink;
  if (K.count == 0) return e->fail(PS_E_NOTREADY, "no sink result outstanding");
  if (K.kind != kind)
    return e->fail(PS_E_STATE, kind == Drain::Sink::kTopics ? "the sink holds queries: ps_sink_take"
                                                            : "the sink holds topics: ps_sink_take_topics");
  auto& R = K.res[K.head];
  K.head ^= 1;
  --K.count;
  if (R.enqueued) {
    HIP_TRY(hipEventSynchronize(R.ev_done), "wait for the sink result");
    R.enqueued = false;
  }
  K.runs_done = std::max(K.runs_done, R.run);  // (its emits are complete: drain_fence waits for none of them)
  *out = &R;
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
  return sink_replace(e, Drain::Sink::kQueries, topic, peer, n, 0, list_cap, id_cap);
}

int ps_sink_take(ps_engine* e, const uint32_t** win_list_out, const uint64_t** list_off_out, const uint32_t** msg_out,
                 uint32_t* n_windows_out, uint32_t* n_lists_out, uint64_t* total_out) {
  if (!e || !win_list_out || !list_off_out || !msg_out || !n_windows_out || !n_lists_out || !total_out) return PS_E_INVAL;
  Drain::Sink::Res* res = nullptr;
  if (const int rc = sink_take_oldest(e, Drain::Sink::kQueries, &res)) return rc;
  auto& R = *res;
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

// ---- ps_sink_set_topics / ps_sink_take_topics ----------------

int ps_sink_set_topics(ps_engine* e, const uint32_t* topic, size_t n, size_t exc_cap, size_t list_cap, size_t id_cap) {
  if (!e || (n && !topic)) return PS_E_INVAL;
  if (e->world > 1) return e->fail(PS_E_STATE, "ps_sink_set_topics on a multi-rank engine");
  if (e->infl_count) return e->fail(PS_E_STATE, "a run in flight: ps_wait first");
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  if (exc_cap >= 0x7FFFFFFFull || list_cap >= 0x7FFFFFFFull) return e->fail(PS_E_RANGE, "too many exceptions or lists");
  if (id_cap > kDrainAsyncMaxIds) return e->fail(PS_E_RANGE, "a sink result holds 2^30 ids at most");
  return sink_replace(e, Drain::Sink::kTopics, topic, nullptr, n, exc_cap, list_cap, id_cap);
}

int ps_sink_take_topics(ps_engine* e, const uint32_t** topic_list_out, const uint64_t** n_nodes_out,
                        const uint64_t** n_full_out, const uint64_t** exc_off_out, const uint32_t** exc_peer_out,
                        const uint32_t** exc_list_out, const uint64_t** list_off_out, const uint32_t** msg_out,
                        uint32_t* n_windows_out, uint32_t* n_lists_out, uint64_t* total_out) {
  if (!e || !topic_list_out || !n_nodes_out || !n_full_out || !exc_off_out || !exc_peer_out || !exc_list_out ||
      !list_off_out || !msg_out || !n_windows_out || !n_lists_out || !total_out)
    return PS_E_INVAL;
  Drain::Sink::Res* res = nullptr;
  if (const int rc = sink_take_oldest(e, Drain::Sink::kTopics, &res)) return rc;
  auto& R = *res;
  const SinkCursor* hdr = reinterpret_cast<const SinkCursor*>(R.h_res);
  *topic_list_out = reinterpret_cast<const uint32_t*>(R.h_res + R.o_wl);
  *n_nodes_out = reinterpret_cast<const uint64_t*>(R.h_res + R.o_nn);
  *n_full_out = reinterpret_cast<const uint64_t*>(R.h_res + R.o_nf);
  *exc_off_out = reinterpret_cast<const uint64_t*>(R.h_res + R.o_eo);
  *exc_peer_out = reinterpret_cast<const uint32_t*>(R.h_res + R.o_ep);
  *exc_list_out = reinterpret_cast<const uint32_t*>(R.h_res + R.o_el);
  *list_off_out = reinterpret_cast<const uint64_t*>(R.h_res + R.o_off);
  *msg_out = reinterpret_cast<const uint32_t*>(R.h_res + R.o_ids);
  *n_windows_out = hdr->windows;
  *n_lists_out = hdr->lists;
  *total_out = hdr->ids;
  if (hdr->windows != R.windows) return e->fail(PS_E_STATE, "sink: the result's window count is not the run's");
  return drain_view_status(e, hdr->err, hdr->over);
}

}  // extern "C"
