// drain_tables.cpp -- what the batched drain keeps per window, not per call
// (drain_impl.hpp): the checks every entry point starts with,
// the window's tables (built on the host or on the device), the resolution of
// queries against them, the count + scan every path runs, the pinned staging.
#include "drain_impl.hpp"

namespace psamd {

// grow-only pinned memory (device-mapped); the old contents are dropped
hipError_t pinned_ensure(uint8_t** h, uint8_t** d, size_t* cap, size_t need) {
  if (need <= *cap) return hipSuccess;
  if (*h) (void)hipHostFree(*h);
  *h = nullptr;
  *cap = 0;
  void* p = nullptr;
  hipError_t rc = hipHostMalloc(&p, std::max<size_t>(need + need / 2, 64 << 10), hipHostMallocMapped | hipHostMallocCoherent);
  if (rc != hipSuccess) return rc;
  *h = static_cast<uint8_t*>(p);
  *cap = std::max<size_t>(need + need / 2, 64 << 10);
  if (d) {
    void* dp = nullptr;
    rc = hipHostGetDevicePointer(&dp, p, 0);
    *d = static_cast<uint8_t*>(dp);
  }
  return rc;
}

// `bytes` of the sink result's pinned staging that no other window of its run
// uses: several windows stage before any of their uploads has run.  A chunk
// too small is left as it is (uploads may still read it) and a larger one
// added; sink_open folds them into one once the run before is complete.
hipError_t sink_stage(Drain::Sink::Res& R, size_t bytes, uint8_t** out) {
  bytes = align256(bytes);
  if (R.arena.empty() || R.arena_used + bytes > R.arena.back().cap) {
    size_t cap = std::max<size_t>(bytes, 64 << 10);
    if (!R.arena.empty()) cap = std::max(cap, 2 * R.arena.back().cap);
    void* p = nullptr;
    const hipError_t rc = hipHostMalloc(&p, cap, hipHostMallocMapped | hipHostMallocCoherent);
    if (rc != hipSuccess) return rc;
    R.arena.push_back({static_cast<uint8_t*>(p), cap});
    R.arena_used = 0;
  }
  *out = R.arena.back().h + R.arena_used;
  R.arena_used += bytes;
  return hipSuccess;
}

// What every entry point needs after its own state checks: the node-space
// mirrors (the peer maps read them), the drain's stream and events
int drain_ready(ps_engine* e) {
  if (const int rc = ensure_mirrors(e)) return rc;
  auto& D = e->drain;
  if (D.copy_stream) return PS_OK;
  for (auto& ev : D.sync.ev_emit) HIP_TRY(hipEventCreateWithFlags(&ev, kStreamEvent), "drain event");
  for (auto& ev : D.sync.ev_copy) HIP_TRY(hipEventCreateWithFlags(&ev, kStreamEvent), "drain event");
  for (auto& ev : D.ev_t) HIP_TRY(hipEventCreate(&ev), "drain event");
  HIP_TRY(hipStreamCreateWithFlags(&D.copy_stream, hipStreamNonBlocking), "drain copy stream");
  return PS_OK;
}

int drain_check_queries(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n) {
  for (size_t q = 0; q < n; ++q)
    if (topic[q] >= e->topics.size() || peer[q] >= e->cfg.n_peers) return e->fail(PS_E_RANGE, "topic or peer out of range");
  return PS_OK;
}

// The state checks of a query-taking call, in the order of DrainEntry: the
// engine's ranks, the window, the slots, then (c.join) the twin and the
// queries' ranges.  The caller has checked its pointers, which reads nothing
// through e, and keeps its own limit on n: value, operands and text differ by
// call, and the synchronous calls test it behind their return for n == 0.
int drain_enter(ps_engine* e, const DrainEntry& c, const uint32_t* topic, const uint32_t* peer, size_t n) {
  if (c.multi_rank && e->world > 1) return e->fail(PS_E_STATE, c.multi_rank);
  if (!e->have_window) return e->fail(PS_E_NOTREADY, c.no_window);
  if (c.slots_full && e->drain.slot_count == 2) return e->fail(PS_E_STATE, c.slots_full);
  if (c.join)
    if (const int rj = twin_join(e)) return rj;
  return drain_check_queries(e, topic, peer, n);
}

namespace {

// the layout of topic t's rows in the last window; its start groups go to `groups`
DrainTopic drain_topic_header(const ps_engine* e, uint32_t t, std::vector<DrainGroup>& groups) {
  const TopicDev& d = e->last_topics[t];
  DrainTopic T{};
  T.wbase = d.wbase;
  T.nbase = d.nbase;
  T.n_nodes = d.n_nodes;
  T.W = d.W;
  T.flags = d.flags & (kTopicMesh | kTopicGroups);
  if (d.flags & kTopicGroups) {
    T.group_lo = static_cast<uint32_t>(groups.size());
    for (const StartGroup& g : e->last_groups[t]) groups.push_back({g.w0, g.wn});
    T.group_n = static_cast<uint32_t>(groups.size()) - T.group_lo;
  }
  return T;
}

}  // namespace

// ---- the two table builds ------------------------------------------------------
//
// drain_tables (host) serves the synchronous calls, drain_tables_async (device)
// the begin calls and the sink; whichever runs first in a window builds the
// tables all of them read.  They stay two implementations: the tests compare
// the device build against the host's.  They do not decide
// alike which topics take the arrival-order layout (kDrainGather):
//  - the host build looks at the window: a topic is kDrainGather where its
//    row bits do not ascend with (start round, publish order);
//  - the device build looks at the plan: every mesh topic of a run with a
//    non-zero start round is kDrainGather, ascending or not.
// A mesh window whose start rounds happen to ascend with publish order so
// gets a mask table from the host and an arrival-order table from the device.
// Every query's ids are the same from both; the list structure ps_drain_shared
// and its kin return (which queries share a list) depends on the build that
// ran first in that window.

// The last window's drain tables, once per window, built on the host.  A
// topic's window messages by row bit: where (start round, publish order)
// ascends with the bit -- every tree layout (plan_window_layout sorts the bits
// so) -- the id table is indexed by bit and a mask marks the message bits;
// else (a mesh window with several start rounds) the ids are stored in
// arrival order beside each one's bit.  A build that fails leaves Tables::seq at
// its older value.
int drain_tables(ps_engine* e) {
  auto& D = e->drain.tab;
  if (D.seq == e->window_seq) return PS_OK;
  const uint32_t nt = static_cast<uint32_t>(e->topics.size());
  struct Ent {
    uint64_t key;  // start round << 32 | message index: arrival order
    uint32_t b, id;
  };
  std::vector<Ent> P;
  std::vector<uint32_t> ids, order;
  std::vector<uint64_t> mask;
  std::vector<DrainGroup> groups;
  D.topics.assign(nt, DrainTopic{});
  for (uint32_t t = 0; t < nt; ++t) {
    const TopicDev& d = e->last_topics[t];
    if (!d.W || !e->last_cnt[t]) continue;
    const WinSlice w = window_slice(e, t);
    const uint32_t* bits = window_bits(e, t);
    P.clear();
    for (uint32_t li = 0; li < w.n; ++li) {
      const uint32_t i = w.idx[li];
      P.push_back({(static_cast<uint64_t>(e->last_msgs[i].start) << 32) | i, window_bit(bits, li), e->last_first + i});
    }
    DrainTopic& T = D.topics[t] = drain_topic_header(e, t, groups);
    std::sort(P.begin(), P.end(), [](const Ent& x, const Ent& y) { return x.b < y.b; });
    bool ordered = true;
    for (size_t k = 1; k < P.size(); ++k) {
      if (P[k].b == P[k - 1].b) return e->fail(PS_E_STATE, "two window messages share a row bit");
      ordered &= P[k].key > P[k - 1].key;
    }
    if ((P.back().b >> 6) >= d.W) return e->fail(PS_E_STATE, "window message bit past the row");
    T.tab0 = ids.size();
    if (ordered) {
      const uint32_t words = (P.back().b >> 6) + 1;
      T.n_pos = words * 64;
      T.aux0 = mask.size();
      ids.resize(ids.size() + T.n_pos, kNone);
      mask.resize(mask.size() + words, 0);
      for (const Ent& x : P) {
        ids[T.tab0 + x.b] = x.id;
        mask[T.aux0 + (x.b >> 6)] |= 1ull << (x.b & 63);
      }
    } else {
      std::sort(P.begin(), P.end(), [](const Ent& x, const Ent& y) { return x.key < y.key; });
      T.flags |= kDrainGather;
      T.n_pos = static_cast<uint32_t>(P.size());
      T.aux0 = order.size();
      for (const Ent& x : P) {
        ids.push_back(x.id);
        order.push_back(x.b);
      }
    }
  }
  auto up = [&](DevBuf& buf, const void* src, size_t bytes) -> hipError_t {
    hipError_t rc = buf.ensure(bytes);
    if (rc == hipSuccess && bytes) rc = hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, e->stream);
    return rc;
  };
  HIP_TRY(up(D.d_topics, D.topics.data(), D.topics.size() * sizeof(DrainTopic)), "drain topics");
  HIP_TRY(up(D.d_groups, groups.data(), groups.size() * sizeof(DrainGroup)), "drain groups");
  HIP_TRY(up(D.d_ids, ids.data(), ids.size() * 4), "drain ids");
  HIP_TRY(up(D.d_mask, mask.data(), mask.size() * 8), "drain masks");
  HIP_TRY(up(D.d_order, order.data(), order.size() * 4), "drain order");
  HIP_TRY(hipStreamSynchronize(e->stream), "sync");  // (the tables above leave scope)
  D.p_topics = D.d_topics.as<DrainTopic>();
  D.p_groups = D.d_groups.as<DrainGroup>();
  D.p_ids = D.d_ids.as<uint32_t>();
  D.p_mask = D.d_mask.as<uint64_t>();
  D.p_order = D.d_order.as<uint32_t>();
  D.seq = e->window_seq;
  return PS_OK;
}

// The last window's tables for the asynchronous drain, once per window: the
// host stages 12 B per window message (run index, row bit, start round) in
// the slot's pinned memory and k_drain_tables builds the id table and the
// mask from them behind the window, with no host wait.  A mesh topic of a
// run with several start rounds keeps the host's arrival-order table
// (kDrainGather, as drain_tables above), staged the same way.  *tail_out:
// `tail` bytes of `st` for the caller's own input, behind the block (`used`
// bytes of it) where one was built, all that is taken where the tables were
// kept.  `timed` (PSAMD_DRAIN_TIMING): the build is waited for and reported.
// A build given up half way is no table: Tables::seq names none until it is complete.
int drain_tables_async(ps_engine* e, const Staging& st, size_t tail, bool timed, size_t* used, uint8_t** tail_out) {
  auto& D = e->drain.tab;
  const char* const what = st.arena ? "alloc sink staging" : "alloc drain staging";
  *used = 0;
  if (D.seq == e->window_seq) {
    HIP_TRY(st.take(tail, tail_out), what);
    return PS_OK;
  }
  D.seq = ~0ull;
  const uint32_t nt = static_cast<uint32_t>(e->topics.size());
  D.topics.assign(nt, DrainTopic{});
  std::vector<DrainGroup> groups;
  std::vector<uint32_t> built, gather;  // topics by build
  uint64_t n_msgs = 0, n_pos = 0, n_gather = 0;
  for (uint32_t t = 0; t < nt; ++t) {
    const TopicDev& d = e->last_topics[t];
    const uint32_t cnt = e->last_cnt[t];
    if (!d.W || !cnt) continue;
    DrainTopic& T = D.topics[t] = drain_topic_header(e, t, groups);
    if ((d.flags & kTopicMesh) && !e->run_zero_start) {
      T.flags |= kDrainGather;
      gather.push_back(t);
      n_gather += cnt;
      continue;
    }
    // the positions in use end with the word of the highest bit (a bit past
    // the row is the kernel's to report: the table never exceeds the row)
    const uint32_t* bits = window_bits(e, t);
    const uint32_t top = bits ? *std::max_element(bits, bits + cnt) : cnt - 1;
    T.n_pos = (std::min<uint32_t>(top >> 6, d.W - 1) + 1) * 64;
    T.tab0 = n_pos;
    T.aux0 = n_pos >> 6;
    n_pos += T.n_pos;
    n_msgs += cnt;
    built.push_back(t);
  }
  if (n_pos + n_gather >= (1ull << 31)) return e->fail(PS_E_RANGE, "drain tables too large: use ps_drain");
  uint64_t g_ids = n_pos, g_ord = 0;
  for (uint32_t t : gather) {
    DrainTopic& T = D.topics[t];
    T.n_pos = e->last_cnt[t];
    T.tab0 = g_ids;
    T.aux0 = g_ord;
    g_ids += T.n_pos;
    g_ord += T.n_pos;
  }
  // the block: topics | groups | built topics | their first messages | idx | bit | start | order | gather ids
  const uint32_t nb = static_cast<uint32_t>(built.size());
  const size_t o_topics = 0;
  const size_t o_groups = align256(o_topics + nt * sizeof(DrainTopic));
  const size_t o_btopic = align256(o_groups + groups.size() * sizeof(DrainGroup));
  const size_t o_msg0 = align256(o_btopic + nb * 4);
  const size_t o_idx = align256(o_msg0 + (nb + 1) * 4);
  const size_t o_bit = align256(o_idx + n_msgs * 4);
  const size_t o_start = align256(o_bit + n_msgs * 4);
  const size_t o_order = align256(o_start + n_msgs * 4);
  const size_t o_gids = align256(o_order + n_gather * 4);
  const size_t block = align256(o_gids + n_gather * 4);
  uint8_t* h = nullptr;
  HIP_TRY(st.take(block + tail, &h), what);
  *tail_out = h + block;
  HIP_TRY(D.d_ablock.ensure(block), "alloc drain tables");
  HIP_TRY(D.d_aids.ensure((n_pos + n_gather) * 4), "alloc drain ids");
  HIP_TRY(D.d_amask.ensure((n_pos >> 6) * 8 + 8), "alloc drain masks");
  HIP_TRY(D.d_akeys.ensure(n_pos * 8), "alloc drain keys");
  std::memcpy(h + o_topics, D.topics.data(), nt * sizeof(DrainTopic));
  if (!groups.empty()) std::memcpy(h + o_groups, groups.data(), groups.size() * sizeof(DrainGroup));
  uint32_t* h_btopic = reinterpret_cast<uint32_t*>(h + o_btopic);
  uint32_t* h_msg0 = reinterpret_cast<uint32_t*>(h + o_msg0);
  uint32_t* h_idx = reinterpret_cast<uint32_t*>(h + o_idx);
  uint32_t* h_bit = reinterpret_cast<uint32_t*>(h + o_bit);
  uint32_t* h_start = reinterpret_cast<uint32_t*>(h + o_start);
  uint32_t j = 0;
  for (uint32_t k = 0; k < nb; ++k) {
    const uint32_t t = built[k];
    h_btopic[k] = t;
    h_msg0[k] = j;
    const WinSlice w = window_slice(e, t);
    const uint32_t* bits = window_bits(e, t);
    for (uint32_t li = 0; li < w.n; ++li, ++j) {
      const uint32_t i = w.idx[li];
      h_idx[j] = i;
      h_bit[j] = window_bit(bits, li);
      h_start[j] = e->last_msgs[i].start;
    }
  }
  h_msg0[nb] = j;
  uint32_t* h_order = reinterpret_cast<uint32_t*>(h + o_order);
  uint32_t* h_gids = reinterpret_cast<uint32_t*>(h + o_gids);
  std::vector<std::pair<uint64_t, uint32_t>> P;  // (key, bit)
  for (uint32_t t : gather) {  // arrival order: (start round, run index) ascending
    const WinSlice w = window_slice(e, t);
    const uint32_t* bits = window_bits(e, t);
    P.resize(w.n);
    for (uint32_t li = 0; li < w.n; ++li)
      P[li] = {static_cast<uint64_t>(e->last_msgs[w.idx[li]].start) << 32 | w.idx[li], window_bit(bits, li)};
    std::sort(P.begin(), P.end());
    const uint64_t o = D.topics[t].aux0;
    for (uint32_t k = 0; k < w.n; ++k) {
      if ((P[k].second >> 6) >= D.topics[t].W) return e->fail(PS_E_STATE, "window message bit past the row");
      h_order[o + k] = P[k].second;
      h_gids[o + k] = e->last_first + static_cast<uint32_t>(P[k].first);
    }
  }
  hipStream_t s = e->stream;
  uint8_t* db = D.d_ablock.as<uint8_t>();
  HIP_TRY(hipMemcpyAsync(db, h, block, hipMemcpyHostToDevice, s), "upload drain tables");
  if (n_gather)
    HIP_TRY(hipMemcpyAsync(D.d_aids.as<uint32_t>() + n_pos, db + o_gids, n_gather * 4, hipMemcpyDeviceToDevice, s),
            "place drain ids");
  D.d_err = reinterpret_cast<uint32_t*>(D.d_amask.as<uint64_t>() + (n_pos >> 6));
  HIP_TRY(hipMemsetAsync(D.d_amask.p, 0, (n_pos >> 6) * 8 + 8, s), "clear drain masks");
  if (n_pos) HIP_TRY(hipMemsetAsync(D.d_aids.p, 0xFF, n_pos * 4, s), "clear drain ids");
  DrainBuild b{};
  b.topics = reinterpret_cast<const DrainTopic*>(db + o_topics);
  b.topic = reinterpret_cast<const uint32_t*>(db + o_btopic);
  b.msg0 = reinterpret_cast<const uint32_t*>(db + o_msg0);
  b.idx = reinterpret_cast<const uint32_t*>(db + o_idx);
  b.bit = reinterpret_cast<const uint32_t*>(db + o_bit);
  b.start = reinterpret_cast<const uint32_t*>(db + o_start);
  b.n_built = nb;
  b.n_msgs = static_cast<uint32_t>(n_msgs);
  b.last_first = e->last_first;
  b.n_pos = n_pos;
  b.ids = D.d_aids.as<uint32_t>();
  b.mask = D.d_amask.as<uint64_t>();
  b.keys = D.d_akeys.as<uint64_t>();
  b.err = D.d_err;
  const PhaseTimer tm{e->drain.ev_t, s, timed};  // (timing runs wait here: the build and its check, device time)
  float build_ms = 0;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_tables(b, s), "k_drain_tables");
  HIP_TRY(tm.end(build_ms), "event");
  if (timed)
    std::fprintf(stderr, "psamd drain tables: topics %u messages %llu positions %llu gather %llu device_ms %.4f\n", nb,
                 static_cast<unsigned long long>(n_msgs), static_cast<unsigned long long>(n_pos),
                 static_cast<unsigned long long>(n_gather), build_ms);
  D.p_topics = b.topics;
  D.p_groups = reinterpret_cast<const DrainGroup*>(db + o_groups);
  D.p_ids = b.ids;
  D.p_mask = b.mask;
  D.p_order = reinterpret_cast<const uint32_t*>(db + o_order);
  D.seq = e->window_seq;
  *used = block;
  return PS_OK;
}

// The device table build's error word: it exists once a device build has
// run; the mask buffer's last word else
int drain_err_word(ps_engine* e, hipStream_t s) {
  auto& D = e->drain.tab;
  if (D.d_err) return PS_OK;
  HIP_TRY(D.d_amask.ensure(8), "alloc drain masks");
  D.d_err = D.d_amask.as<uint32_t>();
  HIP_TRY(hipMemsetAsync(D.d_err, 0, 8, s), "clear drain error");
  return PS_OK;
}

// queries -> (topic, node, first segment) in `out`; an empty answer has no
// segment.  Returns the segments; it stops at kDrainRowLimit or above (the
// caller's error).  `bound`, if asked for: the ids at most (every resolved
// query may hold all of its topic's window messages).
uint64_t drain_resolve(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, DrainQuery* out,
                       uint64_t* bound) {
  const auto& D = e->drain;
  uint64_t n_segs = 0, ids = 0;
  for (size_t q = 0; q < n && n_segs < kDrainRowLimit; ++q) {
    const uint32_t t = topic[q];
    const uint32_t* map = nullptr;
    out[q] = DrainQuery{t, 0, static_cast<uint32_t>(n_segs), 0};
    const uint32_t u = drain_node(e, t, peer[q], map);
    if (u == kNone) continue;
    out[q].node = u;
    n_segs += ceil_div(D.tab.topics[t].n_pos, kDrainSegBits);
    ids += e->last_cnt[t];
  }
  if (bound) *bound = ids;
  return n_segs;
}

// (all but the queries: the engine's current row set over the window's tables)
DrainArgs drain_args(const ps_engine* e, const Drain::Tables& T) {
  DrainArgs a{};
  a.seen = e->rows.seen.as<uint64_t>();
  a.gen = e->rows.gen.as<uint8_t>();
  a.gen_cur = e->rows.gen_cur;
  a.topics = T.p_topics;
  a.groups = T.p_groups;
  a.mask = T.p_mask;
  a.order = T.p_order;
  a.ids = T.p_ids;
  return a;
}

// The queries to the device (a.queries from here on), every segment's ids
// counted and the counts scanned into B.d_off (n_segs + 1 offsets), on stream
// s; the buffers only grow.  The count is one timed phase; the scan's is left
// open, for the caller to end behind whatever it adds to it.
int drain_count_scan(ps_engine* e, DrainArgs& a, uint32_t n_segs, Drain::Scratch& B, const DrainQuery* queries,
                     size_t n_queries, hipStream_t s, const PhaseTimer& tm, float& count_ms) {
  const size_t n_off = static_cast<size_t>(n_segs) + 1;
  HIP_TRY(B.d_queries.ensure(n_queries * sizeof(DrainQuery)), "alloc drain queries");
  HIP_TRY(B.d_cnt.ensure(n_off * 8), "alloc drain counts");
  HIP_TRY(B.d_off.ensure(n_off * 8), "alloc drain offsets");
  size_t scan_bytes = 0;
  HIP_TRY(drain_scan(nullptr, &scan_bytes, B.d_cnt.as<uint64_t>(), B.d_off.as<uint64_t>(), n_segs + 1, s),
          "size drain scan");
  HIP_TRY(B.d_scan.ensure(scan_bytes), "alloc drain scan");
  HIP_TRY(hipMemcpyAsync(B.d_queries.p, queries, n_queries * sizeof(DrainQuery), hipMemcpyHostToDevice, s),
          "upload drain queries");
  a.queries = B.d_queries.as<DrainQuery>();
  a.n_queries = static_cast<uint32_t>(n_queries);
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_count(a, n_segs, B.d_cnt.as<uint64_t>(), s), "k_drain_count");
  HIP_TRY(tm.end(count_ms), "event");
  HIP_TRY(tm.begin(), "event");
  scan_bytes = B.d_scan.bytes;
  HIP_TRY(drain_scan(B.d_scan.p, &scan_bytes, B.d_cnt.as<uint64_t>(), B.d_off.as<uint64_t>(), n_segs + 1, s), "drain scan");
  return PS_OK;
}

void drain_destroy(ps_engine* e) {
  auto& D = e->drain;
  if (D.copy_stream) {
    (void)hipStreamSynchronize(D.copy_stream);
    (void)hipStreamDestroy(D.copy_stream);
  }
  for (auto& r : D.sink.res) {
    for (auto& c : r.arena) (void)hipHostFree(c.h);
    if (r.h_res) (void)hipHostFree(r.h_res);
    if (r.ev_done) (void)hipEventDestroy(r.ev_done);
  }
  for (auto& f : D.sink.fence)
    if (f.ev) (void)hipEventDestroy(f.ev);
  for (hipEvent_t ev : {D.sync.ev_emit[0], D.sync.ev_emit[1], D.sync.ev_copy[0], D.sync.ev_copy[1], D.ev_t[0], D.ev_t[1],
                        D.slot[0].ev_emit, D.slot[0].ev_done, D.slot[1].ev_emit, D.slot[1].ev_done})
    if (ev) (void)hipEventDestroy(ev);
  for (auto& sl : D.slot)
    for (uint8_t* h : {sl.h_in, sl.h_res})
      if (h) (void)hipHostFree(h);
  if (D.aud.h_ids) (void)hipHostFree(D.aud.h_ids);
  for (auto* S : D.standing()) standing_destroy(*S);
  for (auto* A : {&D.load.ans, &D.hops.ans, &D.down.ans, &D.cut.ans, &D.report.ans, &D.spread_trk.ans})
    if (A->h_out) (void)hipHostFree(A->h_out);
  for (hipEvent_t ev : D.spread_trk.ev_t)
    if (ev) (void)hipEventDestroy(ev);
  for (uint8_t* h : {D.dist.h_out, D.dist.h_off, D.dist.h_rec})
    if (h) (void)hipHostFree(h);
  if (D.spread.h_out) (void)hipHostFree(D.spread.h_out);
  for (hipEvent_t ev : D.blame_trk.ev_t)
    if (ev) (void)hipEventDestroy(ev);
  for (uint8_t* h : {D.blame.h_off, D.blame.h_rec, D.blame.h_out, D.blame_trk.h_cur, D.blame_trk.h_off, D.blame_trk.h_rec})
    if (h) (void)hipHostFree(h);
}

}  // namespace psamd
