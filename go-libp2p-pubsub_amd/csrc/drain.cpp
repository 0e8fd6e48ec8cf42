// drain.cpp -- the host side of the batched drain (kernels: drain.hip;
// DESIGN.md §5.5): ps_drain, ps_drain_shared, ps_drain_begin / ps_drain_end,
// ps_drain_shared_begin / ps_drain_shared_end, the sink (ps_sink_set /
// ps_sink_take, §5.5e): the shared drain behind every window of a run, and
// ps_drain_topics (§5.5f): a topic's audience as one list plus exceptions.
//
// What the paths rely on, between them and with run.cpp:
//  - D.seq / D.p_*: one set of device tables per window, built by whichever
//    path runs first (drain_tables on the host, drain_tables_async on the
//    device; the sink always builds its window's) and reused by the others.
//  - D.d_err lives behind the mask words of the device build; it is created
//    (8 bytes, cleared) on first use when only host builds have run.
//    ps_drain_shared passes a zero word behind its header instead.
//  - ps_drain's slabs: ev_copy[k & 1] is waited on before slab k is emitted,
//    slab k - 1 is copied while slab k is emitted; under timing the copy runs
//    in line on `stream`.
//  - Slot::seen / emit_pending / ev_emit and Sink::fence (the last sink emit
//    over each row set) are read by drain_fence (run.cpp).
//  - ps_drain_shared_begin and the sink run one pass over their queries
//    (shared_stage, shared_caps, shared_pass), each with buffers of its own.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "engine.hpp"

using namespace psamd;

namespace {

using Drain = ps_engine::Drain;
using hclock = std::chrono::steady_clock;

double ms_since(hclock::time_point t0) { return std::chrono::duration<double, std::milli>(hclock::now() - t0).count(); }

// segments (or classify steps) one call may hold: the kernels index them in 32 bits
constexpr uint64_t kDrainRowLimit = 0x7FFFFFFFull;
// ids one asynchronous drain may hold at most (its buffers are sized by an
// upper bound, not by the total): larger drains go through ps_drain's slabs
constexpr uint64_t kDrainAsyncMaxIds = 1ull << 30;

size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

// PSAMD_DRAIN_TIMING: one phase on stream s between the two timing events,
// waited for at its end.  Off: nothing is recorded and nothing waits.
struct PhaseTimer {
  const hipEvent_t* ev;
  hipStream_t s;
  bool on;
  hipError_t begin() const { return on ? hipEventRecord(ev[0], s) : hipSuccess; }
  hipError_t end(float& ms) const {
    if (!on) return hipSuccess;
    hipError_t r = hipEventRecord(ev[1], s);
    if (r == hipSuccess) r = hipEventSynchronize(ev[1]);
    float t = 0;
    if (r == hipSuccess) r = hipEventElapsedTime(&t, ev[0], ev[1]);
    ms += t;
    return r;
  }
};

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

// Where one call stages its input: a slot's pinned h_in, all of it (one call
// takes once), or a region of a sink result's arena
struct Staging {
  Drain::Slot* slot;
  Drain::Sink::Res* arena;
  hipError_t take(size_t bytes, uint8_t** out) const {
    if (arena) return sink_stage(*arena, bytes, out);
    const hipError_t rc = pinned_ensure(&slot->h_in, nullptr, &slot->in_cap, bytes);
    *out = slot->h_in;
    return rc;
  }
};

// What every entry point needs after its own state checks: the node-space
// mirrors (the peer maps read them), the drain's stream and events
int drain_ready(ps_engine* e) {
  if (const int rc = ensure_mirrors(e)) return rc;
  auto& D = e->drain;
  if (D.copy_stream) return PS_OK;
  for (auto& ev : D.ev_emit) HIP_TRY(hipEventCreateWithFlags(&ev, kStreamEvent), "drain event");
  for (auto& ev : D.ev_copy) HIP_TRY(hipEventCreateWithFlags(&ev, kStreamEvent), "drain event");
  for (auto& ev : D.ev_t) HIP_TRY(hipEventCreate(&ev), "drain event");
  HIP_TRY(hipStreamCreateWithFlags(&D.copy_stream, hipStreamNonBlocking), "drain copy stream");
  return PS_OK;
}

int drain_check_queries(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n) {
  for (size_t q = 0; q < n; ++q)
    if (topic[q] >= e->topics.size() || peer[q] >= e->cfg.n_peers) return e->fail(PS_E_RANGE, "topic or peer out of range");
  return PS_OK;
}

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

// The last window's drain tables, once per window, built on the host.  A
// topic's window messages by row bit: where (start round, publish order)
// ascends with the bit -- every tree layout (plan_window_layout sorts the bits
// so) -- the id table is indexed by bit and a mask marks the message bits;
// else (a mesh window with several start rounds) the ids are stored in
// arrival order beside each one's bit.  A build that fails leaves D.seq at
// its older value.
int drain_tables(ps_engine* e) {
  auto& D = e->drain;
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
// A build given up half way is no table: D.seq names none until it is complete.
int drain_tables_async(ps_engine* e, const Staging& st, size_t tail, bool timed, size_t* used, uint8_t** tail_out) {
  auto& D = e->drain;
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
  const PhaseTimer tm{D.ev_t, s, timed};  // (timing runs wait here: the build and its check, device time)
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

// The node query (t, peer) reads, kNone where its answer is empty: a topic
// idle in the window, the root, a peer not subscribed or another rank's.
// `map`: topic t's peer map once looked up (a caller may keep it per topic).
uint32_t drain_node(ps_engine* e, uint32_t t, uint32_t peer, const uint32_t*& map) {
  if (!e->drain.topics[t].n_pos) return kNone;
  if (!map) map = peer_node_map(e, t, e->last_topics[t]).data();
  return map[peer];
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
    n_segs += ceil_div(D.topics[t].n_pos, kDrainSegBits);
    ids += e->last_cnt[t];
  }
  if (bound) *bound = ids;
  return n_segs;
}

DrainArgs drain_args(const ps_engine* e) {  // (all but the queries)
  const auto& D = e->drain;
  DrainArgs a{};
  a.seen = e->d_seen.as<uint64_t>();
  a.gen = e->d_gen.as<uint8_t>();
  a.gen_cur = e->gen_cur;
  a.topics = D.p_topics;
  a.groups = D.p_groups;
  a.mask = D.p_mask;
  a.order = D.p_order;
  a.ids = D.p_ids;
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

// ps_drain_shared's queries sorted for the classify pass (both forms of the
// call).  queries[q] = (topic, node) of every query; D.verdict[q] = 0 for a
// query the classify pass decides (a row of a mask-layout topic), else
// kOnHost | the verdict: nothing for a query without a row, any | missing --
// a private list -- for a row of an arrival-order (kDrainGather) topic.  The
// classified queries, sorted by topic (a counting sort: a topic's rows have
// one width), go to D.cqueries, one bin per topic.  The sort is stable: a
// topic's queries keep their order (k_drain_first relies on it).
constexpr uint32_t kOnHost = 0x80000000u;
using SharedSort = Drain::SharedSort;
int drain_shared_sort(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, DrainQuery* queries,
                      SharedSort* R) {
  auto& D = e->drain;
  const uint32_t nt = static_cast<uint32_t>(D.topics.size());
  D.verdict.assign(n, kOnHost);
  std::vector<uint32_t> per_topic(nt + 1, 0);
  std::vector<const uint32_t*> peer_map(nt, nullptr);  // (looked up once per topic, not per query)
  for (size_t q = 0; q < n; ++q) {
    const uint32_t t = topic[q];
    DrainQuery& Q = queries[q];
    Q = DrainQuery{t, 0, 0, 0};
    const uint32_t u = drain_node(e, t, peer[q], peer_map[t]);
    if (u == kNone) continue;
    Q.node = u;
    ++R->n_rows;
    R->row_ids += e->last_cnt[t];
    R->max_segs = std::max(R->max_segs, ceil_div(D.topics[t].n_pos, kDrainSegBits));
    if (D.topics[t].flags & kDrainGather) {
      D.verdict[q] = kOnHost | kDrainRowAny | kDrainRowMissing;
      ++R->n_gather;
      R->gather_ids += e->last_cnt[t];
    } else {
      D.verdict[q] = 0;
      ++per_topic[t + 1];
    }
  }
  uint64_t n_waves64 = 0;
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t n_q = per_topic[t + 1];
    per_topic[t + 1] += per_topic[t];
    if (!n_q) continue;
    DrainClassBin B{};
    B.topic = t;
    B.q0 = per_topic[t];
    B.n_q = n_q;
    B.wave0 = static_cast<uint32_t>(n_waves64);
    B.words = D.topics[t].n_pos / 64;
    uint64_t steps = 0;  // of 64 lanes; a wave runs kDrainClassPer of them
    if (B.words <= 64) {
      while ((1u << B.lanes_log2) < B.words) ++B.lanes_log2;
      steps = ((static_cast<uint64_t>(n_q) << B.lanes_log2) + 63) / 64;
    } else {
      B.waves = ceil_div(B.words, 64u);
      steps = static_cast<uint64_t>(n_q) * B.waves;
    }
    n_waves64 += (steps + kDrainClassPer - 1) / kDrainClassPer;
    if (n_waves64 * kDrainClassPer >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
    R->bins.push_back(B);
    R->bin_ids += e->last_cnt[t];
  }
  R->n_waves = static_cast<uint32_t>(n_waves64);
  R->n_class = per_topic[nt];
  D.cqueries.resize(R->n_class);
  for (size_t q = 0; q < n; ++q)
    if (D.verdict[q] == 0) D.cqueries[per_topic[queries[q].topic]++] = DrainClassQuery{queries[q].node, static_cast<uint32_t>(q)};
  return PS_OK;
}

// The slot the next asynchronous drain takes, its events made
int drain_next_slot(ps_engine* e, Drain::Slot** out) {
  auto& D = e->drain;
  auto& S = D.slot[(D.slot_head + D.slot_count) & 1];
  if (!S.ev_emit) {
    HIP_TRY(hipEventCreateWithFlags(&S.ev_emit, kStreamEvent), "drain event");
    // (the host reads the view after ev_done: it keeps the system-scope release)
    HIP_TRY(hipEventCreateWithFlags(&S.ev_done, hipEventDisableTiming), "drain event");
  }
  *out = &S;
  return PS_OK;
}

// The device table build's error word: it exists once a device build has
// run; the mask buffer's last word else
int drain_err_word(ps_engine* e, hipStream_t s) {
  auto& D = e->drain;
  if (D.d_err) return PS_OK;
  HIP_TRY(D.d_amask.ensure(8), "alloc drain masks");
  D.d_err = D.d_amask.as<uint32_t>();
  HIP_TRY(hipMemsetAsync(D.d_err, 0, 8, s), "clear drain error");
  return PS_OK;
}

// ---- the shared-list pass: ps_drain_shared_begin's, and the sink's per window ----

// Its input, one block and one upload: queries | initial verdicts | sorted queries | bins
struct SharedLayout {
  size_t n;
  uint32_t nt;
  size_t o_v, o_cq, o_bins, tail;
  SharedLayout(size_t n_queries, uint32_t n_topics)
      : n(n_queries),
        nt(n_topics),
        o_v(align256(n * sizeof(DrainQuery))),
        o_cq(o_v + align256(n * 4)),
        o_bins(o_cq + align256(n * sizeof(DrainClassQuery))),
        tail(o_bins + align256(nt * sizeof(DrainClassBin))) {}
};

// The block filled at c (L.tail bytes): drain_shared_sort's queries, the
// verdicts the passes start from (0 where the classify pass decides), the
// sorted queries and the bins.  No std::vector is a copy's source afterwards.
int shared_stage(ps_engine* e, const uint32_t* topic, const uint32_t* peer, const SharedLayout& L, uint8_t* c,
                 SharedSort* R) {
  auto& D = e->drain;
  if (const int rc = drain_shared_sort(e, topic, peer, L.n, reinterpret_cast<DrainQuery*>(c), R)) return rc;
  uint32_t* const hv = reinterpret_cast<uint32_t*>(c + L.o_v);
  for (size_t q = 0; q < L.n; ++q) hv[q] = D.verdict[q] & ~kOnHost;
  if (R->n_class) std::memcpy(c + L.o_cq, D.cqueries.data(), static_cast<size_t>(R->n_class) * sizeof(DrainClassQuery));
  if (!R->bins.empty()) std::memcpy(c + L.o_bins, R->bins.data(), R->bins.size() * sizeof(DrainClassBin));
  return PS_OK;
}

// One window's caps and segment bound.  `own`: the engine's caps (the size of
// the answer while full rows share) replace the caller's.  False: more rows
// than the kernels index (the numbering scan keeps the segments in the low
// half of its key).
bool shared_caps(const Drain& D, const SharedSort& R, size_t n, bool own, size_t* list_cap, size_t* id_cap,
                 uint32_t* seg_bound) {
  if (own) {
    *list_cap = D.share ? R.bins.size() + R.n_gather : R.n_rows;
    *id_cap = D.share ? R.bin_ids + R.gather_ids : R.row_ids;
  }
  const uint64_t bound = static_cast<uint64_t>(*list_cap) * R.max_segs;
  *seg_bound = static_cast<uint32_t>(bound);
  return bound < kDrainRowLimit && static_cast<uint64_t>(n) * R.max_segs < kDrainRowLimit;
}

// The pass on `stream`, nothing waited for (but a timed phase): the block at
// h uploaded, k_drain_classify over its verdict words, the list assignment
// into at most list_cap lists (list_of_query: n words), then count and scan
// over the lists.  Every buffer and grid is sized by n and the caps -- the
// counts stay in the control block on the device -- and B only grows.
// ms: classify, assign, count; the scan's phase is left open, as
// drain_count_scan leaves it.  *args: queries = the lists (the kernels read
// their number from *ctl); B.scratch.d_off: seg_bound + 1 offsets.
int shared_pass(ps_engine* e, Drain::ListBufs& B, const SharedLayout& L, const uint8_t* h, const SharedSort& R,
                size_t list_cap, uint32_t seg_bound, uint32_t* list_of_query, const PhaseTimer& tm, float* ms,
                DrainArgs* args, DrainCtl** ctl_out) {
  auto& D = e->drain;
  auto& C = B.scratch;
  hipStream_t s = e->stream;
  const size_t n = L.n, n_off = static_cast<size_t>(seg_bound) + 1;
  const size_t o_first = align256(sizeof(DrainCtl));
  HIP_TRY(B.d_in.ensure(L.tail), "alloc drain input");
  HIP_TRY(B.d_key.ensure(2 * n * 8), "alloc drain keys");
  HIP_TRY(B.d_aux.ensure(o_first + L.nt * 4), "alloc drain control");
  HIP_TRY(C.d_queries.ensure(list_cap * sizeof(DrainQuery)), "alloc drain lists");
  HIP_TRY(C.d_cnt.ensure(n_off * 8), "alloc drain counts");
  HIP_TRY(C.d_off.ensure(n_off * 8), "alloc drain offsets");
  uint64_t* const cnt = C.d_cnt.as<uint64_t>();
  uint64_t* const off = C.d_off.as<uint64_t>();
  uint64_t* const key = B.d_key.as<uint64_t>();
  size_t scan_bytes = 0, scan_keys = 0;  // one temporary for both scans
  HIP_TRY(drain_scan(nullptr, &scan_bytes, cnt, off, seg_bound + 1, s), "size drain scan");
  HIP_TRY(drain_scan(nullptr, &scan_keys, key, key + n, static_cast<uint32_t>(n), s), "size drain scan");
  HIP_TRY(C.d_scan.ensure(std::max(scan_bytes, scan_keys)), "alloc drain scan");

  uint8_t* const din = B.d_in.as<uint8_t>();
  uint8_t* const aux = B.d_aux.as<uint8_t>();
  DrainCtl* const ctl = reinterpret_cast<DrainCtl*>(aux);
  HIP_TRY(hipMemcpyAsync(din, h, L.tail, hipMemcpyHostToDevice, s), "upload drain queries");
  HIP_TRY(hipMemsetAsync(aux + o_first, 0xFF, L.nt * 4, s), "preset drain firsts");
  if (const int rc = drain_err_word(e, s)) return rc;

  DrainArgs a = drain_args(e);
  uint32_t* const verdict = reinterpret_cast<uint32_t*>(din + L.o_v);
  const DrainClassQuery* const sorted = reinterpret_cast<const DrainClassQuery*>(din + L.o_cq);
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_classify(a, reinterpret_cast<const DrainClassBin*>(din + L.o_bins), static_cast<uint32_t>(R.bins.size()),
                                sorted, R.n_waves, verdict, s),
          "k_drain_classify");
  HIP_TRY(tm.end(ms[0]), "event");
  DrainAssign g{};
  g.topics = D.p_topics;
  g.queries = reinterpret_cast<const DrainQuery*>(din);
  g.verdict = verdict;
  g.sorted = sorted;
  g.n_sorted = R.n_class;
  g.n = static_cast<uint32_t>(n);
  g.share = D.share;
  g.first = reinterpret_cast<uint32_t*>(aux + o_first);
  g.key = key;
  g.key_off = key + n;
  g.scan_temp = C.d_scan.p;
  g.scan_bytes = C.d_scan.bytes;
  g.lists = C.d_queries.as<DrainQuery>();
  g.list_cap = static_cast<uint32_t>(list_cap);
  g.seg_bound = seg_bound;
  g.list_of_query = list_of_query;
  g.ctl = ctl;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_assign(g, s), "drain list assignment");
  HIP_TRY(tm.end(ms[1]), "event");
  a.queries = g.lists;
  a.n_queries = 0;  // (the kernels read it from the control block)
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_count_dev(a, ctl, seg_bound, cnt, s), "k_drain_count_dev");
  HIP_TRY(tm.end(ms[2]), "event");
  HIP_TRY(tm.begin(), "event");
  scan_bytes = C.d_scan.bytes;
  HIP_TRY(drain_scan(C.d_scan.p, &scan_bytes, cnt, off, seg_bound + 1, s), "drain scan");
  *args = a;
  *ctl_out = ctl;
  return PS_OK;
}

// ---- what the two asynchronous forms share around their slots ------------------

// A begin call fails between drain_tables_async and the taking of its slot:
// a table block staged in the slot's memory (`staged`) must have left it
// before the next begin writes there
int drain_give_up(ps_engine* e, bool staged, int code, const char* what) {
  if (staged) HIP_TRY(hipStreamSynchronize(e->stream), "sync");
  return e->fail(code, what);
}

// The slot is taken with a view the host wrote.  Nothing of it is on the GPU
// but a table block it staged: the end call then waits for that upload.
int drain_slot_host_view(ps_engine* e, Drain::Slot& S, bool staged) {
  if (staged) {
    HIP_TRY(hipEventRecord(S.ev_done, e->stream), "event");
    S.enqueued = true;
  }
  ++e->drain.slot_count;
  return PS_OK;
}

// What an end call returns for the error and overflow words of its view
int drain_view_status(ps_engine* e, uint64_t err, uint32_t over) {
  if (err)
    return e->fail(PS_E_STATE, err & kDrainErrBit ? "drain tables: a window message bit past the row or shared"
                                                  : "drain tables: row bits do not ascend in arrival order");
  if (over) return e->fail(PS_E_RANGE, over & kDrainOverLists ? "more lists than list_cap" : "more ids than id_cap");
  return PS_OK;
}

// An asynchronous drain's last steps, behind its last kernel on `stream`:
// that kernel is the last reader of the window's rows (run.cpp: drain_fence);
// the slot is taken; the view leaves on the copy stream, beside whatever
// `stream` runs next (to_host), or was written in place (mapped memory).
int drain_slot_enqueued(ps_engine* e, Drain::Slot& S, size_t res_bytes, bool to_host) {
  auto& D = e->drain;
  hipStream_t s = e->stream;
  HIP_TRY(hipEventRecord(S.ev_emit, s), "event");
  S.seen = e->d_seen.p;
  S.emit_pending = true;
  S.enqueued = true;
  ++D.slot_count;
  if (!to_host) {
    HIP_TRY(hipEventRecord(S.ev_done, s), "event");
  } else {
    HIP_TRY(hipStreamWaitEvent(D.copy_stream, S.ev_emit, 0), "wait");
    HIP_TRY(hipMemcpyAsync(S.h_res, S.d_res.p, res_bytes, hipMemcpyDeviceToHost, D.copy_stream), "read drain view");
    HIP_TRY(hipEventRecord(S.ev_done, D.copy_stream), "event");
  }
  return PS_OK;
}

// The oldest slot leaves the queue; its view is complete on return
int drain_slot_complete(ps_engine* e, Drain::Slot& S) {
  auto& D = e->drain;
  D.slot_head ^= 1;
  --D.slot_count;
  if (S.enqueued) {
    HIP_TRY(hipEventSynchronize(S.ev_done), "wait for the drain");
    S.emit_pending = false;
    S.enqueued = false;
  }
  return PS_OK;
}

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
  if (static_cast<uint64_t>(e->pending.size()) * ((!D.share || paced) ? most : 1u) <= kDrainAsyncMaxIds) return PS_OK;
  uint64_t bound = 0;
  for (const RunMsg& m : e->pending) {
    const bool priv = !D.share || (paced && e->topics[m.topic].kind == Kind::Children);
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
    key.push_back(static_cast<uint64_t>(D.topics[t].flags) << 32 | D.topics[t].n_pos);
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
  c.err = D.d_err;
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
    if (f.seen == e->d_seen.p) F = &f;
  for (auto& f : K.fence)
    if (!F && (!f.seen || f.seen != e->d_seen_b.p)) F = &f;
  if (!F) return e->fail(PS_E_STATE, "sink: no fence entry for the row set");
  if (!F->ev) HIP_TRY(hipEventCreateWithFlags(&F->ev, kStreamEvent), "sink event");
  HIP_TRY(hipEventRecord(F->ev, s), "event");
  F->seen = e->d_seen.p;
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
  if (D.timing)
    std::fprintf(stderr, "psamd sink: queries %zu windows %u list_cap %zu id_cap %zu view_bytes %zu host_us %.1f\n", n,
                 R.windows, R.list_cap, R.id_cap, res_bytes, 1e3 * (K.host_ms + ms_since(t_host0)));
  return PS_OK;
}

void psamd::drain_destroy(ps_engine* e) {
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
  for (hipEvent_t ev : {D.ev_emit[0], D.ev_emit[1], D.ev_copy[0], D.ev_copy[1], D.ev_t[0], D.ev_t[1], D.slot[0].ev_emit,
                        D.slot[0].ev_done, D.slot[1].ev_emit, D.slot[1].ev_done})
    if (ev) (void)hipEventDestroy(ev);
  for (auto& sl : D.slot)
    for (uint8_t* h : {sl.h_in, sl.h_res})
      if (h) (void)hipHostFree(h);
  if (D.aud.h_ids) (void)hipHostFree(D.aud.h_ids);
}

extern "C" {

// ---- ps_drain -----------------------------------------------

int ps_drain(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, uint64_t* off_out, uint32_t* msg_out,
             size_t cap, uint64_t* total_out) {
  if (!e || !off_out || !total_out || (n && (!topic || !peer)) || (cap && !msg_out)) return PS_E_INVAL;
  if (!e->have_window) return e->fail(PS_E_NOTREADY, "no completed run");
  if (const int rj = twin_join(e)) return rj;
  if (const int rq = drain_check_queries(e, topic, peer, n)) return rq;
  off_out[0] = 0;
  *total_out = 0;
  if (n == 0) return PS_OK;
  if (n >= 0xFFFFFFFFull) return e->fail(PS_E_RANGE, "too many queries");
  auto& D = e->drain;
  // (PSAMD_DRAIN_TIMING: the host phases of the call, the first after a window above all)
  double host_ms[3] = {0, 0, 0};  // node-space mirrors, table build + upload, queries (peer maps)
  auto h0 = hclock::now();
  int rc = drain_ready(e);
  host_ms[0] = ms_since(h0);
  h0 = hclock::now();
  const bool tables_built = D.seq != e->window_seq;
  if (!rc) rc = drain_tables(e);
  host_ms[1] = ms_since(h0);
  if (rc) return rc;
  hipStream_t s = e->stream;
  h0 = hclock::now();
  D.queries.resize(n);
  const uint64_t n_segs64 = drain_resolve(e, topic, peer, n, D.queries.data(), nullptr);
  if (n_segs64 >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  const uint32_t n_segs = static_cast<uint32_t>(n_segs64);
  host_ms[2] = ms_since(h0);
  D.off.assign(static_cast<size_t>(n_segs) + 1, 0);
  float ms[4] = {0, 0, 0, 0};  // count, scan, emit, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.timing};
  DrainArgs a = drain_args(e);
  auto& B = D.scratch;
  if (n_segs) {
    if ((rc = drain_count_scan(e, a, n_segs, B, D.queries.data(), n, s, tm, ms[0]))) return rc;
    HIP_TRY(tm.end(ms[1]), "event");
    HIP_TRY(hipMemcpyAsync(D.off.data(), B.d_off.p, (static_cast<size_t>(n_segs) + 1) * 8, hipMemcpyDeviceToHost, s),
            "read drain offsets");
    HIP_TRY(hipStreamSynchronize(s), "sync");
  }
  const uint64_t total = D.off[n_segs];
  for (size_t q = 0; q < n; ++q) off_out[q] = D.off[D.queries[q].seg0];
  off_out[n] = total;
  *total_out = total;
  if (total > cap) {
    if (D.timing)
      std::fprintf(stderr, "psamd drain: queries %zu sizing host_mirrors_ms %.4f host_tables_ms %.4f (%s) host_queries_ms %.4f\n",
                   n, host_ms[0], host_ms[1], tables_built ? "built" : "kept", host_ms[2]);
    return e->fail(PS_E_RANGE, "output buffer too small");
  }

  // emit, slab by slab: the segments [lo, hi) whose ids fit one slab; slab k
  // is copied out on the copy stream while slab k + 1 is emitted
  const uint64_t slab = std::min<uint64_t>(D.slab_ids, std::max<uint64_t>(total, 1));
  // both slabs, sized once (behind the copies of an earlier drain: all complete)
  for (DevBuf& buf : D.d_slab) HIP_TRY(buf.ensure(slab * 4), "alloc drain slab");
  uint64_t pend_base = 0, pend_len = 0;  // the slab emitted last, not yet copied
  uint32_t lo = 0, k = 0;  // k: slabs emitted; slab j lives in d_slab[j & 1]
  // slab j's copy: behind its emit, on the copy stream (timing: in line)
  auto copy_out = [&](uint32_t j) -> int {
    hipStream_t cs = D.timing ? s : D.copy_stream;
    if (!D.timing) HIP_TRY(hipStreamWaitEvent(cs, D.ev_emit[j & 1], 0), "wait");
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(hipMemcpyAsync(msg_out + pend_base, D.d_slab[j & 1].p, pend_len * 4, hipMemcpyDeviceToHost, cs),
            "read drain slab");
    HIP_TRY(tm.end(ms[3]), "event");
    HIP_TRY(hipEventRecord(D.ev_copy[j & 1], cs), "event");
    return PS_OK;
  };
  while (lo < n_segs && D.off[lo] < total) {
    const uint64_t base = D.off[lo];
    const uint32_t hi =
        static_cast<uint32_t>(std::upper_bound(D.off.begin() + lo, D.off.end(), base + slab) - D.off.begin()) - 1;
    // (a segment holds at most kDrainSegBits <= slab ids, or all that is left: hi > lo)
    if (hi <= lo) return e->fail(PS_E_STATE, "drain slab smaller than a segment");
    const uint64_t len = D.off[hi] - base;
    HIP_TRY(hipStreamWaitEvent(s, D.ev_copy[k & 1], 0), "wait");  // (slab k - 2 has left the buffer)
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_drain_emit(a, lo, hi, B.d_off.as<uint64_t>(), base, D.d_slab[k & 1].as<uint32_t>(), len, D.staged, s),
            "k_drain_emit");
    HIP_TRY(tm.end(ms[2]), "event");
    HIP_TRY(hipEventRecord(D.ev_emit[k & 1], s), "event");
    if (k)  // the slab before goes out while this one is emitted
      if (const int rcc = copy_out(k - 1)) return rcc;
    pend_base = base;
    pend_len = len;
    ++k;
    lo = hi;
  }
  if (k)
    if (const int rcc = copy_out(k - 1)) return rcc;
  HIP_TRY(hipStreamSynchronize(D.copy_stream), "sync");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  if (D.timing)
    std::fprintf(stderr,
                 "psamd drain: queries %zu segments %u ids %llu slabs %u emit %s count_ms %.4f scan_ms %.4f emit_ms %.4f "
                 "copy_ms %.4f host_mirrors_ms %.4f host_tables_ms %.4f (%s) host_queries_ms %.4f\n",
                 n, n_segs, static_cast<unsigned long long>(total), k, D.staged ? "lds" : "direct", ms[0], ms[1], ms[2],
                 ms[3], host_ms[0], host_ms[1], tables_built ? "built" : "kept", host_ms[2]);
  return PS_OK;
}

// ---- ps_drain_shared ---------------------------------------

// ps_drain's answer with equal lists stored once.  k_drain_classify compares
// every queried row of a mask-layout topic with the topic's message mask:
// no message bit -> PS_NONE, every message bit -> the topic's shared list
// (emitted from the mask itself), anything else -> a list of its own through
// the count / scan / emit passes ps_drain uses.  The queries of arrival-order
// (kDrainGather) topics have no mask to compare with: each takes a private
// list.  Device -> host: 4 B x n verdicts, 8 B x (n_lists + 2) offsets, 4 B x
// total ids.
int ps_drain_shared(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, uint32_t* list_out,
                    uint64_t* list_off_out, size_t list_cap, uint32_t* msg_out, size_t cap, uint32_t* n_lists_out,
                    uint64_t* total_out) {
  if (!e || !list_off_out || !n_lists_out || !total_out || (n && (!topic || !peer || !list_out)) || (cap && !msg_out))
    return PS_E_INVAL;
  if (e->world > 1) return e->fail(PS_E_STATE, "ps_drain_shared on a multi-rank engine: use ps_drain");
  if (!e->have_window) return e->fail(PS_E_NOTREADY, "no completed run");
  if (const int rj = twin_join(e)) return rj;
  if (const int rq = drain_check_queries(e, topic, peer, n)) return rq;
  *n_lists_out = 0;
  *total_out = 0;
  if (n == 0) {
    list_off_out[0] = 0;
    return PS_OK;
  }
  if (n >= 0x7FFFFFFFull) return e->fail(PS_E_RANGE, "too many queries");
  auto& D = e->drain;
  double host_ms[2] = {0, 0};  // mirrors + tables + bins, list numbering
  auto h0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  float ms[5] = {0, 0, 0, 0, 0};  // classify, count, scan, emit, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.timing};

  const uint32_t nt = static_cast<uint32_t>(D.topics.size());
  D.queries.resize(n);
  SharedSort R;
  if ((rc = drain_shared_sort(e, topic, peer, n, D.queries.data(), &R))) return rc;
  const std::vector<DrainClassBin>& bins = R.bins;
  const uint32_t n_waves = R.n_waves, n_class = R.n_class;
  host_ms[0] = ms_since(h0);

  DrainArgs a = drain_args(e);
  if (n_class) {
    std::vector<uint32_t> got(n);
    HIP_TRY(D.d_cbins.ensure(bins.size() * sizeof(DrainClassBin)), "alloc drain bins");
    HIP_TRY(D.d_cqueries.ensure(static_cast<size_t>(n_class) * sizeof(DrainClassQuery)), "alloc drain queries");
    HIP_TRY(D.d_verdict.ensure(n * 4), "alloc drain verdicts");
    HIP_TRY(hipMemcpyAsync(D.d_cbins.p, bins.data(), bins.size() * sizeof(DrainClassBin), hipMemcpyHostToDevice, s),
            "upload drain bins");
    HIP_TRY(hipMemcpyAsync(D.d_cqueries.p, D.cqueries.data(), static_cast<size_t>(n_class) * sizeof(DrainClassQuery),
                           hipMemcpyHostToDevice, s),
            "upload drain queries");
    HIP_TRY(hipMemsetAsync(D.d_verdict.p, 0, n * 4, s), "clear drain verdicts");
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_drain_classify(a, D.d_cbins.as<DrainClassBin>(), static_cast<uint32_t>(bins.size()),
                                  D.d_cqueries.as<DrainClassQuery>(), n_waves, D.d_verdict.as<uint32_t>(), s),
            "k_drain_classify");
    HIP_TRY(tm.end(ms[0]), "event");
    HIP_TRY(hipMemcpyAsync(got.data(), D.d_verdict.p, n * 4, hipMemcpyDeviceToHost, s), "read drain verdicts");
    HIP_TRY(hipStreamSynchronize(s), "sync");  // (bins leaves scope; the verdicts number the lists)
    for (size_t q = 0; q < n; ++q)
      if (D.verdict[q] == 0) D.verdict[q] = got[q];
  }

  // lists, numbered by first use: one per topic with a full query, one per other query
  h0 = hclock::now();
  std::vector<uint32_t> topic_list(nt, PS_NONE);
  std::vector<DrainQuery> lists;
  uint64_t n_segs64 = 0;
  for (size_t q = 0; q < n; ++q) {
    const uint32_t v = D.verdict[q], t = topic[q];
    if (!(v & kDrainRowAny)) {
      list_out[q] = PS_NONE;
      continue;
    }
    const bool full = !(v & kDrainRowMissing) && D.share;
    if (full && topic_list[t] != PS_NONE) {
      list_out[q] = topic_list[t];
      continue;
    }
    list_out[q] = static_cast<uint32_t>(lists.size());
    if (full) topic_list[t] = list_out[q];
    lists.push_back(DrainQuery{t, full ? kDrainMaskRow : D.queries[q].node, static_cast<uint32_t>(n_segs64), 0});
    n_segs64 += ceil_div(D.topics[t].n_pos, kDrainSegBits);
    if (n_segs64 >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  }
  const uint32_t n_lists = static_cast<uint32_t>(lists.size());
  const uint32_t n_segs = static_cast<uint32_t>(n_segs64);
  host_ms[1] = ms_since(h0);
  *n_lists_out = n_lists;
  D.hdr.assign(static_cast<size_t>(n_lists) + 2, 0);
  auto& B = D.scratch;
  if (n_lists) {
    // (k_drain_offsets copies an error word behind the total: none here, a zero behind the header)
    HIP_TRY(D.d_hdr.ensure((D.hdr.size() + 1) * 8), "alloc drain header");
    uint32_t* const d_zero = reinterpret_cast<uint32_t*>(D.d_hdr.as<uint64_t>() + D.hdr.size());
    HIP_TRY(hipMemsetAsync(d_zero, 0, 8, s), "clear drain error");
    if ((rc = drain_count_scan(e, a, n_segs, B, lists.data(), n_lists, s, tm, ms[1]))) return rc;
    HIP_TRY(launch_drain_offsets(a.queries, n_lists, B.d_off.as<uint64_t>(), n_segs, d_zero, D.d_hdr.as<uint64_t>(), s),
            "k_drain_offsets");
    HIP_TRY(tm.end(ms[2]), "event");
    HIP_TRY(hipMemcpyAsync(D.hdr.data(), D.d_hdr.p, D.hdr.size() * 8, hipMemcpyDeviceToHost, s), "read drain offsets");
    HIP_TRY(hipStreamSynchronize(s), "sync");  // (lists leaves scope; the total sizes the output)
  }
  const uint64_t total = D.hdr[n_lists];
  *total_out = total;
  if (list_cap >= n_lists) std::memcpy(list_off_out, D.hdr.data(), (static_cast<size_t>(n_lists) + 1) * 8);
  if (list_cap < n_lists || total > cap) return e->fail(PS_E_RANGE, "output buffer too small");
  if (total) {
    HIP_TRY(D.d_lists.ensure(total * 4), "alloc drain lists");
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_drain_emit(a, 0, n_segs, B.d_off.as<uint64_t>(), 0, D.d_lists.as<uint32_t>(), total, D.staged, s),
            "k_drain_emit");
    HIP_TRY(tm.end(ms[3]), "event");
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(hipMemcpyAsync(msg_out, D.d_lists.p, total * 4, hipMemcpyDeviceToHost, s), "read drain lists");
    HIP_TRY(tm.end(ms[4]), "event");
    HIP_TRY(hipStreamSynchronize(s), "sync");
  }
  if (D.timing)
    std::fprintf(stderr,
                 "psamd drain_shared: queries %zu classified %u waves %u lists %u segments %u ids %llu classify_ms %.4f "
                 "count_ms %.4f scan_ms %.4f emit_ms %.4f copy_ms %.4f host_queries_ms %.4f host_lists_ms %.4f\n",
                 n, n_class, n_waves, n_lists, n_segs, static_cast<unsigned long long>(total), ms[0], ms[1], ms[2], ms[3],
                 ms[4], host_ms[0], host_ms[1]);
  return PS_OK;
}

// ---- ps_drain_topics ----------------------------------------

// ps_drain_shared's answer for every non-root node of the named topics, with
// no query per subscriber: the host cuts each topic's node range into strips,
// k_audience_classify streams the strips' rows into one verdict byte per node
// and two counts per strip, a scan of the counts places the nodes that are
// not full, and k_audience_emit writes those (peer, node, verdict) in node
// order.  One wait brings the counts and the first kAudPrefix records; the
// lists -- a topic's shared one where a row is full, a private one per "any"
// exception -- then go through the count / scan / emit passes unchanged.
int ps_drain_topics(ps_engine* e, const uint32_t* topic, size_t n, const uint32_t** topic_list_out,
                    const uint64_t** n_nodes_out, const uint64_t** n_full_out, const uint64_t** exc_off_out,
                    const uint32_t** exc_peer_out, const uint32_t** exc_list_out, const uint64_t** list_off_out,
                    const uint32_t** msg_out, uint32_t* n_lists_out, uint64_t* total_out) {
  if (!e || !topic_list_out || !n_nodes_out || !n_full_out || !exc_off_out || !exc_peer_out || !exc_list_out ||
      !list_off_out || !msg_out || !n_lists_out || !total_out || (n && !topic))
    return PS_E_INVAL;
  if (e->world > 1) return e->fail(PS_E_STATE, "ps_drain_topics on a multi-rank engine: use ps_drain");
  if (!e->have_window) return e->fail(PS_E_NOTREADY, "no completed run");
  if (const int rj = twin_join(e)) return rj;
  const uint32_t nt = static_cast<uint32_t>(e->topics.size());
  for (size_t i = 0; i < n; ++i)
    if (topic[i] >= nt) return e->fail(PS_E_RANGE, "topic out of range");
  {
    std::vector<uint8_t> named(nt, 0);
    for (size_t i = 0; i < n; ++i)
      if (named[topic[i]]++) return e->fail(PS_E_INVAL, "a topic named twice");
  }
  auto& D = e->drain;
  auto& A = D.aud;
  double host_ms[2] = {0, 0};  // mirrors + tables + strips, lists
  auto h0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  float ms[5] = {0, 0, 0, 0, 0};  // classify, scan, emit, lists (count, scan, emit), copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.timing};

  // the strips: each topic's non-root nodes, in request order
  A.strips.clear();
  A.n_nodes.assign(std::max<size_t>(n, 1), 0);
  A.n_full.assign(std::max<size_t>(n, 1), 0);
  A.topic_list.assign(std::max<size_t>(n, 1), PS_NONE);
  A.exc_off.assign(n + 1, 0);
  std::vector<uint64_t> strip0(n + 1, 0);  // entry i's first strip
  uint64_t n_verdicts = 0, row_bytes = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = topic[i];
    const TopicDev& d = e->last_topics[t];
    const uint32_t u0 = (d.flags & kTopicRootLocal) ? 1 : 0;
    const uint32_t nn = d.n_nodes > u0 ? d.n_nodes - u0 : 0;
    A.n_nodes[i] = nn;
    strip0[i] = A.strips.size();
    const DrainTopic& T = D.topics[t];
    if (!T.n_pos || !nn) continue;
    uint32_t lanes = 1;  // words a row takes in a load
    if (!(T.flags & kDrainGather)) {
      const uint32_t words = T.n_pos / 64;
      while (lanes < words && lanes < 64) lanes *= 2;
      lanes = std::max(lanes, words);
      row_bytes += static_cast<uint64_t>(nn) * words * 8;
    }
    const uint32_t per = std::max(1u, kAudStripBytes / (lanes * 8));
    for (uint32_t k = 0; k < nn; k += per) {
      const uint32_t c = std::min(per, nn - k);
      A.strips.push_back(AudStrip{t, u0 + k, c, d.nbase, n_verdicts});
      n_verdicts += c;
    }
    if (A.strips.size() >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  }
  strip0[n] = A.strips.size();
  const uint32_t ns = static_cast<uint32_t>(A.strips.size());
  host_ms[0] = ms_since(h0);

  // classify, scan, emit; the counts and the first records in one wait
  constexpr uint64_t kAudPrefix = 1ull << 16;
  const size_t o_node = align256(n_verdicts * 4), o_v = 2 * o_node;
  A.strip_off.assign(static_cast<size_t>(ns) + 1, 0);
  A.strip_full.assign(std::max<uint32_t>(ns, 1), 0);
  uint64_t n_exc = 0;
  if (ns) {
    HIP_TRY(A.d_strips.ensure(static_cast<size_t>(ns) * sizeof(AudStrip)), "alloc audience strips");
    HIP_TRY(A.d_verdict.ensure(n_verdicts), "alloc audience verdicts");
    HIP_TRY(A.d_exc.ensure(2 * (static_cast<size_t>(ns) + 1) * 8), "alloc audience counts");
    HIP_TRY(A.d_full.ensure(static_cast<size_t>(ns) * 4), "alloc audience counts");
    HIP_TRY(A.d_rec.ensure(o_v + n_verdicts), "alloc audience records");
    uint64_t* const cnt = A.d_exc.as<uint64_t>();
    uint64_t* const off = cnt + ns + 1;
    size_t scan_bytes = 0;
    HIP_TRY(drain_scan(nullptr, &scan_bytes, cnt, off, ns + 1, s), "size drain scan");
    HIP_TRY(D.scratch.d_scan.ensure(scan_bytes), "alloc drain scan");
    HIP_TRY(hipMemcpyAsync(A.d_strips.p, A.strips.data(), static_cast<size_t>(ns) * sizeof(AudStrip), hipMemcpyHostToDevice, s),
            "upload audience strips");
    AudArgs g{};
    g.strips = A.d_strips.as<AudStrip>();
    g.n_strips = ns;
    g.share = D.share;
    g.verdict = A.d_verdict.as<uint8_t>();
    g.n_exc = cnt;
    g.n_full = A.d_full.as<uint32_t>();
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_audience_classify(drain_args(e), g, s), "k_audience_classify");
    HIP_TRY(tm.end(ms[0]), "event");
    HIP_TRY(tm.begin(), "event");
    scan_bytes = D.scratch.d_scan.bytes;
    HIP_TRY(drain_scan(D.scratch.d_scan.p, &scan_bytes, cnt, off, ns + 1, s), "drain scan");
    HIP_TRY(tm.end(ms[1]), "event");
    uint8_t* const rec = A.d_rec.as<uint8_t>();
    AudEmit o{};
    o.node_peer = e->d_node_peer.as<uint32_t>();
    o.off = off;
    o.peer = reinterpret_cast<uint32_t*>(rec);
    o.node = reinterpret_cast<uint32_t*>(rec + o_node);
    o.verdict = rec + o_v;
    o.cap = n_verdicts;
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_audience_emit(g, o, s), "k_audience_emit");
    HIP_TRY(tm.end(ms[2]), "event");
    // (records from `lo` on, up to `hi`: the prefix now, the rest once the count is known)
    auto read_records = [&](uint64_t lo, uint64_t hi) -> hipError_t {
      if (hi <= lo) return hipSuccess;
      hipError_t r = hipMemcpyAsync(A.exc_peer.data() + lo, o.peer + lo, (hi - lo) * 4, hipMemcpyDeviceToHost, s);
      if (r == hipSuccess) r = hipMemcpyAsync(A.exc_node.data() + lo, o.node + lo, (hi - lo) * 4, hipMemcpyDeviceToHost, s);
      if (r == hipSuccess) r = hipMemcpyAsync(A.exc_verdict.data() + lo, o.verdict + lo, hi - lo, hipMemcpyDeviceToHost, s);
      return r;
    };
    const uint64_t pre = std::min<uint64_t>(n_verdicts, kAudPrefix);
    A.exc_peer.resize(pre);
    A.exc_node.resize(pre);
    A.exc_verdict.resize(pre);
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(hipMemcpyAsync(A.strip_off.data(), off, (static_cast<size_t>(ns) + 1) * 8, hipMemcpyDeviceToHost, s),
            "read audience offsets");
    HIP_TRY(hipMemcpyAsync(A.strip_full.data(), g.n_full, static_cast<size_t>(ns) * 4, hipMemcpyDeviceToHost, s),
            "read audience counts");
    HIP_TRY(read_records(0, pre), "read audience records");
    HIP_TRY(hipStreamSynchronize(s), "sync");
    n_exc = A.strip_off[ns];
    if (n_exc > n_verdicts) return e->fail(PS_E_STATE, "audience: more exceptions than nodes");
    if (n_exc > pre) {
      A.exc_peer.resize(n_exc);
      A.exc_node.resize(n_exc);
      A.exc_verdict.resize(n_exc);
      HIP_TRY(read_records(pre, n_exc), "read audience records");
      HIP_TRY(hipStreamSynchronize(s), "sync");
    }
    HIP_TRY(tm.end(ms[4]), "event");
  }
  A.exc_peer.resize(std::max<uint64_t>(n_exc, 1));
  A.exc_list.assign(std::max<uint64_t>(n_exc, 1), PS_NONE);

  // lists, in request order: a topic's shared list where a row holds it, then
  // a private one per exception that holds a message
  h0 = hclock::now();
  std::vector<DrainQuery> lists;
  uint64_t n_segs64 = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = topic[i];
    const uint32_t segs = ceil_div(D.topics[t].n_pos, kDrainSegBits);
    A.exc_off[i] = A.strip_off[strip0[i]];
    A.exc_off[i + 1] = A.strip_off[strip0[i + 1]];
    for (uint64_t k = strip0[i]; k < strip0[i + 1]; ++k) A.n_full[i] += A.strip_full[k];
    if (A.n_full[i]) {
      A.topic_list[i] = static_cast<uint32_t>(lists.size());
      lists.push_back(DrainQuery{t, kDrainMaskRow, static_cast<uint32_t>(n_segs64), 0});
      n_segs64 += segs;
    }
    for (uint64_t k = A.exc_off[i]; k < A.exc_off[i + 1]; ++k) {
      if (!(A.exc_verdict[k] & kDrainRowAny)) continue;
      if (n_segs64 + segs >= kDrainRowLimit || lists.size() + 1 >= 0x7FFFFFFFull)
        return e->fail(PS_E_RANGE, "too many rows in one drain");
      A.exc_list[k] = static_cast<uint32_t>(lists.size());
      lists.push_back(DrainQuery{t, A.exc_node[k], static_cast<uint32_t>(n_segs64), 0});
      n_segs64 += segs;
    }
    if (n_segs64 >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  }
  const uint32_t n_lists = static_cast<uint32_t>(lists.size());
  const uint32_t n_segs = static_cast<uint32_t>(n_segs64);
  host_ms[1] = ms_since(h0);
  A.list_off.assign(static_cast<size_t>(n_lists) + 2, 0);
  uint64_t total = 0;
  if (n_lists) {
    DrainArgs a = drain_args(e);
    auto& B = D.scratch;
    HIP_TRY(D.d_hdr.ensure((A.list_off.size() + 1) * 8), "alloc drain header");
    uint32_t* const d_zero = reinterpret_cast<uint32_t*>(D.d_hdr.as<uint64_t>() + A.list_off.size());
    HIP_TRY(hipMemsetAsync(d_zero, 0, 8, s), "clear drain error");
    float count_ms = 0;
    if ((rc = drain_count_scan(e, a, n_segs, B, lists.data(), n_lists, s, tm, count_ms))) return rc;
    HIP_TRY(launch_drain_offsets(a.queries, n_lists, B.d_off.as<uint64_t>(), n_segs, d_zero, D.d_hdr.as<uint64_t>(), s),
            "k_drain_offsets");
    HIP_TRY(tm.end(ms[3]), "event");
    ms[3] += count_ms;
    HIP_TRY(hipMemcpyAsync(A.list_off.data(), D.d_hdr.p, A.list_off.size() * 8, hipMemcpyDeviceToHost, s),
            "read drain offsets");
    HIP_TRY(hipStreamSynchronize(s), "sync");  // (lists leaves scope; the total sizes the ids)
    total = A.list_off[n_lists];
    if (total) {
      HIP_TRY(D.d_lists.ensure(total * 4), "alloc drain lists");
      HIP_TRY(pinned_ensure(&A.h_ids, nullptr, &A.ids_cap, total * 4), "alloc audience ids");
      HIP_TRY(tm.begin(), "event");
      HIP_TRY(launch_drain_emit(a, 0, n_segs, B.d_off.as<uint64_t>(), 0, D.d_lists.as<uint32_t>(), total, D.staged, s),
              "k_drain_emit");
      HIP_TRY(tm.end(ms[3]), "event");
      HIP_TRY(tm.begin(), "event");
      HIP_TRY(hipMemcpyAsync(A.h_ids, D.d_lists.p, total * 4, hipMemcpyDeviceToHost, s), "read drain lists");
      HIP_TRY(tm.end(ms[4]), "event");
      HIP_TRY(hipStreamSynchronize(s), "sync");
    }
  }
  if (!A.h_ids) HIP_TRY(pinned_ensure(&A.h_ids, nullptr, &A.ids_cap, 4), "alloc audience ids");
  *topic_list_out = A.topic_list.data();
  *n_nodes_out = A.n_nodes.data();
  *n_full_out = A.n_full.data();
  *exc_off_out = A.exc_off.data();
  *exc_peer_out = A.exc_peer.data();
  *exc_list_out = A.exc_list.data();
  *list_off_out = A.list_off.data();
  *msg_out = reinterpret_cast<const uint32_t*>(A.h_ids);
  *n_lists_out = n_lists;
  *total_out = total;
  if (D.timing)
    std::fprintf(stderr,
                 "psamd drain_topics: topics %zu strips %u nodes %llu row_bytes %llu exceptions %llu lists %u segments %u ids "
                 "%llu classify_ms %.4f scan_ms %.4f emit_ms %.4f lists_ms %.4f copy_ms %.4f host_strips_ms %.4f "
                 "host_lists_ms %.4f\n",
                 n, ns, static_cast<unsigned long long>(n_verdicts), static_cast<unsigned long long>(row_bytes),
                 static_cast<unsigned long long>(n_exc), n_lists, n_segs, static_cast<unsigned long long>(total), ms[0],
                 ms[1], ms[2], ms[3], ms[4], host_ms[0], host_ms[1]);
  return PS_OK;
}

// ---- ps_drain_begin / ps_drain_end -------------------------

int ps_drain_begin(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n) {
  if (!e || (n && (!topic || !peer))) return PS_E_INVAL;
  if (e->world > 1) return e->fail(PS_E_STATE, "ps_drain_begin on a multi-rank engine: use ps_drain");
  if (!e->have_window) return e->fail(PS_E_NOTREADY, "no run enqueued");
  auto& D = e->drain;
  if (D.slot_count == 2) return e->fail(PS_E_STATE, "two drains outstanding: ps_drain_end first");
  if (const int rq = drain_check_queries(e, topic, peer, n)) return rq;
  if (n >= 0x7FFFFFFFull) return e->fail(PS_E_RANGE, "too many queries");
  const auto t_host0 = hclock::now();
  // behind the last launch of the window: `stream` follows a twin's tstream
  if (const int rj = twin_join(e)) return rj;
  int rc = drain_ready(e);
  if (rc) return rc;
  Drain::Slot* slot = nullptr;
  if ((rc = drain_next_slot(e, &slot))) return rc;
  auto& S = *slot;
  hipStream_t s = e->stream;
  S.n = n;
  S.shared = false;
  size_t used = 0;
  uint8_t* h = nullptr;
  if ((rc = drain_tables_async(e, Staging{&S, nullptr}, align256(n * sizeof(DrainQuery)), D.timing, &used, &h))) return rc;

  // the queries, resolved straight into the slot's staging behind the tables
  DrainQuery* hq = reinterpret_cast<DrainQuery*>(h);
  uint64_t bound = 0;
  const uint64_t n_segs64 = drain_resolve(e, topic, peer, n, hq, &bound);
  if (n_segs64 >= kDrainRowLimit || bound > kDrainAsyncMaxIds)
    return drain_give_up(e, used, PS_E_RANGE, n_segs64 >= kDrainRowLimit ? "too many rows in one drain"
                                                                         : "drain may exceed 2^30 ids: use ps_drain");
  const uint32_t n_segs = static_cast<uint32_t>(n_segs64);
  S.hdr_bytes = align256((n + 2) * 8);
  S.bound = bound;
  const size_t res_bytes = S.hdr_bytes + bound * 4;
  HIP_TRY(pinned_ensure(&S.h_res, &S.h_res_dev, &S.res_cap, res_bytes), "alloc drain view");
  S.enqueued = false;
  if (n_segs == 0) {  // nothing to read: the view is n + 1 zeros
    std::memset(S.h_res, 0, (n + 2) * 8);
    return drain_slot_host_view(e, S, used);
  }
  if (!D.mapped_out) HIP_TRY(S.d_res.ensure(res_bytes), "alloc drain result");
  DrainArgs a = drain_args(e);
  const PhaseTimer untimed{D.ev_t, s, false};  // (nothing here may wait for the stream)
  float none = 0;
  if ((rc = drain_count_scan(e, a, n_segs, S.lb.scratch, hq, n, s, untimed, none))) return rc;
  uint8_t* res = D.mapped_out ? S.h_res_dev : S.d_res.as<uint8_t>();
  if ((rc = drain_err_word(e, s))) return rc;
  const uint64_t* seg_off = S.lb.scratch.d_off.as<uint64_t>();
  HIP_TRY(launch_drain_offsets(a.queries, a.n_queries, seg_off, n_segs, D.d_err, reinterpret_cast<uint64_t*>(res), s),
          "k_drain_offsets");
  HIP_TRY(launch_drain_emit(a, 0, n_segs, seg_off, 0, reinterpret_cast<uint32_t*>(res + S.hdr_bytes), bound, true, s),
          "k_drain_emit");
  if ((rc = drain_slot_enqueued(e, S, res_bytes, !D.mapped_out))) return rc;
  if (D.timing)
    std::fprintf(stderr, "psamd drain_begin: queries %zu segments %u bound %llu tables %s out %s host_us %.1f\n", n, n_segs,
                 static_cast<unsigned long long>(bound), used ? "built" : "kept", D.mapped_out ? "mapped" : "copy",
                 1e3 * ms_since(t_host0));
  return PS_OK;
}

int ps_drain_end(ps_engine* e, const uint64_t** off_out, const uint32_t** msg_out, uint64_t* total_out) {
  if (!e || !off_out || !msg_out || !total_out) return PS_E_INVAL;
  auto& D = e->drain;
  if (D.slot_count == 0) return e->fail(PS_E_NOTREADY, "no drain outstanding");
  auto& S = D.slot[D.slot_head];
  if (S.shared) return e->fail(PS_E_STATE, "the oldest drain is a shared one: ps_drain_shared_end");
  if (const int rc = drain_slot_complete(e, S)) return rc;
  const uint64_t* hdr = reinterpret_cast<const uint64_t*>(S.h_res);
  *off_out = hdr;
  *msg_out = reinterpret_cast<const uint32_t*>(S.h_res + S.hdr_bytes);
  *total_out = hdr[S.n];
  if (const int rc = drain_view_status(e, hdr[S.n + 1], 0)) return rc;
  if (hdr[S.n] > S.bound) return e->fail(PS_E_STATE, "drain total above its bound");
  return PS_OK;
}

// ---- ps_drain_shared_begin / ps_drain_shared_end -----------

// ps_drain_shared's answer enqueued behind the last run, with no host wait:
// tables (device build), classify, the list assignment (what the host loop of
// ps_drain_shared does between its waits: k_drain_first / _keys / scan /
// _lists), then count / scan / offsets / emit over the lists with the counts
// read from the slot's control block, all on `stream`; the view (header,
// list_off, list_of_query, ids) leaves in one copy on the copy stream.  The
// host knows only the caps: every buffer and grid is sized by them.
int ps_drain_shared_begin(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, size_t list_cap,
                          size_t id_cap) {
  if (!e || (n && (!topic || !peer))) return PS_E_INVAL;
  if (e->world > 1) return e->fail(PS_E_STATE, "ps_drain_shared_begin on a multi-rank engine: use ps_drain");
  if (!e->have_window) return e->fail(PS_E_NOTREADY, "no run enqueued");
  auto& D = e->drain;
  if (D.slot_count == 2) return e->fail(PS_E_STATE, "two drains outstanding: end one first");
  if (const int rq = drain_check_queries(e, topic, peer, n)) return rq;
  if (n >= 0x7FFFFFFFull || list_cap >= 0x7FFFFFFFull) return e->fail(PS_E_RANGE, "too many queries or lists");
  const auto t_host0 = hclock::now();
  if (const int rj = twin_join(e)) return rj;
  int rc = drain_ready(e);
  if (rc) return rc;
  Drain::Slot* slot = nullptr;
  if ((rc = drain_next_slot(e, &slot))) return rc;
  auto& S = *slot;
  hipStream_t s = e->stream;
  const uint32_t nt = static_cast<uint32_t>(e->topics.size());

  // staged in the slot's pinned input, behind the table block where one is
  // built.  From here to the slot's taking a failure gives the slot up.
  const SharedLayout L(n, nt);
  size_t used = 0;
  uint8_t* h = nullptr;
  if ((rc = drain_tables_async(e, Staging{&S, nullptr}, L.tail, D.timing, &used, &h))) return rc;
  SharedSort R;
  if (shared_stage(e, topic, peer, L, h, &R)) return drain_give_up(e, used, PS_E_RANGE, "too many rows in one drain");

  // the caps: the engine's or the caller's
  uint32_t seg_bound = 0;
  const bool rows_fit = shared_caps(D, R, n, list_cap == 0 && id_cap == 0, &list_cap, &id_cap, &seg_bound);
  if (id_cap > kDrainAsyncMaxIds) return drain_give_up(e, used, PS_E_RANGE, "drain may exceed 2^30 ids: use ps_drain_shared");
  if (!rows_fit) return drain_give_up(e, used, PS_E_RANGE, "too many rows in one drain");

  S.n = n;
  S.shared = true;
  S.list_cap = list_cap;
  S.id_cap = id_cap;
  S.o_off = align256(sizeof(DrainSharedHdr));
  S.o_lq = S.o_off + align256((list_cap + 1) * 8);
  S.o_ids = S.o_lq + align256(n * 4);
  const size_t res_bytes = S.o_ids + id_cap * 4;
  HIP_TRY(pinned_ensure(&S.h_res, &S.h_res_dev, &S.res_cap, res_bytes), "alloc drain view");
  S.enqueued = false;
  if (R.n_rows == 0) {  // no row to read: no list, written here
    std::memset(S.h_res, 0, S.o_off + 8);
    std::memset(S.h_res + S.o_lq, 0xFF, n * 4);
    return drain_slot_host_view(e, S, used);
  }

  // (PSAMD_DRAIN_TIMING: the phases run apart and are waited for; else nothing here waits)
  float ms[5] = {0, 0, 0, 0, 0};  // classify, assign, count, scan + offsets, emit
  const PhaseTimer tm{D.ev_t, s, D.timing};
  HIP_TRY(S.d_res.ensure(res_bytes), "alloc drain result");
  uint8_t* const res = S.d_res.as<uint8_t>();
  DrainArgs a{};
  DrainCtl* ctl = nullptr;
  if ((rc = shared_pass(e, S.lb, L, h, R, list_cap, seg_bound, reinterpret_cast<uint32_t*>(res + S.o_lq), tm, ms, &a, &ctl)))
    return rc;
  const uint64_t* const seg_off = S.lb.scratch.d_off.as<uint64_t>();
  HIP_TRY(launch_drain_offsets_dev(a.queries, ctl, static_cast<uint32_t>(list_cap), seg_off, id_cap, D.d_err,
                                   reinterpret_cast<DrainSharedHdr*>(res), reinterpret_cast<uint64_t*>(res + S.o_off), s),
          "k_drain_offsets_dev");
  HIP_TRY(tm.end(ms[3]), "event");
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_emit_dev(a, ctl, seg_bound, seg_off, reinterpret_cast<uint32_t*>(res + S.o_ids), id_cap, s),
          "k_drain_emit_dev");
  HIP_TRY(tm.end(ms[4]), "event");
  // classify reads every queried row, count and emit the private ones: the
  // event behind the emit covers them all, with or without a segment
  if ((rc = drain_slot_enqueued(e, S, res_bytes, true))) return rc;
  if (D.timing)
    std::fprintf(stderr,
                 "psamd drain_shared_begin: queries %zu classified %u waves %u list_cap %zu id_cap %zu seg_bound %u tables %s "
                 "classify_ms %.4f assign_ms %.4f count_ms %.4f scan_ms %.4f emit_ms %.4f view_bytes %zu host_us %.1f\n",
                 n, R.n_class, R.n_waves, list_cap, id_cap, seg_bound, used ? "built" : "kept", ms[0], ms[1], ms[2], ms[3],
                 ms[4], res_bytes, 1e3 * ms_since(t_host0));
  return PS_OK;
}

int ps_drain_shared_end(ps_engine* e, const uint32_t** list_out, const uint64_t** list_off_out, const uint32_t** msg_out,
                        uint32_t* n_lists_out, uint64_t* total_out) {
  if (!e || !list_out || !list_off_out || !msg_out || !n_lists_out || !total_out) return PS_E_INVAL;
  auto& D = e->drain;
  if (D.slot_count == 0) return e->fail(PS_E_NOTREADY, "no drain outstanding");
  auto& S = D.slot[D.slot_head];
  if (!S.shared) return e->fail(PS_E_STATE, "the oldest drain is not a shared one: ps_drain_end");
  if (const int rc = drain_slot_complete(e, S)) return rc;
  const DrainSharedHdr* hdr = reinterpret_cast<const DrainSharedHdr*>(S.h_res);
  *list_out = reinterpret_cast<const uint32_t*>(S.h_res + S.o_lq);
  *list_off_out = reinterpret_cast<const uint64_t*>(S.h_res + S.o_off);
  *msg_out = reinterpret_cast<const uint32_t*>(S.h_res + S.o_ids);
  *n_lists_out = hdr->n_lists;
  *total_out = hdr->total;
  return drain_view_status(e, hdr->err, hdr->over);
}

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
