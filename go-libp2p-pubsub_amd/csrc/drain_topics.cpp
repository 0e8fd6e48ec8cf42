// drain_topics.cpp -- ps_drain_topics (drain_impl.hpp): each
// named topic's audience as one shared list plus exceptions.  Its lists go
// through the synchronous list tail of drain_shared.cpp.
#include "drain_impl.hpp"

using namespace psamd;

extern "C" {

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
  if (const int rc = drain_enter(e, {"ps_drain_topics on a multi-rank engine: use ps_drain", "no completed run", nullptr, true}))
    return rc;
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
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

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
    const DrainTopic& T = D.tab.topics[t];
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
    HIP_TRY(D.sync.scratch.d_scan.ensure(scan_bytes), "alloc drain scan");
    HIP_TRY(hipMemcpyAsync(A.d_strips.p, A.strips.data(), static_cast<size_t>(ns) * sizeof(AudStrip), hipMemcpyHostToDevice, s),
            "upload audience strips");
    AudArgs g{};
    g.strips = A.d_strips.as<AudStrip>();
    g.n_strips = ns;
    g.share = D.env.share;
    g.verdict = A.d_verdict.as<uint8_t>();
    g.n_exc = cnt;
    g.n_full = A.d_full.as<uint32_t>();
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_audience_classify(drain_args(e, D.tab), g, s), "k_audience_classify");
    HIP_TRY(tm.end(ms[0]), "event");
    HIP_TRY(tm.begin(), "event");
    scan_bytes = D.sync.scratch.d_scan.bytes;
    HIP_TRY(drain_scan(D.sync.scratch.d_scan.p, &scan_bytes, cnt, off, ns + 1, s), "drain scan");
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
    const uint32_t segs = ceil_div(D.tab.topics[t].n_pos, kDrainSegBits);
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
  DrainArgs a = drain_args(e, D.tab);
  float count_ms = 0;
  if ((rc = drain_list_offsets(e, a, lists, n_segs, A.list_off, tm, count_ms, ms[3]))) return rc;
  ms[3] += count_ms;
  const uint64_t total = A.list_off[n_lists];
  // (the pinned ids grow before Sync::d_lists, which drain_list_ids grows: allocations only, no enqueued work moves)
  if (total) HIP_TRY(pinned_ensure(&A.h_ids, nullptr, &A.ids_cap, total * 4), "alloc audience ids");
  if ((rc = drain_list_ids(e, a, n_segs, total, A.h_ids, tm, ms[3], ms[4]))) return rc;
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
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd drain_topics: topics %zu strips %u nodes %llu row_bytes %llu exceptions %llu lists %u segments %u ids "
                 "%llu classify_ms %.4f scan_ms %.4f emit_ms %.4f lists_ms %.4f copy_ms %.4f host_strips_ms %.4f "
                 "host_lists_ms %.4f\n",
                 n, ns, static_cast<unsigned long long>(n_verdicts), static_cast<unsigned long long>(row_bytes),
                 static_cast<unsigned long long>(n_exc), n_lists, n_segs, static_cast<unsigned long long>(total), ms[0],
                 ms[1], ms[2], ms[3], ms[4], host_ms[0], host_ms[1]);
  return PS_OK;
}

}  // extern "C"
