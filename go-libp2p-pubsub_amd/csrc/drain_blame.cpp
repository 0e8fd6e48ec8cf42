// drain_blame.cpp -- each missed subscriber and its cut point (drain_impl.hpp;
// DESIGN.md §5.5q): for every non-root node of the named tree topics that lacks
// window messages, its peer, the peer of the nearest cut point on its path to
// the root -- the node that lacks messages under a full parent --, both BFS
// levels and the messages it lacks.  ps_topic_blame lists them per topic as
// records in node order, lent from pinned memory; ps_blame answers explicit
// (topic, peer) queries.  Both block and read the last window.  The plan, the
// input block and the front of the pass (k_audience_classify,
// k_audience_weights) are the downstream pass's (drain_downstream.cpp:
// down_sync_stage, down_front); behind them k_blame_top and one k_blame_level
// launch per level, the bottom-up passes' work list walked backwards, then
// k_blame_count, the scan and k_blame_emit, or k_blame_gather.  Stream order is
// the only order between the launches.  Buffers of their own.
#include "drain_impl.hpp"

using namespace psamd;

namespace {

using Blame = Drain::Blame;

static_assert(kBlameNone == PS_NONE, "the kernels' none is the ABI's");

// The front and the top-down sweep over the block `din` (K.ns > 0) on
// `stream`; *g: the kernels' arguments, the record side left null.
// ms: classify, weights, sweep (PSAMD_DRAIN_TIMING)
int blame_sweep(ps_engine* e, Blame& H, const uint8_t* din, const Down::Shape& K, const PhaseTimer& tm, float* ms,
                BlameArgs* g) {
  hipStream_t s = e->stream;
  if (const int rc = down_front(e, H.front, din, K, tm, ms, &g->d)) return rc;
  HIP_TRY(H.d_cut.ensure(K.n_nodes * 8), "alloc blame words");
  g->cut_node = H.d_cut.as<uint32_t>();
  g->cut_level = g->cut_node + K.n_nodes;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_blame_top(*g, s), "k_blame_top");
  // (the bottom-up order backwards: every entry's level `top` first)
  for (size_t j = K.launch.size(); j-- > 1;) HIP_TRY(launch_blame_level(*g, K.launch[j - 1], K.launch[j], s), "k_blame_level");
  HIP_TRY(tm.end(ms[2]), "event");
  return PS_OK;
}

// the state checks both calls share behind their pointer checks; the topics'
// ranges are the caller's
int blame_no_mesh(ps_engine* e, const uint32_t* topic, size_t n, const char* who) {
  for (size_t i = 0; i < n; ++i)
    if (hops_is_mesh(e, topic[i])) return e->fail(PS_E_STATE, std::string(who) + ": a mesh topic has no cut points");
  return PS_OK;
}

// topic t's level table describes the node space the last window ran on
bool blame_levels_sane(const ps_engine* e, uint32_t t) {
  const auto& lv = e->topics[t].level_off;
  bool ok = lv.size() >= 2 && lv[0] == 0 && lv.back() == e->last_topics[t].n_nodes;
  for (size_t d = 0; ok && d + 1 < lv.size(); ++d) ok = lv[d] <= lv[d + 1];
  return ok;
}

}  // namespace

extern "C" {

// ---- ps_topic_blame ----------------------------------------------

int ps_topic_blame(ps_engine* e, const uint32_t* topic, size_t n, const uint64_t** rec_off_out, const uint32_t** rec_peer_out,
                   const uint32_t** rec_cut_peer_out, const uint32_t** rec_hop_out, const uint32_t** rec_cut_hop_out,
                   const uint32_t** rec_missed_out, uint64_t* total_out) {
  const uint32_t** const outs[5] = {rec_peer_out, rec_cut_peer_out, rec_hop_out, rec_cut_hop_out, rec_missed_out};
  if (!e || (n && !topic) || !rec_off_out || !total_out) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_topic_blame on a multi-rank engine", "no completed run", nullptr, true})) return rc;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  if (const int rc = blame_no_mesh(e, topic, n, "ps_topic_blame")) return rc;
  auto& D = e->drain;
  auto& H = D.blame;
  const auto t_host0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  float ms[6] = {0, 0, 0, 0, 0, 0};  // classify, weights, sweep, count + scan, emit, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  Down::Shape K;
  if ((rc = down_sync_stage(e, H.stage, topic, n, "blame", &K))) return rc;
  const double host_ms = ms_since(t_host0);

  size_t asked = 0;
  for (auto* o : outs) asked += o != nullptr;
  HIP_TRY(pinned_ensure(&H.h_off, nullptr, &H.off_cap, (n + 1) * 8), "alloc blame offsets");
  uint64_t* const h_off = reinterpret_cast<uint64_t*>(H.h_off);
  uint64_t total = 0;
  size_t h_stride = 0;
  if (K.ns == 0) {
    // no row to read: no record
    std::memset(h_off, 0, (n + 1) * 8);
    HIP_TRY(pinned_ensure(&H.h_rec, nullptr, &H.rec_cap, 1), "alloc blame view");
  } else {
    // the record arrays on the device hold every non-root node of the named
    // topics, so nothing waits between the scan and the emit; the pinned view
    // is sized by the total, behind the one wait for it
    const uint64_t cap = K.n_verdicts;
    const size_t d_stride = align256(cap * 4);
    const size_t n_off = static_cast<size_t>(K.ns) + 1;
    HIP_TRY(H.front.d_in.ensure(K.bytes), "alloc blame strips");
    HIP_TRY(H.d_cnt.ensure(n_off * 8), "alloc blame counts");
    HIP_TRY(H.d_off.ensure(n_off * 8), "alloc blame offsets");
    HIP_TRY(H.d_rec_off.ensure((n + 1) * 8), "alloc blame offsets");
    HIP_TRY(H.d_rec.ensure(std::max<size_t>(asked, 1) * d_stride), "alloc blame records");
    size_t scan_bytes = 0;
    HIP_TRY(drain_scan(nullptr, &scan_bytes, H.d_cnt.as<uint64_t>(), H.d_off.as<uint64_t>(), K.ns + 1, s), "size blame scan");
    HIP_TRY(H.d_scan.ensure(scan_bytes), "alloc blame scan");
    HIP_TRY(hipMemcpyAsync(H.front.d_in.p, H.stage.data(), K.bytes, hipMemcpyHostToDevice, s), "upload blame strips");
    BlameArgs g{};
    if ((rc = blame_sweep(e, H, H.front.d_in.as<uint8_t>(), K, tm, ms, &g))) return rc;
    g.n_rec = H.d_cnt.as<uint64_t>();
    g.off = H.d_off.as<uint64_t>();
    g.rec_off = H.d_rec_off.as<uint64_t>();
    g.cap = cap;
    uint32_t** const recs[5] = {&g.rec_peer, &g.rec_cut_peer, &g.rec_hop, &g.rec_cut_hop, &g.rec_missed};
    for (size_t i = 0, j = 0; i < 5; ++i)
      if (outs[i]) *recs[i] = reinterpret_cast<uint32_t*>(H.d_rec.as<uint8_t>() + j++ * d_stride);
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_blame_count(g, s), "k_blame_count");
    scan_bytes = H.d_scan.bytes;
    HIP_TRY(drain_scan(H.d_scan.p, &scan_bytes, g.n_rec, H.d_off.as<uint64_t>(), K.ns + 1, s), "blame scan");
    HIP_TRY(tm.end(ms[3]), "event");
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_blame_emit(g, s), "k_blame_emit");
    HIP_TRY(tm.end(ms[4]), "event");
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(hipMemcpyAsync(h_off, g.rec_off, (n + 1) * 8, hipMemcpyDeviceToHost, s), "read blame offsets");
    HIP_TRY(hipStreamSynchronize(s), "sync");
    total = h_off[n];
    if (total > cap) return e->fail(PS_E_STATE, "ps_topic_blame: more records than nodes");
    h_stride = align256(total * 4);
    HIP_TRY(pinned_ensure(&H.h_rec, nullptr, &H.rec_cap, std::max<size_t>(asked * h_stride, 1)), "alloc blame view");
    // one copy per array asked for
    for (size_t i = 0, j = 0; i < 5 && total; ++i)
      if (outs[i]) {
        HIP_TRY(hipMemcpyAsync(H.h_rec + j * h_stride, *recs[i], total * 4, hipMemcpyDeviceToHost, s), "read blame records");
        ++j;
      }
    HIP_TRY(hipStreamSynchronize(s), "sync");
    HIP_TRY(tm.end(ms[5]), "event");
  }
  *rec_off_out = h_off;
  for (size_t i = 0, j = 0; i < 5; ++i)
    if (outs[i]) *outs[i] = reinterpret_cast<const uint32_t*>(H.h_rec + j++ * h_stride);
  *total_out = total;
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd topic_blame: topics %zu strips %u nodes %llu row_bytes %llu work %u launches %zu records %llu "
                 "copied_bytes %llu classify_ms %.4f weights_ms %.4f sweep_ms %.4f count_scan_ms %.4f emit_ms %.4f copy_ms %.4f "
                 "host_strips_ms %.4f\n",
                 n, K.ns, static_cast<unsigned long long>(K.n_nodes), static_cast<unsigned long long>(K.row_bytes),
                 K.launch.empty() ? 0u : K.launch.back(), K.launch.empty() ? size_t(0) : K.launch.size() + 5,
                 static_cast<unsigned long long>(total), static_cast<unsigned long long>((n + 1) * 8 + asked * total * 4), ms[0],
                 ms[1], ms[2], ms[3], ms[4], ms[5], host_ms);
  return PS_OK;
}

// ---- ps_blame ----------------------------------------------------

int ps_blame(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, uint32_t* cut_peer_out, uint32_t* hop_out,
             uint32_t* cut_hop_out, uint32_t* missed_out) {
  uint32_t* const outs[4] = {cut_peer_out, hop_out, cut_hop_out, missed_out};
  if (!e || (n && (!topic || !peer)) || (!cut_peer_out && !hop_out && !cut_hop_out && !missed_out)) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_blame on a multi-rank engine", "no completed run", nullptr, true}, topic, peer, n))
    return rc;
  if (n >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many queries in one ps_blame");
  // the distinct topics among the queries, in the order they first appear:
  // the sweep runs once over each
  const uint32_t nt = static_cast<uint32_t>(e->topics.size());
  std::vector<uint32_t> slot(nt, kNone), dt;
  for (size_t q = 0; q < n; ++q)
    if (slot[topic[q]] == kNone) {
      slot[topic[q]] = static_cast<uint32_t>(dt.size());
      dt.push_back(topic[q]);
    }
  if (const int rc = blame_no_mesh(e, dt.data(), dt.size(), "ps_blame")) return rc;
  if (n == 0) return PS_OK;
  auto& D = e->drain;
  auto& H = D.blame;
  const auto t_host0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  float ms[5] = {0, 0, 0, 0, 0};  // classify, weights, sweep, gather, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  Down::Shape K;
  if ((rc = down_sync_stage(e, H.stage, dt.data(), dt.size(), "blame", &K))) return rc;
  const DownEntry* const de = reinterpret_cast<const DownEntry*>(H.stage.data());

  // the gather's block: queries | the table by topic id | the level tables
  size_t n_lvl = 0;
  for (const uint32_t t : dt) {
    if (!e->last_topics[t].n_nodes) continue;  // no query of it resolves
    if (!blame_levels_sane(e, t)) return e->fail(PS_E_STATE, "blame: a topic was set anew since the last window: run first");
    n_lvl += e->topics[t].level_off.size();
  }
  const size_t o_tab = align256(n * sizeof(DrainQuery)), o_lvl = o_tab + align256(nt * sizeof(BlameTopic));
  const size_t q_bytes = o_lvl + align256(std::max<size_t>(n_lvl, 1) * 4);
  H.qstage.assign(q_bytes, 0);
  DrainQuery* const hq = reinterpret_cast<DrainQuery*>(H.qstage.data());
  BlameTopic* const ht = reinterpret_cast<BlameTopic*>(H.qstage.data() + o_tab);
  uint32_t* const hl = reinterpret_cast<uint32_t*>(H.qstage.data() + o_lvl);
  uint32_t lvl0 = 0;
  for (size_t i = 0; i < dt.size(); ++i) {
    const uint32_t t = dt[i];
    if (!e->last_topics[t].n_nodes) continue;
    const auto& lv = e->topics[t].level_off;
    ht[t] = BlameTopic{de[i].c_t ? static_cast<uint32_t>(i) : kBlameNone, lvl0, static_cast<uint32_t>(lv.size()) - 2, 0};
    std::copy(lv.begin(), lv.end(), hl + lvl0);
    lvl0 += static_cast<uint32_t>(lv.size());
  }
  // a query's node: the root 0, a subscriber its node, anything else none --
  // also in a topic idle in the window, whose level is still asked for
  std::vector<const uint32_t*> maps(dt.size(), nullptr);
  for (size_t q = 0; q < n; ++q) {
    const uint32_t t = topic[q];
    const TopicDev& d = e->last_topics[t];
    uint32_t u = kBlameNone;
    if (d.n_nodes) {
      if ((d.flags & kTopicRootLocal) && e->node_peer[d.nbase] == peer[q]) {
        u = 0;
      } else {
        const uint32_t*& map = maps[slot[t]];
        if (!map) map = peer_node_map(e, t, d).data();
        u = map[peer[q]];
      }
    }
    hq[q] = DrainQuery{t, u, 0, 0};
  }
  const double host_ms = ms_since(t_host0);

  HIP_TRY(H.d_q.ensure(q_bytes), "alloc blame queries");
  HIP_TRY(H.d_out.ensure(4 * n * 4), "alloc blame answers");
  HIP_TRY(pinned_ensure(&H.h_out, nullptr, &H.out_cap, 4 * n * 4), "alloc blame view");
  HIP_TRY(hipMemcpyAsync(H.d_q.p, H.qstage.data(), q_bytes, hipMemcpyHostToDevice, s), "upload blame queries");
  BlameArgs g{};
  if (K.ns) {
    HIP_TRY(H.front.d_in.ensure(K.bytes), "alloc blame strips");
    HIP_TRY(hipMemcpyAsync(H.front.d_in.p, H.stage.data(), K.bytes, hipMemcpyHostToDevice, s), "upload blame strips");
    if ((rc = blame_sweep(e, H, H.front.d_in.as<uint8_t>(), K, tm, ms, &g))) return rc;
  }
  BlameGather G{};
  G.queries = H.d_q.as<DrainQuery>();
  G.n = static_cast<uint32_t>(n);
  G.topics = reinterpret_cast<const BlameTopic*>(H.d_q.as<uint8_t>() + o_tab);
  G.levels = reinterpret_cast<const uint32_t*>(H.d_q.as<uint8_t>() + o_lvl);
  uint32_t* const out = H.d_out.as<uint32_t>();
  G.cut_peer = out;
  G.hop = out + n;
  G.cut_hop = out + 2 * n;
  G.missed = out + 3 * n;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_blame_gather(g, G, s), "k_blame_gather");
  HIP_TRY(tm.end(ms[3]), "event");
  // one copy: from the first array asked for to the last
  size_t lo = 0, hi = 4;
  while (!outs[lo]) ++lo;
  while (!outs[hi - 1]) --hi;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(hipMemcpyAsync(H.h_out + lo * n * 4, out + lo * n, (hi - lo) * n * 4, hipMemcpyDeviceToHost, s), "read blame answers");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  HIP_TRY(tm.end(ms[4]), "event");
  for (size_t i = lo; i < hi; ++i)
    if (outs[i]) std::memcpy(outs[i], H.h_out + i * n * 4, n * 4);
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd blame: queries %zu topics %zu strips %u nodes %llu work %u classify_ms %.4f weights_ms %.4f sweep_ms %.4f "
                 "gather_ms %.4f copy_ms %.4f host_ms %.4f\n",
                 n, dt.size(), K.ns, static_cast<unsigned long long>(K.n_nodes), K.launch.empty() ? 0u : K.launch.back(), ms[0],
                 ms[1], ms[2], ms[3], ms[4], host_ms);
  return PS_OK;
}

}  // extern "C"
