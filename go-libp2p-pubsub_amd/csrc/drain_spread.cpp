// drain_spread.cpp -- hops and duplicate copies for meshes and trees alike
// (drain_impl.hpp): per named topic, by hop, the forwarders
// the window reached and the messages they hold, the nodes it left out, and
// per peer the copies sent to it and those beyond what it received.
// ps_topic_spread answers for the last window, blocking.  It cuts the topics
// into the audience pass's strips (aud_stage), runs the unchanged
// k_audience_classify over them and k_spread_nodes (for a mesh's unreached
// nodes k_spread_unreached too) behind it, then a frontier
// BFS over the node space's child lists, one k_spread_level launch per level:
// where the levels end is the device's to know, so the host reads the frontier
// count between batches of launches.  k_spread_sum and k_spread_dup close the
// pass.  Buffers of its own; nothing here is another family's.  The entry
// table and the kernels' arguments are built by functions the tracker
// (drain_spread_track.cpp) calls too, over its own buffers.
#include "drain_impl.hpp"

using namespace psamd;

namespace {

static_assert(sizeof(SpreadEntry) == 32, "SpreadEntry is uploaded as laid out here");
static_assert(kHopsCols == PS_MAX_ROUNDS, "a column per round of ps_stats");

constexpr uint32_t kSpreadBatch0 = 8, kSpreadBatchMax = 64;  // level launches between two reads of the frontier count

// a topic takes part: it had messages in the window and its root is a node
bool spread_active(const ps_engine* e, uint32_t t) {
  const TopicDev& d = e->last_topics[t];
  return e->drain.tab.topics[t].n_pos && e->last_cnt[t] && d.n_nodes && (d.flags & kTopicRootLocal);
}

}  // namespace

// ---- what the blocking call and the tracker share (drain_impl.hpp) -----------------

void psamd::spread_entries(ps_engine* e, const uint32_t* topic, size_t n, const AudEntry* ae, const AudShape& A,
                           SpreadEntry* se, SpreadItem* roots, SpreadPlan* P) {
  uint64_t n_nodes = 0;
  uint32_t n_roots = 0, n_mesh = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = topic[i];
    const TopicDev& d = e->last_topics[t];
    SpreadEntry E{t, ae[i].strip0, 0, d.nbase, 0, static_cast<uint32_t>(n_nodes), hops_is_mesh(e, t) ? 1u : 0u, 0};
    if (spread_active(e, t)) {
      E.c_t = e->last_cnt[t];
      E.nn = d.n_nodes;
      n_nodes += d.n_nodes;
      roots[n_roots++] = SpreadItem{static_cast<uint32_t>(i), 0};
      n_mesh += E.mesh;
    }
    se[i] = E;
  }
  se[n] = SpreadEntry{0, A.ns, 0, 0, 0, static_cast<uint32_t>(n_nodes), 0, 0};
  *P = SpreadPlan{n_nodes, n_roots, n_mesh};
}

int psamd::spread_ensure(ps_engine* e, Drain::Spread::Pass& B, const AudShape& A, const SpreadPlan& P) {
  HIP_TRY(B.d_verdict.ensure(A.n_verdicts), "alloc spread verdicts");
  HIP_TRY(B.d_exc.ensure((static_cast<size_t>(A.ns) + 1) * 8), "alloc spread counts");
  HIP_TRY(B.d_full.ensure(static_cast<size_t>(A.ns) * 4), "alloc spread counts");
  HIP_TRY(B.d_scratch.ensure(2 * P.n_nodes * 4), "alloc spread words");
  HIP_TRY(B.d_queue.ensure(kSpreadCntBytes + 2 * P.n_nodes * sizeof(SpreadItem)), "alloc spread queues");
  return PS_OK;
}

SpreadArgs psamd::spread_args(ps_engine* e, const Drain::Spread::Pass& B, size_t o_strips, size_t n, const AudShape& A,
                              const SpreadPlan& P, uint32_t n_edges, uint64_t* out, const SpreadOut& O) {
  const auto& D = e->drain;
  SpreadArgs p{};
  p.strips = reinterpret_cast<const AudStrip*>(B.d_in.as<uint8_t>() + o_strips);
  p.n_strips = A.ns;
  p.entries = B.d_in.as<SpreadEntry>();
  p.n = static_cast<uint32_t>(n);
  p.verdict = B.d_verdict.as<uint8_t>();
  p.n_exc = B.d_exc.as<uint64_t>();
  p.count_rows = D.env.load_rows;
  p.wide = D.env.spread_wide;
  p.node_peer = e->d_node_peer.as<uint32_t>();
  p.row_ptr = e->d_row_ptr.as<uint32_t>();
  p.col = e->d_col.as<uint32_t>();
  p.n_edges = n_edges;
  p.n_peers = e->cfg.n_peers;
  p.k = B.d_scratch.as<uint32_t>();
  p.hop = p.k + P.n_nodes;
  p.cnt = B.d_queue.as<uint32_t>();
  p.queue = reinterpret_cast<SpreadItem*>(B.d_queue.as<uint8_t>() + kSpreadCntBytes);
  p.q_cap = static_cast<uint32_t>(P.n_nodes);
  p.reached = out + O.reached;
  p.deliv = out + O.deliv;
  p.unreached = out + O.unreached;
  p.holders = out + O.holders;
  p.visited = out + O.visited;
  p.recv = out + O.recv;
  p.copies = out + O.copies;
  p.dup = out + O.dup;
  return p;
}

AudArgs psamd::spread_classify_args(ps_engine* e, const SpreadArgs& p, const Drain::Spread::Pass& B) {
  AudArgs g{};
  g.strips = p.strips;
  g.n_strips = p.n_strips;
  g.share = e->drain.env.share;
  g.verdict = B.d_verdict.as<uint8_t>();
  g.n_exc = B.d_exc.as<uint64_t>();
  g.n_full = B.d_full.as<uint32_t>();
  return g;
}

extern "C" {

// ---- ps_topic_spread -------------------------------------------

int ps_topic_spread(ps_engine* e, const uint32_t* topic, size_t n, uint64_t* reached_out, uint64_t* deliv_out,
                    uint64_t* unreached_out, uint64_t* stranded_out, uint64_t* copies_out, uint64_t* dup_out) {
  if (!e || (n && !topic) ||
      (!reached_out && !deliv_out && !unreached_out && !stranded_out && !copies_out && !dup_out))
    return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_topic_spread on a multi-rank engine", "no completed run", nullptr, true})) return rc;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  auto& D = e->drain;
  auto& H = D.spread;
  const auto t_host0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  // a tree's record starts afresh when it is set anew over another kind: what
  // stands for it now is not the window's (a mesh has no such record)
  for (size_t i = 0; i < n; ++i)
    if (!hops_is_mesh(e, topic[i]) && hops_active(e, topic[i]) && !hops_levels_stand(e, topic[i]))
      return e->fail(PS_E_STATE, "spread: a topic was set anew since the last window: run first");
  hipStream_t s = e->stream;
  const size_t np = e->cfg.n_peers;
  float ms[5] = {0, 0, 0, 0, 0};  // classify, nodes, levels, sum, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  // the input block: entries | strips, the entries staged behind aud_stage's
  size_t o = 0;
  uint64_t strips_max = 0;
  (void)aud_stage_bytes(e, topic, n, &o, &strips_max);
  if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  const size_t o_strips = align256((n + 1) * sizeof(SpreadEntry));
  H.stage.resize(o_strips + strips_max * sizeof(AudStrip));
  uint8_t* const hs = H.stage.data();
  std::vector<AudEntry> ae(n + 1);
  AudShape A;
  if (!aud_stage(e, topic, n, ae.data(), reinterpret_cast<AudStrip*>(hs + o_strips), strips_max, &A))
    return e->fail(PS_E_STATE, "spread: more strips than staged");
  // the entries, the roots as the first frontier behind its count
  SpreadEntry* const se = reinterpret_cast<SpreadEntry*>(hs);
  H.seed.assign(kSpreadCntBytes + n * sizeof(SpreadItem), 0);
  SpreadPlan P;
  spread_entries(e, topic, n, ae.data(), A, se, reinterpret_cast<SpreadItem*>(H.seed.data() + kSpreadCntBytes), &P);
  const uint64_t n_nodes = P.n_nodes;
  const uint32_t n_roots = P.n_roots, n_mesh = P.n_mesh;
  if (n_nodes >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many nodes in one spread");
  std::memcpy(H.seed.data(), &n_roots, 4);
  const double host_ms = ms_since(t_host0);

  const SpreadOut O(n, np);
  const size_t in_bytes = o_strips + static_cast<size_t>(A.ns) * sizeof(AudStrip);
  const size_t out_bytes = O.words * 8;
  auto& B = H.pass;
  HIP_TRY(B.d_in.ensure(in_bytes), "alloc spread strips");
  if (const int rc2 = spread_ensure(e, B, A, P)) return rc2;
  HIP_TRY(H.d_out.ensure(out_bytes), "alloc spread sums");
  // (the frontier count lands behind the output block's copy)
  HIP_TRY(pinned_ensure(&H.h_out, nullptr, &H.out_cap, out_bytes + 8), "alloc spread view");
  uint64_t* const out = H.d_out.as<uint64_t>();
  HIP_TRY(hipMemsetAsync(out, 0, out_bytes, s), "clear spread sums");
  uint32_t launches = 0;  // level launches: the levels, and what the last batch ran past them
  if (n_roots) {
    HIP_TRY(hipMemcpyAsync(B.d_in.p, hs, in_bytes, hipMemcpyHostToDevice, s), "upload spread strips");
    HIP_TRY(hipMemcpyAsync(B.d_queue.p, H.seed.data(), kSpreadCntBytes + n_roots * sizeof(SpreadItem), hipMemcpyHostToDevice, s),
            "upload spread roots");
    // the hop words: none
    HIP_TRY(hipMemsetAsync(B.d_scratch.as<uint32_t>() + n_nodes, 0xFF, n_nodes * 4, s), "clear spread hops");
    const DrainArgs a = drain_args(e, D.tab);
    const SpreadArgs p = spread_args(e, B, o_strips, n, A, P, e->row_ptr.empty() ? 0u : e->row_ptr.back(), out, O);
    const AudArgs g = spread_classify_args(e, p, B);
    if (A.ns) {
      HIP_TRY(tm.begin(), "event");
      HIP_TRY(launch_audience_classify(a, g, s), "k_audience_classify");
      HIP_TRY(tm.end(ms[0]), "event");
    }
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_spread_nodes(a, p, s), "k_spread_nodes");
    // (a mesh's node space may hold a peer twice: its unreached nodes are counted from the child entries)
    if (unreached_out && n_mesh) HIP_TRY(launch_spread_unreached(p, s), "k_spread_unreached");
    HIP_TRY(tm.end(ms[1]), "event");
    // The levels: a batch of launches, then the count of the frontier the
    // next launch would read.  A launch over an empty frontier leaves the next
    // one empty, so the levels end at the first zero read; a forwarder enters a
    // frontier once, so there are fewer frontiers than nodes.
    const uint32_t blocks = spread_level_blocks(P);
    uint32_t* const h_cnt = reinterpret_cast<uint32_t*>(H.h_out + out_bytes);
    uint32_t batch = kSpreadBatch0;
    for (bool more = true; more;) {
      HIP_TRY(tm.begin(), "event");
      for (uint32_t b = 0; b < batch; ++b, ++launches) HIP_TRY(launch_spread_level(p, launches, blocks, s), "k_spread_level");
      HIP_TRY(hipMemcpyAsync(h_cnt, p.cnt + launches % 3, 4, hipMemcpyDeviceToHost, s), "read the frontier count");
      HIP_TRY(hipStreamSynchronize(s), "sync");
      HIP_TRY(tm.end(ms[2]), "event");
      more = *h_cnt != 0;
      if (more && launches >= n_nodes) return e->fail(PS_E_STATE, "spread: more levels than nodes");
      batch = std::min(2 * batch, kSpreadBatchMax);
    }
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_spread_sum(p, s), "k_spread_sum");
    if (dup_out) HIP_TRY(launch_spread_dup(p, s), "k_spread_dup");
    HIP_TRY(tm.end(ms[3]), "event");
  }
  // two copies at most: the per-topic part, and the peer arrays asked for
  HIP_TRY(tm.begin(), "event");
  if (n) HIP_TRY(hipMemcpyAsync(H.h_out, out, O.recv * 8, hipMemcpyDeviceToHost, s), "read spread sums");
  if (copies_out || dup_out) {
    const size_t lo = copies_out ? O.copies : O.dup, hi = dup_out ? O.words : O.dup;
    HIP_TRY(hipMemcpyAsync(H.h_out + lo * 8, out + lo, (hi - lo) * 8, hipMemcpyDeviceToHost, s), "read spread sums");
  }
  HIP_TRY(hipStreamSynchronize(s), "sync");
  HIP_TRY(tm.end(ms[4]), "event");
  const uint64_t* const h = reinterpret_cast<const uint64_t*>(H.h_out);
  if (n && reached_out) std::memcpy(reached_out, h + O.reached, n * kHopsCols * 8);
  if (n && deliv_out) std::memcpy(deliv_out, h + O.deliv, n * kHopsCols * 8);
  if (n && unreached_out) std::memcpy(unreached_out, h + O.unreached, n * 8);
  if (stranded_out)
    for (size_t i = 0; i < n; ++i) stranded_out[i] = h[O.holders + i] - h[O.visited + i];
  if (copies_out) std::memcpy(copies_out, h + O.copies, np * 8);
  if (dup_out) std::memcpy(dup_out, h + O.dup, np * 8);
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd topic_spread: topics %zu strips %u nodes %llu row_bytes %llu level_launches %u classify_ms %.4f "
                 "nodes_ms %.4f levels_ms %.4f sum_ms %.4f copy_ms %.4f host_strips_ms %.4f\n",
                 n, A.ns, static_cast<unsigned long long>(n_nodes), static_cast<unsigned long long>(A.row_bytes), launches,
                 ms[0], ms[1], ms[2], ms[3], ms[4], host_ms);
  return PS_OK;
}

}  // extern "C"
