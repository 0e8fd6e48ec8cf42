// drain_downstream.cpp -- the audience behind each peer (drain_impl.hpp;
// DESIGN.md §5.5k): for each peer, over the named tree topics, how many nodes
// hang strictly below its nodes and how many of the window's deliveries went to
// them -- what would have been lost had the peer dropped.  ps_peer_downstream
// answers for the last window, blocking; ps_downstream_track registers standing
// topics whose pass run.cpp's hooks enqueue behind every window of a run, into
// totals that ps_downstream_take copies and clears.  Both cut the topics into
// the audience pass's strips (aud_stage), run the unchanged k_audience_classify
// over them, k_audience_weights behind it, then the bottom-up pass over the
// BFS levels: one k_downstream_level launch per level over a work list the
// host cuts from the level tables (TopicHost::level_off, as the hop pass reads
// them), and k_downstream_top for the narrow levels under the roots.  Stream
// order is the only order between the launches.  Buffers of their own.
#include "drain_impl.hpp"

using namespace psamd;

// ---- what the passes over subtrees share (drain_impl.hpp; drain_cut.cpp too) -----

namespace {

// The levels [0, top) of a level table are k_downstream_top's: from the root
// down to the first level wider than a block.  The deepest level holds leaves
// and takes no work, so top stops there.
uint32_t down_top(const std::vector<uint32_t>& lv) {
  const uint32_t depth = static_cast<uint32_t>(lv.size()) - 2;
  uint32_t d = 0;
  while (d < depth && lv[d + 1] - lv[d] <= kDownBlock) ++d;
  return d;
}

}  // namespace

int psamd::down_plan(ps_engine* e, const uint32_t* topic, size_t n, const char* who, DownReq* R) {
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = topic[i];
    if (hops_is_mesh(e, t)) continue;
    R->topic.push_back(t);
    if (!hops_active(e, t)) continue;
    if (!hops_levels_stand(e, t))
      return e->fail(PS_E_STATE, std::string(who) + ": a topic was set anew since the last window: run first");
    const auto& lv = e->topics[t].level_off;
    const uint32_t depth = static_cast<uint32_t>(lv.size()) - 2;
    R->n_lvl += lv.size();
    R->n_nodes += lv.back();
    for (uint32_t d = down_top(lv); d < depth; ++d) R->n_work += ceil_div(lv[d + 1] - lv[d], kDownBlock);
  }
  if (R->n_work >= kDrainRowLimit) return e->fail(PS_E_RANGE, std::string("too many rows in one ") + who + " pass");
  return PS_OK;
}

// where the parts of the pass's input block lie: entries | levels | work | strips
void psamd::down_layout(const DownReq& R, Down::Shape* K) {
  K->n = R.topic.size();
  K->o_lvl = align256((K->n + 1) * sizeof(DownEntry));
  K->o_work = K->o_lvl + align256(std::max<size_t>(R.n_lvl, 1) * 4);
  K->o_strips = K->o_work + align256(std::max<size_t>(R.n_work, 1) * sizeof(DownWork));
}

// aud_stage's entries [n + 1] as the downstream pass's, into de; the level
// tables into lv and the work list into wk where they are given (with the
// launches' bounds in the shape); the shape's counts
void psamd::down_entries(ps_engine* e, const DownReq& R, const AudEntry* ae, const AudShape& A, DownEntry* de, uint32_t* lv,
                         DownWork* wk, Down::Shape* K) {
  const size_t n = R.topic.size();
  uint32_t lvl0 = 0, n0 = 0, launches = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = R.topic[i];
    DownEntry d{t, ae[i].strip0, 0, e->last_topics[t].nbase, 0, 0, n0, 0};
    if (hops_active(e, t)) {
      const auto& src = e->topics[t].level_off;
      d.c_t = e->last_cnt[t];
      d.lvl0 = lvl0;
      d.depth = static_cast<uint32_t>(src.size()) - 2;
      d.top = down_top(src);
      if (lv) std::copy(src.begin(), src.end(), lv + lvl0);
      lvl0 += static_cast<uint32_t>(src.size());
      n0 += src.back();
      launches = std::max(launches, d.depth - d.top);
    }
    de[i] = d;
  }
  de[n] = DownEntry{0, A.ns, 0, 0, 0, 0, n0, 0};
  K->ns = A.ns;
  K->n_verdicts = A.n_verdicts;
  K->row_bytes = A.row_bytes;
  K->n_nodes = n0;
  if (!wk) return;
  // launch j = 1 ..: every entry's level j above its deepest, while that is not the top kernel's
  uint32_t w = 0;
  K->launch.assign(1, 0);
  for (uint32_t j = 1; j <= launches; ++j) {
    for (size_t i = 0; i < n; ++i) {
      const DownEntry& d = de[i];
      if (!d.c_t || d.depth - d.top < j) continue;
      const uint32_t* const l = lv + d.lvl0;
      const uint32_t lev = d.depth - j;
      for (uint32_t u = l[lev]; u < l[lev + 1]; u += kDownBlock)
        wk[w++] = DownWork{static_cast<uint32_t>(i), lev, u, std::min(u + kDownBlock, l[lev + 1])};
    }
    K->launch.push_back(w);
  }
}

// The front of a pass over the block `din` (K.ns > 0) on `stream`: its buffers,
// classify and the weights; *out: the kernels' arguments, the sums left null.
// ms: classify, weights (PSAMD_DRAIN_TIMING)
int psamd::down_front(ps_engine* e, Down::Pass& P, const uint8_t* din, const Down::Shape& K, const PhaseTimer& tm, float* ms,
                      DownArgs* out) {
  auto& D = e->drain;
  hipStream_t s = e->stream;
  HIP_TRY(P.d_verdict.ensure(K.n_verdicts), "alloc downstream verdicts");
  HIP_TRY(P.d_exc.ensure((static_cast<size_t>(K.ns) + 1) * 8), "alloc downstream counts");
  HIP_TRY(P.d_full.ensure(static_cast<size_t>(K.ns) * 4), "alloc downstream counts");
  HIP_TRY(P.d_scratch.ensure(K.n_nodes * 16), "alloc downstream weights");
  const DrainArgs a = drain_args(e, D.tab);
  AudArgs g{};
  g.strips = reinterpret_cast<const AudStrip*>(din + K.o_strips);
  g.n_strips = K.ns;
  g.share = D.env.share;
  g.verdict = P.d_verdict.as<uint8_t>();
  g.n_exc = P.d_exc.as<uint64_t>();
  g.n_full = P.d_full.as<uint32_t>();
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_audience_classify(a, g, s), "k_audience_classify");
  HIP_TRY(tm.end(ms[0]), "event");
  DownArgs d{};
  d.strips = g.strips;
  d.n_strips = K.ns;
  d.entries = reinterpret_cast<const DownEntry*>(din);
  d.n = static_cast<uint32_t>(K.n);
  d.levels = reinterpret_cast<const uint32_t*>(din + K.o_lvl);
  d.work = reinterpret_cast<const DownWork*>(din + K.o_work);
  d.verdict = g.verdict;
  d.n_exc = g.n_exc;
  d.count_rows = D.env.load_rows;
  d.node_peer = e->d_node_peer.as<uint32_t>();
  d.row_ptr = e->d_row_ptr.as<uint32_t>();
  // the scratch: w_k | k | w_n, a word per node each
  d.w_k = P.d_scratch.as<uint64_t>();
  d.k = reinterpret_cast<uint32_t*>(d.w_k + K.n_nodes);
  d.w_n = d.k + K.n_nodes;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_audience_weights(a, d, s), "k_audience_weights");
  HIP_TRY(tm.end(ms[1]), "event");
  *out = d;
  return PS_OK;
}

namespace {

// classify, the weights, the level launches and the top kernel over the block
// `din` on `stream`, into below / carried.  ms: classify, weights, levels + top
// (PSAMD_DRAIN_TIMING)
int down_pass(ps_engine* e, Down::Pass& P, const uint8_t* din, const Down::Shape& K, uint64_t* below, uint64_t* carried,
              const PhaseTimer& tm, float* ms) {
  if (K.ns == 0) return PS_OK;  // no row to read: nothing to add
  hipStream_t s = e->stream;
  DownArgs d{};
  if (const int rc = down_front(e, P, din, K, tm, ms, &d)) return rc;
  d.below = below;
  d.carried = carried;
  HIP_TRY(tm.begin(), "event");
  for (size_t j = 0; j + 1 < K.launch.size(); ++j)
    HIP_TRY(launch_downstream_level(d, K.launch[j], K.launch[j + 1], s), "k_downstream_level");
  HIP_TRY(launch_downstream_top(d, s), "k_downstream_top");
  HIP_TRY(tm.end(ms[2]), "event");
  return PS_OK;
}

}  // namespace

// ---- the standing pass's window hook (run.cpp calls it) --------------------------

// The window just remembered, added to the totals: its tables (built here
// where nobody has), the entry table -- per window: it carries the window's
// message counts --, and the level tables, work list and strips, read where the
// last window left them on the device while what they are cut from stays, then
// the pass.  All on `stream`, behind the window and in front of the next
// node-space rebuild, which `stream` runs too; nothing waits, and no host
// mirror of the node space is read.
int psamd::downstream_window(ps_engine* e) {
  auto& D = e->drain;
  auto& H = D.down;
  if (!H.st.on || !H.st.open) return PS_OK;
  Down::Shape K;
  size_t n = 0;
  int rc = down_window_stage(e, H.st, H.track, H.kept, &K, &n);
  if (rc) return rc;
  const PhaseTimer untimed{D.ev_t, e->stream, false};
  float none[3] = {0, 0, 0};
  uint64_t* const acc = H.d_acc.as<uint64_t>();
  if ((rc = down_pass(e, H.track, H.track.d_in.as<uint8_t>(), K, acc, acc + e->cfg.n_peers, untimed, none))) return rc;
  return standing_window_done(e, H.st, H.st.topic.size() - n);  // the mesh topics of this window
}

// What a standing pass over subtrees (tracker S, open; named S.name in
// messages) does in front of its kernels: the window's tables, then the input
// block in P.d_in -- whole, or the entry table alone while S.strip_key stands
// and `kept` is its shape.  *K: its shape; *n_tree: the tree topics among the
// standing ones.
int psamd::down_window_stage(ps_engine* e, Drain::Standing& S, Down::Pass& P, Down::Shape& kept, Down::Shape* Kout,
                             size_t* n_tree) {
  const std::string w(S.name);
  Drain::Sink::Res* Rp = nullptr;
  int rc = standing_window_begin(e, S, &Rp);
  if (rc) return rc;
  auto& R = *Rp;
  hipStream_t s = e->stream;
  DownReq Q;
  if ((rc = down_plan(e, S.topic.data(), S.topic.size(), S.name, &Q))) return rc;
  const size_t n = Q.topic.size();
  const uint32_t* const topic = Q.topic.data();

  std::vector<uint64_t> key{e->graph_epoch, n, Q.n_lvl, Q.n_work};
  for (size_t i = 0; i < n; ++i) {
    (void)standing_key_topic(e, topic[i], &key);
    key.push_back(topic[i]);
  }
  Down::Shape& K = *Kout;
  down_layout(Q, &K);
  std::vector<AudEntry> ae(n + 1);
  AudShape A;
  uint8_t* hs = nullptr;
  if (standing_key_stands(S, key)) {
    HIP_TRY(sink_stage(R, K.o_lvl, &hs), "alloc subtree pass staging");
    aud_stage(e, topic, n, ae.data(), nullptr, ~0ull, &A);
    down_entries(e, Q, ae.data(), A, reinterpret_cast<DownEntry*>(hs), nullptr, nullptr, &K);
    if (K.ns != kept.ns || K.n_verdicts != kept.n_verdicts || K.n_nodes != kept.n_nodes || K.o_strips != kept.o_strips)
      return e->fail(PS_E_STATE, w + ": the kept strips are not the window's");
    K.bytes = kept.bytes;
    K.launch = kept.launch;
    HIP_TRY(hipMemcpyAsync(P.d_in.p, hs, (n + 1) * sizeof(DownEntry), hipMemcpyHostToDevice, s), "upload subtree pass entries");
  } else {
    size_t o = 0;
    uint64_t strips_max = 0;
    (void)aud_stage_bytes(e, topic, n, &o, &strips_max);
    if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one " + w + " window");
    HIP_TRY(sink_stage(R, K.o_strips + strips_max * sizeof(AudStrip), &hs), "alloc subtree pass staging");
    if (!aud_stage(e, topic, n, ae.data(), reinterpret_cast<AudStrip*>(hs + K.o_strips), strips_max, &A))
      return e->fail(PS_E_STATE, w + ": more strips than staged");
    down_entries(e, Q, ae.data(), A, reinterpret_cast<DownEntry*>(hs), reinterpret_cast<uint32_t*>(hs + K.o_lvl),
                 reinterpret_cast<DownWork*>(hs + K.o_work), &K);
    K.bytes = K.o_strips + static_cast<size_t>(K.ns) * sizeof(AudStrip);
    HIP_TRY(P.d_in.ensure(K.bytes), "alloc subtree pass strips");
    HIP_TRY(hipMemcpyAsync(P.d_in.p, hs, K.bytes, hipMemcpyHostToDevice, s), "upload subtree pass strips");
    kept = K;
    S.strip_key = key;
  }
  *n_tree = n;
  return PS_OK;
}

// A blocking call's input block over the named tree topics (none a mesh), cut
// whole into `stage`; *K: its shape
int psamd::down_sync_stage(ps_engine* e, std::vector<uint8_t>& stage, const uint32_t* topic, size_t n, const char* who,
                           Down::Shape* Kout) {
  DownReq Q;
  if (const int rc = down_plan(e, topic, n, who, &Q)) return rc;
  Down::Shape& K = *Kout;
  down_layout(Q, &K);
  size_t o = 0;
  uint64_t strips_max = 0;
  (void)aud_stage_bytes(e, topic, n, &o, &strips_max);
  if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  stage.resize(K.o_strips + strips_max * sizeof(AudStrip));
  uint8_t* const hs = stage.data();
  std::vector<AudEntry> ae(n + 1);
  AudShape A;
  if (!aud_stage(e, topic, n, ae.data(), reinterpret_cast<AudStrip*>(hs + K.o_strips), strips_max, &A))
    return e->fail(PS_E_STATE, std::string(who) + ": more strips than staged");
  down_entries(e, Q, ae.data(), A, reinterpret_cast<DownEntry*>(hs), reinterpret_cast<uint32_t*>(hs + K.o_lvl),
               reinterpret_cast<DownWork*>(hs + K.o_work), &K);
  K.bytes = K.o_strips + static_cast<size_t>(K.ns) * sizeof(AudStrip);
  return PS_OK;
}

extern "C" {

// ---- ps_peer_downstream -----------------------------------------

int ps_peer_downstream(ps_engine* e, const uint32_t* topic, size_t n, uint64_t* below_out, uint64_t* carried_out) {
  if (!e || (n && !topic) || (!below_out && !carried_out)) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_peer_downstream on a multi-rank engine", "no completed run", nullptr, true})) return rc;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (hops_is_mesh(e, topic[i])) return e->fail(PS_E_STATE, "ps_peer_downstream: a mesh topic has no subtrees");
  auto& D = e->drain;
  auto& H = D.down;
  auto& Ans = H.ans;
  const auto t_host0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  const size_t np = e->cfg.n_peers;
  float ms[4] = {0, 0, 0, 0};  // classify, weights, levels + top, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  Down::Shape K;
  if ((rc = down_sync_stage(e, Ans.stage, topic, n, "downstream", &K))) return rc;
  uint8_t* const hs = Ans.stage.data();
  const double host_ms = ms_since(t_host0);

  HIP_TRY(H.sync.d_in.ensure(K.bytes), "alloc downstream strips");
  HIP_TRY(Ans.d_out.ensure(2 * np * 8), "alloc downstream sums");
  HIP_TRY(pinned_ensure(&Ans.h_out, nullptr, &Ans.out_cap, 2 * np * 8), "alloc downstream view");
  uint64_t* const out = Ans.d_out.as<uint64_t>();
  HIP_TRY(hipMemsetAsync(out, 0, 2 * np * 8, s), "clear downstream sums");
  if (K.ns) HIP_TRY(hipMemcpyAsync(H.sync.d_in.p, hs, K.bytes, hipMemcpyHostToDevice, s), "upload downstream strips");
  if ((rc = down_pass(e, H.sync, H.sync.d_in.as<uint8_t>(), K, out, out + np, tm, ms))) return rc;
  // one copy: both arrays, or the one that was asked for
  const size_t lo = below_out ? 0 : np, hi = carried_out ? 2 * np : np;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(hipMemcpyAsync(Ans.h_out + lo * 8, out + lo, (hi - lo) * 8, hipMemcpyDeviceToHost, s), "read downstream sums");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  HIP_TRY(tm.end(ms[3]), "event");
  if (below_out) std::memcpy(below_out, Ans.h_out, np * 8);
  if (carried_out) std::memcpy(carried_out, Ans.h_out + np * 8, np * 8);
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd peer_downstream: topics %zu strips %u nodes %llu row_bytes %llu work %u launches %zu classify_ms %.4f "
                 "weights_ms %.4f levels_ms %.4f copy_ms %.4f host_strips_ms %.4f\n",
                 n, K.ns, static_cast<unsigned long long>(K.n_nodes), static_cast<unsigned long long>(K.row_bytes),
                 K.launch.empty() ? 0u : K.launch.back(), K.launch.empty() ? size_t(2) : K.launch.size() + 1, ms[0], ms[1], ms[2],
                 ms[3], host_ms);
  return PS_OK;
}

// ---- ps_downstream_track / ps_downstream_take -------------------

int ps_downstream_track(ps_engine* e, const uint32_t* topic, size_t n) {
  if (!e || (n && !topic)) return PS_E_INVAL;
  auto& H = e->drain.down;
  if (const int rc = standing_track_check(e, H.st, topic, n)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (hops_child_lists_mesh(e->topics[topic[i]]))
      return e->fail(PS_E_STATE, "ps_downstream_track: a mesh topic has no subtrees");
  if (const int rc = standing_quiesce(e, H.st)) return rc;
  standing_retrack(H.st, topic, n);
  auto& P = H.track;
  return standing_totals(e, H.st, H.d_acc, 2 * static_cast<size_t>(e->cfg.n_peers) * 8,
                         {&P.d_in, &P.d_verdict, &P.d_exc, &P.d_full, &P.d_scratch});
}

int ps_downstream_take(ps_engine* e, uint64_t* below_out, uint64_t* carried_out, uint64_t* n_windows_out,
                       uint64_t* n_skipped_out) {
  if (!e || !n_windows_out || !n_skipped_out) return PS_E_INVAL;
  auto& H = e->drain.down;
  auto& S = H.st;
  const size_t np = e->cfg.n_peers;
  if (const int rc = standing_take_totals(e, S, H.d_acc, H.ans, 2 * np * 8)) return rc;
  if (below_out) std::memcpy(below_out, H.ans.h_out, np * 8);
  if (carried_out) std::memcpy(carried_out, H.ans.h_out + np * 8, np * 8);
  *n_windows_out = S.windows;
  *n_skipped_out = S.skipped;
  S.windows = S.skipped = 0;
  return PS_OK;
}

}  // extern "C"
