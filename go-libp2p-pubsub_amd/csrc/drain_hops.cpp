// drain_hops.cpp -- deliveries by hop per topic (drain_impl.hpp; DESIGN.md
// §5.5j): for each named tree topic, by BFS level, how many nodes the level
// has, how many of them the window reached and how many messages they hold.
// ps_topic_hops answers for the last window, blocking; ps_hops_track registers
// standing topics whose pass run.cpp's hooks enqueue behind every window of a
// run, into totals that ps_hops_take copies and clears.  Both cut the topics
// into the audience pass's strips (aud_stage), run the unchanged
// k_audience_classify over them and k_audience_hops / k_audience_hops_sum
// behind it, with buffers of their own.  A node's level comes from the host's
// level tables (TopicHost::level_off), which every node-space build leaves --
// the GPU rebuild from the readback it makes anyway -- so nothing is read back
// for this pass.
#include "drain_impl.hpp"

using namespace psamd;

using Hops = Drain::Hops;

static_assert(kHopsCols == PS_MAX_ROUNDS, "a column per round of ps_stats");

// ---- the plan and the entry table of a pass over tree levels (drain_impl.hpp; drain_report.cpp too) --

int psamd::hops_plan(ps_engine* e, const uint32_t* topic, size_t n, HopsReq* R) {
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = topic[i];
    if (hops_is_mesh(e, t)) continue;
    R->topic.push_back(t);
    R->row.push_back(static_cast<uint32_t>(i));
    if (!hops_active(e, t)) continue;
    if (!hops_levels_stand(e, t)) return e->fail(PS_E_STATE, "hops: a topic was set anew since the last window: run first");
    R->n_lvl += e->topics[t].level_off.size();
  }
  return PS_OK;
}

namespace {

// where the parts of the pass's input block lie: entries | levels | strips
void hops_layout(const HopsReq& R, Hops::Shape* K) {
  K->n = R.topic.size();
  K->o_lvl = align256((K->n + 1) * sizeof(HopsEntry));
  K->o_strips = K->o_lvl + align256(std::max<size_t>(R.n_lvl, 1) * 4);
}

}  // namespace

// aud_stage's entries [n + 1] as the hop pass's, into he; the level tables
// into lv where it is given; the shape's counts
void psamd::hops_entries(ps_engine* e, const HopsReq& R, const AudEntry* ae, const AudShape& A, HopsEntry* he, uint32_t* lv,
                         Hops::Shape* K) {
  const size_t n = R.topic.size();
  uint32_t lvl0 = 0;
  uint64_t part0 = 0;
  K->max_cols = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = R.topic[i];
    HopsEntry h{t, ae[i].strip0, 0, R.row[i], 0, 0, 1, static_cast<uint32_t>(part0)};
    if (hops_active(e, t)) {
      const DrainTopic& T = e->drain.tab.topics[t];
      const auto& src = e->topics[t].level_off;
      h.c_t = e->last_cnt[t];
      h.lvl0 = lvl0;
      h.depth = static_cast<uint32_t>(src.size()) - 2;
      h.per = aud_strip_nodes(T.flags & kDrainGather, T.n_pos / 64);
      if (lv) std::copy(src.begin(), src.end(), lv + lvl0);
      lvl0 += static_cast<uint32_t>(src.size());
      part0 += static_cast<uint64_t>(ae[i + 1].strip0 - ae[i].strip0) + h.depth;
      K->max_cols = std::max(K->max_cols, std::min(h.depth, kHopsCols - 1));
    }
    he[i] = h;
  }
  he[n] = HopsEntry{0, A.ns, 0, 0, 0, 0, 1, static_cast<uint32_t>(part0)};
  K->ns = A.ns;
  K->n_verdicts = A.n_verdicts;
  K->row_bytes = A.row_bytes;
  K->n_parts = part0;
}

namespace {

// classify, then the two hop kernels, over the block `din` on `stream`, into
// the three [rows][PS_MAX_ROUNDS] arrays.  ms: classify, hops, sum (PSAMD_DRAIN_TIMING)
int hops_pass(ps_engine* e, Hops::Pass& P, const uint8_t* din, const Hops::Shape& K, uint64_t* nodes, uint64_t* reached,
              uint64_t* deliv, const PhaseTimer& tm, float* ms) {
  if (K.ns == 0) return PS_OK;  // no row to read: nothing to add
  auto& D = e->drain;
  hipStream_t s = e->stream;
  if (K.n_parts >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one hop pass");
  HIP_TRY(P.d_verdict.ensure(K.n_verdicts), "alloc hop verdicts");
  HIP_TRY(P.d_exc.ensure((static_cast<size_t>(K.ns) + 1) * 8), "alloc hop counts");
  HIP_TRY(P.d_full.ensure(static_cast<size_t>(K.ns) * 4), "alloc hop counts");
  HIP_TRY(P.d_part_r.ensure(K.n_parts * 4), "alloc hop partials");
  HIP_TRY(P.d_part_d.ensure(K.n_parts * 8), "alloc hop partials");
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
  HopsArgs h{};
  h.strips = g.strips;
  h.n_strips = K.ns;
  h.entries = reinterpret_cast<const HopsEntry*>(din);
  h.n = static_cast<uint32_t>(K.n);
  h.levels = reinterpret_cast<const uint32_t*>(din + K.o_lvl);
  h.verdict = g.verdict;
  h.n_exc = g.n_exc;
  h.count_rows = D.env.load_rows;
  h.max_cols = K.max_cols;
  h.part_reached = P.d_part_r.as<uint32_t>();
  h.part_deliv = P.d_part_d.as<uint64_t>();
  h.nodes = nodes;
  h.reached = reached;
  h.deliv = deliv;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_audience_hops(a, h, s), "k_audience_hops");
  HIP_TRY(tm.end(ms[1]), "event");
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_audience_hops_sum(h, s), "k_audience_hops_sum");
  HIP_TRY(tm.end(ms[2]), "event");
  return PS_OK;
}

size_t hops_total_bytes(size_t n) { return 3 * n * kHopsCols * 8; }

}  // namespace

// ---- what the passes over tree levels ask of a topic (the downstream pass too) --

bool psamd::hops_is_mesh(const ps_engine* e, uint32_t t) { return (e->last_topics[t].flags & kTopicMesh) != 0; }

bool psamd::hops_active(ps_engine* e, uint32_t t) {
  uint32_t u0 = 0;
  return e->drain.tab.topics[t].n_pos && aud_nodes(e, t, &u0);
}

// The level table of an active topic is the last window's: one root, every
// level from 1 on non-empty, n_nodes behind the last.  It is written by the
// node-space build alone, and a build drops the last window, so it can only
// differ after the topic was set anew over another kind (its record starts
// afresh, the table empty) with no run since.
bool psamd::hops_levels_stand(ps_engine* e, uint32_t t) {
  uint32_t u0 = 0;
  (void)aud_nodes(e, t, &u0);
  const auto& lv = e->topics[t].level_off;
  // (lv[1] == u0: the strips start at the first node of level 1, which is
  // what k_audience_hops_sum's (lv[d] - lv[1]) / per counts strips from)
  bool ok = lv.size() >= 3 && lv[0] == 0 && lv[1] == u0 && u0 == 1 && lv.back() == e->last_topics[t].n_nodes;
  for (size_t d = 1; ok && d + 1 < lv.size(); ++d) ok = lv[d] < lv[d + 1];
  return ok;
}

// The topic as it is defined now builds into a mesh (graph.cpp's rule: a node
// with two parents, or the root with one, among those the root reaches).
// Only child lists can: a parent array and a join tree give one parent each.
bool psamd::hops_child_lists_mesh(const TopicHost& T) {
  if (!T.exists || T.kind != Kind::Children || T.rp.empty()) return false;
  std::vector<uint8_t> met(T.rp.size() - 1, 0);
  std::vector<uint32_t> todo{T.root};
  met[T.root] = 1;
  while (!todo.empty()) {
    const uint32_t p = todo.back();
    todo.pop_back();
    for (uint32_t k = T.rp[p]; k < T.rp[p + 1]; ++k) {
      if (met[T.cl[k]]++) return true;
      todo.push_back(T.cl[k]);
    }
  }
  return false;
}

// ---- the standing pass's window hook (run.cpp calls it) --------------------------

// The window just remembered, added to the totals: its tables (built here
// where nobody has), the entry table -- per window: it carries the window's
// message counts --, and the level tables and strips, read where the last
// window left them on the device while what they are cut from stays, then
// classify and the two hop kernels.  All on `stream`, behind the window and in
// front of the next node-space rebuild, which `stream` runs too; nothing
// waits.  The level tables are the host's of the node space this window ran
// on: the run built it before its first window, and nothing but a build
// writes them.
int psamd::hops_window(ps_engine* e) {
  auto& D = e->drain;
  auto& H = D.hops;
  auto& S = H.st;
  if (!S.on || !S.open) return PS_OK;
  Drain::Sink::Res* Rp = nullptr;
  int rc = standing_window_begin(e, S, &Rp);
  if (rc) return rc;
  auto& R = *Rp;
  hipStream_t s = e->stream;
  HopsReq Q;
  if ((rc = hops_plan(e, S.topic.data(), S.topic.size(), &Q))) return rc;
  const size_t n = Q.topic.size();
  const uint32_t* const topic = Q.topic.data();

  std::vector<uint64_t> key{e->graph_epoch, n, Q.n_lvl};
  for (size_t i = 0; i < n; ++i) {
    (void)standing_key_topic(e, topic[i], &key);
    key.push_back(static_cast<uint64_t>(Q.row[i]) << 32 | topic[i]);
  }
  Hops::Shape K;
  hops_layout(Q, &K);
  std::vector<AudEntry> ae(n + 1);
  AudShape A;
  uint8_t* hs = nullptr;
  if (standing_key_stands(S, key)) {
    HIP_TRY(sink_stage(R, K.o_lvl, &hs), "alloc hop staging");
    aud_stage(e, topic, n, ae.data(), nullptr, ~0ull, &A);
    hops_entries(e, Q, ae.data(), A, reinterpret_cast<HopsEntry*>(hs), nullptr, &K);
    if (K.ns != H.kept.ns || K.n_verdicts != H.kept.n_verdicts || K.n_parts != H.kept.n_parts || K.o_strips != H.kept.o_strips)
      return e->fail(PS_E_STATE, "hops: the kept strips are not the window's");
    K.bytes = H.kept.bytes;
    HIP_TRY(hipMemcpyAsync(H.track.d_in.p, hs, (n + 1) * sizeof(HopsEntry), hipMemcpyHostToDevice, s), "upload hop entries");
  } else {
    size_t o = 0;
    uint64_t strips_max = 0;
    (void)aud_stage_bytes(e, topic, n, &o, &strips_max);
    if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one hop window");
    HIP_TRY(sink_stage(R, K.o_strips + strips_max * sizeof(AudStrip), &hs), "alloc hop staging");
    if (!aud_stage(e, topic, n, ae.data(), reinterpret_cast<AudStrip*>(hs + K.o_strips), strips_max, &A))
      return e->fail(PS_E_STATE, "hops: more strips than staged");
    hops_entries(e, Q, ae.data(), A, reinterpret_cast<HopsEntry*>(hs), reinterpret_cast<uint32_t*>(hs + K.o_lvl), &K);
    K.bytes = K.o_strips + static_cast<size_t>(K.ns) * sizeof(AudStrip);
    HIP_TRY(H.track.d_in.ensure(K.bytes), "alloc hop strips");
    HIP_TRY(hipMemcpyAsync(H.track.d_in.p, hs, K.bytes, hipMemcpyHostToDevice, s), "upload hop strips");
    H.kept = K;
    S.strip_key = key;
  }
  const PhaseTimer untimed{D.ev_t, s, false};
  float none[3] = {0, 0, 0};
  uint64_t* const acc = H.d_acc.as<uint64_t>();
  const size_t rows = S.topic.size() * kHopsCols;
  if ((rc = hops_pass(e, H.track, H.track.d_in.as<uint8_t>(), K, acc, acc + rows, acc + 2 * rows, untimed, none))) return rc;
  return standing_window_done(e, S, S.topic.size() - n);  // the mesh topics of this window
}

extern "C" {

// ---- ps_topic_hops ---------------------------------------------

int ps_topic_hops(ps_engine* e, const uint32_t* topic, size_t n, uint64_t* nodes_out, uint64_t* reached_out,
                  uint64_t* deliv_out) {
  if (!e || (n && !topic) || (!nodes_out && !reached_out && !deliv_out)) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_topic_hops on a multi-rank engine", "no completed run", nullptr, true})) return rc;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (hops_is_mesh(e, topic[i])) return e->fail(PS_E_STATE, "ps_topic_hops: a mesh topic has no hop per node");
  if (n == 0) return PS_OK;
  auto& D = e->drain;
  auto& H = D.hops;
  auto& Ans = H.ans;
  const auto t_host0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  float ms[4] = {0, 0, 0, 0};  // classify, hops, sum, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  HopsReq Q;
  if ((rc = hops_plan(e, topic, n, &Q))) return rc;
  Hops::Shape K;
  hops_layout(Q, &K);
  size_t o = 0;
  uint64_t strips_max = 0;
  (void)aud_stage_bytes(e, topic, n, &o, &strips_max);
  if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  Ans.stage.resize(K.o_strips + strips_max * sizeof(AudStrip));
  uint8_t* const hs = Ans.stage.data();
  std::vector<AudEntry> ae(n + 1);
  AudShape A;
  if (!aud_stage(e, topic, n, ae.data(), reinterpret_cast<AudStrip*>(hs + K.o_strips), strips_max, &A))
    return e->fail(PS_E_STATE, "hops: more strips than staged");
  hops_entries(e, Q, ae.data(), A, reinterpret_cast<HopsEntry*>(hs), reinterpret_cast<uint32_t*>(hs + K.o_lvl), &K);
  K.bytes = K.o_strips + static_cast<size_t>(K.ns) * sizeof(AudStrip);
  const double host_ms = ms_since(t_host0);

  const size_t rows = n * kHopsCols, out_bytes = hops_total_bytes(n);
  HIP_TRY(H.sync.d_in.ensure(K.bytes), "alloc hop strips");
  HIP_TRY(Ans.d_out.ensure(out_bytes), "alloc hop sums");
  HIP_TRY(pinned_ensure(&Ans.h_out, nullptr, &Ans.out_cap, out_bytes), "alloc hop view");
  uint64_t* const out = Ans.d_out.as<uint64_t>();
  HIP_TRY(hipMemsetAsync(out, 0, out_bytes, s), "clear hop sums");
  if (K.ns) HIP_TRY(hipMemcpyAsync(H.sync.d_in.p, hs, K.bytes, hipMemcpyHostToDevice, s), "upload hop strips");
  if ((rc = hops_pass(e, H.sync, H.sync.d_in.as<uint8_t>(), K, out, out + rows, out + 2 * rows, tm, ms))) return rc;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(hipMemcpyAsync(Ans.h_out, out, out_bytes, hipMemcpyDeviceToHost, s), "read hop sums");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  HIP_TRY(tm.end(ms[3]), "event");
  if (nodes_out) std::memcpy(nodes_out, Ans.h_out, rows * 8);
  if (reached_out) std::memcpy(reached_out, Ans.h_out + rows * 8, rows * 8);
  if (deliv_out) std::memcpy(deliv_out, Ans.h_out + 2 * rows * 8, rows * 8);
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd topic_hops: topics %zu strips %u nodes %llu row_bytes %llu partials %llu classify_ms %.4f hops_ms %.4f "
                 "sum_ms %.4f copy_ms %.4f host_strips_ms %.4f\n",
                 n, K.ns, static_cast<unsigned long long>(K.n_verdicts), static_cast<unsigned long long>(K.row_bytes),
                 static_cast<unsigned long long>(K.n_parts), ms[0], ms[1], ms[2], ms[3], host_ms);
  return PS_OK;
}

// ---- ps_hops_track / ps_hops_take ------------------------------

int ps_hops_track(ps_engine* e, const uint32_t* topic, size_t n) {
  if (!e || (n && !topic)) return PS_E_INVAL;
  auto& H = e->drain.hops;
  if (const int rc = standing_track_check(e, H.st, topic, n)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (hops_child_lists_mesh(e->topics[topic[i]]))
      return e->fail(PS_E_STATE, "ps_hops_track: a mesh topic has no hop per node");
  if (const int rc = standing_quiesce(e, H.st)) return rc;
  standing_retrack(H.st, topic, n);
  auto& P = H.track;
  return standing_totals(e, H.st, H.d_acc, hops_total_bytes(n),
                         {&P.d_in, &P.d_verdict, &P.d_exc, &P.d_full, &P.d_part_r, &P.d_part_d});
}

int ps_hops_take(ps_engine* e, uint64_t* nodes_out, uint64_t* reached_out, uint64_t* deliv_out, uint64_t* n_windows_out,
                 uint64_t* n_skipped_out) {
  if (!e || !n_windows_out || !n_skipped_out) return PS_E_INVAL;
  auto& H = e->drain.hops;
  auto& S = H.st;
  const size_t rows = S.topic.size() * kHopsCols;
  if (const int rc = standing_take_totals(e, S, H.d_acc, H.ans, hops_total_bytes(S.topic.size()))) return rc;
  const uint8_t* const h = H.ans.h_out;
  if (nodes_out) std::memcpy(nodes_out, h, rows * 8);
  if (reached_out) std::memcpy(reached_out, h + rows * 8, rows * 8);
  if (deliv_out) std::memcpy(deliv_out, h + 2 * rows * 8, rows * 8);
  *n_windows_out = S.windows;
  *n_skipped_out = S.skipped;
  S.windows = S.skipped = 0;
  return PS_OK;
}

}  // extern "C"
