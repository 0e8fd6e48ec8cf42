// drain_cut.cpp -- losses blamed on their cut points (drain_impl.hpp; DESIGN.md
// §5.5l): for each peer, over the named tree topics, what its own nodes missed
// of the window's messages, and for its cut points -- nodes that lack messages
// under a full parent -- how many there are, how many nodes hang behind them
// and how many deliveries did not happen at and behind them.  ps_peer_cut
// answers for the last window, blocking; ps_cut_track registers standing topics
// whose pass run.cpp's hooks enqueue behind every window of a run, into totals
// that ps_cut_take copies and clears.  The plan, the input block and the front
// of the pass (k_audience_classify, k_audience_weights) are the downstream
// pass's (drain_downstream.cpp: down_plan .. down_window_stage); behind them
// k_audience_missed over the strips, one k_cut_level launch per level over the
// same work list, and k_cut_top.  Stream order is the only order between the
// launches.  Buffers of their own.
#include "drain_impl.hpp"

using namespace psamd;

namespace {

using Cut = Drain::Cut;

// classify, the weights, the misses, the level launches and the top kernel
// over the block `din` on `stream`, into out: missed | cuts | orphaned | lost,
// [n_peers] each.  ms: classify, weights, missed, levels + top (PSAMD_DRAIN_TIMING)
int cut_pass(ps_engine* e, Cut::Pass& P, const uint8_t* din, const Cut::Shape& K, uint64_t* out, const PhaseTimer& tm,
             float* ms) {
  if (K.ns == 0) return PS_OK;  // no row to read: nothing to add
  hipStream_t s = e->stream;
  const size_t np = e->cfg.n_peers;
  CutArgs g{};
  if (const int rc = down_front(e, P, din, K, tm, ms, &g.d)) return rc;
  g.missed = out;
  g.cuts = out + np;
  g.orphaned = out + 2 * np;
  g.lost = out + 3 * np;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_audience_missed(g, s), "k_audience_missed");
  HIP_TRY(tm.end(ms[2]), "event");
  HIP_TRY(tm.begin(), "event");
  for (size_t j = 0; j + 1 < K.launch.size(); ++j)
    HIP_TRY(launch_cut_level(g, K.launch[j], K.launch[j + 1], s), "k_cut_level");
  HIP_TRY(launch_cut_top(g, s), "k_cut_top");
  HIP_TRY(tm.end(ms[3]), "event");
  return PS_OK;
}

}  // namespace

// ---- the standing pass's window hook (run.cpp calls it) --------------------------

// The window just remembered, added to the totals, as downstream_window adds
// its own: all on `stream`, nothing waits.
int psamd::cut_window(ps_engine* e) {
  auto& D = e->drain;
  auto& H = D.cut;
  if (!H.st.on || !H.st.open) return PS_OK;
  Cut::Shape K;
  size_t n = 0;
  int rc = down_window_stage(e, H.st, H.track, H.kept, &K, &n);
  if (rc) return rc;
  const PhaseTimer untimed{D.ev_t, e->stream, false};
  float none[4] = {0, 0, 0, 0};
  if ((rc = cut_pass(e, H.track, H.track.d_in.as<uint8_t>(), K, H.d_acc.as<uint64_t>(), untimed, none))) return rc;
  return standing_window_done(e, H.st, H.st.topic.size() - n);  // the mesh topics of this window
}

extern "C" {

// ---- ps_peer_cut -------------------------------------------------

int ps_peer_cut(ps_engine* e, const uint32_t* topic, size_t n, uint64_t* missed_out, uint64_t* cuts_out,
                uint64_t* orphaned_out, uint64_t* lost_out) {
  uint64_t* const outs[4] = {missed_out, cuts_out, orphaned_out, lost_out};
  if (!e || (n && !topic) || (!missed_out && !cuts_out && !orphaned_out && !lost_out)) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_peer_cut on a multi-rank engine", "no completed run", nullptr, true})) return rc;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (hops_is_mesh(e, topic[i])) return e->fail(PS_E_STATE, "ps_peer_cut: a mesh topic has no subtrees");
  auto& D = e->drain;
  auto& H = D.cut;
  auto& Ans = H.ans;
  const auto t_host0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  const size_t np = e->cfg.n_peers;
  float ms[5] = {0, 0, 0, 0, 0};  // classify, weights, missed, levels + top, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  Cut::Shape K;
  if ((rc = down_sync_stage(e, Ans.stage, topic, n, "cut", &K))) return rc;
  const double host_ms = ms_since(t_host0);

  HIP_TRY(H.sync.d_in.ensure(K.bytes), "alloc cut strips");
  HIP_TRY(Ans.d_out.ensure(4 * np * 8), "alloc cut sums");
  HIP_TRY(pinned_ensure(&Ans.h_out, nullptr, &Ans.out_cap, 4 * np * 8), "alloc cut view");
  uint64_t* const out = Ans.d_out.as<uint64_t>();
  HIP_TRY(hipMemsetAsync(out, 0, 4 * np * 8, s), "clear cut sums");
  if (K.ns) HIP_TRY(hipMemcpyAsync(H.sync.d_in.p, Ans.stage.data(), K.bytes, hipMemcpyHostToDevice, s), "upload cut strips");
  if ((rc = cut_pass(e, H.sync, H.sync.d_in.as<uint8_t>(), K, out, tm, ms))) return rc;
  // one copy: from the first array asked for to the last
  size_t lo = 0, hi = 4;
  while (!outs[lo]) ++lo;
  while (!outs[hi - 1]) --hi;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(hipMemcpyAsync(Ans.h_out + lo * np * 8, out + lo * np, (hi - lo) * np * 8, hipMemcpyDeviceToHost, s), "read cut sums");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  HIP_TRY(tm.end(ms[4]), "event");
  for (size_t i = lo; i < hi; ++i)
    if (outs[i]) std::memcpy(outs[i], Ans.h_out + i * np * 8, np * 8);
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd peer_cut: topics %zu strips %u nodes %llu row_bytes %llu work %u launches %zu classify_ms %.4f "
                 "weights_ms %.4f missed_ms %.4f levels_ms %.4f copy_ms %.4f host_strips_ms %.4f\n",
                 n, K.ns, static_cast<unsigned long long>(K.n_nodes), static_cast<unsigned long long>(K.row_bytes),
                 K.launch.empty() ? 0u : K.launch.back(), K.launch.empty() ? size_t(3) : K.launch.size() + 2, ms[0], ms[1], ms[2],
                 ms[3], ms[4], host_ms);
  return PS_OK;
}

// ---- ps_cut_track / ps_cut_take ----------------------------------

int ps_cut_track(ps_engine* e, const uint32_t* topic, size_t n) {
  if (!e || (n && !topic)) return PS_E_INVAL;
  auto& H = e->drain.cut;
  if (const int rc = standing_track_check(e, H.st, topic, n)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (hops_child_lists_mesh(e->topics[topic[i]])) return e->fail(PS_E_STATE, "ps_cut_track: a mesh topic has no subtrees");
  if (const int rc = standing_quiesce(e, H.st)) return rc;
  standing_retrack(H.st, topic, n);
  auto& P = H.track;
  return standing_totals(e, H.st, H.d_acc, 4 * static_cast<size_t>(e->cfg.n_peers) * 8,
                         {&P.d_in, &P.d_verdict, &P.d_exc, &P.d_full, &P.d_scratch});
}

int ps_cut_take(ps_engine* e, uint64_t* missed_out, uint64_t* cuts_out, uint64_t* orphaned_out, uint64_t* lost_out,
                uint64_t* n_windows_out, uint64_t* n_skipped_out) {
  if (!e || !n_windows_out || !n_skipped_out) return PS_E_INVAL;
  auto& H = e->drain.cut;
  auto& S = H.st;
  const size_t np = e->cfg.n_peers;
  if (const int rc = standing_take_totals(e, S, H.d_acc, H.ans, 4 * np * 8)) return rc;
  uint64_t* const outs[4] = {missed_out, cuts_out, orphaned_out, lost_out};
  for (size_t i = 0; i < 4; ++i)
    if (outs[i]) std::memcpy(outs[i], H.ans.h_out + i * np * 8, np * 8);
  *n_windows_out = S.windows;
  *n_skipped_out = S.skipped;
  S.windows = S.skipped = 0;
  return PS_OK;
}

}  // extern "C"
