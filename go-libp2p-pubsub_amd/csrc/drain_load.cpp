// drain_load.cpp -- per-peer load (drain_impl.hpp): how many
// messages each peer received and how many copies it sent, summed over the
// named topics.  ps_peer_load answers for the last window, blocking;
// ps_load_track registers standing topics whose pass run.cpp's hooks enqueue
// behind every window of a run, into totals that ps_load_take copies and
// clears.  Both cut the topics into the audience pass's strips (aud_stage),
// run the unchanged k_audience_classify over them and k_audience_load behind
// it, with buffers of their own.
#include "drain_impl.hpp"

using namespace psamd;

namespace {

using Load = Drain::Load;

static_assert(sizeof(LoadEntry) == sizeof(AudEntry), "aud_stage's entry table is rewritten in place");

// aud_stage's entries [n + 1], rewritten as the load pass's: the topic's
// window messages and its root's node in place of the list segments
void load_entries(const ps_engine* e, uint8_t* entries, size_t n) {
  for (size_t i = 0; i <= n; ++i) {
    AudEntry a;
    std::memcpy(&a, entries + i * sizeof(AudEntry), sizeof a);
    LoadEntry l{a.topic, a.strip0, 0, kLoadNoRoot};
    if (i < n) {
      const TopicDev& d = e->last_topics[a.topic];
      if (e->drain.tab.topics[a.topic].n_pos) l.c_t = e->last_cnt[a.topic];
      if ((d.flags & kTopicRootLocal) && d.n_nodes) l.root = d.nbase;
    }
    std::memcpy(entries + i * sizeof(LoadEntry), &l, sizeof l);
  }
}

// classify, then load, over the entries and strips of `din` on `stream`, into
// recv / sent.  ms: classify, load (PSAMD_DRAIN_TIMING)
int load_pass(ps_engine* e, Load::Pass& P, const uint8_t* din, size_t o_strips, size_t n, uint32_t ns, uint64_t n_verdicts,
              uint64_t* recv, uint64_t* sent, const PhaseTimer& tm, float* ms) {
  if (ns == 0) return PS_OK;  // no row to read: nothing to add
  auto& D = e->drain;
  hipStream_t s = e->stream;
  HIP_TRY(P.d_verdict.ensure(n_verdicts), "alloc load verdicts");
  HIP_TRY(P.d_exc.ensure((static_cast<size_t>(ns) + 1) * 8), "alloc load counts");
  HIP_TRY(P.d_full.ensure(static_cast<size_t>(ns) * 4), "alloc load counts");
  const DrainArgs a = drain_args(e, D.tab);
  AudArgs g{};
  g.strips = reinterpret_cast<const AudStrip*>(din + o_strips);
  g.n_strips = ns;
  g.share = D.env.share;
  g.verdict = P.d_verdict.as<uint8_t>();
  g.n_exc = P.d_exc.as<uint64_t>();
  g.n_full = P.d_full.as<uint32_t>();
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_audience_classify(a, g, s), "k_audience_classify");
  HIP_TRY(tm.end(ms[0]), "event");
  LoadArgs l{};
  l.strips = g.strips;
  l.n_strips = ns;
  l.entries = reinterpret_cast<const LoadEntry*>(din);
  l.n = static_cast<uint32_t>(n);
  l.verdict = g.verdict;
  l.node_peer = e->d_node_peer.as<uint32_t>();
  l.row_ptr = e->d_row_ptr.as<uint32_t>();
  l.count_rows = D.env.load_rows;
  l.recv = recv;
  l.sent = sent;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_audience_load(a, l, s), "k_audience_load");
  HIP_TRY(tm.end(ms[1]), "event");
  return PS_OK;
}

}  // namespace

// ---- the standing pass's window hook (run.cpp calls it) --------------------------

// The window just remembered, added to the totals: its tables (built here
// where nobody has), the entry table -- per window: it carries the window's
// message counts -- and the strips, read where the last window left them on
// the device while what they are cut from stays, then classify and load.  All
// on `stream`, behind the window and in front of the next node-space rebuild,
// which `stream` runs too; nothing waits.
int psamd::load_window(ps_engine* e) {
  auto& D = e->drain;
  auto& L = D.load;
  auto& S = L.st;
  if (!S.on || !S.open) return PS_OK;
  const size_t n = S.topic.size();
  const uint32_t* const topic = S.topic.data();
  Drain::Sink::Res* Rp = nullptr;
  int rc = standing_window_begin(e, S, &Rp);
  if (rc) return rc;
  auto& R = *Rp;
  hipStream_t s = e->stream;

  std::vector<uint64_t> key{e->graph_epoch, n};
  for (size_t i = 0; i < n; ++i) {
    const uint32_t u0 = standing_key_topic(e, topic[i], &key);
    key.push_back(u0);
  }
  const size_t o_strips = align256((n + 1) * sizeof(LoadEntry));
  AudShape A;
  uint8_t* hs = nullptr;
  if (standing_key_stands(S, key)) {
    HIP_TRY(sink_stage(R, o_strips, &hs), "alloc load staging");
    aud_stage(e, topic, n, reinterpret_cast<AudEntry*>(hs), nullptr, ~0ull, &A);
    if (A.ns != L.kept.ns || A.n_verdicts != L.kept.n_verdicts)
      return e->fail(PS_E_STATE, "load: the kept strips are not the window's");
    load_entries(e, hs, n);
    HIP_TRY(hipMemcpyAsync(L.track.d_in.p, hs, (n + 1) * sizeof(LoadEntry), hipMemcpyHostToDevice, s), "upload load entries");
  } else {
    size_t o = 0;
    uint64_t strips_max = 0;
    const size_t bytes = aud_stage_bytes(e, topic, n, &o, &strips_max);
    if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one load window");
    HIP_TRY(sink_stage(R, bytes, &hs), "alloc load staging");
    if (!aud_stage(e, topic, n, reinterpret_cast<AudEntry*>(hs), reinterpret_cast<AudStrip*>(hs + o_strips), strips_max, &A))
      return e->fail(PS_E_STATE, "load: more strips than staged");
    load_entries(e, hs, n);
    const size_t in_bytes = o_strips + static_cast<size_t>(A.ns) * sizeof(AudStrip);
    HIP_TRY(L.track.d_in.ensure(in_bytes), "alloc load strips");
    HIP_TRY(hipMemcpyAsync(L.track.d_in.p, hs, in_bytes, hipMemcpyHostToDevice, s), "upload load strips");
    L.kept = {A.ns, A.n_verdicts};
    S.strip_key = key;
  }
  const PhaseTimer untimed{D.ev_t, s, false};
  float none[2] = {0, 0};
  uint64_t* const acc = L.d_acc.as<uint64_t>();
  if ((rc = load_pass(e, L.track, L.track.d_in.as<uint8_t>(), o_strips, n, A.ns, A.n_verdicts, acc, acc + e->cfg.n_peers,
                      untimed, none)))
    return rc;
  return standing_window_done(e, S, 0);
}

extern "C" {

// ---- ps_peer_load ---------------------------------------------

int ps_peer_load(ps_engine* e, const uint32_t* topic, size_t n, uint64_t* recv_out, uint64_t* sent_out) {
  if (!e || (n && !topic) || (!recv_out && !sent_out)) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_peer_load on a multi-rank engine", "no completed run", nullptr, true})) return rc;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  auto& D = e->drain;
  auto& L = D.load;
  auto& Ans = L.ans;
  const auto t_host0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  const size_t np = e->cfg.n_peers;
  float ms[3] = {0, 0, 0};  // classify, load, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  size_t o_strips = 0;
  uint64_t strips_max = 0;
  const size_t bytes = aud_stage_bytes(e, topic, n, &o_strips, &strips_max);
  if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  Ans.stage.resize(bytes);
  AudShape A;
  if (!aud_stage(e, topic, n, reinterpret_cast<AudEntry*>(Ans.stage.data()),
                 reinterpret_cast<AudStrip*>(Ans.stage.data() + o_strips), strips_max, &A))
    return e->fail(PS_E_STATE, "load: more strips than staged");
  load_entries(e, Ans.stage.data(), n);
  const double host_ms = ms_since(t_host0);

  const size_t in_bytes = o_strips + static_cast<size_t>(A.ns) * sizeof(AudStrip);
  HIP_TRY(L.sync.d_in.ensure(in_bytes), "alloc load strips");
  HIP_TRY(Ans.d_out.ensure(2 * np * 8), "alloc load sums");
  HIP_TRY(pinned_ensure(&Ans.h_out, nullptr, &Ans.out_cap, 2 * np * 8), "alloc load view");
  uint64_t* const out = Ans.d_out.as<uint64_t>();
  HIP_TRY(hipMemsetAsync(out, 0, 2 * np * 8, s), "clear load sums");
  if (A.ns) HIP_TRY(hipMemcpyAsync(L.sync.d_in.p, Ans.stage.data(), in_bytes, hipMemcpyHostToDevice, s), "upload load strips");
  if ((rc = load_pass(e, L.sync, L.sync.d_in.as<uint8_t>(), o_strips, n, A.ns, A.n_verdicts, out, out + np, tm, ms))) return rc;
  // one copy: both arrays, or the one that was asked for
  const size_t lo = recv_out ? 0 : np, hi = sent_out ? 2 * np : np;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(hipMemcpyAsync(Ans.h_out + lo * 8, out + lo, (hi - lo) * 8, hipMemcpyDeviceToHost, s), "read load sums");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  HIP_TRY(tm.end(ms[2]), "event");
  if (recv_out) std::memcpy(recv_out, Ans.h_out, np * 8);
  if (sent_out) std::memcpy(sent_out, Ans.h_out + np * 8, np * 8);
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd peer_load: topics %zu strips %u nodes %llu row_bytes %llu classify_ms %.4f load_ms %.4f copy_ms %.4f "
                 "host_strips_ms %.4f\n",
                 n, A.ns, static_cast<unsigned long long>(A.n_verdicts), static_cast<unsigned long long>(A.row_bytes), ms[0],
                 ms[1], ms[2], host_ms);
  return PS_OK;
}

// ---- ps_load_track / ps_load_take ------------------------------

int ps_load_track(ps_engine* e, const uint32_t* topic, size_t n) {
  if (!e || (n && !topic)) return PS_E_INVAL;
  auto& L = e->drain.load;
  if (const int rc = standing_track_check(e, L.st, topic, n)) return rc;
  if (const int rc = standing_quiesce(e, L.st)) return rc;
  standing_retrack(L.st, topic, n);
  auto& P = L.track;
  return standing_totals(e, L.st, L.d_acc, 2 * static_cast<size_t>(e->cfg.n_peers) * 8,
                         {&P.d_in, &P.d_verdict, &P.d_exc, &P.d_full});
}

int ps_load_take(ps_engine* e, uint64_t* recv_out, uint64_t* sent_out, uint64_t* n_windows_out) {
  if (!e || !n_windows_out) return PS_E_INVAL;
  auto& L = e->drain.load;
  const size_t np = e->cfg.n_peers;
  if (const int rc = standing_take_totals(e, L.st, L.d_acc, L.ans, 2 * np * 8)) return rc;
  if (recv_out) std::memcpy(recv_out, L.ans.h_out, np * 8);
  if (sent_out) std::memcpy(sent_out, L.ans.h_out + np * 8, np * 8);
  *n_windows_out = L.st.windows;
  L.st.windows = 0;
  return PS_OK;
}

}  // extern "C"
