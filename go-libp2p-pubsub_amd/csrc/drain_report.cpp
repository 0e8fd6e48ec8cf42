// drain_report.cpp -- the four answers from one pass (drain_impl.hpp; DESIGN.md
// §5.5m): per-peer load, deliveries by hop, the audience behind each peer and
// the losses blamed on their cut points, the sections selected in `what`, each
// array bit for bit what its own call writes.  ps_peer_report answers for the
// last window, blocking; ps_report_track registers standing topics and
// sections whose pass run.cpp's hooks enqueue behind every window of a run,
// into totals that ps_report_take copies and clears.  Both cut the topics into
// the audience pass's strips -- the tree topics first, in the hop pass's and
// the downstream pass's order, then the topics that feed the load section
// alone --, and run one k_audience_classify, k_report_nodes, the unchanged
// k_audience_hops_sum and one bottom-up sweep.  Buffers of their own.
#include "drain_impl.hpp"

using namespace psamd;

namespace {

using Report = Drain::Report;

static_assert(PS_REPORT_LOAD == kReportLoad && PS_REPORT_HOPS == kReportHops && PS_REPORT_DOWNSTREAM == kReportDown &&
                  PS_REPORT_CUT == kReportCut && PS_REPORT_ALL == kReportAll,
              "the kernels' section bits are the header's");

constexpr uint32_t kTreeSections = kReportAll & ~kReportLoad;
constexpr uint32_t kSubtreeSections = kReportDown | kReportCut;

// the section of each of ps_report's eleven arrays, in the struct's order
constexpr uint32_t kArraySection[11] = {kReportLoad, kReportLoad, kReportHops, kReportHops, kReportHops, kReportDown,
                                        kReportDown, kReportCut,  kReportCut,  kReportCut,  kReportCut};

void report_outs(const ps_report& r, uint64_t* (&p)[11]) {
  uint64_t* const all[11] = {r.recv, r.sent, r.nodes, r.reached, r.deliv, r.below, r.carried, r.missed, r.cuts, r.orphaned, r.lost};
  std::copy(all, all + 11, p);
}

// an output block over n topics: the arrays in ps_report's order
Report::Out report_out(size_t np, size_t n) {
  Report::Out o;
  for (size_t i = 0; i < 11; ++i) o.off[i + 1] = o.off[i] + (kArraySection[i] == kReportHops ? n * kHopsCols : np);
  return o;
}

// A request as the pass takes it: the tree topics (none where the load section
// alone is selected: no level is read then), and behind them the topics that
// feed the load section alone -- the meshes of the window's node space
struct Req {
  std::vector<uint32_t> order;  // aud_stage's topics: the trees, then the rest
  HopsReq hq;                   // the trees with their rows in the request
  DownReq dq;                   // ... and what their level launches come to
  size_t n_mesh = 0;            // meshes among the named topics
};

int report_plan(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what, Req* R) {
  if (what == kReportLoad) {
    R->order.assign(topic, topic + n);
    return PS_OK;
  }
  int rc = down_plan(e, topic, n, "report", &R->dq);
  if (!rc) rc = hops_plan(e, topic, n, &R->hq);
  if (rc) return rc;
  R->order = R->hq.topic;
  for (size_t i = 0; i < n; ++i)
    if (hops_is_mesh(e, topic[i])) {
      R->n_mesh += 1;
      if (what & kReportLoad) R->order.push_back(topic[i]);
    }
  return PS_OK;
}

// where the parts of the pass's input block lie: report entries | hop entries |
// downstream entries | levels | work | strips
void report_layout(const Req& R, Report::Shape* K) {
  K->n = R.order.size();
  K->n_tree = R.hq.topic.size();
  K->o_hops = align256((K->n + 1) * sizeof(ReportEntry));
  K->o_down = K->o_hops + align256((K->n_tree + 1) * sizeof(HopsEntry));
  K->o_lvl = K->o_down + align256((K->n_tree + 1) * sizeof(DownEntry));
  K->o_work = K->o_lvl + align256(std::max<size_t>(R.dq.n_lvl, 1) * 4);
  K->o_strips = K->o_work + align256(std::max<size_t>(R.dq.n_work, 1) * sizeof(DownWork));
}

// aud_stage's entries [n + 1] over R.order as the pass's three tables into the
// block `hs`; the level tables and the work list too where `whole` (else they
// stand on the device, with the launches' bounds in the kept shape)
void report_entries(ps_engine* e, const Req& R, const AudEntry* ae, const AudShape& A, uint8_t* hs, bool whole,
                    Report::Shape* K) {
  const size_t n = K->n, nt = K->n_tree;
  ReportEntry* const re = reinterpret_cast<ReportEntry*>(hs);
  HopsEntry* const he = reinterpret_cast<HopsEntry*>(hs + K->o_hops);
  DownEntry* const de = reinterpret_cast<DownEntry*>(hs + K->o_down);
  Drain::Hops::Shape HK;
  Drain::Downstream::Shape DK;
  hops_entries(e, R.hq, ae, A, he, nullptr, &HK);
  down_entries(e, R.dq, ae, A, de, whole ? reinterpret_cast<uint32_t*>(hs + K->o_lvl) : nullptr,
               whole ? reinterpret_cast<DownWork*>(hs + K->o_work) : nullptr, &DK);
  // the tree strips end where the others begin
  he[nt].strip0 = de[nt].strip0 = ae[nt].strip0;
  for (size_t i = 0; i <= n; ++i) {
    ReportEntry r{};
    r.topic = ae[i].topic;
    r.strip0 = ae[i].strip0;
    r.root = kLoadNoRoot;
    if (i < n) {
      const TopicDev& d = e->last_topics[r.topic];
      if (e->drain.tab.topics[r.topic].n_pos) r.c_t = e->last_cnt[r.topic];
      if ((d.flags & kTopicRootLocal) && d.n_nodes) r.root = d.nbase;
    }
    if (i < nt) {
      r.tree = 1;
      r.lvl0 = he[i].lvl0;
      r.depth = he[i].depth;
      r.part0 = he[i].part0;
      r.n0 = de[i].n0;
    }
    re[i] = r;
  }
  K->ns = A.ns;
  K->n_verdicts = A.n_verdicts;
  K->row_bytes = A.row_bytes;
  K->max_cols = HK.max_cols;
  K->n_parts = HK.n_parts;
  K->n_nodes = DK.n_nodes;
  if (whole) K->launch = DK.launch;
}

// The pass over the block `din` on `stream`, into the block `out` laid out by
// O: classify, k_report_nodes, the hop sums, the bottom-up sweep.
// ms: classify, nodes, hop sums, levels + top (PSAMD_DRAIN_TIMING)
int report_pass(ps_engine* e, Report::Pass& P, const uint8_t* din, const Report::Shape& K, uint32_t what, uint64_t* out,
                const Report::Out& O, const PhaseTimer& tm, float* ms) {
  if (K.ns == 0) return PS_OK;  // no row to read: nothing to add
  auto& D = e->drain;
  hipStream_t s = e->stream;
  const bool hops = (what & kReportHops) && K.n_tree, sub = (what & kSubtreeSections) && K.n_tree;
  if (hops && K.n_parts >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one report pass");
  HIP_TRY(P.d_verdict.ensure(K.n_verdicts), "alloc report verdicts");
  HIP_TRY(P.d_exc.ensure((static_cast<size_t>(K.ns) + 1) * 8), "alloc report counts");
  HIP_TRY(P.d_full.ensure(static_cast<size_t>(K.ns) * 4), "alloc report counts");
  if (hops) {
    HIP_TRY(P.d_part_r.ensure(K.n_parts * 4), "alloc report partials");
    HIP_TRY(P.d_part_d.ensure(K.n_parts * 8), "alloc report partials");
  }
  if (sub) HIP_TRY(P.d_scratch.ensure(K.n_nodes * 16), "alloc report weights");
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

  // the sections the kernels see: without a tree topic the load section alone
  const uint32_t w = K.n_tree ? what : what & kReportLoad;
  if (!w) return PS_OK;
  const uint32_t* const levels = reinterpret_cast<const uint32_t*>(din + K.o_lvl);
  CutArgs c{};
  c.d.strips = g.strips;
  c.d.n_strips = K.ns;
  c.d.entries = reinterpret_cast<const DownEntry*>(din + K.o_down);
  c.d.n = static_cast<uint32_t>(K.n_tree);
  c.d.levels = levels;
  c.d.work = reinterpret_cast<const DownWork*>(din + K.o_work);
  c.d.verdict = g.verdict;
  c.d.n_exc = g.n_exc;
  c.d.count_rows = D.env.load_rows;
  c.d.node_peer = e->d_node_peer.as<uint32_t>();
  c.d.row_ptr = e->d_row_ptr.as<uint32_t>();
  if (sub) {
    // the scratch: w_k | k | w_n, a word per node each
    c.d.w_k = P.d_scratch.as<uint64_t>();
    c.d.k = reinterpret_cast<uint32_t*>(c.d.w_k + K.n_nodes);
    c.d.w_n = c.d.k + K.n_nodes;
  }
  c.d.below = out + O.off[5];
  c.d.carried = out + O.off[6];
  c.missed = out + O.off[7];
  c.cuts = out + O.off[8];
  c.orphaned = out + O.off[9];
  c.lost = out + O.off[10];

  ReportArgs r{};
  r.strips = g.strips;
  r.n_strips = K.ns;
  r.entries = reinterpret_cast<const ReportEntry*>(din);
  r.n = static_cast<uint32_t>(K.n);
  r.what = w;
  r.levels = levels;
  r.verdict = g.verdict;
  r.n_exc = g.n_exc;
  r.count_rows = D.env.load_rows;
  r.node_peer = c.d.node_peer;
  r.row_ptr = c.d.row_ptr;
  r.recv = out + O.off[0];
  r.sent = out + O.off[1];
  r.part_reached = P.d_part_r.as<uint32_t>();
  r.part_deliv = P.d_part_d.as<uint64_t>();
  r.k = c.d.k;
  r.missed = c.missed;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_report_nodes(a, r, s), "k_report_nodes");
  HIP_TRY(tm.end(ms[1]), "event");

  if (hops) {
    HopsArgs h{};
    h.strips = g.strips;
    h.n_strips = K.ns;
    h.entries = reinterpret_cast<const HopsEntry*>(din + K.o_hops);
    h.n = static_cast<uint32_t>(K.n_tree);
    h.levels = levels;
    h.verdict = g.verdict;
    h.n_exc = g.n_exc;
    h.count_rows = D.env.load_rows;
    h.max_cols = K.max_cols;
    h.part_reached = r.part_reached;
    h.part_deliv = r.part_deliv;
    h.nodes = out + O.off[2];
    h.reached = out + O.off[3];
    h.deliv = out + O.off[4];
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_audience_hops_sum(h, s), "k_audience_hops_sum");
    HIP_TRY(tm.end(ms[2]), "event");
  }
  if (sub) {
    const uint32_t both = what & kSubtreeSections;
    HIP_TRY(tm.begin(), "event");
    for (size_t j = 0; j + 1 < K.launch.size(); ++j) {
      const uint32_t w0 = K.launch[j], w1 = K.launch[j + 1];
      if (both == kSubtreeSections) HIP_TRY(launch_report_level(c, w0, w1, s), "k_report_level");
      else if (both == kReportDown) HIP_TRY(launch_downstream_level(c.d, w0, w1, s), "k_downstream_level");
      else HIP_TRY(launch_cut_level(c, w0, w1, s), "k_cut_level");
    }
    if (both == kSubtreeSections) HIP_TRY(launch_report_top(c, s), "k_report_top");
    else if (both == kReportDown) HIP_TRY(launch_downstream_top(c.d, s), "k_downstream_top");
    else HIP_TRY(launch_cut_top(c, s), "k_cut_top");
    HIP_TRY(tm.end(ms[3]), "event");
  }
  return PS_OK;
}

// the checks both entry points make on `what` and the caller's struct
bool report_args_ok(uint32_t what, const ps_report* out, size_t out_size, bool need_array) {
  if (!out || out_size != sizeof(ps_report) || what == 0 || (what & ~kReportAll)) return false;
  if (!need_array) return true;
  uint64_t* p[11];
  report_outs(*out, p);
  for (uint32_t sec = 1; sec <= kReportCut; sec <<= 1) {
    if (!(what & sec)) continue;
    bool any = false;
    for (size_t i = 0; i < 11; ++i) any |= kArraySection[i] == sec && p[i];
    if (!any) return false;
  }
  return true;
}

// the arrays asked for out of the pinned copy `h` of a block laid out by O
// (copied from word `lo` on)
void report_give(const ps_report& out, uint32_t what, const Report::Out& O, const uint8_t* h) {
  uint64_t* p[11];
  report_outs(out, p);
  for (size_t i = 0; i < 11; ++i)
    if ((what & kArraySection[i]) && p[i] && O.off[i + 1] > O.off[i])
      std::memcpy(p[i], h + O.off[i] * 8, (O.off[i + 1] - O.off[i]) * 8);
}

}  // namespace

// ---- the standing pass's window hook (run.cpp calls it) --------------------------

// The window just remembered, added to the totals, as the four standing passes
// add theirs: its tables (built here where nobody has), the three entry tables
// -- per window: they carry the window's message counts --, and the level
// tables, work list and strips, read where the last window left them on the
// device while what they are cut from stays, then the pass.  All on `stream`,
// behind the window and in front of the next node-space rebuild; nothing waits.
int psamd::report_window(ps_engine* e) {
  auto& D = e->drain;
  auto& H = D.report;
  auto& S = H.st;
  if (!S.on || !S.open) return PS_OK;
  Drain::Sink::Res* Rp = nullptr;
  int rc = standing_window_begin(e, S, &Rp);
  if (rc) return rc;
  auto& R = *Rp;
  hipStream_t s = e->stream;
  Req Q;
  if ((rc = report_plan(e, S.topic.data(), S.topic.size(), H.what, &Q))) return rc;
  const size_t n = Q.order.size();
  const uint32_t* const topic = Q.order.data();

  std::vector<uint64_t> key{e->graph_epoch, n, Q.hq.topic.size(), Q.dq.n_lvl, Q.dq.n_work, H.what};
  for (size_t i = 0; i < n; ++i) {
    const uint32_t u0 = standing_key_topic(e, topic[i], &key);
    key.push_back(static_cast<uint64_t>(u0) << 32 | topic[i]);
    key.push_back(i < Q.hq.row.size() ? Q.hq.row[i] : ~0ull);
  }
  Report::Shape K;
  report_layout(Q, &K);
  std::vector<AudEntry> ae(n + 1);
  AudShape A;
  uint8_t* hs = nullptr;
  if (standing_key_stands(S, key)) {
    HIP_TRY(sink_stage(R, K.o_lvl, &hs), "alloc report staging");
    aud_stage(e, topic, n, ae.data(), nullptr, ~0ull, &A);
    report_entries(e, Q, ae.data(), A, hs, false, &K);
    if (K.ns != H.kept.ns || K.n_verdicts != H.kept.n_verdicts || K.n_nodes != H.kept.n_nodes || K.n_parts != H.kept.n_parts ||
        K.o_strips != H.kept.o_strips)
      return e->fail(PS_E_STATE, "report: the kept strips are not the window's");
    K.bytes = H.kept.bytes;
    K.launch = H.kept.launch;
    HIP_TRY(hipMemcpyAsync(H.track.d_in.p, hs, K.o_lvl, hipMemcpyHostToDevice, s), "upload report entries");
  } else {
    size_t o = 0;
    uint64_t strips_max = 0;
    (void)aud_stage_bytes(e, topic, n, &o, &strips_max);
    if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one report window");
    HIP_TRY(sink_stage(R, K.o_strips + strips_max * sizeof(AudStrip), &hs), "alloc report staging");
    if (!aud_stage(e, topic, n, ae.data(), reinterpret_cast<AudStrip*>(hs + K.o_strips), strips_max, &A))
      return e->fail(PS_E_STATE, "report: more strips than staged");
    report_entries(e, Q, ae.data(), A, hs, true, &K);
    K.bytes = K.o_strips + static_cast<size_t>(K.ns) * sizeof(AudStrip);
    HIP_TRY(H.track.d_in.ensure(K.bytes), "alloc report strips");
    HIP_TRY(hipMemcpyAsync(H.track.d_in.p, hs, K.bytes, hipMemcpyHostToDevice, s), "upload report strips");
    H.kept = K;
    S.strip_key = key;
  }
  const PhaseTimer untimed{D.ev_t, s, false};
  float none[4] = {0, 0, 0, 0};
  const Report::Out O = report_out(e->cfg.n_peers, S.topic.size());
  if ((rc = report_pass(e, H.track, H.track.d_in.as<uint8_t>(), K, H.what, H.d_acc.as<uint64_t>(), O, untimed, none))) return rc;
  // the mesh topics of this window, where a tree section is selected
  return standing_window_done(e, S, (H.what & kTreeSections) ? Q.n_mesh : 0);
}

extern "C" {

// ---- ps_peer_report ----------------------------------------------

int ps_peer_report(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what, const ps_report* out_p, size_t out_size) {
  if (!e || (n && !topic) || !report_args_ok(what, out_p, out_size, true)) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_peer_report on a multi-rank engine", "no completed run", nullptr, true})) return rc;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  if (what & kTreeSections)
    for (size_t i = 0; i < n; ++i)
      if (hops_is_mesh(e, topic[i])) return e->fail(PS_E_STATE, "ps_peer_report: a mesh topic answers the load section alone");
  auto& D = e->drain;
  auto& H = D.report;
  auto& Ans = H.ans;
  const auto t_host0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  float ms[5] = {0, 0, 0, 0, 0};  // classify, nodes, hop sums, levels + top, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  Req Q;
  if ((rc = report_plan(e, topic, n, what, &Q))) return rc;
  Report::Shape K;
  report_layout(Q, &K);
  size_t o = 0;
  uint64_t strips_max = 0;
  (void)aud_stage_bytes(e, Q.order.data(), Q.order.size(), &o, &strips_max);
  if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  Ans.stage.resize(K.o_strips + strips_max * sizeof(AudStrip));
  uint8_t* const hs = Ans.stage.data();
  std::vector<AudEntry> ae(Q.order.size() + 1);
  AudShape A;
  if (!aud_stage(e, Q.order.data(), Q.order.size(), ae.data(), reinterpret_cast<AudStrip*>(hs + K.o_strips), strips_max, &A))
    return e->fail(PS_E_STATE, "report: more strips than staged");
  report_entries(e, Q, ae.data(), A, hs, true, &K);
  K.bytes = K.o_strips + static_cast<size_t>(K.ns) * sizeof(AudStrip);
  const double host_ms = ms_since(t_host0);

  const Report::Out O = report_out(e->cfg.n_peers, n);
  const size_t out_bytes = O.off[11] * 8;
  HIP_TRY(H.sync.d_in.ensure(K.bytes), "alloc report strips");
  HIP_TRY(Ans.d_out.ensure(out_bytes), "alloc report sums");
  HIP_TRY(pinned_ensure(&Ans.h_out, nullptr, &Ans.out_cap, out_bytes), "alloc report view");
  uint64_t* const out = Ans.d_out.as<uint64_t>();
  HIP_TRY(hipMemsetAsync(out, 0, out_bytes, s), "clear report sums");
  if (K.ns) HIP_TRY(hipMemcpyAsync(H.sync.d_in.p, hs, K.bytes, hipMemcpyHostToDevice, s), "upload report strips");
  if ((rc = report_pass(e, H.sync, H.sync.d_in.as<uint8_t>(), K, what, out, O, tm, ms))) return rc;
  // one copy: from the first array asked for to the last
  uint64_t* p[11];
  report_outs(*out_p, p);
  size_t lo = 11, hi = 0;
  for (size_t i = 0; i < 11; ++i)
    if ((what & kArraySection[i]) && p[i]) {
      lo = std::min(lo, i);
      hi = i + 1;
    }
  HIP_TRY(tm.begin(), "event");
  if (O.off[hi] > O.off[lo])
    HIP_TRY(hipMemcpyAsync(Ans.h_out + O.off[lo] * 8, out + O.off[lo], (O.off[hi] - O.off[lo]) * 8, hipMemcpyDeviceToHost, s),
            "read report sums");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  HIP_TRY(tm.end(ms[4]), "event");
  report_give(*out_p, what, O, Ans.h_out);
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd peer_report: topics %zu what %u strips %u nodes %llu row_bytes %llu partials %llu work %u launches %zu "
                 "classify_ms %.4f nodes_ms %.4f sum_ms %.4f levels_ms %.4f copy_ms %.4f host_strips_ms %.4f\n",
                 n, what, K.ns, static_cast<unsigned long long>(K.n_nodes), static_cast<unsigned long long>(K.row_bytes),
                 static_cast<unsigned long long>(K.n_parts), K.launch.empty() ? 0u : K.launch.back(),
                 K.launch.empty() ? size_t(0) : K.launch.size() - 1, ms[0], ms[1], ms[2], ms[3], ms[4], host_ms);
  return PS_OK;
}

// ---- ps_report_track / ps_report_take -----------------------------

int ps_report_track(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what) {
  if (!e || (n && !topic) || what == 0 || (what & ~kReportAll)) return PS_E_INVAL;
  auto& H = e->drain.report;
  if (const int rc = standing_track_check(e, H.st, topic, n)) return rc;
  if (what & kTreeSections)
    for (size_t i = 0; i < n; ++i)
      if (hops_child_lists_mesh(e->topics[topic[i]]))
        return e->fail(PS_E_STATE, "ps_report_track: a mesh topic answers the load section alone");
  if (const int rc = standing_quiesce(e, H.st)) return rc;
  standing_retrack(H.st, topic, n);
  H.what = what;
  auto& P = H.track;
  return standing_totals(e, H.st, H.d_acc, report_out(e->cfg.n_peers, n).off[11] * 8,
                         {&P.d_in, &P.d_verdict, &P.d_exc, &P.d_full, &P.d_part_r, &P.d_part_d, &P.d_scratch});
}

int ps_report_take(ps_engine* e, const ps_report* out_p, size_t out_size, uint64_t* n_windows_out, uint64_t* n_skipped_out) {
  if (!e || !out_p || out_size != sizeof(ps_report) || !n_windows_out || !n_skipped_out) return PS_E_INVAL;
  auto& H = e->drain.report;
  auto& S = H.st;
  const Report::Out O = report_out(e->cfg.n_peers, S.topic.size());
  if (const int rc = standing_take_totals(e, S, H.d_acc, H.ans, O.off[11] * 8)) return rc;
  report_give(*out_p, H.what, O, H.ans.h_out);
  *n_windows_out = S.windows;
  *n_skipped_out = S.skipped;
  S.windows = S.skipped = 0;
  return PS_OK;
}

}  // extern "C"
