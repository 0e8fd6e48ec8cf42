// drain_spread_track.cpp -- hops and duplicate copies behind every window
// (drain_impl.hpp): ps_spread_track registers standing topics,
// meshes and trees alike, whose spread pass run.cpp's hooks enqueue behind every
// window of a run; ps_spread_take copies the totals since the last take.  A
// window's pass is ps_topic_spread's (drain_spread.cpp) -- the same entry
// table, strips and kernels -- but for where the levels end: the window's last
// round r is the host's by the time the hook runs, and no hop the pass can
// report lies beyond it, so level launches 0 .. r are enqueued whole and
// k_spread_track_close behind them counts the window as truncated should the
// next frontier hold anything.  Every sum the kernels leave is an atomic add,
// so they add into the totals as they add into the blocking call's cleared
// block.  Stream order is the only order between the launches; nothing waits.
// Buffers of its own.
#include "drain_impl.hpp"

using namespace psamd;

namespace {

using Track = Drain::SpreadTrack;

// the totals: the truncated windows, then the blocking call's output block
constexpr size_t kSpreadAccHead = 1;
size_t spread_acc_bytes(size_t n, size_t np) { return (kSpreadAccHead + SpreadOut(n, np).words) * 8; }

// what an index into the child lists is checked against: the edges where the
// host's copy of the node space stands, else the words d_col holds (a GPU-built
// node space is not read back for this pass)
uint32_t spread_edge_bound(const ps_engine* e) {
  if (e->mirrors_valid) return e->row_ptr.empty() ? 0u : e->row_ptr.back();
  return static_cast<uint32_t>(std::min<size_t>(e->d_col.bytes / 4, 0xFFFFFFFFu));
}

}  // namespace

// ---- the standing pass's window hook (run.cpp calls it) --------------------------

// The window just remembered, added to the totals: its tables (built here
// where nobody has), the entry table and the first frontier -- per window: they
// carry the window's message counts and which topics take part --, the strips,
// read where the last window left them on the device while what they are cut
// from stays, the scratch words cleared, then the pass.  All on `stream`,
// behind the window and in front of the next node-space rebuild, which `stream`
// runs too; nothing waits.
int psamd::spread_window(ps_engine* e) {
  auto& D = e->drain;
  auto& T = D.spread_trk;
  auto& S = T.st;
  if (!S.on || !S.open) return PS_OK;
  const auto t_host0 = hclock::now();
  const size_t n = S.topic.size();
  const uint32_t* const topic = S.topic.data();
  Drain::Sink::Res* Rp = nullptr;
  int rc = standing_window_begin(e, S, &Rp);
  if (rc) return rc;
  auto& R = *Rp;
  hipStream_t s = e->stream;
  auto& B = T.track;

  std::vector<uint64_t> key{e->graph_epoch, n};
  for (size_t i = 0; i < n; ++i) {
    const uint32_t u0 = standing_key_topic(e, topic[i], &key);
    key.push_back(static_cast<uint64_t>(u0) << 32 | topic[i]);
  }
  // one region of the run's staging: entries | first frontier (its three
  // counts in front) | strips, the last part where the kept block does not stand
  const size_t o_seed = align256((n + 1) * sizeof(SpreadEntry));
  const size_t o_strips = o_seed + align256(kSpreadCntBytes + n * sizeof(SpreadItem));
  // (on the device the strips follow the entries, as the blocking call lays them out)
  const size_t d_strips = o_seed;
  std::vector<AudEntry> ae(n + 1);
  AudShape A;
  uint8_t* hs = nullptr;
  const bool kept = standing_key_stands(S, key);
  uint64_t staged_bytes = 0;
  if (kept) {
    HIP_TRY(sink_stage(R, o_strips, &hs), "alloc spread staging");
    aud_stage(e, topic, n, ae.data(), nullptr, ~0ull, &A);
    if (A.ns != T.kept.ns || A.n_verdicts != T.kept.n_verdicts)
      return e->fail(PS_E_STATE, "spread: the kept strips are not the window's");
  } else {
    size_t o = 0;
    uint64_t strips_max = 0;
    (void)aud_stage_bytes(e, topic, n, &o, &strips_max);
    if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one spread window");
    HIP_TRY(sink_stage(R, o_strips + strips_max * sizeof(AudStrip), &hs), "alloc spread staging");
    if (!aud_stage(e, topic, n, ae.data(), reinterpret_cast<AudStrip*>(hs + o_strips), strips_max, &A))
      return e->fail(PS_E_STATE, "spread: more strips than staged");
  }
  std::memset(hs + o_seed, 0, kSpreadCntBytes);
  SpreadPlan P;
  spread_entries(e, topic, n, ae.data(), A, reinterpret_cast<SpreadEntry*>(hs),
                 reinterpret_cast<SpreadItem*>(hs + o_seed + kSpreadCntBytes), &P);
  if (P.n_nodes >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many nodes in one spread window");
  std::memcpy(hs + o_seed, &P.n_roots, 4);
  // the strips stay on the device whether or not a topic takes part in this window
  if (!kept) {
    const size_t strip_bytes = static_cast<size_t>(A.ns) * sizeof(AudStrip);
    HIP_TRY(B.d_in.ensure(d_strips + strip_bytes), "alloc spread strips");
    if (strip_bytes)
      HIP_TRY(hipMemcpyAsync(B.d_in.as<uint8_t>() + d_strips, hs + o_strips, strip_bytes, hipMemcpyHostToDevice, s),
              "upload spread strips");
    staged_bytes += strip_bytes;
    T.kept.ns = A.ns;
    T.kept.n_verdicts = A.n_verdicts;
    S.strip_key = key;
  }
  uint32_t launches = 0;
  float ms[4] = {0, 0, 0, 0};  // classify, nodes, levels + close, sum (PSAMD_DRAIN_TIMING)
  // (the events are the pass's own: no blocking call need have created the drain's)
  for (auto& ev : T.ev_t)
    if (D.env.timing && !ev) HIP_TRY(hipEventCreate(&ev), "spread event");
  const PhaseTimer tm{T.ev_t, s, D.env.timing};
  const double host_ms = ms_since(t_host0);
  if (P.n_roots) {  // (no topic takes part: the window adds nothing)
    if ((rc = spread_ensure(e, B, A, P))) return rc;
    HIP_TRY(hipMemcpyAsync(B.d_in.p, hs, (n + 1) * sizeof(SpreadEntry), hipMemcpyHostToDevice, s), "upload spread entries");
    HIP_TRY(hipMemcpyAsync(B.d_queue.p, hs + o_seed, kSpreadCntBytes + P.n_roots * sizeof(SpreadItem), hipMemcpyHostToDevice, s),
            "upload spread roots");
    staged_bytes += (n + 1) * sizeof(SpreadEntry) + kSpreadCntBytes + P.n_roots * sizeof(SpreadItem);
    // the per-node words: no messages, no hop
    HIP_TRY(hipMemsetAsync(B.d_scratch.p, 0, P.n_nodes * 4, s), "clear spread words");
    HIP_TRY(hipMemsetAsync(B.d_scratch.as<uint32_t>() + P.n_nodes, 0xFF, P.n_nodes * 4, s), "clear spread hops");
    uint64_t* const acc = T.d_acc.as<uint64_t>();
    const SpreadOut O(n, e->cfg.n_peers);
    const DrainArgs a = drain_args(e, D.tab);
    const SpreadArgs p = spread_args(e, B, d_strips, n, A, P, spread_edge_bound(e), acc + kSpreadAccHead, O);
    const AudArgs g = spread_classify_args(e, p, B);
    if (A.ns) {
      HIP_TRY(tm.begin(), "event");
      HIP_TRY(launch_audience_classify(a, g, s), "k_audience_classify");
      HIP_TRY(tm.end(ms[0]), "event");
    }
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_spread_nodes(a, p, s), "k_spread_nodes");
    // (a take may ask for the unreached nodes of any window since the last one)
    if (P.n_mesh) HIP_TRY(launch_spread_unreached(p, s), "k_spread_unreached");
    HIP_TRY(tm.end(ms[1]), "event");
    // The levels 0 .. r: a forwarder's hop is at most the round it was reached
    // in, and the window ended with round r.  A launch over
    // an empty frontier leaves the next one empty.
    const uint64_t want = std::min<uint64_t>(static_cast<uint64_t>(e->last_rounds) + 1, D.env.spread_track_levels);
    const uint32_t blocks = spread_level_blocks(P);
    HIP_TRY(tm.begin(), "event");
    for (; launches < want; ++launches) HIP_TRY(launch_spread_level(p, launches, blocks, s), "k_spread_level");
    HIP_TRY(launch_spread_track_close(p.cnt, launches, acc, s), "k_spread_track_close");
    HIP_TRY(tm.end(ms[2]), "event");
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_spread_sum(p, s), "k_spread_sum");
    HIP_TRY(tm.end(ms[3]), "event");
    T.level_launches += launches;
  }
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd spread_track: window %llu topics %zu strips %u nodes %llu row_bytes %llu rounds %u level_launches %u "
                 "staged_bytes %llu kept %d classify_ms %.4f nodes_ms %.4f levels_ms %.4f sum_ms %.4f host_ms %.4f\n",
                 static_cast<unsigned long long>(S.windows), n, A.ns, static_cast<unsigned long long>(P.n_nodes),
                 static_cast<unsigned long long>(A.row_bytes), e->last_rounds, launches,
                 static_cast<unsigned long long>(staged_bytes), kept ? 1 : 0, ms[0], ms[1], ms[2], ms[3], host_ms);
  return standing_window_done(e, S, 0);
}

extern "C" {

// ---- ps_spread_track / ps_spread_take ----------------------------

int ps_spread_track(ps_engine* e, const uint32_t* topic, size_t n) {
  if (!e || (n && !topic)) return PS_E_INVAL;
  auto& T = e->drain.spread_trk;
  if (const int rc = standing_track_check(e, T.st, topic, n)) return rc;
  if (const int rc = standing_quiesce(e, T.st)) return rc;
  standing_retrack(T.st, topic, n);
  T.level_launches = 0;
  auto& P = T.track;
  return standing_totals(e, T.st, T.d_acc, spread_acc_bytes(n, e->cfg.n_peers),
                         {&P.d_in, &P.d_verdict, &P.d_exc, &P.d_full, &P.d_scratch, &P.d_queue});
}

int ps_spread_take(ps_engine* e, uint64_t* reached_out, uint64_t* deliv_out, uint64_t* unreached_out, uint64_t* stranded_out,
                   uint64_t* copies_out, uint64_t* dup_out, uint64_t* n_windows_out, uint64_t* n_truncated_out) {
  if (!e || !n_windows_out || !n_truncated_out) return PS_E_INVAL;
  auto& D = e->drain;
  auto& T = D.spread_trk;
  auto& S = T.st;
  if (const int rc = standing_take_enter(e, S)) return rc;
  const auto t0 = hclock::now();
  const size_t n = S.topic.size(), np = e->cfg.n_peers;
  const SpreadOut O(n, np);
  const size_t bytes = spread_acc_bytes(n, np);
  HIP_TRY(pinned_ensure(&T.ans.h_out, nullptr, &T.ans.out_cap, bytes), "alloc spread view");
  if (const int rc = standing_take_event(e, S)) return rc;
  // every pass ran on `stream`: dup over the totals behind them, two copies at
  // most -- the count and the per-topic part, and the peer arrays asked for --,
  // the clearing behind the copies and in front of whatever runs next, one wait
  hipStream_t s = e->stream;
  uint64_t* const acc = T.d_acc.as<uint64_t>();
  uint64_t* const out = acc + kSpreadAccHead;
  if (dup_out) {
    SpreadArgs p{};
    p.n_peers = static_cast<uint32_t>(np);
    p.recv = out + O.recv;
    p.copies = out + O.copies;
    p.dup = out + O.dup;
    HIP_TRY(launch_spread_dup(p, s), "k_spread_dup");
  }
  size_t copied = (kSpreadAccHead + O.recv) * 8;
  HIP_TRY(hipMemcpyAsync(T.ans.h_out, acc, copied, hipMemcpyDeviceToHost, s), "read spread totals");
  if (copies_out || dup_out) {
    const size_t lo = kSpreadAccHead + (copies_out ? O.copies : O.dup), hi = kSpreadAccHead + (dup_out ? O.words : O.dup);
    HIP_TRY(hipMemcpyAsync(T.ans.h_out + lo * 8, acc + lo, (hi - lo) * 8, hipMemcpyDeviceToHost, s), "read spread totals");
    copied += (hi - lo) * 8;
  }
  HIP_TRY(hipMemsetAsync(acc, 0, bytes, s), "clear spread totals");
  HIP_TRY(hipEventRecord(S.ev_take, s), "event");
  HIP_TRY(hipEventSynchronize(S.ev_take), "wait for the spread totals");
  standing_settled(S);
  const uint64_t* const h = reinterpret_cast<const uint64_t*>(T.ans.h_out) + kSpreadAccHead;
  if (n && reached_out) std::memcpy(reached_out, h + O.reached, n * kHopsCols * 8);
  if (n && deliv_out) std::memcpy(deliv_out, h + O.deliv, n * kHopsCols * 8);
  if (n && unreached_out) std::memcpy(unreached_out, h + O.unreached, n * 8);
  if (stranded_out)
    for (size_t i = 0; i < n; ++i) stranded_out[i] = h[O.holders + i] - h[O.visited + i];
  if (copies_out) std::memcpy(copies_out, h + O.copies, np * 8);
  if (dup_out) std::memcpy(dup_out, h + O.dup, np * 8);
  *n_windows_out = S.windows;
  *n_truncated_out = h[-static_cast<ptrdiff_t>(kSpreadAccHead)];
  if (D.env.timing)
    std::fprintf(stderr, "psamd spread_take: windows %llu topics %zu truncated %llu level_launches %llu copied_bytes %llu take_ms %.4f\n",
                 static_cast<unsigned long long>(S.windows), n, static_cast<unsigned long long>(*n_truncated_out),
                 static_cast<unsigned long long>(T.level_launches), static_cast<unsigned long long>(copied), ms_since(t0));
  S.windows = 0;
  T.level_launches = 0;
  return PS_OK;
}

}  // extern "C"
