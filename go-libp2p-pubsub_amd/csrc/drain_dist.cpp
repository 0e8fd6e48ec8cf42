// drain_dist.cpp -- a rank's share of the report on a sharded engine
// (drain_impl.hpp): ps_dist_report answers the load, hop and
// downstream sections of ps_peer_report for the nodes this rank owns, on the
// node numbering the last window ran on -- one rank's BFS order or a sharded
// rank's.  The front is the report's: the audience pass's strips (aud_stage)
// and the unchanged k_audience_classify; k_dist_nodes behind it feeds recv /
// sent, the hop partials (k_dist_hops_sum adds them up) and the k word.  The
// downstream section is a sweep that pushes sums from child to parent, one
// k_dist_sweep_level per absolute level from the deepest named topic's depth
// down to the roots; where some edge between a level and the one above crosses
// ranks, the level's send records go through Transport::exchange and
// k_dist_apply adds what arrived.  Which levels exchange and where every record
// lies follows from the replicated topology (TopicHost::gcnt) and the request
// alone, so the ranks make the same exchanges in the same order with no
// handshake.  Blocking; buffers of its own.
//   ps_dist_cut answers ps_peer_cut the same way, through the
// same front, plan and sweep (dist_stage .. dist_sweep): k_dist_cut_nodes
// writes the k word and the misses, k_dist_cut_fill and one exchange in the
// opposite direction bring every remote parent's k to its children's ranks
// ahead of the sweep, and k_dist_cut_level decides at the child -- k < c_t under
// a parent with k == c_t -- and pushes as the sweep does.
//   ps_dist_blame answers ps_topic_blame for the nodes this
// rank owns, through the same front and plan: k_dist_nodes leaves the k word,
// then the sweep's work list is walked from level 1 down -- ahead of a level
// whose edges from the level above cross ranks, k_dist_blame_fill and one
// exchange bring the remote parents' (cut peer, cut hop) pairs, and
// k_dist_blame_level decides at the child.  k_dist_blame_count, the scan and
// k_dist_blame_emit turn the words into records, lent from pinned memory.
#include "drain_impl.hpp"

using namespace psamd;

namespace {

static_assert(PS_REPORT_DIST == (kReportLoad | kReportHops | kReportDown), "the sections ps_dist_report answers");
static_assert(sizeof(DistRec) == 16, "a sweep record is two 64-bit words");

// the section of each of the seven arrays the call may write, in ps_report's order
constexpr uint32_t kArraySection[7] = {kReportLoad, kReportLoad, kReportHops, kReportHops, kReportHops, kReportDown, kReportDown};

void dist_outs(const ps_report& r, uint64_t* (&p)[7]) {
  uint64_t* const all[7] = {r.recv, r.sent, r.nodes, r.reached, r.deliv, r.below, r.carried};
  std::copy(all, all + 7, p);
}

bool dist_args_ok(uint32_t what, const ps_report* out, size_t out_size) {
  if (!out || out_size != sizeof(ps_report) || what == 0 || (what & ~static_cast<uint32_t>(PS_REPORT_DIST))) return false;
  uint64_t* p[7];
  dist_outs(*out, p);
  for (uint32_t sec = 1; sec <= kReportDown; sec <<= 1) {
    if (!(what & sec)) continue;
    bool any = false;
    for (size_t i = 0; i < 7; ++i) any |= kArraySection[i] == sec && p[i];
    if (!any) return false;
  }
  return true;
}

// one exchange of the sweep: the level whose nodes pushed, the regions in
// bytes per rank, the apply items behind it
struct Xchg {
  uint32_t level = 0;
  std::vector<uint64_t> s_off, s_len, r_off, r_len;
  uint32_t a0 = 0, a1 = 0;
};

// What one call's pass is laid out by: the input block (entries | levels |
// send bases | work | apply | strips) and the sweep's launches
struct Plan {
  std::vector<DistEntry> entries;  // [n + 1]
  std::vector<uint32_t> levels, send_base;
  std::vector<DistWork> work;
  std::vector<DistApply> apply;
  std::vector<uint32_t> launch;  // work items of level max_depth - j: [launch[j], launch[j + 1])
  std::vector<Xchg> xchg;        // by descending level
  uint32_t max_depth = 0;        // the deepest entry's depth (the sweep's first level)
  uint32_t max_cols = 0;         // ... kHopsCols - 1 at most (the hop sums' columns)
  uint64_t n_parts = 0;          // hop partial slots: an entry's strips + depth
  uint64_t n_words = 0;          // per-node words: k, acc_n, acc_k each
  uint64_t n_send = 0, n_recv = 0;
  size_t o_lvl = 0, o_base = 0, o_work = 0, o_apply = 0, o_strips = 0;
  // ps_dist_cut alone (dist_cut_plan): the downward exchange ahead of the
  // sweep -- its fill items, the received runs' first words per (entry, level,
  // owner) as send_base, its regions in bytes per rank -- behind the strips
  bool cut = false;
  std::vector<DistApply> fill;
  std::vector<uint32_t> down_base;
  Xchg down;
  bool down_on = false;              // some named tree topic has a cross-rank edge
  uint64_t n_dsend = 0, n_drecv = 0;  // words
  size_t o_fill = 0, o_dbase = 0;
  // ps_dist_blame alone (dist_blame_plan): a downward exchange per level that
  // has a cross-rank edge, by ascending level, a0 .. a1 its fill items;
  // n_dsend, n_drecv and down_base count 8-byte pairs
  std::vector<Xchg> downs;
};

// which downward exchange a pass stages behind the sweep's tables
enum class DownKind { none, cut, blame };

// the rank's own level table of a tree topic stands for the last window's
// nodes: level 0 the root where this rank owns it, no level running backwards
// (a sharded rank's level may be empty), n_nodes behind the last
bool dist_levels_stand(ps_engine* e, uint32_t t) {
  const TopicDev& d = e->last_topics[t];
  const auto& lv = e->topics[t].level_off;
  if (!e->topics[t].exists || lv.size() < 2) return d.n_nodes == 0;
  uint32_t u0 = 0;
  (void)aud_nodes(e, t, &u0);
  bool ok = lv[0] == 0 && lv[1] == (d.n_nodes ? u0 : 0u) && lv.back() == d.n_nodes;
  for (size_t k = 0; ok && k + 1 < lv.size(); ++k) ok = lv[k] <= lv[k + 1];
  return ok;
}

int dist_plan(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what, const AudEntry* ae, Plan* P) {
  const uint32_t W = static_cast<uint32_t>(std::max(e->world, 1)), me = static_cast<uint32_t>(e->rank);
  const bool levels = what & (kReportHops | kReportDown), sweep = what & kReportDown;
  P->entries.assign(n + 1, DistEntry{});
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = topic[i];
    const TopicDev& d = e->last_topics[t];
    DistEntry E{};
    E.topic = t;
    E.strip0 = ae[i].strip0;
    E.c_t = e->drain.tab.topics[t].n_pos ? e->last_cnt[t] : 0;
    E.root = (d.flags & kTopicRootLocal) && d.n_nodes ? d.nbase : kLoadNoRoot;
    E.tree = hops_is_mesh(e, t) ? 0 : 1;
    E.nbase = d.nbase;
    E.nn = d.n_nodes;
    if (E.tree && levels) {
      if (!dist_levels_stand(e, t)) return e->fail(PS_E_STATE, "dist report: a topic was set anew since the last window: run first");
      const auto& lv = e->topics[t].level_off;
      E.lvl0 = static_cast<uint32_t>(P->levels.size());
      if (lv.size() >= 2) {
        E.depth = static_cast<uint32_t>(lv.size()) - 2;
        P->levels.insert(P->levels.end(), lv.begin(), lv.end());
      } else {
        P->levels.insert(P->levels.end(), 2, 0u);
      }
      if (what & kReportHops) {
        const DrainTopic& T = e->drain.tab.topics[t];
        E.per = aud_strip_nodes(T.flags & kDrainGather, T.n_pos / 64);
        E.part0 = static_cast<uint32_t>(P->n_parts);
        if (ae[i + 1].strip0 > ae[i].strip0) {
          P->n_parts += static_cast<uint64_t>(ae[i + 1].strip0 - ae[i].strip0) + E.depth;
          P->max_cols = std::max(P->max_cols, std::min(E.depth, kHopsCols - 1));
        }
      }
      if (sweep) {
        E.n0 = static_cast<uint32_t>(P->n_words);
        P->n_words += E.nn;
        E.sb0 = static_cast<uint32_t>(P->send_base.size());
        if (W > 1) P->send_base.resize(P->send_base.size() + static_cast<size_t>(E.depth + 1) * W, 0);
        P->max_depth = std::max(P->max_depth, E.depth);
      }
    }
    P->entries[i] = E;
  }
  P->entries[n].strip0 = ae[n].strip0;
  if (P->n_words >= kDrainRowLimit || P->n_parts >= kDrainRowLimit)
    return e->fail(PS_E_RANGE, "too many nodes in one dist report");
  if (!sweep) return PS_OK;

  // the launches, the deepest level first; behind a level whose edges to the
  // level above cross ranks somewhere, its exchange
  P->launch.assign(1, 0);
  for (uint32_t L = P->max_depth + 1; L-- > 0;) {
    for (size_t i = 0; i < n; ++i) {
      const DistEntry& E = P->entries[i];
      if (!E.tree || !E.c_t || !E.nn || L > E.depth) continue;
      const uint32_t lo = P->levels[E.lvl0 + L], hi = std::min(P->levels[E.lvl0 + L + 1], E.nn);
      for (uint32_t u = lo; u < hi; u += kDownBlock)
        P->work.push_back(DistWork{static_cast<uint32_t>(i), u, std::min(hi, u + kDownBlock)});
    }
    P->launch.push_back(static_cast<uint32_t>(P->work.size()));
    if (W == 1 || L == 0) continue;
    Xchg X;
    X.level = L;
    X.s_off.assign(W, 0), X.s_len.assign(W, 0), X.r_off.assign(W, 0), X.r_len.assign(W, 0);
    X.a0 = static_cast<uint32_t>(P->apply.size());
    uint64_t crossing = 0;
    for (uint32_t q = 0; q < W; ++q) {
      X.s_off[q] = P->n_send * sizeof(DistRec);
      X.r_off[q] = P->n_recv * sizeof(DistRec);
      for (size_t i = 0; i < n; ++i) {
        const DistEntry& E = P->entries[i];
        const TopicHost& T = e->topics[E.topic];
        if (!E.tree || L > E.depth || T.gcnt.size() < static_cast<size_t>(E.depth + 2) * W * W) continue;
        const uint32_t* gc = &T.gcnt[static_cast<size_t>(L) * W * W];
        // the records this rank's nodes of level L push to their parents at q,
        // and those q's nodes push to this rank's parents
        const uint32_t out_n = q == me ? 0 : gc[q * W + me], in_n = q == me ? 0 : gc[me * W + q];
        P->send_base[E.sb0 + L * W + q] = static_cast<uint32_t>(P->n_send);
        P->n_send += out_n;
        const uint32_t pl0 = e->dist_slots.pl_off[E.topic][static_cast<size_t>(L) * W + q];
        for (uint32_t j = 0; j < in_n; j += kDownBlock)
          P->apply.push_back(DistApply{static_cast<uint32_t>(i), static_cast<uint32_t>(P->n_recv) + j, pl0 + j,
                                       std::min(kDownBlock, in_n - j)});
        P->n_recv += in_n;
        if (q == 0)
          for (uint32_t a = 0; a < W; ++a)
            for (uint32_t b = 0; b < W; ++b)
              if (a != b) crossing += gc[a * W + b];
      }
      X.s_len[q] = P->n_send * sizeof(DistRec) - X.s_off[q];
      X.r_len[q] = P->n_recv * sizeof(DistRec) - X.r_off[q];
    }
    X.a1 = static_cast<uint32_t>(P->apply.size());
    if (crossing) P->xchg.push_back(std::move(X));
  }
  if (P->n_send >= kDrainRowLimit || P->n_recv >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many records in one dist report");
  return PS_OK;
}

// ps_dist_cut's downward exchange over a sweep's plan: the sweep's regions
// with the two ranks swapped, a 32-bit word where the sweep has a record, all
// levels in one exchange.  The region me -> q holds, level by level and entry
// by entry, the gcnt[(L * world + me) * world + q] parents' words of plist; the
// one received from a is found through down_base as the sweep's send regions
// are through send_base.  A region is padded to whole 16-byte units.
int dist_cut_plan(ps_engine* e, size_t n, Plan* P) {
  const uint32_t W = static_cast<uint32_t>(std::max(e->world, 1)), me = static_cast<uint32_t>(e->rank);
  P->cut = true;
  P->down_base.assign(P->send_base.size(), 0);
  if (W == 1) return PS_OK;
  Xchg& X = P->down;
  X.s_off.assign(W, 0), X.s_len.assign(W, 0), X.r_off.assign(W, 0), X.r_len.assign(W, 0);
  uint64_t crossing = 0;
  for (uint32_t q = 0; q < W; ++q) {
    X.s_off[q] = P->n_dsend * 4;
    X.r_off[q] = P->n_drecv * 4;
    for (uint32_t L = 1; L <= P->max_depth; ++L)
      for (size_t i = 0; i < n; ++i) {
        const DistEntry& E = P->entries[i];
        const TopicHost& T = e->topics[E.topic];
        if (!E.tree || L > E.depth || T.gcnt.size() < static_cast<size_t>(E.depth + 2) * W * W) continue;
        const uint32_t* gc = &T.gcnt[static_cast<size_t>(L) * W * W];
        // the words this rank's parents send to their children at q, and those
        // q's parents send to this rank's children of level L
        const uint32_t out_n = q == me ? 0 : gc[me * W + q], in_n = q == me ? 0 : gc[q * W + me];
        const uint32_t pl0 = e->dist_slots.pl_off[E.topic][static_cast<size_t>(L) * W + q];
        for (uint32_t j = 0; j < out_n; j += kDownBlock)
          P->fill.push_back(DistApply{static_cast<uint32_t>(i), static_cast<uint32_t>(P->n_dsend) + j, pl0 + j,
                                      std::min(kDownBlock, out_n - j)});
        P->n_dsend += out_n;
        P->down_base[E.sb0 + L * W + q] = static_cast<uint32_t>(P->n_drecv);
        P->n_drecv += in_n;
        if (q == 0)
          for (uint32_t a = 0; a < W; ++a)
            for (uint32_t b = 0; b < W; ++b)
              if (a != b) crossing += gc[a * W + b];
      }
    P->n_dsend = (P->n_dsend + 3) & ~3ull;
    P->n_drecv = (P->n_drecv + 3) & ~3ull;
    X.s_len[q] = P->n_dsend * 4 - X.s_off[q];
    X.r_len[q] = P->n_drecv * 4 - X.r_off[q];
  }
  P->down_on = crossing != 0;
  if (P->n_dsend >= kDrainRowLimit || P->n_drecv >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many records in one dist cut");
  return PS_OK;
}

// ps_dist_blame's downward exchanges over a sweep's plan: dist_cut_plan's
// layout -- the sweep's regions with the two ranks swapped, found through
// down_base per (entry, level, owner) -- with an 8-byte pair where the cut has
// a word, and an exchange per level: a level's pairs exist only once the level
// above has run.  Level L's region me -> q holds, entry by entry, the
// gcnt[(L * world + me) * world + q] parents' pairs of plist, padded to whole
// 16-byte units.  Whether a level exchanges follows from gcnt alone, whatever
// c_t is: every rank makes the same exchanges in the same order.
int dist_blame_plan(ps_engine* e, size_t n, Plan* P) {
  const uint32_t W = static_cast<uint32_t>(std::max(e->world, 1)), me = static_cast<uint32_t>(e->rank);
  P->cut = true;
  P->down_base.assign(P->send_base.size(), 0);
  if (W == 1) return PS_OK;
  for (uint32_t L = 1; L <= P->max_depth; ++L) {
    Xchg X;
    X.level = L;
    X.s_off.assign(W, 0), X.s_len.assign(W, 0), X.r_off.assign(W, 0), X.r_len.assign(W, 0);
    X.a0 = static_cast<uint32_t>(P->fill.size());
    uint64_t crossing = 0;
    for (uint32_t q = 0; q < W; ++q) {
      X.s_off[q] = P->n_dsend * 8;
      X.r_off[q] = P->n_drecv * 8;
      for (size_t i = 0; i < n; ++i) {
        const DistEntry& E = P->entries[i];
        const TopicHost& T = e->topics[E.topic];
        if (!E.tree || L > E.depth || T.gcnt.size() < static_cast<size_t>(E.depth + 2) * W * W) continue;
        const uint32_t* gc = &T.gcnt[static_cast<size_t>(L) * W * W];
        // the pairs this rank's parents send to their children at q, and those
        // q's parents send to this rank's children of level L
        const uint32_t out_n = q == me ? 0 : gc[me * W + q], in_n = q == me ? 0 : gc[q * W + me];
        const uint32_t pl0 = e->dist_slots.pl_off[E.topic][static_cast<size_t>(L) * W + q];
        for (uint32_t j = 0; j < out_n; j += kDownBlock)
          P->fill.push_back(DistApply{static_cast<uint32_t>(i), static_cast<uint32_t>(P->n_dsend) + j, pl0 + j,
                                      std::min(kDownBlock, out_n - j)});
        P->n_dsend += out_n;
        P->down_base[E.sb0 + L * W + q] = static_cast<uint32_t>(P->n_drecv);
        P->n_drecv += in_n;
        if (q == 0)
          for (uint32_t a = 0; a < W; ++a)
            for (uint32_t b = 0; b < W; ++b)
              if (a != b) crossing += gc[a * W + b];
      }
      P->n_dsend = (P->n_dsend + 1) & ~1ull;
      P->n_drecv = (P->n_drecv + 1) & ~1ull;
      X.s_len[q] = P->n_dsend * 8 - X.s_off[q];
      X.r_len[q] = P->n_drecv * 8 - X.r_off[q];
    }
    X.a1 = static_cast<uint32_t>(P->fill.size());
    if (crossing) P->downs.push_back(std::move(X));
  }
  if (P->n_dsend >= kDrainRowLimit || P->n_drecv >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many records in one dist blame");
  return PS_OK;
}

// the slot tables of the node space the last window ran on, on the device
int dist_slots_ready(ps_engine* e) {
  auto& S = e->dist_slots;
  if (S.epoch == e->graph_epoch) return PS_OK;
  if (const int rc = build_dist_slots(e, &S)) return rc;
  HIP_TRY(S.d_gslot.ensure(S.gslot.size() * 4), "alloc dist slots");
  HIP_TRY(S.d_plist.ensure(S.plist.size() * 4), "alloc dist slots");
  if (!S.gslot.empty())
    HIP_TRY(hipMemcpyAsync(S.d_gslot.p, S.gslot.data(), S.gslot.size() * 4, hipMemcpyHostToDevice, e->stream), "upload dist slots");
  if (!S.plist.empty())
    HIP_TRY(hipMemcpyAsync(S.d_plist.p, S.plist.data(), S.plist.size() * 4, hipMemcpyHostToDevice, e->stream), "upload dist slots");
  HIP_TRY(hipStreamSynchronize(e->stream), "sync");  // (pageable sources)
  S.epoch = e->graph_epoch;
  return PS_OK;
}

template <class T>
void put(uint8_t* at, const std::vector<T>& v) {
  if (!v.empty()) std::memcpy(at, v.data(), v.size() * sizeof(T));
}

// ---- what ps_dist_report, ps_dist_cut and ps_dist_blame share -------------------------

// The strips' shape (the plan reads the entries' first strips), the plan, then
// the input block in Dist::stage; down: ps_dist_cut's or ps_dist_blame's
// downward exchange too
int dist_stage(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what, DownKind down, Plan* Pp, Drain::AudShape* Ap,
               size_t* in_bytes) {
  const bool cut = down != DownKind::none;
  auto& H = e->drain.dist;
  Plan& P = *Pp;
  Drain::AudShape& A = *Ap;
  size_t o = 0;
  uint64_t strips_max = 0;
  (void)aud_stage_bytes(e, topic, n, &o, &strips_max);
  if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  std::vector<AudEntry> ae(n + 1);
  (void)aud_stage(e, topic, n, ae.data(), nullptr, ~0ull, &A);  // (the shape and the entries' first strips alone)
  if (const int rc = dist_plan(e, topic, n, what, ae.data(), &P)) return rc;
  if (cut)
    if (const int rc = down == DownKind::blame ? dist_blame_plan(e, n, &P) : dist_cut_plan(e, n, &P)) return rc;
  P.o_lvl = align256((n + 1) * sizeof(DistEntry));
  P.o_base = P.o_lvl + align256(std::max<size_t>(P.levels.size(), 1) * 4);
  P.o_work = P.o_base + align256(std::max<size_t>(P.send_base.size(), 1) * 4);
  P.o_apply = P.o_work + align256(std::max<size_t>(P.work.size(), 1) * sizeof(DistWork));
  P.o_strips = P.o_apply + align256(std::max<size_t>(P.apply.size(), 1) * sizeof(DistApply));
  P.o_fill = P.o_strips + (cut ? align256(std::max<size_t>(A.ns, 1) * sizeof(AudStrip)) : std::max<size_t>(A.ns, 1) * sizeof(AudStrip));
  P.o_dbase = P.o_fill + (cut ? align256(std::max<size_t>(P.fill.size(), 1) * sizeof(DistApply)) : 0);
  *in_bytes = P.o_dbase + (cut ? std::max<size_t>(P.down_base.size(), 1) * 4 : 0);
  H.stage.resize(*in_bytes);
  uint8_t* const hs = H.stage.data();
  if (A.ns && !aud_stage(e, topic, n, ae.data(), reinterpret_cast<AudStrip*>(hs + P.o_strips), A.ns, &A))
    return e->fail(PS_E_STATE, "dist report: more strips than staged");
  put(hs, P.entries);
  put(hs + P.o_lvl, P.levels);
  put(hs + P.o_base, P.send_base);
  put(hs + P.o_work, P.work);
  put(hs + P.o_apply, P.apply);
  put(hs + P.o_fill, P.fill);
  put(hs + P.o_dbase, P.down_base);
  return PS_OK;
}

// The buffers both passes work in, and what they add into cleared once up
// front: no send region is rewritten while a peer may read it
int dist_buffers(ps_engine* e, const Plan& P, const Drain::AudShape& A, size_t in_bytes, bool hops) {
  auto& H = e->drain.dist;
  hipStream_t s = e->stream;
  const size_t scratch_bytes = static_cast<size_t>(P.n_words) * 20;
  HIP_TRY(H.d_in.ensure(in_bytes), "alloc dist report input");
  HIP_TRY(H.d_verdict.ensure(A.n_verdicts), "alloc dist report verdicts");
  HIP_TRY(H.d_exc.ensure((static_cast<size_t>(A.ns) + 1) * 8), "alloc dist report counts");
  HIP_TRY(H.d_full.ensure(static_cast<size_t>(A.ns) * 4), "alloc dist report counts");
  if (hops) {
    const size_t n_parts = std::max<size_t>(P.n_parts, 1);
    HIP_TRY(H.d_part_r.ensure(n_parts * 4), "alloc dist report partials");
    HIP_TRY(H.d_part_d.ensure(n_parts * 8), "alloc dist report partials");
  }
  HIP_TRY(H.d_scratch.ensure(scratch_bytes), "alloc dist report words");
  HIP_TRY(H.d_send.ensure(P.n_send * sizeof(DistRec)), "alloc dist report records");
  HIP_TRY(H.d_recv.ensure(P.n_recv * sizeof(DistRec)), "alloc dist report records");
  if (scratch_bytes) HIP_TRY(hipMemsetAsync(H.d_scratch.p, 0, scratch_bytes, s), "clear dist report words");
  if (P.n_send) HIP_TRY(hipMemsetAsync(H.d_send.p, 0, P.n_send * sizeof(DistRec), s), "clear dist report records");
  return PS_OK;
}

// The front of both passes: the block's upload, one k_audience_classify over
// the strips (ms0: its time), and the pass's arguments but for its sums
int dist_front(ps_engine* e, const Plan& P, const Drain::AudShape& A, size_t in_bytes, size_t n, uint32_t what, const DrainArgs& a,
               const PhaseTimer& tm, float& ms0, DistArgs* rp) {
  auto& D = e->drain;
  auto& H = D.dist;
  hipStream_t s = e->stream;
  HIP_TRY(hipMemcpyAsync(H.d_in.p, H.stage.data(), in_bytes, hipMemcpyHostToDevice, s), "upload dist report input");
  const uint8_t* const din = H.d_in.as<uint8_t>();
  AudArgs g{};
  g.strips = reinterpret_cast<const AudStrip*>(din + P.o_strips);
  g.n_strips = A.ns;
  g.share = D.env.share;
  g.verdict = H.d_verdict.as<uint8_t>();
  g.n_exc = H.d_exc.as<uint64_t>();
  g.n_full = H.d_full.as<uint32_t>();
  if (A.ns) {
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_audience_classify(a, g, s), "k_audience_classify");
    HIP_TRY(tm.end(ms0), "event");
  }
  const bool ranks = (what & kReportDown) && e->world > 1;
  DistArgs& r = *rp;
  r = DistArgs{};
  r.strips = g.strips;
  r.n_strips = A.ns;
  r.entries = reinterpret_cast<const DistEntry*>(din);
  r.n = static_cast<uint32_t>(n);
  r.what = what;
  r.world = static_cast<uint32_t>(std::max(e->world, 1));
  r.levels = reinterpret_cast<const uint32_t*>(din + P.o_lvl);
  r.verdict = g.verdict;
  r.n_exc = g.n_exc;
  r.count_rows = D.env.load_rows;
  r.node_peer = e->d_node_peer.as<uint32_t>();
  r.node_parent = e->d_node_parent.as<uint32_t>();
  r.row_ptr = e->d_row_ptr.as<uint32_t>();
  r.part_reached = H.d_part_r.as<uint32_t>();
  r.part_deliv = H.d_part_d.as<uint64_t>();
  r.n_parts = static_cast<uint32_t>(std::max<size_t>(P.n_parts, 1));
  r.acc_n = H.d_scratch.as<uint64_t>();
  r.acc_k = r.acc_n + P.n_words;
  r.k = reinterpret_cast<uint32_t*>(r.acc_k + P.n_words);
  r.work = reinterpret_cast<const DistWork*>(din + P.o_work);
  r.gslot = ranks ? e->dist_slots.d_gslot.as<uint32_t>() : nullptr;
  r.send_base = reinterpret_cast<const uint32_t*>(din + P.o_base);
  r.send = H.d_send.as<DistRec>();
  r.n_send = static_cast<uint32_t>(P.n_send);
  r.apply = reinterpret_cast<const DistApply*>(din + P.o_apply);
  r.plist = e->dist_slots.d_plist.as<uint32_t>();
  r.rcv = H.d_recv.as<DistRec>();
  r.n_recv = static_cast<uint32_t>(P.n_recv);
  r.n_plist = static_cast<uint32_t>(e->dist_slots.plist.size());
  return PS_OK;
}

// The sweep: level(L, w0, w1) launches the pass's kernel over a level's work
// items, the deepest level first; behind a level whose edges cross ranks, its
// exchange and k_dist_apply.  Adds the exchanges made and the bytes shipped.
template <class Level>
int dist_sweep(ps_engine* e, const Plan& P, const DistArgs& r, Level&& level, const char* kernel, uint64_t* exchanges,
               uint64_t* bytes_sent) {
  auto& H = e->drain.dist;
  hipStream_t s = e->stream;
  size_t x = 0;
  for (size_t j = 0; j + 1 < P.launch.size(); ++j) {
    const uint32_t L = P.max_depth - static_cast<uint32_t>(j);
    HIP_TRY(level(L, P.launch[j], P.launch[j + 1]), kernel);
    if (x == P.xchg.size() || P.xchg[x].level != L) continue;
    const Xchg& X = P.xchg[x++];
    std::string xerr;
    const hipError_t xe = e->transport->exchange(H.d_send.as<uint8_t>(), X.s_off, X.s_len, H.d_recv.as<uint8_t>(), X.r_off,
                                                 X.r_len, s, &xerr);
    if (xe != hipSuccess) return e->fail(PS_E_DEVICE, xerr);
    *exchanges += 1;
    for (const uint64_t b : X.s_len) *bytes_sent += b;
    HIP_TRY(launch_dist_apply(r, X.a0, X.a1, s), "k_dist_apply");
  }
  return PS_OK;
}

}  // namespace

extern "C" {

// ---- ps_dist_report -----------------------------------------------

int ps_dist_report(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what, const ps_report* out_p, size_t out_size) {
  if (!e || (n && !topic) || !dist_args_ok(what, out_p, out_size)) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {nullptr, "no completed run", nullptr, false})) return rc;
  if (e->world > 1 && e->infl_count) return e->fail(PS_E_STATE, "a run in flight: ps_wait first");
  if (const int rj = twin_join(e)) return rj;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  if (what != kReportLoad)
    for (size_t i = 0; i < n; ++i)
      if (hops_is_mesh(e, topic[i])) return e->fail(PS_E_STATE, "ps_dist_report: a mesh topic answers the load section alone");
  const bool sweep = what & kReportDown, ranks = e->world > 1;
  if (sweep && ranks && (e->graph_dirty || !e->transport))
    return e->fail(PS_E_STATE, "ps_dist_report: the topics changed since the last run: run first");
  auto& D = e->drain;
  auto& H = D.dist;
  const auto t_host0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (!rc && sweep && ranks) rc = dist_slots_ready(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  float ms[5] = {0, 0, 0, 0, 0};  // classify, nodes, hop sums, sweep, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  Plan P;
  AudShape A;
  size_t in_bytes = 0;
  if ((rc = dist_stage(e, topic, n, what, DownKind::none, &P, &A, &in_bytes))) return rc;
  const double host_ms = ms_since(t_host0);

  // the output block: the seven arrays in ps_report's order
  const size_t np = e->cfg.n_peers;
  size_t off[8] = {0};
  for (size_t i = 0; i < 7; ++i) off[i + 1] = off[i] + (kArraySection[i] == kReportHops ? n * kHopsCols : np);
  const size_t out_bytes = off[7] * 8;
  HIP_TRY(H.d_out.ensure(out_bytes), "alloc dist report sums");
  HIP_TRY(pinned_ensure(&H.h_out, nullptr, &H.out_cap, out_bytes), "alloc dist report view");
  if ((rc = dist_buffers(e, P, A, in_bytes, what & kReportHops))) return rc;
  uint64_t* const out = H.d_out.as<uint64_t>();
  HIP_TRY(hipMemsetAsync(out, 0, std::max<size_t>(out_bytes, 8), s), "clear dist report sums");

  const DrainArgs a = drain_args(e, D.tab);
  DistArgs r{};
  if ((rc = dist_front(e, P, A, in_bytes, n, what, a, tm, ms[0], &r))) return rc;
  r.recv = out + off[0];
  r.sent = out + off[1];
  r.nodes = out + off[2];
  r.reached = out + off[3];
  r.deliv = out + off[4];
  r.below = out + off[5];
  r.carried = out + off[6];
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_dist_nodes(a, r, s), "k_dist_nodes");
  HIP_TRY(tm.end(ms[1]), "event");
  if (what & kReportHops) {
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_dist_hops_sum(r, P.max_cols, s), "k_dist_hops_sum");
    HIP_TRY(tm.end(ms[2]), "event");
  }

  // (PSAMD_DRAIN_TIMING's line) exchanges made, bytes shipped in them, bytes of the send and receive records
  uint64_t exchanges = 0, bytes_sent = 0;
  const uint64_t slot_bytes = (P.n_send + P.n_recv) * sizeof(DistRec);
  if (sweep) {
    HIP_TRY(tm.begin(), "event");
    const auto level = [&](uint32_t L, uint32_t w0, uint32_t w1) { return launch_dist_sweep_level(r, L, w0, w1, s); };
    if ((rc = dist_sweep(e, P, r, level, "k_dist_sweep_level", &exchanges, &bytes_sent))) return rc;
    HIP_TRY(tm.end(ms[3]), "event");
  }

  // one copy: from the first array asked for to the last
  uint64_t* p[7];
  dist_outs(*out_p, p);
  size_t lo = 7, hi = 0;
  for (size_t i = 0; i < 7; ++i)
    if ((what & kArraySection[i]) && p[i]) {
      lo = std::min(lo, i);
      hi = i + 1;
    }
  HIP_TRY(tm.begin(), "event");
  if (hi > lo && off[hi] > off[lo])
    HIP_TRY(hipMemcpyAsync(H.h_out + off[lo] * 8, out + off[lo], (off[hi] - off[lo]) * 8, hipMemcpyDeviceToHost, s),
            "read dist report sums");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  HIP_TRY(tm.end(ms[4]), "event");
  for (size_t i = 0; i < 7; ++i)
    if ((what & kArraySection[i]) && p[i] && off[i + 1] > off[i]) std::memcpy(p[i], H.h_out + off[i] * 8, (off[i + 1] - off[i]) * 8);
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd dist_report: rank %d topics %zu what %u strips %u nodes %llu work %zu launches %zu exchanges %llu "
                 "sent_bytes %llu slot_bytes %llu classify_ms %.4f nodes_ms %.4f sum_ms %.4f sweep_ms %.4f copy_ms %.4f host_plan_ms %.4f\n",
                 e->rank, n, what, A.ns, static_cast<unsigned long long>(P.n_words), P.work.size(),
                 P.launch.empty() ? size_t(0) : P.launch.size() - 1, static_cast<unsigned long long>(exchanges),
                 static_cast<unsigned long long>(bytes_sent), static_cast<unsigned long long>(slot_bytes), ms[0], ms[1], ms[2],
                 ms[3], ms[4], host_ms);
  return PS_OK;
}

// ---- ps_dist_cut ----------------------------------------------------

int ps_dist_cut(ps_engine* e, const uint32_t* topic, size_t n, uint64_t* missed_out, uint64_t* cuts_out,
                uint64_t* orphaned_out, uint64_t* lost_out) {
  uint64_t* const outs[4] = {missed_out, cuts_out, orphaned_out, lost_out};
  if (!e || (n && !topic) || (!missed_out && !cuts_out && !orphaned_out && !lost_out)) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {nullptr, "no completed run", nullptr, false})) return rc;
  if (e->world > 1 && e->infl_count) return e->fail(PS_E_STATE, "a run in flight: ps_wait first");
  if (const int rj = twin_join(e)) return rj;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (hops_is_mesh(e, topic[i])) return e->fail(PS_E_STATE, "ps_dist_cut: a mesh topic has no subtrees");
  const bool ranks = e->world > 1;
  if (ranks && (e->graph_dirty || !e->transport))
    return e->fail(PS_E_STATE, "ps_dist_cut: the topics changed since the last run: run first");
  auto& D = e->drain;
  auto& H = D.dist;
  const auto t_host0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (!rc && ranks) rc = dist_slots_ready(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  float ms[5] = {0, 0, 0, 0, 0};  // classify, nodes, fill + downward exchange, sweep, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  Plan P;
  AudShape A;
  size_t in_bytes = 0;
  if ((rc = dist_stage(e, topic, n, kReportDown, DownKind::cut, &P, &A, &in_bytes))) return rc;
  const double host_ms = ms_since(t_host0);

  // the output block: missed | cuts | orphaned | lost
  const size_t np = e->cfg.n_peers, out_bytes = 4 * np * 8;
  HIP_TRY(H.d_out.ensure(out_bytes), "alloc dist cut sums");
  HIP_TRY(H.d_dsend.ensure(P.n_dsend * 4), "alloc dist cut words");
  HIP_TRY(H.d_drecv.ensure(P.n_drecv * 4), "alloc dist cut words");
  HIP_TRY(pinned_ensure(&H.h_out, nullptr, &H.out_cap, out_bytes), "alloc dist cut view");
  if ((rc = dist_buffers(e, P, A, in_bytes, false))) return rc;
  uint64_t* const out = H.d_out.as<uint64_t>();
  HIP_TRY(hipMemsetAsync(out, 0, std::max<size_t>(out_bytes, 8), s), "clear dist cut sums");
  if (P.n_dsend) HIP_TRY(hipMemsetAsync(H.d_dsend.p, 0, P.n_dsend * 4, s), "clear dist cut words");

  const DrainArgs a = drain_args(e, D.tab);
  DistCutArgs g{};
  if ((rc = dist_front(e, P, A, in_bytes, n, kReportDown, a, tm, ms[0], &g.d))) return rc;
  const uint8_t* const din = H.d_in.as<uint8_t>();
  g.missed = out;
  g.cuts = out + np;
  g.orphaned = out + 2 * np;
  g.lost = out + 3 * np;
  g.fill = reinterpret_cast<const DistApply*>(din + P.o_fill);
  g.down_send = H.d_dsend.as<uint32_t>();
  g.down_recv = H.d_drecv.as<uint32_t>();
  g.down_base = reinterpret_cast<const uint32_t*>(din + P.o_dbase);
  g.n_down_send = static_cast<uint32_t>(P.n_dsend);
  g.n_down_recv = static_cast<uint32_t>(P.n_drecv);
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_dist_cut_nodes(a, g, s), "k_dist_cut_nodes");
  HIP_TRY(tm.end(ms[1]), "event");

  // the parents' k to the children's ranks: one exchange, all levels, ahead of the sweep
  uint64_t exchanges = 0, bytes_sent = 0;
  const uint64_t slot_bytes = (P.n_send + P.n_recv) * sizeof(DistRec) + (P.n_dsend + P.n_drecv) * 4;
  if (P.down_on) {
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_dist_cut_fill(g, static_cast<uint32_t>(P.fill.size()), s), "k_dist_cut_fill");
    std::string xerr;
    const Xchg& X = P.down;
    const hipError_t xe = e->transport->exchange(H.d_dsend.as<uint8_t>(), X.s_off, X.s_len, H.d_drecv.as<uint8_t>(), X.r_off,
                                                 X.r_len, s, &xerr);
    if (xe != hipSuccess) return e->fail(PS_E_DEVICE, xerr);
    exchanges += 1;
    for (const uint64_t b : X.s_len) bytes_sent += b;
    HIP_TRY(tm.end(ms[2]), "event");
  }
  HIP_TRY(tm.begin(), "event");
  const auto level = [&](uint32_t L, uint32_t w0, uint32_t w1) { return launch_dist_cut_level(g, L, w0, w1, s); };
  if ((rc = dist_sweep(e, P, g.d, level, "k_dist_cut_level", &exchanges, &bytes_sent))) return rc;
  HIP_TRY(tm.end(ms[3]), "event");

  // one copy: from the first array asked for to the last
  size_t lo = 0, hi = 4;
  while (!outs[lo]) ++lo;
  while (!outs[hi - 1]) --hi;
  HIP_TRY(tm.begin(), "event");
  if (np) HIP_TRY(hipMemcpyAsync(H.h_out + lo * np * 8, out + lo * np, (hi - lo) * np * 8, hipMemcpyDeviceToHost, s), "read dist cut sums");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  HIP_TRY(tm.end(ms[4]), "event");
  for (size_t i = lo; i < hi; ++i)
    if (outs[i] && np) std::memcpy(outs[i], H.h_out + i * np * 8, np * 8);
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd dist_cut: rank %d topics %zu strips %u nodes %llu work %zu launches %zu exchanges %llu "
                 "sent_bytes %llu slot_bytes %llu classify_ms %.4f nodes_ms %.4f down_ms %.4f sweep_ms %.4f copy_ms %.4f host_plan_ms %.4f\n",
                 e->rank, n, A.ns, static_cast<unsigned long long>(P.n_words), P.work.size(),
                 P.launch.empty() ? size_t(0) : P.launch.size() - 1, static_cast<unsigned long long>(exchanges),
                 static_cast<unsigned long long>(bytes_sent), static_cast<unsigned long long>(slot_bytes), ms[0], ms[1], ms[2],
                 ms[3], ms[4], host_ms);
  return PS_OK;
}

// ---- ps_dist_blame --------------------------------------------------

int ps_dist_blame(ps_engine* e, const uint32_t* topic, size_t n, const uint64_t** rec_off_out, const uint32_t** rec_peer_out,
                  const uint32_t** rec_cut_peer_out, const uint32_t** rec_hop_out, const uint32_t** rec_cut_hop_out,
                  const uint32_t** rec_missed_out, uint64_t* total_out) {
  const uint32_t** const outs[5] = {rec_peer_out, rec_cut_peer_out, rec_hop_out, rec_cut_hop_out, rec_missed_out};
  if (!e || (n && !topic) || !rec_off_out || !total_out) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {nullptr, "no completed run", nullptr, false})) return rc;
  if (e->world > 1 && e->infl_count) return e->fail(PS_E_STATE, "a run in flight: ps_wait first");
  if (const int rj = twin_join(e)) return rj;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (hops_is_mesh(e, topic[i])) return e->fail(PS_E_STATE, "ps_dist_blame: a mesh topic has no cut points");
  const bool ranks = e->world > 1;
  if (ranks && (e->graph_dirty || !e->transport))
    return e->fail(PS_E_STATE, "ps_dist_blame: the topics changed since the last run: run first");
  auto& D = e->drain;
  auto& H = D.dist;
  const auto t_host0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (!rc && ranks) rc = dist_slots_ready(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  float ms[6] = {0, 0, 0, 0, 0, 0};  // classify, nodes, fills + exchanges + sweep, count + scan, emit, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  Plan P;
  AudShape A;
  size_t in_bytes = 0;
  if ((rc = dist_stage(e, topic, n, kReportDown, DownKind::blame, &P, &A, &in_bytes))) return rc;
  const double host_ms = ms_since(t_host0);

  // the record arrays on the device hold every non-root node of the rank's
  // strips, so nothing waits between the scan and the emit; the pinned view is
  // sized by the total, behind the one wait for it
  size_t asked = 0;
  for (auto* o : outs) asked += o != nullptr;
  const uint64_t cap = A.n_verdicts;
  const size_t d_stride = align256(cap * 4), n_off = static_cast<size_t>(A.ns) + 1;
  HIP_TRY(pinned_ensure(&H.h_off, nullptr, &H.off_cap, (n + 1) * 8), "alloc dist blame offsets");
  uint64_t* const h_off = reinterpret_cast<uint64_t*>(H.h_off);
  HIP_TRY(H.d_dsend.ensure(P.n_dsend * 8), "alloc dist blame pairs");
  HIP_TRY(H.d_drecv.ensure(P.n_drecv * 8), "alloc dist blame pairs");
  HIP_TRY(H.d_cut.ensure(std::max<size_t>(P.n_words, 1) * 8), "alloc dist blame words");
  HIP_TRY(H.d_cnt.ensure(n_off * 8), "alloc dist blame counts");
  HIP_TRY(H.d_off.ensure(n_off * 8), "alloc dist blame offsets");
  HIP_TRY(H.d_rec_off.ensure((n + 1) * 8), "alloc dist blame offsets");
  HIP_TRY(H.d_rec.ensure(std::max<size_t>(std::max<size_t>(asked, 1) * d_stride, 1)), "alloc dist blame records");
  size_t scan_bytes = 0;
  HIP_TRY(drain_scan(nullptr, &scan_bytes, H.d_cnt.as<uint64_t>(), H.d_off.as<uint64_t>(), A.ns + 1, s), "size dist blame scan");
  HIP_TRY(H.d_scan.ensure(scan_bytes), "alloc dist blame scan");
  if ((rc = dist_buffers(e, P, A, in_bytes, false))) return rc;
  // (no send region is rewritten within the call: a level has regions of its own)
  if (P.n_dsend) HIP_TRY(hipMemsetAsync(H.d_dsend.p, 0, P.n_dsend * 8, s), "clear dist blame pairs");

  const DrainArgs a = drain_args(e, D.tab);
  DistBlameArgs g{};
  if ((rc = dist_front(e, P, A, in_bytes, n, kReportDown, a, tm, ms[0], &g.d))) return rc;
  const uint8_t* const din = H.d_in.as<uint8_t>();
  g.cut_peer = H.d_cut.as<uint32_t>();
  g.cut_hop = g.cut_peer + std::max<size_t>(P.n_words, 1);
  g.fill = reinterpret_cast<const DistApply*>(din + P.o_fill);
  g.down_send = H.d_dsend.as<uint2>();
  g.down_recv = H.d_drecv.as<uint2>();
  g.down_base = reinterpret_cast<const uint32_t*>(din + P.o_dbase);
  g.n_down_send = static_cast<uint32_t>(P.n_dsend);
  g.n_down_recv = static_cast<uint32_t>(P.n_drecv);
  g.n_rec = H.d_cnt.as<uint64_t>();
  g.off = H.d_off.as<uint64_t>();
  g.rec_off = H.d_rec_off.as<uint64_t>();
  g.cap = cap;
  uint32_t** const recs[5] = {&g.rec_peer, &g.rec_cut_peer, &g.rec_hop, &g.rec_cut_hop, &g.rec_missed};
  for (size_t i = 0, j = 0; i < 5; ++i)
    if (outs[i]) *recs[i] = reinterpret_cast<uint32_t*>(H.d_rec.as<uint8_t>() + j++ * d_stride);
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_dist_nodes(a, g.d, s), "k_dist_nodes");  // (the k word alone: k_dist_nodes<false, false, true>)
  HIP_TRY(tm.end(ms[1]), "event");

  // top-down: ahead of level L's launch its parents' pairs to the children's
  // ranks, where some edge into the level crosses ranks
  uint64_t exchanges = 0, bytes_sent = 0;
  const uint64_t slot_bytes = (P.n_dsend + P.n_drecv) * 8;
  HIP_TRY(tm.begin(), "event");
  size_t x = 0;
  for (uint32_t L = 1; L <= P.max_depth; ++L) {
    if (x < P.downs.size() && P.downs[x].level == L) {
      const Xchg& X = P.downs[x++];
      HIP_TRY(launch_dist_blame_fill(g, X.a0, X.a1, s), "k_dist_blame_fill");
      std::string xerr;
      const hipError_t xe = e->transport->exchange(H.d_dsend.as<uint8_t>(), X.s_off, X.s_len, H.d_drecv.as<uint8_t>(), X.r_off,
                                                   X.r_len, s, &xerr);
      if (xe != hipSuccess) return e->fail(PS_E_DEVICE, xerr);
      exchanges += 1;
      for (const uint64_t b : X.s_len) bytes_sent += b;
    }
    // (the sweep's work list holds the deepest level first)
    const size_t j = P.max_depth - L;
    if (j + 1 < P.launch.size()) HIP_TRY(launch_dist_blame_level(g, L, P.launch[j], P.launch[j + 1], s), "k_dist_blame_level");
  }
  HIP_TRY(tm.end(ms[2]), "event");

  // the records; the one wait before the copies is local, and behind every
  // exchange of the call
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_dist_blame_count(g, s), "k_dist_blame_count");
  scan_bytes = H.d_scan.bytes;
  HIP_TRY(drain_scan(H.d_scan.p, &scan_bytes, g.n_rec, H.d_off.as<uint64_t>(), A.ns + 1, s), "dist blame scan");
  HIP_TRY(tm.end(ms[3]), "event");
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_dist_blame_emit(g, s), "k_dist_blame_emit");
  HIP_TRY(tm.end(ms[4]), "event");
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(hipMemcpyAsync(h_off, g.rec_off, (n + 1) * 8, hipMemcpyDeviceToHost, s), "read dist blame offsets");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  const uint64_t total = h_off[n];
  if (total > cap) return e->fail(PS_E_STATE, "ps_dist_blame: more records than nodes");
  const size_t h_stride = align256(total * 4);
  HIP_TRY(pinned_ensure(&H.h_rec, nullptr, &H.rec_cap, std::max<size_t>(asked * h_stride, 1)), "alloc dist blame view");
  // one copy per array asked for
  for (size_t i = 0, j = 0; i < 5 && total; ++i)
    if (outs[i]) {
      HIP_TRY(hipMemcpyAsync(H.h_rec + j * h_stride, *recs[i], total * 4, hipMemcpyDeviceToHost, s), "read dist blame records");
      ++j;
    }
  HIP_TRY(hipStreamSynchronize(s), "sync");
  HIP_TRY(tm.end(ms[5]), "event");
  *rec_off_out = h_off;
  for (size_t i = 0, j = 0; i < 5; ++i)
    if (outs[i]) *outs[i] = reinterpret_cast<const uint32_t*>(H.h_rec + j++ * h_stride);
  *total_out = total;
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd dist_blame: rank %d topics %zu strips %u nodes %llu work %zu launches %u exchanges %llu sent_bytes %llu "
                 "slot_bytes %llu records %llu copied_bytes %llu classify_ms %.4f nodes_ms %.4f sweep_ms %.4f count_scan_ms %.4f "
                 "emit_ms %.4f copy_ms %.4f host_plan_ms %.4f\n",
                 e->rank, n, A.ns, static_cast<unsigned long long>(P.n_words), P.work.size(), P.max_depth,
                 static_cast<unsigned long long>(exchanges), static_cast<unsigned long long>(bytes_sent),
                 static_cast<unsigned long long>(slot_bytes), static_cast<unsigned long long>(total),
                 static_cast<unsigned long long>((n + 1) * 8 + asked * total * 4), ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], host_ms);
  return PS_OK;
}

}  // extern "C"
