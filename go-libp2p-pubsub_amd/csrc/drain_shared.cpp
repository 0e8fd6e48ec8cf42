// drain_shared.cpp -- the drain with equal lists stored once (drain_impl.hpp;
// DESIGN.md §5.5c, §5.5d): ps_drain_shared, ps_drain_shared_begin / _end, the
// sort of the queries both run first, the shared-list pass of the
// asynchronous form (the sink runs it per window) and the list tail of the
// synchronous one (ps_drain_topics runs it too).
#include "drain_impl.hpp"

using namespace psamd;

namespace {

// The shared calls' queries sorted for the classify pass.  queries[q] =
// (topic, node) of every query; Sort::verdict[q] = 0 for a query the classify
// pass decides (a row of a mask-layout topic), else kOnHost | the verdict:
// nothing for a query without a row, any | missing -- a private list -- for a
// row of an arrival-order (kDrainGather) topic.  The classified queries,
// sorted by topic (a counting sort: a topic's rows have one width), go to
// Sort::cqueries, one bin per topic.  The sort is stable: a topic's queries
// keep their order (k_drain_first relies on it).
int drain_shared_sort(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, DrainQuery* queries,
                      SharedSort* R) {
  auto& D = e->drain;
  const uint32_t nt = static_cast<uint32_t>(D.tab.topics.size());
  D.sort.verdict.assign(n, kOnHost);
  std::vector<uint32_t> per_topic(nt + 1, 0);
  std::vector<const uint32_t*> peer_map(nt, nullptr);  // (looked up once per topic, not per query)
  for (size_t q = 0; q < n; ++q) {
    const uint32_t t = topic[q];
    DrainQuery& Q = queries[q];
    Q = DrainQuery{t, 0, 0, 0};
    const uint32_t u = drain_node(e, t, peer[q], peer_map[t]);
    if (u == kNone) continue;
    Q.node = u;
    ++R->n_rows;
    R->row_ids += e->last_cnt[t];
    R->max_segs = std::max(R->max_segs, ceil_div(D.tab.topics[t].n_pos, kDrainSegBits));
    if (D.tab.topics[t].flags & kDrainGather) {
      D.sort.verdict[q] = kOnHost | kDrainRowAny | kDrainRowMissing;
      ++R->n_gather;
      R->gather_ids += e->last_cnt[t];
    } else {
      D.sort.verdict[q] = 0;
      ++per_topic[t + 1];
    }
  }
  uint64_t n_waves64 = 0;
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t n_q = per_topic[t + 1];
    per_topic[t + 1] += per_topic[t];
    if (!n_q) continue;
    DrainClassBin B{};
    B.topic = t;
    B.q0 = per_topic[t];
    B.n_q = n_q;
    B.wave0 = static_cast<uint32_t>(n_waves64);
    B.words = D.tab.topics[t].n_pos / 64;
    uint64_t steps = 0;  // of 64 lanes; a wave runs kDrainClassPer of them
    if (B.words <= 64) {
      while ((1u << B.lanes_log2) < B.words) ++B.lanes_log2;
      steps = ((static_cast<uint64_t>(n_q) << B.lanes_log2) + 63) / 64;
    } else {
      B.waves = ceil_div(B.words, 64u);
      steps = static_cast<uint64_t>(n_q) * B.waves;
    }
    n_waves64 += (steps + kDrainClassPer - 1) / kDrainClassPer;
    if (n_waves64 * kDrainClassPer >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
    R->bins.push_back(B);
    R->bin_ids += e->last_cnt[t];
  }
  R->n_waves = static_cast<uint32_t>(n_waves64);
  R->n_class = per_topic[nt];
  D.sort.cqueries.resize(R->n_class);
  for (size_t q = 0; q < n; ++q)
    if (D.sort.verdict[q] == 0)
      D.sort.cqueries[per_topic[queries[q].topic]++] = DrainClassQuery{queries[q].node, static_cast<uint32_t>(q)};
  return PS_OK;
}

}  // namespace

namespace psamd {

// ---- the shared-list pass: ps_drain_shared_begin's, and the sink's per window ----

// The block filled at c (L.tail bytes): drain_shared_sort's queries, the
// verdicts the passes start from (0 where the classify pass decides), the
// sorted queries and the bins.  No std::vector is a copy's source afterwards.
int shared_stage(ps_engine* e, const uint32_t* topic, const uint32_t* peer, const SharedLayout& L, uint8_t* c,
                 SharedSort* R) {
  auto& D = e->drain;
  if (const int rc = drain_shared_sort(e, topic, peer, L.n, reinterpret_cast<DrainQuery*>(c), R)) return rc;
  uint32_t* const hv = reinterpret_cast<uint32_t*>(c + L.o_v);
  for (size_t q = 0; q < L.n; ++q) hv[q] = D.sort.verdict[q] & ~kOnHost;
  if (R->n_class) std::memcpy(c + L.o_cq, D.sort.cqueries.data(), static_cast<size_t>(R->n_class) * sizeof(DrainClassQuery));
  if (!R->bins.empty()) std::memcpy(c + L.o_bins, R->bins.data(), R->bins.size() * sizeof(DrainClassBin));
  return PS_OK;
}

// One window's caps and segment bound.  `own`: the engine's caps (the size of
// the answer while full rows share) replace the caller's.  False: more rows
// than the kernels index (the numbering scan keeps the segments in the low
// half of its key).
bool shared_caps(const Drain& D, const SharedSort& R, size_t n, bool own, size_t* list_cap, size_t* id_cap,
                 uint32_t* seg_bound) {
  if (own) {
    *list_cap = D.env.share ? R.bins.size() + R.n_gather : R.n_rows;
    *id_cap = D.env.share ? R.bin_ids + R.gather_ids : R.row_ids;
  }
  const uint64_t bound = static_cast<uint64_t>(*list_cap) * R.max_segs;
  *seg_bound = static_cast<uint32_t>(bound);
  return bound < kDrainRowLimit && static_cast<uint64_t>(n) * R.max_segs < kDrainRowLimit;
}

// The pass on `stream`, nothing waited for (but a timed phase): the block at
// h uploaded, k_drain_classify over its verdict words, the list assignment
// into at most list_cap lists (list_of_query: n words), then count and scan
// over the lists.  Every buffer and grid is sized by n and the caps -- the
// counts stay in the control block on the device -- and B only grows.
// ms: classify, assign, count; the scan's phase is left open, as
// drain_count_scan leaves it.  *args: queries = the lists (the kernels read
// their number from *ctl); B.scratch.d_off: seg_bound + 1 offsets.
int shared_pass(ps_engine* e, Drain::ListBufs& B, const SharedLayout& L, const uint8_t* h, const SharedSort& R,
                size_t list_cap, uint32_t seg_bound, uint32_t* list_of_query, const PhaseTimer& tm, float* ms,
                DrainArgs* args, DrainCtl** ctl_out) {
  auto& D = e->drain;
  auto& C = B.scratch;
  hipStream_t s = e->stream;
  const size_t n = L.n, n_off = static_cast<size_t>(seg_bound) + 1;
  const size_t o_first = align256(sizeof(DrainCtl));
  HIP_TRY(B.d_in.ensure(L.tail), "alloc drain input");
  HIP_TRY(B.d_key.ensure(2 * n * 8), "alloc drain keys");
  HIP_TRY(B.d_aux.ensure(o_first + L.nt * 4), "alloc drain control");
  HIP_TRY(C.d_queries.ensure(list_cap * sizeof(DrainQuery)), "alloc drain lists");
  HIP_TRY(C.d_cnt.ensure(n_off * 8), "alloc drain counts");
  HIP_TRY(C.d_off.ensure(n_off * 8), "alloc drain offsets");
  uint64_t* const cnt = C.d_cnt.as<uint64_t>();
  uint64_t* const off = C.d_off.as<uint64_t>();
  uint64_t* const key = B.d_key.as<uint64_t>();
  size_t scan_bytes = 0, scan_keys = 0;  // one temporary for both scans
  HIP_TRY(drain_scan(nullptr, &scan_bytes, cnt, off, seg_bound + 1, s), "size drain scan");
  HIP_TRY(drain_scan(nullptr, &scan_keys, key, key + n, static_cast<uint32_t>(n), s), "size drain scan");
  HIP_TRY(C.d_scan.ensure(std::max(scan_bytes, scan_keys)), "alloc drain scan");

  uint8_t* const din = B.d_in.as<uint8_t>();
  uint8_t* const aux = B.d_aux.as<uint8_t>();
  DrainCtl* const ctl = reinterpret_cast<DrainCtl*>(aux);
  HIP_TRY(hipMemcpyAsync(din, h, L.tail, hipMemcpyHostToDevice, s), "upload drain queries");
  HIP_TRY(hipMemsetAsync(aux + o_first, 0xFF, L.nt * 4, s), "preset drain firsts");
  if (const int rc = drain_err_word(e, s)) return rc;

  DrainArgs a = drain_args(e, D.tab);
  uint32_t* const verdict = reinterpret_cast<uint32_t*>(din + L.o_v);
  const DrainClassQuery* const sorted = reinterpret_cast<const DrainClassQuery*>(din + L.o_cq);
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_classify(a, reinterpret_cast<const DrainClassBin*>(din + L.o_bins), static_cast<uint32_t>(R.bins.size()),
                                sorted, R.n_waves, verdict, s),
          "k_drain_classify");
  HIP_TRY(tm.end(ms[0]), "event");
  DrainAssign g{};
  g.topics = D.tab.p_topics;
  g.queries = reinterpret_cast<const DrainQuery*>(din);
  g.verdict = verdict;
  g.sorted = sorted;
  g.n_sorted = R.n_class;
  g.n = static_cast<uint32_t>(n);
  g.share = D.env.share;
  g.first = reinterpret_cast<uint32_t*>(aux + o_first);
  g.key = key;
  g.key_off = key + n;
  g.scan_temp = C.d_scan.p;
  g.scan_bytes = C.d_scan.bytes;
  g.lists = C.d_queries.as<DrainQuery>();
  g.list_cap = static_cast<uint32_t>(list_cap);
  g.seg_bound = seg_bound;
  g.list_of_query = list_of_query;
  g.ctl = ctl;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_assign(g, s), "drain list assignment");
  HIP_TRY(tm.end(ms[1]), "event");
  a.queries = g.lists;
  a.n_queries = 0;  // (the kernels read it from the control block)
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_count_dev(a, ctl, seg_bound, cnt, s), "k_drain_count_dev");
  HIP_TRY(tm.end(ms[2]), "event");
  HIP_TRY(tm.begin(), "event");
  scan_bytes = C.d_scan.bytes;
  HIP_TRY(drain_scan(C.d_scan.p, &scan_bytes, cnt, off, seg_bound + 1, s), "drain scan");
  *args = a;
  *ctl_out = ctl;
  return PS_OK;
}

// ---- the synchronous list tail: ps_drain_shared's, and ps_drain_topics' -------

// The offsets of `lists` (list queries the host numbered, n_segs segments in
// all) into hdr: lists.size() + 1 offsets, the last one the total, and a zero
// (k_drain_offsets copies an error word behind the total: none here, a zero
// behind the header on the device).  Count, scan and k_drain_offsets in
// Sync::scratch, then one wait: `lists` may leave scope and the total sizes
// the ids.  a.queries: the lists on the device, for drain_list_ids.
int drain_list_offsets(ps_engine* e, DrainArgs& a, const std::vector<DrainQuery>& lists, uint32_t n_segs,
                       std::vector<uint64_t>& hdr, const PhaseTimer& tm, float& count_ms, float& scan_ms) {
  auto& Y = e->drain.sync;
  hipStream_t s = e->stream;
  const uint32_t n_lists = static_cast<uint32_t>(lists.size());
  hdr.assign(static_cast<size_t>(n_lists) + 2, 0);
  if (!n_lists) return PS_OK;
  HIP_TRY(Y.d_hdr.ensure((hdr.size() + 1) * 8), "alloc drain header");
  uint32_t* const d_zero = reinterpret_cast<uint32_t*>(Y.d_hdr.as<uint64_t>() + hdr.size());
  HIP_TRY(hipMemsetAsync(d_zero, 0, 8, s), "clear drain error");
  if (const int rc = drain_count_scan(e, a, n_segs, Y.scratch, lists.data(), n_lists, s, tm, count_ms)) return rc;
  HIP_TRY(launch_drain_offsets(a.queries, n_lists, Y.scratch.d_off.as<uint64_t>(), n_segs, d_zero, Y.d_hdr.as<uint64_t>(), s),
          "k_drain_offsets");
  HIP_TRY(tm.end(scan_ms), "event");
  HIP_TRY(hipMemcpyAsync(hdr.data(), Y.d_hdr.p, hdr.size() * 8, hipMemcpyDeviceToHost, s), "read drain offsets");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  return PS_OK;
}

// ... and their `total` ids, emitted into Sync::d_lists and copied to `out`
// (host memory of the caller's), waited for.  Nothing to do for no id.
int drain_list_ids(ps_engine* e, const DrainArgs& a, uint32_t n_segs, uint64_t total, void* out, const PhaseTimer& tm,
                   float& emit_ms, float& copy_ms) {
  auto& D = e->drain;
  auto& Y = D.sync;
  hipStream_t s = e->stream;
  if (!total) return PS_OK;
  HIP_TRY(Y.d_lists.ensure(total * 4), "alloc drain lists");
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_emit(a, 0, n_segs, Y.scratch.d_off.as<uint64_t>(), 0, Y.d_lists.as<uint32_t>(), total, D.env.staged, s),
          "k_drain_emit");
  HIP_TRY(tm.end(emit_ms), "event");
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(hipMemcpyAsync(out, Y.d_lists.p, total * 4, hipMemcpyDeviceToHost, s), "read drain lists");
  HIP_TRY(tm.end(copy_ms), "event");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  return PS_OK;
}

}  // namespace psamd

extern "C" {

// ---- ps_drain_shared ---------------------------------------

// ps_drain's answer with equal lists stored once.  k_drain_classify compares
// every queried row of a mask-layout topic with the topic's message mask:
// no message bit -> PS_NONE, every message bit -> the topic's shared list
// (emitted from the mask itself), anything else -> a list of its own through
// the count / scan / emit passes ps_drain uses.  The queries of arrival-order
// (kDrainGather) topics have no mask to compare with: each takes a private
// list.  Device -> host: 4 B x n verdicts, 8 B x (n_lists + 2) offsets, 4 B x
// total ids.
int ps_drain_shared(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, uint32_t* list_out,
                    uint64_t* list_off_out, size_t list_cap, uint32_t* msg_out, size_t cap, uint32_t* n_lists_out,
                    uint64_t* total_out) {
  if (!e || !list_off_out || !n_lists_out || !total_out || (n && (!topic || !peer || !list_out)) || (cap && !msg_out))
    return PS_E_INVAL;
  if (const int rc0 = drain_enter(e, {"ps_drain_shared on a multi-rank engine: use ps_drain", "no completed run", nullptr, true},
                                 topic, peer, n))
    return rc0;
  *n_lists_out = 0;
  *total_out = 0;
  if (n == 0) {
    list_off_out[0] = 0;
    return PS_OK;
  }
  if (n >= 0x7FFFFFFFull) return e->fail(PS_E_RANGE, "too many queries");
  auto& D = e->drain;
  double host_ms[2] = {0, 0};  // mirrors + tables + bins, list numbering
  auto h0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  float ms[5] = {0, 0, 0, 0, 0};  // classify, count, scan, emit, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  const uint32_t nt = static_cast<uint32_t>(D.tab.topics.size());
  D.sync.queries.resize(n);
  SharedSort R;
  if ((rc = drain_shared_sort(e, topic, peer, n, D.sync.queries.data(), &R))) return rc;
  const std::vector<DrainClassBin>& bins = R.bins;
  const uint32_t n_waves = R.n_waves, n_class = R.n_class;
  host_ms[0] = ms_since(h0);

  DrainArgs a = drain_args(e, D.tab);
  if (n_class) {
    std::vector<uint32_t> got(n);
    HIP_TRY(D.sync.d_cbins.ensure(bins.size() * sizeof(DrainClassBin)), "alloc drain bins");
    HIP_TRY(D.sync.d_cqueries.ensure(static_cast<size_t>(n_class) * sizeof(DrainClassQuery)), "alloc drain queries");
    HIP_TRY(D.sync.d_verdict.ensure(n * 4), "alloc drain verdicts");
    HIP_TRY(hipMemcpyAsync(D.sync.d_cbins.p, bins.data(), bins.size() * sizeof(DrainClassBin), hipMemcpyHostToDevice, s),
            "upload drain bins");
    HIP_TRY(hipMemcpyAsync(D.sync.d_cqueries.p, D.sort.cqueries.data(), static_cast<size_t>(n_class) * sizeof(DrainClassQuery),
                           hipMemcpyHostToDevice, s),
            "upload drain queries");
    HIP_TRY(hipMemsetAsync(D.sync.d_verdict.p, 0, n * 4, s), "clear drain verdicts");
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_drain_classify(a, D.sync.d_cbins.as<DrainClassBin>(), static_cast<uint32_t>(bins.size()),
                                  D.sync.d_cqueries.as<DrainClassQuery>(), n_waves, D.sync.d_verdict.as<uint32_t>(), s),
            "k_drain_classify");
    HIP_TRY(tm.end(ms[0]), "event");
    HIP_TRY(hipMemcpyAsync(got.data(), D.sync.d_verdict.p, n * 4, hipMemcpyDeviceToHost, s), "read drain verdicts");
    HIP_TRY(hipStreamSynchronize(s), "sync");  // (bins leaves scope; the verdicts number the lists)
    for (size_t q = 0; q < n; ++q)
      if (D.sort.verdict[q] == 0) D.sort.verdict[q] = got[q];
  }

  // lists, numbered by first use: one per topic with a full query, one per other query
  h0 = hclock::now();
  std::vector<uint32_t> topic_list(nt, PS_NONE);
  std::vector<DrainQuery> lists;
  uint64_t n_segs64 = 0;
  for (size_t q = 0; q < n; ++q) {
    const uint32_t v = D.sort.verdict[q], t = topic[q];
    if (!(v & kDrainRowAny)) {
      list_out[q] = PS_NONE;
      continue;
    }
    const bool full = !(v & kDrainRowMissing) && D.env.share;
    if (full && topic_list[t] != PS_NONE) {
      list_out[q] = topic_list[t];
      continue;
    }
    list_out[q] = static_cast<uint32_t>(lists.size());
    if (full) topic_list[t] = list_out[q];
    lists.push_back(DrainQuery{t, full ? kDrainMaskRow : D.sync.queries[q].node, static_cast<uint32_t>(n_segs64), 0});
    n_segs64 += ceil_div(D.tab.topics[t].n_pos, kDrainSegBits);
    if (n_segs64 >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  }
  const uint32_t n_lists = static_cast<uint32_t>(lists.size());
  const uint32_t n_segs = static_cast<uint32_t>(n_segs64);
  host_ms[1] = ms_since(h0);
  *n_lists_out = n_lists;
  if ((rc = drain_list_offsets(e, a, lists, n_segs, D.sync.hdr, tm, ms[1], ms[2]))) return rc;
  const uint64_t total = D.sync.hdr[n_lists];
  *total_out = total;
  if (list_cap >= n_lists) std::memcpy(list_off_out, D.sync.hdr.data(), (static_cast<size_t>(n_lists) + 1) * 8);
  if (list_cap < n_lists || total > cap) return e->fail(PS_E_RANGE, "output buffer too small");
  if ((rc = drain_list_ids(e, a, n_segs, total, msg_out, tm, ms[3], ms[4]))) return rc;
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd drain_shared: queries %zu classified %u waves %u lists %u segments %u ids %llu classify_ms %.4f "
                 "count_ms %.4f scan_ms %.4f emit_ms %.4f copy_ms %.4f host_queries_ms %.4f host_lists_ms %.4f\n",
                 n, n_class, n_waves, n_lists, n_segs, static_cast<unsigned long long>(total), ms[0], ms[1], ms[2], ms[3],
                 ms[4], host_ms[0], host_ms[1]);
  return PS_OK;
}

// ---- ps_drain_shared_begin / ps_drain_shared_end -----------

// ps_drain_shared's answer enqueued behind the last run, with no host wait:
// tables (device build), classify, the list assignment (what the host loop of
// ps_drain_shared does between its waits: k_drain_first / _keys / scan /
// _lists), then count / scan / offsets / emit over the lists with the counts
// read from the slot's control block, all on `stream`; the view (header,
// list_off, list_of_query, ids) leaves in one copy on the copy stream.  The
// host knows only the caps: every buffer and grid is sized by them.
int ps_drain_shared_begin(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, size_t list_cap,
                          size_t id_cap) {
  if (!e || (n && (!topic || !peer))) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_drain_shared_begin on a multi-rank engine: use ps_drain", "no run enqueued",
                                    "two drains outstanding: end one first", false},
                                topic, peer, n))
    return rc;
  if (n >= 0x7FFFFFFFull || list_cap >= 0x7FFFFFFFull) return e->fail(PS_E_RANGE, "too many queries or lists");
  auto& D = e->drain;
  const auto t_host0 = hclock::now();
  const uint32_t nt = static_cast<uint32_t>(e->topics.size());

  // staged in the slot's pinned input, behind the table block where one is
  // built.  From here to the slot's taking a failure gives the slot up.
  const SharedLayout L(n, nt);
  Drain::Slot* slot = nullptr;
  size_t used = 0;
  uint8_t* h = nullptr;
  int rc = drain_begin_slot(e, L.tail, D.env.timing, &slot, &used, &h);
  if (rc) return rc;
  auto& S = *slot;
  hipStream_t s = e->stream;
  SharedSort R;
  if (shared_stage(e, topic, peer, L, h, &R)) return drain_give_up(e, used, PS_E_RANGE, "too many rows in one drain");

  // the caps: the engine's or the caller's
  uint32_t seg_bound = 0;
  const bool rows_fit = shared_caps(D, R, n, list_cap == 0 && id_cap == 0, &list_cap, &id_cap, &seg_bound);
  if (id_cap > kDrainAsyncMaxIds) return drain_give_up(e, used, PS_E_RANGE, "drain may exceed 2^30 ids: use ps_drain_shared");
  if (!rows_fit) return drain_give_up(e, used, PS_E_RANGE, "too many rows in one drain");

  S.n = n;
  S.kind = Drain::Slot::kShared;
  S.list_cap = list_cap;
  S.id_cap = id_cap;
  S.o_off = align256(sizeof(DrainSharedHdr));
  S.o_lq = S.o_off + align256((list_cap + 1) * 8);
  S.o_ids = S.o_lq + align256(n * 4);
  const size_t res_bytes = S.o_ids + id_cap * 4;
  HIP_TRY(pinned_ensure(&S.h_res, &S.h_res_dev, &S.res_cap, res_bytes), "alloc drain view");
  S.enqueued = false;
  if (R.n_rows == 0) {  // no row to read: no list, written here
    std::memset(S.h_res, 0, S.o_off + 8);
    std::memset(S.h_res + S.o_lq, 0xFF, n * 4);
    return drain_slot_host_view(e, S, used);
  }

  // (PSAMD_DRAIN_TIMING: the phases run apart and are waited for; else nothing here waits)
  float ms[5] = {0, 0, 0, 0, 0};  // classify, assign, count, scan + offsets, emit
  const PhaseTimer tm{D.ev_t, s, D.env.timing};
  HIP_TRY(S.d_res.ensure(res_bytes), "alloc drain result");
  uint8_t* const res = S.d_res.as<uint8_t>();
  DrainArgs a{};
  DrainCtl* ctl = nullptr;
  if ((rc = shared_pass(e, S.lb, L, h, R, list_cap, seg_bound, reinterpret_cast<uint32_t*>(res + S.o_lq), tm, ms, &a, &ctl)))
    return rc;
  const uint64_t* const seg_off = S.lb.scratch.d_off.as<uint64_t>();
  HIP_TRY(launch_drain_offsets_dev(a.queries, ctl, static_cast<uint32_t>(list_cap), seg_off, id_cap, D.tab.d_err,
                                   reinterpret_cast<DrainSharedHdr*>(res), reinterpret_cast<uint64_t*>(res + S.o_off), s),
          "k_drain_offsets_dev");
  HIP_TRY(tm.end(ms[3]), "event");
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_emit_dev(a, ctl, seg_bound, seg_off, reinterpret_cast<uint32_t*>(res + S.o_ids), id_cap, s),
          "k_drain_emit_dev");
  HIP_TRY(tm.end(ms[4]), "event");
  // classify reads every queried row, count and emit the private ones: the
  // event behind the emit covers them all, with or without a segment
  if ((rc = drain_slot_enqueued(e, S, res_bytes, true))) return rc;
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd drain_shared_begin: queries %zu classified %u waves %u list_cap %zu id_cap %zu seg_bound %u tables %s "
                 "classify_ms %.4f assign_ms %.4f count_ms %.4f scan_ms %.4f emit_ms %.4f view_bytes %zu host_us %.1f\n",
                 n, R.n_class, R.n_waves, list_cap, id_cap, seg_bound, used ? "built" : "kept", ms[0], ms[1], ms[2], ms[3],
                 ms[4], res_bytes, 1e3 * ms_since(t_host0));
  return PS_OK;
}

int ps_drain_shared_end(ps_engine* e, const uint32_t** list_out, const uint64_t** list_off_out, const uint32_t** msg_out,
                        uint32_t* n_lists_out, uint64_t* total_out) {
  if (!e || !list_out || !list_off_out || !msg_out || !n_lists_out || !total_out) return PS_E_INVAL;
  auto& D = e->drain;
  if (D.slot_count == 0) return e->fail(PS_E_NOTREADY, "no drain outstanding");
  auto& S = D.slot[D.slot_head];
  if (S.kind != Drain::Slot::kShared)
    return e->fail(PS_E_STATE, S.kind == Drain::Slot::kPlain ? "the oldest drain is not a shared one: ps_drain_end"
                                                              : "the oldest drain is a topics one: ps_drain_topics_end");
  if (const int rc = drain_slot_complete(e, S)) return rc;
  const DrainSharedHdr* hdr = reinterpret_cast<const DrainSharedHdr*>(S.h_res);
  *list_out = reinterpret_cast<const uint32_t*>(S.h_res + S.o_lq);
  *list_off_out = reinterpret_cast<const uint64_t*>(S.h_res + S.o_off);
  *msg_out = reinterpret_cast<const uint32_t*>(S.h_res + S.o_ids);
  *n_lists_out = hdr->n_lists;
  *total_out = hdr->total;
  return drain_view_status(e, hdr->err, hdr->over);
}

}  // extern "C"
