// drain_topics.cpp -- ps_drain_topics (drain_impl.hpp): each
// named topic's audience as one shared list plus exceptions.  Its lists go
// through the synchronous list tail of drain_shared.cpp.  And
// ps_drain_topics_begin / _end (§5.5g): the same answer enqueued behind a
// running batch, the totals and the list numbering on the device.
#include "drain_impl.hpp"

using namespace psamd;

// nodes one strip holds of rows `words` mask words wide (kernels.hpp,
// AudStrip): a row counted at the lanes it takes in a load, one for the rows
// of an arrival-order topic, which are not read
uint32_t psamd::aud_strip_nodes(bool gather, uint32_t words) {
  uint32_t lanes = 1;
  if (!gather) {
    while (lanes < words && lanes < 64) lanes *= 2;
    lanes = std::max(lanes, words);
  }
  return std::max(1u, kAudStripBytes / (lanes * 8));
}

// ---- what the topics calls share ------------------------------------------------

int psamd::aud_check_topics(ps_engine* e, const uint32_t* topic, size_t n) {
  const uint32_t nt = static_cast<uint32_t>(e->topics.size());
  for (size_t i = 0; i < n; ++i)
    if (topic[i] >= nt) return e->fail(PS_E_RANGE, "topic out of range");
  std::vector<uint8_t> named(nt, 0);
  for (size_t i = 0; i < n; ++i)
    if (named[topic[i]]++) return e->fail(PS_E_INVAL, "a topic named twice");
  return PS_OK;
}

uint32_t psamd::aud_nodes(const ps_engine* e, uint32_t t, uint32_t* u0) {
  const TopicDev& d = e->last_topics[t];
  *u0 = (d.flags & kTopicRootLocal) ? 1 : 0;
  return d.n_nodes > *u0 ? d.n_nodes - *u0 : 0;
}

// ---- the audience pass (ps_drain_topics_begin, the audience sink) ---------------

// The strips at most, before the tables stand (a staging is taken once, with
// them): a topic's rows counted at the mask words its highest window bit
// gives, as both table builds lay a mask out; an arrival-order topic's strips
// are longer, so it takes fewer.
size_t psamd::aud_stage_bytes(ps_engine* e, const uint32_t* topic, size_t n, size_t* o_strips, uint64_t* strips_max) {
  uint64_t most = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = topic[i], cnt = e->last_cnt[t];
    const TopicDev& d = e->last_topics[t];
    uint32_t u0 = 0;
    const uint32_t nn = aud_nodes(e, t, &u0);
    if (!d.W || !cnt || !nn) continue;
    const uint32_t* bits = window_bits(e, t);
    const uint32_t top = bits ? *std::max_element(bits, bits + cnt) : cnt - 1;
    const uint32_t per = aud_strip_nodes(false, std::min<uint32_t>(top >> 6, d.W - 1) + 1);
    most += ceil_div(nn, per);
  }
  *strips_max = most;
  *o_strips = align256((n + 1) * sizeof(AudEntry));
  return *o_strips + most * sizeof(AudStrip);
}

bool psamd::aud_stage(ps_engine* e, const uint32_t* topic, size_t n, AudEntry* entries, AudStrip* strips,
                      uint64_t strips_max, AudShape* out) {
  const auto& D = e->drain;
  AudShape A;
  uint64_t ns64 = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = topic[i];
    const DrainTopic& T = D.tab.topics[t];
    uint32_t u0 = 0;
    const uint32_t nn = aud_nodes(e, t, &u0);
    const uint32_t segs = ceil_div(T.n_pos, kDrainSegBits);
    if (entries) entries[i] = AudEntry{t, static_cast<uint32_t>(ns64), segs, 0};
    if (!T.n_pos || !nn) continue;
    const bool gather = T.flags & kDrainGather;
    if (!gather) A.row_bytes += static_cast<uint64_t>(nn) * (T.n_pos / 64) * 8;
    const uint32_t per = aud_strip_nodes(gather, T.n_pos / 64);
    if (ns64 + ceil_div(nn, per) > strips_max) return false;
    if (!strips) {
      ns64 += ceil_div(nn, per);
      A.n_verdicts += nn;
    }
    for (uint32_t k = 0; strips && k < nn; k += per) {
      const uint32_t c = std::min(per, nn - k);
      strips[ns64++] = AudStrip{t, u0 + k, c, e->last_topics[t].nbase, A.n_verdicts};
      A.n_verdicts += c;
    }
    A.max_segs = std::max(A.max_segs, segs);
    // the topic's shared list and a private one per node of an arrival-order
    // topic; every node's where full rows do not share
    const uint64_t lists = D.env.share ? 1 + (gather ? nn : 0) : nn;
    A.own_lists += lists;
    A.own_ids += lists * e->last_cnt[t];
  }
  A.ns = static_cast<uint32_t>(ns64);
  if (entries) entries[n] = AudEntry{0, A.ns, 0, 0};
  A.own_exc = std::max<uint64_t>(std::min<uint64_t>(A.n_verdicts, kAudPrefix), 1);
  A.own_lists = std::max<uint64_t>(A.own_lists, 1);
  *out = A;
  return true;
}

bool psamd::aud_caps(const AudShape& A, size_t n, size_t* exc_cap, size_t* list_cap, size_t* id_cap, uint32_t* seg_bound) {
  if (!*exc_cap) *exc_cap = A.own_exc;
  if (!*list_cap) *list_cap = A.own_lists;
  if (!*id_cap) *id_cap = A.own_ids;
  const uint64_t bound = static_cast<uint64_t>(*list_cap) * A.max_segs;
  // (the numbering scans keep the segments in the low half of their keys)
  if (*list_cap >= 0x7FFFFFFFull || *exc_cap >= 0x7FFFFFFFull || bound >= kDrainRowLimit ||
      (static_cast<uint64_t>(*exc_cap) + n) * A.max_segs >= kDrainRowLimit)
    return false;
  *seg_bound = static_cast<uint32_t>(bound);
  return true;
}

int psamd::aud_pass(ps_engine* e, const AudBufs& B, const AudEntry* d_entries, const AudStrip* d_strips, size_t n,
                    const AudShape& A, size_t exc_cap, size_t list_cap, uint32_t seg_bound, const AudView& view,
                    const PhaseTimer& tm, float* ms, DrainArgs* args, DrainCtl** ctl_out) {
  auto& D = e->drain;
  hipStream_t s = e->stream;
  auto& C = B.lb->scratch;
  const uint32_t ns = A.ns;
  const uint64_t n_verdicts = A.n_verdicts;
  const size_t o_node = align256(n_verdicts * 4), o_v = 2 * o_node;
  const size_t n_off = static_cast<size_t>(seg_bound) + 1;
  HIP_TRY(B.lb->d_key.ensure(2 * (n + 1 + exc_cap + 1) * 8), "alloc drain keys");
  HIP_TRY(B.lb->d_aux.ensure(align256(sizeof(DrainCtl))), "alloc drain control");
  HIP_TRY(B.d_verdict->ensure(n_verdicts), "alloc audience verdicts");
  HIP_TRY(B.d_exc->ensure(2 * (static_cast<size_t>(ns) + 1) * 8), "alloc audience counts");
  HIP_TRY(B.d_full->ensure(static_cast<size_t>(ns) * 4), "alloc audience counts");
  HIP_TRY(B.d_rec->ensure(o_v + n_verdicts), "alloc audience records");
  HIP_TRY(C.d_queries.ensure(list_cap * sizeof(DrainQuery)), "alloc drain lists");
  HIP_TRY(C.d_cnt.ensure(n_off * 8), "alloc drain counts");
  HIP_TRY(C.d_off.ensure(n_off * 8), "alloc drain offsets");
  uint64_t* const strip_cnt = B.d_exc->as<uint64_t>();
  uint64_t* const strip_off = strip_cnt + ns + 1;
  uint64_t* const ekey = B.lb->d_key.as<uint64_t>();
  uint64_t* const rkey = ekey + 2 * (n + 1);
  uint64_t* const cnt = C.d_cnt.as<uint64_t>();
  uint64_t* const off = C.d_off.as<uint64_t>();
  size_t scan_bytes = 0;  // one temporary for the four scans
  for (const uint32_t len : {ns + 1, static_cast<uint32_t>(exc_cap) + 1, static_cast<uint32_t>(n) + 1, seg_bound + 1}) {
    size_t b = 0;
    HIP_TRY(drain_scan(nullptr, &b, cnt, off, len, s), "size drain scan");
    scan_bytes = std::max(scan_bytes, b);
  }
  HIP_TRY(C.d_scan.ensure(scan_bytes), "alloc drain scan");

  uint8_t* const rec = B.d_rec->as<uint8_t>();
  DrainCtl* const ctl = B.lb->d_aux.as<DrainCtl>();
  DrainArgs a = drain_args(e, D.tab);
  AudArgs g{};
  g.strips = d_strips;
  g.n_strips = ns;
  g.share = D.env.share;
  g.verdict = B.d_verdict->as<uint8_t>();
  g.n_exc = strip_cnt;
  g.n_full = B.d_full->as<uint32_t>();
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_audience_classify(a, g, s), "k_audience_classify");
  HIP_TRY(tm.end(ms[0]), "event");
  HIP_TRY(tm.begin(), "event");
  size_t sb = C.d_scan.bytes;
  HIP_TRY(drain_scan(C.d_scan.p, &sb, strip_cnt, strip_off, ns + 1, s), "drain scan");
  HIP_TRY(tm.end(ms[1]), "event");
  AudEmit o{};
  o.node_peer = e->d_node_peer.as<uint32_t>();
  o.off = strip_off;
  o.peer = reinterpret_cast<uint32_t*>(rec);
  o.node = reinterpret_cast<uint32_t*>(rec + o_node);
  o.verdict = rec + o_v;
  o.cap = n_verdicts;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_audience_emit(g, o, s), "k_audience_emit");
  HIP_TRY(tm.end(ms[2]), "event");

  AudAssign q{};
  q.entries = d_entries;
  q.n = static_cast<uint32_t>(n);
  q.n_strips = ns;
  q.strip_full = g.n_full;
  q.strip_off = strip_off;
  q.rec_peer = o.peer;
  q.rec_node = o.node;
  q.rec_verdict = o.verdict;
  q.exc_cap = static_cast<uint32_t>(exc_cap);
  q.list_cap = static_cast<uint32_t>(list_cap);
  q.seg_bound = seg_bound;
  q.ekey = ekey;
  q.ekey_off = ekey + n + 1;
  q.rkey = rkey;
  q.rkey_off = rkey + exc_cap + 1;
  q.scan_temp = C.d_scan.p;
  q.scan_bytes = C.d_scan.bytes;
  q.topic_list = view.topic_list;
  q.n_full = view.n_full;
  q.exc_off = view.exc_off;
  q.exc_peer = view.exc_peer;
  q.exc_list = view.exc_list;
  q.lists = C.d_queries.as<DrainQuery>();
  q.ctl = ctl;
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_audience_assign(q, s), "audience list assignment");
  HIP_TRY(tm.end(ms[3]), "event");
  a.queries = q.lists;
  a.n_queries = 0;  // (the kernels read it from the control block)
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_count_dev(a, ctl, seg_bound, cnt, s), "k_drain_count_dev");
  HIP_TRY(tm.end(ms[4]), "event");
  HIP_TRY(tm.begin(), "event");
  sb = C.d_scan.bytes;
  HIP_TRY(drain_scan(C.d_scan.p, &sb, cnt, off, seg_bound + 1, s), "drain scan");
  HIP_TRY(tm.end(ms[5]), "event");
  *args = a;
  *ctl_out = ctl;
  return PS_OK;
}

extern "C" {

// ---- ps_drain_topics ----------------------------------------

// ps_drain_shared's answer for every non-root node of the named topics, with
// no query per subscriber: the host cuts each topic's node range into strips,
// k_audience_classify streams the strips' rows into one verdict byte per node
// and two counts per strip, a scan of the counts places the nodes that are
// not full, and k_audience_emit writes those (peer, node, verdict) in node
// order.  One wait brings the counts and the first kAudPrefix records; the
// lists -- a topic's shared one where a row is full, a private one per "any"
// exception -- then go through the count / scan / emit passes unchanged.
int ps_drain_topics(ps_engine* e, const uint32_t* topic, size_t n, const uint32_t** topic_list_out,
                    const uint64_t** n_nodes_out, const uint64_t** n_full_out, const uint64_t** exc_off_out,
                    const uint32_t** exc_peer_out, const uint32_t** exc_list_out, const uint64_t** list_off_out,
                    const uint32_t** msg_out, uint32_t* n_lists_out, uint64_t* total_out) {
  if (!e || !topic_list_out || !n_nodes_out || !n_full_out || !exc_off_out || !exc_peer_out || !exc_list_out ||
      !list_off_out || !msg_out || !n_lists_out || !total_out || (n && !topic))
    return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_drain_topics on a multi-rank engine: use ps_drain", "no completed run", nullptr, true}))
    return rc;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  auto& D = e->drain;
  auto& A = D.aud;
  double host_ms[2] = {0, 0};  // mirrors + tables + strips, lists
  auto h0 = hclock::now();
  int rc = drain_ready(e);
  if (!rc) rc = drain_tables(e);
  if (rc) return rc;
  hipStream_t s = e->stream;
  float ms[5] = {0, 0, 0, 0, 0};  // classify, scan, emit, lists (count, scan, emit), copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};

  // the strips: each topic's non-root nodes, in request order
  A.strips.clear();
  A.n_nodes.assign(std::max<size_t>(n, 1), 0);
  A.n_full.assign(std::max<size_t>(n, 1), 0);
  A.topic_list.assign(std::max<size_t>(n, 1), PS_NONE);
  A.exc_off.assign(n + 1, 0);
  std::vector<uint64_t> strip0(n + 1, 0);  // entry i's first strip
  uint64_t n_verdicts = 0, row_bytes = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = topic[i];
    const TopicDev& d = e->last_topics[t];
    uint32_t u0 = 0;
    const uint32_t nn = aud_nodes(e, t, &u0);
    A.n_nodes[i] = nn;
    strip0[i] = A.strips.size();
    const DrainTopic& T = D.tab.topics[t];
    if (!T.n_pos || !nn) continue;
    if (!(T.flags & kDrainGather)) row_bytes += static_cast<uint64_t>(nn) * (T.n_pos / 64) * 8;
    const uint32_t per = aud_strip_nodes(T.flags & kDrainGather, T.n_pos / 64);
    for (uint32_t k = 0; k < nn; k += per) {
      const uint32_t c = std::min(per, nn - k);
      A.strips.push_back(AudStrip{t, u0 + k, c, d.nbase, n_verdicts});
      n_verdicts += c;
    }
    if (A.strips.size() >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  }
  strip0[n] = A.strips.size();
  const uint32_t ns = static_cast<uint32_t>(A.strips.size());
  host_ms[0] = ms_since(h0);

  // classify, scan, emit; the counts and the first records in one wait
  const size_t o_node = align256(n_verdicts * 4), o_v = 2 * o_node;
  A.strip_off.assign(static_cast<size_t>(ns) + 1, 0);
  A.strip_full.assign(std::max<uint32_t>(ns, 1), 0);
  uint64_t n_exc = 0;
  if (ns) {
    HIP_TRY(A.d_strips.ensure(static_cast<size_t>(ns) * sizeof(AudStrip)), "alloc audience strips");
    HIP_TRY(A.d_verdict.ensure(n_verdicts), "alloc audience verdicts");
    HIP_TRY(A.d_exc.ensure(2 * (static_cast<size_t>(ns) + 1) * 8), "alloc audience counts");
    HIP_TRY(A.d_full.ensure(static_cast<size_t>(ns) * 4), "alloc audience counts");
    HIP_TRY(A.d_rec.ensure(o_v + n_verdicts), "alloc audience records");
    uint64_t* const cnt = A.d_exc.as<uint64_t>();
    uint64_t* const off = cnt + ns + 1;
    size_t scan_bytes = 0;
    HIP_TRY(drain_scan(nullptr, &scan_bytes, cnt, off, ns + 1, s), "size drain scan");
    HIP_TRY(D.sync.scratch.d_scan.ensure(scan_bytes), "alloc drain scan");
    HIP_TRY(hipMemcpyAsync(A.d_strips.p, A.strips.data(), static_cast<size_t>(ns) * sizeof(AudStrip), hipMemcpyHostToDevice, s),
            "upload audience strips");
    AudArgs g{};
    g.strips = A.d_strips.as<AudStrip>();
    g.n_strips = ns;
    g.share = D.env.share;
    g.verdict = A.d_verdict.as<uint8_t>();
    g.n_exc = cnt;
    g.n_full = A.d_full.as<uint32_t>();
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_audience_classify(drain_args(e, D.tab), g, s), "k_audience_classify");
    HIP_TRY(tm.end(ms[0]), "event");
    HIP_TRY(tm.begin(), "event");
    scan_bytes = D.sync.scratch.d_scan.bytes;
    HIP_TRY(drain_scan(D.sync.scratch.d_scan.p, &scan_bytes, cnt, off, ns + 1, s), "drain scan");
    HIP_TRY(tm.end(ms[1]), "event");
    uint8_t* const rec = A.d_rec.as<uint8_t>();
    AudEmit o{};
    o.node_peer = e->d_node_peer.as<uint32_t>();
    o.off = off;
    o.peer = reinterpret_cast<uint32_t*>(rec);
    o.node = reinterpret_cast<uint32_t*>(rec + o_node);
    o.verdict = rec + o_v;
    o.cap = n_verdicts;
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_audience_emit(g, o, s), "k_audience_emit");
    HIP_TRY(tm.end(ms[2]), "event");
    // (records from `lo` on, up to `hi`: the prefix now, the rest once the count is known)
    auto read_records = [&](uint64_t lo, uint64_t hi) -> hipError_t {
      if (hi <= lo) return hipSuccess;
      hipError_t r = hipMemcpyAsync(A.exc_peer.data() + lo, o.peer + lo, (hi - lo) * 4, hipMemcpyDeviceToHost, s);
      if (r == hipSuccess) r = hipMemcpyAsync(A.exc_node.data() + lo, o.node + lo, (hi - lo) * 4, hipMemcpyDeviceToHost, s);
      if (r == hipSuccess) r = hipMemcpyAsync(A.exc_verdict.data() + lo, o.verdict + lo, hi - lo, hipMemcpyDeviceToHost, s);
      return r;
    };
    const uint64_t pre = std::min<uint64_t>(n_verdicts, kAudPrefix);
    A.exc_peer.resize(pre);
    A.exc_node.resize(pre);
    A.exc_verdict.resize(pre);
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(hipMemcpyAsync(A.strip_off.data(), off, (static_cast<size_t>(ns) + 1) * 8, hipMemcpyDeviceToHost, s),
            "read audience offsets");
    HIP_TRY(hipMemcpyAsync(A.strip_full.data(), g.n_full, static_cast<size_t>(ns) * 4, hipMemcpyDeviceToHost, s),
            "read audience counts");
    HIP_TRY(read_records(0, pre), "read audience records");
    HIP_TRY(hipStreamSynchronize(s), "sync");
    n_exc = A.strip_off[ns];
    if (n_exc > n_verdicts) return e->fail(PS_E_STATE, "audience: more exceptions than nodes");
    if (n_exc > pre) {
      A.exc_peer.resize(n_exc);
      A.exc_node.resize(n_exc);
      A.exc_verdict.resize(n_exc);
      HIP_TRY(read_records(pre, n_exc), "read audience records");
      HIP_TRY(hipStreamSynchronize(s), "sync");
    }
    HIP_TRY(tm.end(ms[4]), "event");
  }
  A.exc_peer.resize(std::max<uint64_t>(n_exc, 1));
  A.exc_list.assign(std::max<uint64_t>(n_exc, 1), PS_NONE);

  // lists, in request order: a topic's shared list where a row holds it, then
  // a private one per exception that holds a message
  h0 = hclock::now();
  std::vector<DrainQuery> lists;
  uint64_t n_segs64 = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t t = topic[i];
    const uint32_t segs = ceil_div(D.tab.topics[t].n_pos, kDrainSegBits);
    A.exc_off[i] = A.strip_off[strip0[i]];
    A.exc_off[i + 1] = A.strip_off[strip0[i + 1]];
    for (uint64_t k = strip0[i]; k < strip0[i + 1]; ++k) A.n_full[i] += A.strip_full[k];
    if (A.n_full[i]) {
      A.topic_list[i] = static_cast<uint32_t>(lists.size());
      lists.push_back(DrainQuery{t, kDrainMaskRow, static_cast<uint32_t>(n_segs64), 0});
      n_segs64 += segs;
    }
    for (uint64_t k = A.exc_off[i]; k < A.exc_off[i + 1]; ++k) {
      if (!(A.exc_verdict[k] & kDrainRowAny)) continue;
      if (n_segs64 + segs >= kDrainRowLimit || lists.size() + 1 >= 0x7FFFFFFFull)
        return e->fail(PS_E_RANGE, "too many rows in one drain");
      A.exc_list[k] = static_cast<uint32_t>(lists.size());
      lists.push_back(DrainQuery{t, A.exc_node[k], static_cast<uint32_t>(n_segs64), 0});
      n_segs64 += segs;
    }
    if (n_segs64 >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  }
  const uint32_t n_lists = static_cast<uint32_t>(lists.size());
  const uint32_t n_segs = static_cast<uint32_t>(n_segs64);
  host_ms[1] = ms_since(h0);
  DrainArgs a = drain_args(e, D.tab);
  float count_ms = 0;
  if ((rc = drain_list_offsets(e, a, lists, n_segs, A.list_off, tm, count_ms, ms[3]))) return rc;
  ms[3] += count_ms;
  const uint64_t total = A.list_off[n_lists];
  // (the pinned ids grow before Sync::d_lists, which drain_list_ids grows: allocations only, no enqueued work moves)
  if (total) HIP_TRY(pinned_ensure(&A.h_ids, nullptr, &A.ids_cap, total * 4), "alloc audience ids");
  if ((rc = drain_list_ids(e, a, n_segs, total, A.h_ids, tm, ms[3], ms[4]))) return rc;
  if (!A.h_ids) HIP_TRY(pinned_ensure(&A.h_ids, nullptr, &A.ids_cap, 4), "alloc audience ids");
  *topic_list_out = A.topic_list.data();
  *n_nodes_out = A.n_nodes.data();
  *n_full_out = A.n_full.data();
  *exc_off_out = A.exc_off.data();
  *exc_peer_out = A.exc_peer.data();
  *exc_list_out = A.exc_list.data();
  *list_off_out = A.list_off.data();
  *msg_out = reinterpret_cast<const uint32_t*>(A.h_ids);
  *n_lists_out = n_lists;
  *total_out = total;
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd drain_topics: topics %zu strips %u nodes %llu row_bytes %llu exceptions %llu lists %u segments %u ids "
                 "%llu classify_ms %.4f scan_ms %.4f emit_ms %.4f lists_ms %.4f copy_ms %.4f host_strips_ms %.4f "
                 "host_lists_ms %.4f\n",
                 n, ns, static_cast<unsigned long long>(n_verdicts), static_cast<unsigned long long>(row_bytes),
                 static_cast<unsigned long long>(n_exc), n_lists, n_segs, static_cast<unsigned long long>(total), ms[0],
                 ms[1], ms[2], ms[3], ms[4], host_ms[0], host_ms[1]);
  return PS_OK;
}

// ---- ps_drain_topics_begin / ps_drain_topics_end -----------

// ps_drain_topics' answer enqueued behind the last run, with no host wait:
// tables (device build), the strips and the entry table in one upload,
// classify / scan / emit as above with the records left on the device, then
// what the host does above between its waits on the device -- the per-topic
// totals, the lists numbered in request order and their segments laid out
// (k_audience_totals / _keys / two scans / _lists) -- and count / scan /
// offsets / emit over the lists with the counts read from the slot's control
// block, all on `stream`; the view leaves in one copy on the copy stream.
// The host knows only the caps: every buffer and grid is sized by them.
int ps_drain_topics_begin(ps_engine* e, const uint32_t* topic, size_t n, size_t exc_cap, size_t list_cap, size_t id_cap) {
  if (!e || (n && !topic)) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_drain_topics_begin on a multi-rank engine: use ps_drain", "no run enqueued",
                                    "two drains outstanding: end one first", false}))
    return rc;
  if (const int rc = aud_check_topics(e, topic, n)) return rc;
  if (exc_cap >= 0x7FFFFFFFull || list_cap >= 0x7FFFFFFFull) return e->fail(PS_E_RANGE, "too many exceptions or lists");
  auto& D = e->drain;
  const auto t_host0 = hclock::now();

  // staged in the slot's pinned input, behind the table block where one is
  // built: the entry table, then the strips (sized before the tables stand).
  // From here to the slot's taking a failure gives the slot up.
  size_t o_strips = 0;
  uint64_t strips_max = 0;
  const size_t stage_bytes = aud_stage_bytes(e, topic, n, &o_strips, &strips_max);
  if (strips_max >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  Drain::Slot* slot = nullptr;
  size_t used = 0;
  uint8_t* h = nullptr;
  int rc = drain_begin_slot(e, stage_bytes, D.env.timing, &slot, &used, &h);
  if (rc) return rc;
  auto& S = *slot;
  hipStream_t s = e->stream;
  AudShape A;
  if (!aud_stage(e, topic, n, reinterpret_cast<AudEntry*>(h), reinterpret_cast<AudStrip*>(h + o_strips), strips_max, &A))
    return drain_give_up(e, used, PS_E_STATE, "audience: more strips than staged");
  const uint32_t ns = A.ns;

  // the caps: the engine's where the caller names none
  uint32_t seg_bound = 0;
  const bool rows_fit = aud_caps(A, n, &exc_cap, &list_cap, &id_cap, &seg_bound);
  if (id_cap > kDrainAsyncMaxIds) return drain_give_up(e, used, PS_E_RANGE, "drain may exceed 2^30 ids: use ps_drain_topics");
  if (!rows_fit) return drain_give_up(e, used, PS_E_RANGE, "too many rows in one drain");

  S.n = n;
  S.kind = Drain::Slot::kTopics;
  S.exc_cap = exc_cap;
  S.list_cap = list_cap;
  S.id_cap = id_cap;
  S.o_tl = align256(sizeof(DrainSharedHdr));
  S.o_nf = S.o_tl + align256(n * 4);
  S.o_eo = S.o_nf + align256(n * 8);
  S.o_ep = S.o_eo + align256((n + 1) * 8);
  S.o_el = S.o_ep + align256(exc_cap * 4);
  S.o_off = S.o_el + align256(exc_cap * 4);
  S.o_ids = S.o_off + align256((list_cap + 1) * 8);
  const size_t res_bytes = S.o_ids + id_cap * 4;
  S.o_nn = align256(res_bytes);  // (behind what the copy brings)
  HIP_TRY(pinned_ensure(&S.h_res, &S.h_res_dev, &S.res_cap, S.o_nn + std::max<size_t>(n, 1) * 8), "alloc drain view");
  uint64_t* const h_nodes = reinterpret_cast<uint64_t*>(S.h_res + S.o_nn);
  for (size_t i = 0; i < n; ++i) {
    uint32_t u0 = 0;
    h_nodes[i] = aud_nodes(e, topic[i], &u0);
  }
  S.enqueued = false;
  if (ns == 0) {  // no row to read: no list, no exception, written here
    std::memset(S.h_res, 0, S.o_ep);
    std::memset(S.h_res + S.o_tl, 0xFF, n * 4);
    std::memset(S.h_res + S.o_off, 0, 8);
    return drain_slot_host_view(e, S, used);
  }

  // (PSAMD_DRAIN_TIMING: the phases run apart and are waited for; else nothing here waits)
  float ms[7] = {0, 0, 0, 0, 0, 0, 0};  // classify, scan, emit, assign, count, scan + offsets, emit
  const PhaseTimer tm{D.ev_t, s, D.env.timing};
  const size_t in_bytes = o_strips + static_cast<size_t>(ns) * sizeof(AudStrip);
  HIP_TRY(S.d_res.ensure(res_bytes), "alloc drain result");
  HIP_TRY(S.lb.d_in.ensure(in_bytes), "alloc drain input");
  uint8_t* const din = S.lb.d_in.as<uint8_t>();
  uint8_t* const res = S.d_res.as<uint8_t>();
  HIP_TRY(hipMemcpyAsync(din, h, in_bytes, hipMemcpyHostToDevice, s), "upload audience strips");
  if ((rc = drain_err_word(e, s))) return rc;
  const AudBufs bufs{&S.lb, &S.d_verdict, &S.d_exc, &S.d_full, &S.d_rec};
  const AudView view{reinterpret_cast<uint32_t*>(res + S.o_tl), reinterpret_cast<uint64_t*>(res + S.o_nf),
                     reinterpret_cast<uint64_t*>(res + S.o_eo), reinterpret_cast<uint32_t*>(res + S.o_ep),
                     reinterpret_cast<uint32_t*>(res + S.o_el)};
  DrainArgs a{};
  DrainCtl* ctl = nullptr;
  if ((rc = aud_pass(e, bufs, reinterpret_cast<const AudEntry*>(din), reinterpret_cast<const AudStrip*>(din + o_strips), n,
                     A, exc_cap, list_cap, seg_bound, view, tm, ms, &a, &ctl)))
    return rc;
  const uint64_t* const off = S.lb.scratch.d_off.as<uint64_t>();
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_offsets_dev(a.queries, ctl, static_cast<uint32_t>(list_cap), off, id_cap, D.tab.d_err,
                                   reinterpret_cast<DrainSharedHdr*>(res), reinterpret_cast<uint64_t*>(res + S.o_off), s),
          "k_drain_offsets_dev");
  HIP_TRY(tm.end(ms[5]), "event");
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_drain_emit_dev(a, ctl, seg_bound, off, reinterpret_cast<uint32_t*>(res + S.o_ids), id_cap, s),
          "k_drain_emit_dev");
  HIP_TRY(tm.end(ms[6]), "event");
  // classify reads every row of the named topics, count and emit the private
  // lists' rows: the event behind the emit covers them all
  if ((rc = drain_slot_enqueued(e, S, res_bytes, true))) return rc;
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd drain_topics_begin: topics %zu strips %u nodes %llu row_bytes %llu exc_cap %zu list_cap %zu id_cap %zu "
                 "seg_bound %u tables %s classify_ms %.4f strip_scan_ms %.4f records_ms %.4f assign_ms %.4f count_ms %.4f "
                 "scan_ms %.4f emit_ms %.4f upload_bytes %zu view_bytes %zu host_us %.1f\n",
                 n, ns, static_cast<unsigned long long>(A.n_verdicts), static_cast<unsigned long long>(A.row_bytes), exc_cap,
                 list_cap, id_cap, seg_bound, used ? "built" : "kept", ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], ms[6],
                 in_bytes, res_bytes, 1e3 * ms_since(t_host0));
  return PS_OK;
}

int ps_drain_topics_end(ps_engine* e, const uint32_t** topic_list_out, const uint64_t** n_nodes_out,
                        const uint64_t** n_full_out, const uint64_t** exc_off_out, const uint32_t** exc_peer_out,
                        const uint32_t** exc_list_out, const uint64_t** list_off_out, const uint32_t** msg_out,
                        uint32_t* n_lists_out, uint64_t* total_out) {
  if (!e || !topic_list_out || !n_nodes_out || !n_full_out || !exc_off_out || !exc_peer_out || !exc_list_out ||
      !list_off_out || !msg_out || !n_lists_out || !total_out)
    return PS_E_INVAL;
  auto& D = e->drain;
  if (D.slot_count == 0) return e->fail(PS_E_NOTREADY, "no drain outstanding");
  auto& S = D.slot[D.slot_head];
  if (S.kind != Drain::Slot::kTopics)
    return e->fail(PS_E_STATE, S.kind == Drain::Slot::kShared ? "the oldest drain is a shared one: ps_drain_shared_end"
                                                              : "the oldest drain is not a topics one: ps_drain_end");
  if (const int rc = drain_slot_complete(e, S)) return rc;
  const DrainSharedHdr* hdr = reinterpret_cast<const DrainSharedHdr*>(S.h_res);
  *topic_list_out = reinterpret_cast<const uint32_t*>(S.h_res + S.o_tl);
  *n_nodes_out = reinterpret_cast<const uint64_t*>(S.h_res + S.o_nn);
  *n_full_out = reinterpret_cast<const uint64_t*>(S.h_res + S.o_nf);
  *exc_off_out = reinterpret_cast<const uint64_t*>(S.h_res + S.o_eo);
  *exc_peer_out = reinterpret_cast<const uint32_t*>(S.h_res + S.o_ep);
  *exc_list_out = reinterpret_cast<const uint32_t*>(S.h_res + S.o_el);
  *list_off_out = reinterpret_cast<const uint64_t*>(S.h_res + S.o_off);
  *msg_out = reinterpret_cast<const uint32_t*>(S.h_res + S.o_ids);
  *n_lists_out = hdr->n_lists;
  *total_out = hdr->total;
  return drain_view_status(e, hdr->err, hdr->over);
}

}  // extern "C"
