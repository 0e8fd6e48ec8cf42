// drain_impl.hpp -- what the host files of the batched drain share (kernels:
// drain.hip).  One file per call family:
//   drain_tables.cpp  per window, not per call: the entry checks, both table
//                     builds, query resolution, count + scan, pinned staging
//   drain_standing.cpp  the tracker lifecycle, once for the seven ps_*_track /
//                     ps_*_take families below: a run's
//                     staging, the front and the back of a window's pass, the
//                     fence per row set, registering topics, the take of the totals
//   drain.cpp         ps_drain, ps_drain_begin / ps_drain_end, the slots
//   drain_shared.cpp  ps_drain_shared, ps_drain_shared_begin / _end (§5.5c, d),
//                     the shared-list pass and the synchronous list tail
//   drain_sink.cpp    ps_sink_set / ps_sink_take and run.cpp's hooks (§5.5e):
//                     the shared drain behind every window of a run; and
//                     ps_sink_set_topics / ps_sink_take_topics (§5.5h): the
//                     audience drain behind every window, through the same hooks
//   drain_topics.cpp  ps_drain_topics (§5.5f): a topic's audience as one list
//                     plus exceptions; ps_drain_topics_begin / _end (§5.5g):
//                     that answer behind a running batch
//   drain_load.cpp    ps_peer_load, ps_load_track / ps_load_take and its window
//                     hook (§5.5i): per-peer recv / sent sums from the audience
//                     pass's strips and verdicts, with buffers of their own
//   drain_hops.cpp    ps_topic_hops, ps_hops_track / ps_hops_take and its window
//                     hook (§5.5j): per tree topic, nodes / reached / deliv by
//                     BFS level from the same strips and verdicts and the
//                     host's level tables, with buffers of their own
//   drain_downstream.cpp  ps_peer_downstream, ps_downstream_track / _take and
//                     its window hook (§5.5k): per peer, the nodes and window
//                     messages below its nodes, bottom-up over the same level
//                     tables behind the same strips and verdicts, with buffers
//                     of their own
//   drain_cut.cpp     ps_peer_cut, ps_cut_track / _take and its window hook
//                     (§5.5l): per peer, what its nodes missed and what was lost
//                     behind its cut points, over the downstream pass's plan
//                     (down_plan .. down_window_stage below), with buffers of
//                     their own
//   drain_report.cpp  ps_peer_report, ps_report_track / _take and its window
//                     hook (§5.5m): the four answers above from one classify,
//                     one per-node kernel and one bottom-up sweep, over the hop
//                     pass's and the downstream pass's plans (hops_plan,
//                     hops_entries, down_plan .. down_entries below), with
//                     buffers of their own
//   drain_dist.cpp    ps_dist_report (§5.5n): a rank's share of the load, hop and
//                     downstream sections on an engine of any rank count --
//                     the audience pass's strips and classify, kernels of its
//                     own for a sharded rank's numbering, and a bottom-up sweep
//                     that crosses ranks through Transport::exchange; blocking
//                     only, with buffers of its own; ps_dist_cut (§5.5o) and
//                     ps_dist_blame (§5.5r) through the same front and plan,
//                     each with a downward exchange of its own
//   drain_spread.cpp ps_topic_spread (§5.5p): hops and duplicate copies for meshes
//                     and trees alike -- the audience pass's strips and classify,
//                     then a frontier BFS over the node space's child lists, one
//                     launch per level; blocking, with buffers of its own; the
//                     entry table and the kernels' arguments for its tracker too
//                     (spread_entries .. spread_args below)
//   drain_spread_track.cpp  ps_spread_track / ps_spread_take and its window hook
//                     (§5.5t): that pass behind every window of a run, meshes
//                     and trees alike -- the window's last round + 1 level
//                     launches enqueued whole, k_spread_track_close behind them
//                     -- into totals, with buffers of its own
//   drain_blame.cpp   ps_topic_blame, ps_blame (§5.5q): each node that lacks
//                     messages with the cut point it hangs behind -- the
//                     downstream pass's plan and front (down_sync_stage,
//                     down_front below), then a top-down sweep over the same
//                     levels, records by count / scan / emit or a gather for
//                     explicit queries; blocking only, with buffers of its own
//   drain_blame_track.cpp  ps_blame_track / ps_blame_take and its window hook
//                     (§5.5s): that pass behind every window of a run, its
//                     records appended at a cursor on the device, over the
//                     downstream pass's window staging (down_window_stage
//                     below), with buffers of its own
// The state is ps_engine::Drain (engine.hpp), grouped by owner.
//
// What the paths rely on, between them and with run.cpp:
//  - Drain::Tables (seq, p_*): one set of device tables per window, built by
//    whichever path runs first (drain_tables on the host, drain_tables_async
//    on the device; the sink always builds its window's) and reused by the others.
//  - Tables::d_err lives behind the mask words of the device build; it is
//    created (8 bytes, cleared) on first use when only host builds have run.
//    The synchronous list tail passes a zero word behind its header instead.
//  - ps_drain's slabs: ev_copy[k & 1] is waited on before slab k is emitted,
//    slab k - 1 is copied while slab k is emitted; under timing the copy runs
//    in line on `stream`.
//  - Slot::seen / emit_pending / ev_emit, Sink::fence (the last sink emit
//    over each row set) and every tracker's Standing::fence (its last standing
//    pass over each) are read by drain_fence (run.cpp).
//  - The seven trackers keep one Drain::Standing each and go through
//    drain_standing.cpp for all of its lifecycle; Drain::standing() lists them
//    in the order run.cpp opens them, runs their *_window hooks
//    (kStandingWindow) and aborts them, and drain_fence, drain_destroy and
//    ps_dist_init*'s refusal walk the same list.  No two share an arena or an
//    event.  A new tracker is a Standing, a *_window function and one row of
//    that table.
//  - ps_drain_shared_begin and the sink run one pass over their queries
//    (shared_stage, shared_caps, shared_pass), each with buffers of its own.
//  - ps_drain_topics_begin and the audience sink run one pass over their topics
//    (aud_stage, aud_caps, aud_pass), each with buffers of its own; the sink
//    keeps its entries and strips on the device between windows of one shape
//    (Sink::strip_key), the begin call uploads them per call.
//  - ps_drain_shared and ps_drain_topics run one tail over their list queries
//    (drain_list_offsets, drain_list_ids) in Drain::Sync; the host numbers the
//    lists, which is what the tests compare the device assignment against.
//  - The three begin calls share the two slots (Slot::kind names the end call
//    that completes one) and what surrounds them: drain_begin_slot,
//    drain_give_up, drain_slot_host_view, drain_slot_enqueued, drain_slot_complete.
//    ps_drain_topics_begin keeps its strips' verdicts, counts and records in
//    the slot, not in Drain::Audience: a synchronous ps_drain_topics may run
//    beside two outstanding drains.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "engine.hpp"

namespace psamd {

using Drain = ps_engine::Drain;
using SharedSort = Drain::SharedSort;
using AudShape = Drain::AudShape;
using hclock = std::chrono::steady_clock;

inline double ms_since(hclock::time_point t0) { return std::chrono::duration<double, std::milli>(hclock::now() - t0).count(); }

// segments (or classify steps) one call may hold: the kernels index them in 32 bits
constexpr uint64_t kDrainRowLimit = 0x7FFFFFFFull;
// ids one asynchronous drain may hold at most (its buffers are sized by an
// upper bound, not by the total): larger drains go through ps_drain's slabs
constexpr uint64_t kDrainAsyncMaxIds = 1ull << 30;
// drain_shared_sort's mark on a verdict the host gives (no classify pass)
constexpr uint32_t kOnHost = 0x80000000u;

inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

// PSAMD_DRAIN_TIMING: one phase on stream s between the two timing events,
// waited for at its end.  Off: nothing is recorded and nothing waits.
struct PhaseTimer {
  const hipEvent_t* ev;
  hipStream_t s;
  bool on;
  hipError_t begin() const { return on ? hipEventRecord(ev[0], s) : hipSuccess; }
  hipError_t end(float& ms) const {
    if (!on) return hipSuccess;
    hipError_t r = hipEventRecord(ev[1], s);
    if (r == hipSuccess) r = hipEventSynchronize(ev[1]);
    float t = 0;
    if (r == hipSuccess) r = hipEventElapsedTime(&t, ev[0], ev[1]);
    ms += t;
    return r;
  }
};

// ---- drain_tables.cpp (each is described where it is defined) ------------------

hipError_t pinned_ensure(uint8_t** h, uint8_t** d, size_t* cap, size_t need);
hipError_t sink_stage(Drain::Sink::Res& R, size_t bytes, uint8_t** out);
inline void release_all(std::initializer_list<DevBuf*> bufs) {
  for (DevBuf* b : bufs) b->release();
}

// Where one call stages its input: a slot's pinned h_in, all of it (one call
// takes once), or a region of a sink result's arena
struct Staging {
  Drain::Slot* slot;
  Drain::Sink::Res* arena;
  hipError_t take(size_t bytes, uint8_t** out) const {
    if (arena) return sink_stage(*arena, bytes, out);
    const hipError_t rc = pinned_ensure(&slot->h_in, nullptr, &slot->in_cap, bytes);
    *out = slot->h_in;
    return rc;
  }
};

// The state checks of a call on the last window, tested in this order; a null
// message: the call has no such check
struct DrainEntry {
  const char* multi_rank;  // PS_E_STATE on a multi-rank engine (ps_drain serves them)
  const char* no_window;   // PS_E_NOTREADY before the first run
  const char* slots_full;  // PS_E_STATE with two drains outstanding (the begin calls)
  // the twin is joined before the queries are read (the synchronous calls);
  // the begin calls join it in drain_begin_slot, behind their limits
  bool join;
};
// (ps_drain_topics takes no (topic, peer) query: it checks its topics itself)
int drain_enter(ps_engine* e, const DrainEntry& c, const uint32_t* topic = nullptr, const uint32_t* peer = nullptr,
                size_t n = 0);
int drain_ready(ps_engine* e);
int drain_check_queries(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n);
int drain_tables(ps_engine* e);
int drain_tables_async(ps_engine* e, const Staging& st, size_t tail, bool timed, size_t* used, uint8_t** tail_out);
int drain_err_word(ps_engine* e, hipStream_t s);
uint64_t drain_resolve(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, DrainQuery* out,
                       uint64_t* bound);
DrainArgs drain_args(const ps_engine* e, const Drain::Tables& T);
int drain_count_scan(ps_engine* e, DrainArgs& a, uint32_t n_segs, Drain::Scratch& B, const DrainQuery* queries,
                     size_t n_queries, hipStream_t s, const PhaseTimer& tm, float& count_ms);

// The node query (t, peer) reads, kNone where its answer is empty: a topic
// idle in the window, the root, a peer not subscribed or another rank's.
// `map`: topic t's peer map once looked up (a caller may keep it per topic).
// (Inline: the resolution and the sort call it once per query.)
inline uint32_t drain_node(ps_engine* e, uint32_t t, uint32_t peer, const uint32_t*& map) {
  if (!e->drain.tab.topics[t].n_pos) return kNone;
  if (!map) map = peer_node_map(e, t, e->last_topics[t]).data();
  return map[peer];
}

// ---- drain.cpp: what the two asynchronous forms share around their slots -------

int drain_begin_slot(ps_engine* e, size_t tail, bool timed, Drain::Slot** slot, size_t* used, uint8_t** tail_out);
int drain_give_up(ps_engine* e, bool staged, int code, const char* what);
int drain_slot_host_view(ps_engine* e, Drain::Slot& S, bool staged);
int drain_view_status(ps_engine* e, uint64_t err, uint32_t over);
int drain_slot_enqueued(ps_engine* e, Drain::Slot& S, size_t res_bytes, bool to_host);
int drain_slot_complete(ps_engine* e, Drain::Slot& S);

// ---- drain_shared.cpp -----------------------------------------------------------

// The shared-list pass's input, one block and one upload: queries | initial
// verdicts | sorted queries | bins
struct SharedLayout {
  size_t n;
  uint32_t nt;
  size_t o_v, o_cq, o_bins, tail;
  SharedLayout(size_t n_queries, uint32_t n_topics)
      : n(n_queries),
        nt(n_topics),
        o_v(align256(n * sizeof(DrainQuery))),
        o_cq(o_v + align256(n * 4)),
        o_bins(o_cq + align256(n * sizeof(DrainClassQuery))),
        tail(o_bins + align256(nt * sizeof(DrainClassBin))) {}
};

// the shared-list pass: ps_drain_shared_begin's, and the sink's per window
int shared_stage(ps_engine* e, const uint32_t* topic, const uint32_t* peer, const SharedLayout& L, uint8_t* c,
                 SharedSort* R);
bool shared_caps(const Drain& D, const SharedSort& R, size_t n, bool own, size_t* list_cap, size_t* id_cap,
                 uint32_t* seg_bound);
int shared_pass(ps_engine* e, Drain::ListBufs& B, const SharedLayout& L, const uint8_t* h, const SharedSort& R,
                size_t list_cap, uint32_t seg_bound, uint32_t* list_of_query, const PhaseTimer& tm, float* ms,
                DrainArgs* args, DrainCtl** ctl_out);
// the synchronous list tail: ps_drain_shared's, and ps_drain_topics'
int drain_list_offsets(ps_engine* e, DrainArgs& a, const std::vector<DrainQuery>& lists, uint32_t n_segs,
                       std::vector<uint64_t>& hdr, const PhaseTimer& tm, float& count_ms, float& scan_ms);
int drain_list_ids(ps_engine* e, const DrainArgs& a, uint32_t n_segs, uint64_t total, void* out, const PhaseTimer& tm,
                   float& emit_ms, float& copy_ms);


// ---- drain_topics.cpp -------------------------------------------------------------

// the checks every topics call makes on its topics: range, then repeats
int aud_check_topics(ps_engine* e, const uint32_t* topic, size_t n);
// topic t's non-root nodes in the last window: the first one and their number
uint32_t aud_nodes(const ps_engine* e, uint32_t t, uint32_t* u0);

// nodes of every strip but a topic's last (the hop pass finds a level's strips by it)
uint32_t aud_strip_nodes(bool gather, uint32_t words);

// the bytes one window's entries and strips take at most, before its tables
// stand: entries | strips (the strips from *o_strips)
size_t aud_stage_bytes(ps_engine* e, const uint32_t* topic, size_t n, size_t* o_strips, uint64_t* strips_max);
// The audience pass: ps_drain_topics_begin's, and the audience sink's per
// window.  aud_stage cuts the entry table and the strips from the named topics'
// node ranges in the last window into `entries` [n + 1] and `strips`
// [strips_max] (false: more strips than staged; both null: the shape alone); aud_caps settles the three caps
// (zero: the engine's) and the segment bound (false: too many rows); aud_pass
// enqueues classify through the segment scan over entries and strips on the
// device, into `view` (window-local) and the buffers' control block.
bool aud_stage(ps_engine* e, const uint32_t* topic, size_t n, AudEntry* entries, AudStrip* strips, uint64_t strips_max,
               AudShape* out);
bool aud_caps(const AudShape& A, size_t n, size_t* exc_cap, size_t* list_cap, size_t* id_cap, uint32_t* seg_bound);
struct AudBufs {
  Drain::ListBufs* lb;  // d_key, d_aux (the control block), scratch: the lists, their counts, offsets, the scans' temporary
  DevBuf *d_verdict, *d_exc, *d_full, *d_rec;
};
struct AudView {
  uint32_t* topic_list;  // [n]
  uint64_t* n_full;      // [n]
  uint64_t* exc_off;     // [n + 1]
  uint32_t* exc_peer;    // [exc_cap]
  uint32_t* exc_list;    // [exc_cap]
};
// ms: classify, strip scan, records, assign, count, segment scan (PSAMD_DRAIN_TIMING)
int aud_pass(ps_engine* e, const AudBufs& B, const AudEntry* d_entries, const AudStrip* d_strips, size_t n,
             const AudShape& A, size_t exc_cap, size_t list_cap, uint32_t seg_bound, const AudView& view,
             const PhaseTimer& tm, float* ms, DrainArgs* args, DrainCtl** ctl_out);

// ---- drain_standing.cpp: the tracker lifecycle, once for the seven families ---------

// (standing_open / standing_abort, around a run: engine.hpp, beside the window hooks)
// every pass enqueued so far is complete: nothing waits for one any more
void standing_settled(Drain::Standing& S);
void standing_destroy(Drain::Standing& S);  // (ps_destroy)
// ps_*_track, in this order with the family's own refusals between them: the
// multi-rank and in-flight refusals and the topic checks; the device, and the
// end of whatever still adds into the totals; then the new topics in place of
// the old ones, the counts zeroed, the kept block dropped
int standing_track_check(ps_engine* e, const Drain::Standing& S, const uint32_t* topic, size_t n);
int standing_quiesce(ps_engine* e, Drain::Standing& S);
void standing_retrack(Drain::Standing& S, const uint32_t* topic, size_t n);
// ... and behind them the totals: cleared on the stream, or released with the
// standing pass's buffers when nothing is tracked any more
int standing_totals(ps_engine* e, Drain::Standing& S, DevBuf& d_acc, size_t bytes, std::initializer_list<DevBuf*> pass);
// ps_*_take: the state checks and the device; the lazily created event; and the
// whole take of `bytes` of totals into A.h_out -- checks, copy, clearing, one
// wait, settled.  The caller hands its arrays out and returns and zeroes the counts.
int standing_take_enter(ps_engine* e, const Drain::Standing& S);
int standing_take_event(ps_engine* e, Drain::Standing& S);
int standing_take_totals(ps_engine* e, Drain::Standing& S, DevBuf& d_acc, Drain::Answer& A, size_t bytes);
// A window's pass (S.on, S.open): the twin joined and the window's tables,
// *R: the run's staging; ... its kernels ...; then the fence of the row set,
// the run's event and the counts
int standing_window_begin(ps_engine* e, Drain::Standing& S, Drain::Sink::Res** R);
int standing_window_done(ps_engine* e, Drain::Standing& S, size_t n_skipped);
// the two words every family's strip_key holds per topic -- table flags |
// n_pos, non-root nodes | node base -- appended; returns the first non-root node
uint32_t standing_key_topic(ps_engine* e, uint32_t t, std::vector<uint64_t>* key);
// the block kept on the device is the window's (true), or the key is dropped
// until the caller has staged the new block and sets it
inline bool standing_key_stands(Drain::Standing& S, const std::vector<uint64_t>& key) {
  if (key == S.strip_key) return true;
  S.strip_key.clear();
  return false;
}

// ---- drain_hops.cpp: what the passes over tree levels ask of a topic ---------------

// topic t is a mesh in the last window's node space: it has no levels
bool hops_is_mesh(const ps_engine* e, uint32_t t);
// topic t has rows to read in the last window (its drain table stands)
bool hops_active(ps_engine* e, uint32_t t);
// an active topic's level table is the last window's (false: set anew over another kind since)
bool hops_levels_stand(ps_engine* e, uint32_t t);
// the topic as it is defined now builds into a mesh
bool hops_child_lists_mesh(const TopicHost& T);

// The tree topics of a request with their positions in it: a mesh topic of
// the window's node space takes no part in the pass
struct HopsReq {
  std::vector<uint32_t> topic, row;
  size_t n_lvl = 0;  // level-table words of the topics with rows to read
};
int hops_plan(ps_engine* e, const uint32_t* topic, size_t n, HopsReq* R);
// aud_stage's entries [n + 1] as the hop pass's, into he; the level tables
// into lv where it is given; the shape's counts (the layout stays the caller's)
void hops_entries(ps_engine* e, const HopsReq& R, const AudEntry* ae, const AudShape& A, HopsEntry* he, uint32_t* lv,
                  Drain::Hops::Shape* K);

// ---- drain_downstream.cpp: what the passes over subtrees share (drain_cut.cpp) ------

using Down = Drain::Downstream;  // (Drain::Cut is the same shape)

// The tree topics of a request (a mesh topic of the window's node space takes
// no part in the pass) and what their level tables come to
struct DownReq {
  std::vector<uint32_t> topic;
  size_t n_lvl = 0;      // level-table words of the topics with rows to read
  size_t n_work = 0;     // work items of their level launches
  uint64_t n_nodes = 0;  // their nodes, roots included: the scratch words
};
// the plan of a request, the layout of its input block (entries | levels |
// work | strips) and the block's first three parts; `who` names the pass in messages
int down_plan(ps_engine* e, const uint32_t* topic, size_t n, const char* who, DownReq* R);
void down_layout(const DownReq& R, Down::Shape* K);
void down_entries(ps_engine* e, const DownReq& R, const AudEntry* ae, const AudShape& A, DownEntry* de, uint32_t* lv,
                  DownWork* wk, Down::Shape* K);
// a pass's buffers, k_audience_classify and k_audience_weights over the block `din`
int down_front(ps_engine* e, Down::Pass& P, const uint8_t* din, const Down::Shape& K, const PhaseTimer& tm, float* ms,
               DownArgs* out);
// a blocking call's block over the named tree topics, whole, into `stage`
int down_sync_stage(ps_engine* e, std::vector<uint8_t>& stage, const uint32_t* topic, size_t n, const char* who,
                    Down::Shape* K);
// the front of a standing subtree pass's window (downstream, cut, blame): the
// block into P.d_in, kept with its shape while S.strip_key stands
int down_window_stage(ps_engine* e, Drain::Standing& S, Down::Pass& P, Down::Shape& kept, Down::Shape* K, size_t* n_tree);

// ---- drain_spread.cpp: what the blocking spread and its tracker share ----------------

constexpr uint32_t kSpreadGridMax = 2048;  // blocks of a level launch at most
constexpr size_t kSpreadCntBytes = 256;    // the three counts in front of the queues

// the output block in 64-bit words: reached | deliv | unreached | holders |
// visited, then in peer space recv | copies | dup
struct SpreadOut {
  size_t reached, deliv, unreached, holders, visited, recv, copies, dup, words;
  SpreadOut(size_t n, size_t np) {
    reached = 0;
    deliv = n * kHopsCols;
    unreached = 2 * n * kHopsCols;
    holders = unreached + n;
    visited = holders + n;
    recv = visited + n;
    copies = recv + np;
    dup = copies + np;
    words = dup + np;
  }
};
// what the entry table comes to: the words of k / hop, the first frontier, the meshes among it
struct SpreadPlan {
  uint64_t n_nodes = 0;
  uint32_t n_roots = 0, n_mesh = 0;
};
// aud_stage's entries [n + 1] as the spread pass's, into se [n + 1]; the roots
// of the topics that take part -- the first frontier -- into roots [n]
void spread_entries(ps_engine* e, const uint32_t* topic, size_t n, const AudEntry* ae, const AudShape& A, SpreadEntry* se,
                    SpreadItem* roots, SpreadPlan* P);
// a pass's buffers but its input block, sized for the plan
int spread_ensure(ps_engine* e, Drain::Spread::Pass& B, const AudShape& A, const SpreadPlan& P);
// the kernels' arguments over a pass's buffers (entries | strips from o_strips
// in B.d_in), adding into the block `out`; n_edges: what an index into the
// child lists is checked against
SpreadArgs spread_args(ps_engine* e, const Drain::Spread::Pass& B, size_t o_strips, size_t n, const AudShape& A,
                       const SpreadPlan& P, uint32_t n_edges, uint64_t* out, const SpreadOut& O);
// classify's arguments over the same buffers
AudArgs spread_classify_args(ps_engine* e, const SpreadArgs& p, const Drain::Spread::Pass& B);
inline uint32_t spread_level_blocks(const SpreadPlan& P) {
  return std::min<uint32_t>(std::max<uint32_t>(ceil_div(P.n_nodes, 256), 1), kSpreadGridMax);
}

}  // namespace psamd
