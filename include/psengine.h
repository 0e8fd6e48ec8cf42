/*
 * psengine.h -- C ABI of the MI355X subtree-dissemination engine.
 *
 * Drop-in boundary for the one hot path of go-libp2p-pubsub v0: flooding
 * published messages down each topic's subscription tree (subtree.go).
 * Plain C types only (no torch, no HIP types): a cgo shim, ctypes or C++ binds
 * it directly.  Every entry point names the reference interface it replaces.
 *
 * Conventions:
 *  - return codes: 0 = PS_OK, negative = PS_E_*; the cgo shim turns a negative
 *    code plus ps_last_error() into a Go `error`.
 *  - caller arrays are borrowed for the duration of the call and copied;
 *    the engine owns all device memory.
 *  - an engine is NOT thread-safe; the caller serialises calls, as
 *    subtree.chlock does in the reference (subtree.go:18,320).
 *  - peers are dense u32 ids [0, n_peers) standing in for peer.ID
 *    (go-libp2p-peer); messages are u32 publish indices returned by
 *    ps_publish (the reference's Message has no ID, pubsub.go:146-153).
 */
#ifndef PSENGINE_H
#define PSENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_NONE 0xFFFFFFFFu
#define PS_HOP_NONE 0xFFu
#define PS_MAX_ROUNDS 256

enum ps_status {
  PS_OK = 0,
  PS_E_INVAL = -1,       /* bad argument                                        */
  PS_E_NOMEM = -2,       /* host or device allocation failed                    */
  PS_E_STATE = -3,       /* peer/topic in the wrong state for the request       */
  PS_E_NOPARENT = -4,    /* redirectJoin found no live child (subtree.go:172)   */
  PS_E_UNREACHABLE = -5, /* join redirected into a closed host (subtree.go:302) */
  PS_E_DEVICE = -6,      /* HIP runtime error                                   */
  PS_E_RANGE = -7,       /* message id / topic id out of range                  */
  PS_E_NOTREADY = -8     /* no completed run holds the requested record         */
};

/* ps_config.flags */
#define PS_F_RECORD_HOPS 0x1u  /* keep (peer,msg)->hop for ps_read_hops (parity) */
#define PS_F_TIME_KERNELS 0x2u /* HIP-event time every expand launch            */
#define PS_F_NO_LAZY_SEEN 0x4u /* clear the seen bitset eagerly per window      */
#define PS_F_COMPACT 0x8u      /* every window through the compaction path (the
                                  general-graph k_expand rounds), trees too     */

typedef struct ps_config {
  uint32_t n_peers;        /* peer id space [0, n_peers)                       */
  uint32_t n_topics;       /* topic slots [0, n_topics)                        */
  uint32_t tree_width;     /* DefaultTreeWidth  (pubsub.go:16), 0 -> 2         */
  uint32_t tree_max_width; /* DefaultTreeMaxWidth (pubsub.go:17), 0 -> 5       */
  uint32_t msg_window;     /* max messages per topic per window, 0 -> 65536,
                              at most 2^30 (PS_E_INVAL above)                  */
  int32_t device;          /* HIP device ordinal                               */
  uint32_t flags;          /* PS_F_*                                           */
  uint32_t reserved;
  uint64_t seed;           /* redirect tie-break stream (Go map order, Q2)     */
} ps_config;

/* ps_stats.expand_mode: how the last window's rounds ran */
#define PS_MODE_COMPACT 0u     /* k_expand over a compacted frontier (flags + scan) */
#define PS_MODE_LEVEL_PULL 2u  /* k_pull: one launch per round, each level pulls its
                                  parents' rows (start groups, multi-GPU windows) */
#define PS_MODE_FLOOD 3u       /* k_flood for the leading rounds (one persistent
                                  launch, each level pulls its parents' rows once
                                  the tasks writing them have published), then
                                  k_pull per round; see ps_stats.flood_rounds     */

typedef struct ps_stats {
  uint64_t deliveries;         /* (peer,msg) pairs delivered by this run        */
  uint64_t duplicates;         /* bits suppressed by the seen test (0 on trees)  */
  uint64_t frontier_entries;   /* frontier nodes expanded                        */
  uint64_t child_visits;       /* (frontier node, child) pairs                   */
  uint64_t edge_words;         /* (child, 64-message word) pairs tested          */
  uint64_t expand_bytes;       /* algorithmic HBM bytes of the expand kernel     */
  uint64_t windows;            /* propagation windows                            */
  uint64_t rounds;             /* synchronous rounds launched                    */
  uint64_t expand_launches;    /* expand kernel launches                         */
  double run_ms;               /* device time of the whole run (HIP events; a
                                  pipelined one-rank window: its start and
                                  reduce-end device stamps -- a reduce held back
                                  into the next window's first launch, or to
                                  ps_wait, ends there)                          */
  double expand_ms;            /* summed expand-kernel device time (TIME flag)   */
  double host_ms;              /* wall time of the ps_run call                   */
  uint32_t expand_mode;        /* hot kernel of the last window: PS_MODE_*       */
  uint32_t flood_rounds;       /* PS_MODE_FLOOD: leading rounds of the last
                                  window run by k_flood (the rest: k_pull)      */
  uint64_t deliveries_per_round[PS_MAX_ROUNDS];
  float expand_ms_per_round[PS_MAX_ROUNDS];   /* TIME flag, summed over windows  */
  uint32_t frontier_per_round[PS_MAX_ROUNDS]; /* expanded entries per round      */
  uint64_t expand_bytes_per_round[PS_MAX_ROUNDS]; /* algorithmic bytes per round */
  uint8_t round_kernel[PS_MAX_ROUNDS]; /* PS_K_*: the launch kind that wrote each
                                          round of the last window              */
  /* the effective plan of the last window (scheduling diagnostics) */
  uint32_t plan_max_rounds;    /* rounds of its longest launch (1: k_pull, 2: pair,
                                  3..7: chain; k_flood counts as 1)            */
  uint32_t prefix_rounds;      /* leading rounds that may run beside the previous
                                  window (0: none)             */
  uint32_t overlapped;         /* windows of this run whose prefix ran beside
                                  their predecessor                             */
  uint32_t xchg_path;          /* N ranks: PS_XCHG_* of the last window         */
  uint64_t xchg_rounds;        /* N ranks: rounds of this run that exchanged     */
  uint64_t xchg_bytes;         /* N ranks: ghost-record bytes this rank received */
  uint32_t level_aligned;      /* the last window ran level-aligned start groups
                                  (ps_plan_opts.align_groups): round_kernel,
                                  expand_bytes_per_round and expand_ms_per_round
                                  are indexed by launch round = BFS level;
                                  deliveries_per_round / frontier_per_round stay
                                  by round (start + level)                      */
  uint32_t reserved2;
} ps_stats;

/* ps_stats.xchg_path: how a multi-rank level window's ghost records moved */
#define PS_XCHG_NONE 0u       /* one rank, or nothing exchanged                */
#define PS_XCHG_ZERO_COPY 1u  /* read in place from the sender's send region
                                 (loopback ranks sharing one process and GPU)  */
#define PS_XCHG_COPY 2u       /* copied into this rank's receive buffer (RCCL
                                 send/recv; the loopback with PS_DIST_F_COPY)  */
#define PS_XCHG_IN_PLACE 3u   /* ghost parents' rows read where their owner
                                 wrote them (PS_DIST_F_INPLACE); only the topic
                                 roots' rows still move as records            */

/* ps_stats.round_kernel */
#define PS_K_NONE 0u
#define PS_K_FLOOD 1u   /* k_flood (its one launch is timed into round 1)      */
#define PS_K_PULL 2u    /* k_pull, one launch for this round                   */
#define PS_K_PAIR 3u    /* k_pull_pair: this round and the next in one launch   */
#define PS_K_PAIR2 4u   /* k_pull_pair: the second round of the launch above    */
#define PS_K_EXPAND 5u  /* k_expand (compaction mode)                          */
/* PS_K_CHAIN names the plan's launch slot: k_pull_chain, or -- a bulk launch
 * of a single-start window on one rank -- k_fill_reach + k_fill_rows for its
 * whole rows (ps_chain_fill_launches counts those) */
#define PS_K_CHAIN 6u   /* k_pull_chain: this round and the next 2-3 in one launch */
#define PS_K_CHAIN2 7u  /* k_pull_chain: a later round of the launch above      */

typedef struct ps_engine ps_engine;

/* ---- lifecycle: NewTopicManager (pubsub.go:26-31) ------------------------ */
int ps_create(const ps_config* cfg, ps_engine** out);
void ps_destroy(ps_engine* e);
const char* ps_last_error(const ps_engine* e);
const char* ps_version(void);

/* ABI guard.  The public structs' layouts are versioned by PS_ABI_VERSION
 * (5: ps_stats gained the plan diagnostics and xchg fields, ps_dist_config
 * its flags word -- a caller built against an older header would read or
 * write past its own structs).  A binding calls ps_abi_check once, with the
 * sizes it was compiled with (PS_ABI_CHECK() in C/C++); PS_E_INVAL on any
 * mismatch, with ps_last_error(NULL) naming it. */
#define PS_ABI_VERSION 5u
uint32_t ps_abi_version(void);
int ps_abi_check(uint32_t abi_version, size_t config_size, size_t stats_size,
                 size_t plan_opts_size, size_t dist_config_size);
#define PS_ABI_CHECK()                                                        \
  ps_abi_check(PS_ABI_VERSION, sizeof(ps_config), sizeof(ps_stats),           \
               sizeof(struct ps_plan_opts), sizeof(struct ps_dist_config))

/* ---- topics: TopicManager.NewTopic + TreeOpts (pubsub.go:49-97),
 *      Topic.Close (pubsub.go:99-103).  width 0 -> engine default.            */
int ps_topic_create(ps_engine* e, uint32_t topic, uint32_t root,
                    uint32_t tree_width, uint32_t tree_max_width);
int ps_topic_close(ps_engine* e, uint32_t topic);

/* ---- membership, restated on the host (sequential by nature):
 * ps_topic_join:  TopicManager.Subscribe -> joinToPeer -> handleJoin /
 *                 redirectJoin / joinParents (client.go:65-94,
 *                 subtree.go:100-307).  status_out[i] (nullable) gets the
 *                 per-peer PS_* code; the call returns the first failure.
 * ps_topic_leave: client.Close -> Part -> redistributeChildren
 *                 (client.go:30-34, subtree.go:46-98,356-375).
 * ps_topic_drop:  host.Close(): abrupt; the parent notices on its next write
 *                 (subtree.go:333-351); that message is lost below the peer. */
int ps_topic_join(ps_engine* e, uint32_t topic, const uint32_t* peers, size_t n,
                  int32_t* status_out);
int ps_topic_leave(ps_engine* e, uint32_t topic, const uint32_t* peers, size_t n);
int ps_topic_drop(ps_engine* e, uint32_t topic, const uint32_t* peers, size_t n);

/* ---- explicit topology (harness / parity inputs) ---------------------------
 * set_tree:     parent[p] for every peer (PS_NONE = not in the tree); the tree
 *               printTree walks (pubsub_test.go:204-229).
 * set_children: general child lists in peer space (row_ptr[n_peers+1],
 *               col[row_ptr[n_peers]]); a peer may have several parents
 *               (mesh), in which case the seen bitset deduplicates.
 * get_parents:  current attached tree (PS_NONE = not attached / orphaned).   */
int ps_topic_set_tree(ps_engine* e, uint32_t topic, uint32_t root, const uint32_t* parent);
int ps_topic_set_children(ps_engine* e, uint32_t topic, uint32_t root,
                          const uint32_t* row_ptr, const uint32_t* col);
int ps_topic_get_parents(ps_engine* e, uint32_t topic, uint32_t* parent_out);
int ps_topic_depth(ps_engine* e, uint32_t topic, uint32_t* depth_out, uint32_t* n_nodes_out);

/* Replace the engine's PS_F_* flags (e.g. PS_F_TIME_KERNELS for an
 * instrumented run between untimed ones); applies to the next ps_run. */
int ps_set_flags(ps_engine* e, uint32_t flags);

/* ---- launch-plan options ----------------------------------
 * The schedule knobs whose defaults were chosen by measurement (the A/B
 * records under profiles/).  ps_create starts from the defaults; a caller
 * pins or changes them only through ps_set_plan_opts -- the environment does
 * not touch them, except for A/B tools that set PSAMD_AB=1 (then the PSAMD_*
 * variables are read at ps_create).  Plans are rebuilt on the next run. */
typedef struct ps_plan_opts {
  uint64_t flood_top_bytes;    /* k_flood runs the leading rounds that each write at
                                  most this many row bytes (4 MiB)              */
  uint64_t overlap_min_bytes;  /* windows of fewer row bytes never overlap (512 MiB) */
  uint64_t launch_bytes;       /* planner: a launch's ramp and tail, as row bytes (16e6) */
  uint32_t flood;              /* 1: k_flood for a one-rank window's leading rounds (1) */
  uint32_t chain_max;          /* rounds per launch at most, single-start windows:
                                  1 = one k_pull per round, 2 = pairs, 3..6 chains (4) */
  uint32_t chain_max_groups;   /* the same for windows with start groups (6)     */
  uint32_t chain_tail;         /* 1: a chain ending at the last round may take one
                                  round more (1)                                */
  uint32_t chain_words;        /* row words a chain wave writes, planner target (4096) */
  uint32_t flood_words;        /* row words per k_flood task (2048)              */
  uint32_t pad_words;          /* rows of at least this many words padded to even (16) */
  uint32_t overlap;            /* 1: pipelined deep windows overlap their leading
                                  launches with the previous window (1)          */
  uint32_t overlap_min_rounds; /* ... windows of at least this many rounds (12) */
  int32_t xchg_overlap;        /* N ranks: exchange on its own stream beside the
                                  locally fed chunks: -1 auto (RCCL yes, loopback
                                  no), 0, 1 (-1)                                */
  uint32_t gpu_build;          /* 1: rebuild a one-rank node space on the GPU (1) */
  uint32_t flood_spin_ticks;   /* k_flood dependency-wait bound, 100-MHz ticks (2e8) */
  uint32_t chain_nt;           /* 1: chain launches store level 0 and their inner
                                  levels non-temporally, 0: plain stores (1)    */
  uint32_t chain_waves;        /* chain launches: resident waves per CU at most,
                                  1..16 (an LDS pad), 0: as many as fit (12)    */
  uint32_t flood_min_rounds;   /* k_flood only when it would run at least this many
                                  leading rounds; fewer go to chain launches (4) */
  uint32_t align_groups;       /* 1: a one-rank window with start groups (paced
                                  publishing) runs level-aligned -- launch round q
                                  writes BFS level q of every start group, each
                                  group's deliveries counted and recorded in its
                                  own round (start + level) -- instead of one
                                  launch schedule over start + depth rounds (1) */
} ps_plan_opts;

int ps_plan_opts_default(ps_plan_opts* out);
/* effective options of an engine (the defaults, or what ps_set_plan_opts set) */
int ps_get_plan_opts(const ps_engine* e, ps_plan_opts* out);
/* PS_E_INVAL on an out-of-range value; PS_E_STATE with runs in flight */
int ps_set_plan_opts(ps_engine* e, const ps_plan_opts* opts);

/* Subscribed-and-live mask over peers (1 = receives and forwards).  A peer
 * whose client stopped reading (client.go:103-131) is 0. Default: all 1. */
int ps_set_live(ps_engine* e, const uint8_t* live);

/* ---- the hot path ----------------------------------------------------------
 * ps_publish:    Topic.PublishMessage (pubsub.go:111-120) for a batch; message
 *                i of the batch gets id *first_msg_id_out + i.
 * ps_publish_at: same, message i enters its topic root at round start_round[i]
 *                (paced / pipelined publishing; hop = round - start_round).
 * ps_run:        forwardMessage (subtree.go:319-354) + processMessages
 *                (client.go:100-132) for every enqueued message, as
 *                synchronous rounds on the GPU, to quiescence.               */
int ps_publish(ps_engine* e, const uint32_t* topic_of_msg, size_t n_msgs,
               uint32_t* first_msg_id_out);
int ps_publish_at(ps_engine* e, const uint32_t* topic_of_msg, const uint32_t* start_round,
                  size_t n_msgs, uint32_t* first_msg_id_out);
int ps_run(ps_engine* e, ps_stats* out);
/* ps_run in two halves, for pipelined batches: ps_run_async plans and enqueues
 * the run and returns while its last window's kernels execute (at most two runs
 * in flight), so the caller can publish and enqueue the next batch; ps_wait
 * completes the oldest run in flight and returns its stats.  Reads
 * (ps_read_*, ps_seen_digest) and membership changes stay stream-ordered
 * behind the runs in flight; ps_run refuses while any is pending.  (A one-rank
 * run's counter reduce may be held back to ride in the next ps_run_async's
 * first launch; ps_wait launches it itself when no run came first.) */
int ps_run_async(ps_engine* e);
int ps_wait(ps_engine* e, ps_stats* out);

/* ---- results of the last ps_run (client.Messages, client.go:26-28) --------
 * ps_read_hops: hop of message `msg` at every peer (PS_HOP_NONE = not
 *               delivered; hops beyond 254 read as 254); needs PS_F_RECORD_HOPS.
 * ps_read_delivered: 1 where `msg` was delivered (seen bit set), any mode,
 *               for messages of the last window of the last run.            */
int ps_read_hops(ps_engine* e, uint32_t msg, uint8_t* hop_per_peer);
int ps_read_delivered(ps_engine* e, uint32_t msg, uint8_t* delivered_per_peer);
/* ps_read_peer_messages: what one subscriber's client.Messages() channel
 *               (client.go:26-28, fed by processMessages client.go:124-128)
 *               yields for `topic` from the last window of the last run: the
 *               delivered message ids in publish order (a tree path is FIFO,
 *               so publish order is arrival order).  *n_out = count; returns
 *               PS_E_RANGE (with *n_out set) when cap is too small. */
int ps_read_peer_messages(ps_engine* e, uint32_t topic, uint32_t peer, uint32_t* msg_out,
                          size_t cap, size_t* n_out);
/* client.Messages() (client.go:26-28,124-128) for n subscribers at once:
 * query q = (topic[q], peer[q]); its message ids, in the order
 * ps_read_peer_messages gives them, are msg_out[off_out[q] .. off_out[q+1]).
 * off_out has n + 1 entries; *total_out = off_out[n].  When total > cap,
 * off_out and *total_out are still filled, msg_out is untouched and the call
 * returns PS_E_RANGE (msg_out == NULL, cap == 0 is the sizing call).  The
 * rows are turned into id lists on the GPU (one count, one scan, one emit per
 * output slab); queries may repeat, in any order; PS_E_RANGE with nothing
 * written for a topic or peer out of range. */
int ps_drain(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, uint64_t* off_out,
             uint32_t* msg_out, size_t cap, uint64_t* total_out);
/* ps_drain in two halves, for pipelined batches (as ps_run_async / ps_wait).
 * ps_drain_begin answers the same queries as ps_drain for the last window of
 * the last run *enqueued* (ps_run, or ps_run_async whether or not ps_wait has
 * returned for it), and only enqueues: it returns while that run may still
 * be executing.  ps_drain_end completes the oldest drain begun and lends the
 * caller its result: query q's ids are (*msg_out)[(*off_out)[q] ..
 * (*off_out)[q+1]), *off_out has n + 1 entries, *total_out = (*off_out)[n],
 * list for list what ps_drain returns for that window.  Both pointers name
 * pinned memory the engine owns, valid until the next ps_drain_begin or
 * ps_destroy.
 *   At most two drains are outstanding (two slots that alternate): a third
 * ps_drain_begin returns PS_E_STATE; ps_drain_end with none outstanding and
 * ps_drain_begin before any run return PS_E_NOTREADY; a topic or peer out of
 * range returns PS_E_RANGE with nothing enqueued and no slot taken; n == 0 is
 * a valid drain (off = {0}).  The result buffers are sized by an upper bound
 * (the window's message count of each resolvable query's topic, summed); a
 * bound above 2^30 ids returns PS_E_RANGE: use ps_drain, which emits in
 * slabs.  A multi-rank engine returns PS_E_STATE.  A run split into several
 * windows drains its last one, as ps_drain does.  ps_drain_end returns
 * PS_E_STATE when the device-side check of the window's tables failed.  When
 * the ps_wait of the run a drain belongs to fails (a k_flood timeout), the
 * view's content is unspecified.  Every other call stays valid, and
 * stream-ordered as before, while drains are outstanding. */
int ps_drain_begin(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n);
int ps_drain_end(ps_engine* e, const uint64_t** off_out, const uint32_t** msg_out, uint64_t* total_out);
/* ps_drain with equal lists stored once.  Within one window every reached
 * subscriber of a topic receives the same messages in the same order, so the
 * answer is a few lists and one list number per query: query q's ids are list
 * l = list_out[q], msg_out[list_off_out[l] .. list_off_out[l+1]), or nothing
 * when list_out[q] == PS_NONE; expanded, that is ps_drain's answer for q, id
 * for id.  The engine does not assume the equality: it compares every queried
 * row with the topic's window messages on the GPU.  A row that holds all of
 * them takes the topic's shared list (emitted once), a row that holds none
 * takes PS_NONE, any other row takes a list of its own; so do the rows of a
 * mesh topic whose window has several start rounds.  Lists are numbered in
 * the order of the first query that uses them.
 *   list_out has n entries and is always filled; list_off_out has
 * list_cap + 1; *n_lists_out and *total_out (= list_off_out[n_lists]) are
 * always set.  When list_cap < n_lists or cap < total the call returns
 * PS_E_RANGE with msg_out untouched, and list_off_out filled only if list_cap
 * suffices (msg_out == NULL, cap == 0 is the sizing call).  PS_E_RANGE with
 * nothing written for a topic or peer out of range; PS_E_NOTREADY before any
 * run; PS_E_STATE on a multi-rank engine (use ps_drain). */
int ps_drain_shared(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, uint32_t* list_out,
                    uint64_t* list_off_out, size_t list_cap, uint32_t* msg_out, size_t cap,
                    uint32_t* n_lists_out, uint64_t* total_out);
/* ps_drain_shared in two halves, for pipelined batches: ps_drain_shared's
 * answer for the window ps_drain_begin reads (the last window of the last run
 * enqueued), enqueued behind that run with no wait in between -- the lists are
 * numbered and laid out on the GPU.  ps_drain_shared_end completes the oldest
 * drain begun and lends the caller its result: (*list_out)[0 .. n),
 * (*list_off_out)[0 .. *n_lists_out] and (*msg_out)[0 .. *total_out) are entry
 * for entry what ps_drain_shared returns for that window.  The pointers name
 * pinned memory the engine owns, valid until the next ps_drain_begin or
 * ps_drain_shared_begin, or ps_destroy.
 *   The view is sized by caps, since the host cannot know the counts without
 * waiting: at most list_cap lists and id_cap ids.  list_cap == 0 && id_cap ==
 * 0 selects the engine's own: one list per distinct topic among the queries
 * that resolve to a row (one per such query of a mesh topic whose window has
 * several start rounds) and those topics' window message counts, summed --
 * the size of the answer, which no healthy engine exceeds.  An id cap above
 * 2^30 returns PS_E_RANGE: use ps_drain_shared.  When the answer exceeds a
 * cap, no id is emitted and ps_drain_shared_end returns PS_E_RANGE;
 * *list_out and *n_lists_out are exact then, *list_off_out and *total_out are
 * exact if n_lists <= list_cap, and the ids are unspecified.
 *   The two slots are ps_drain_begin's: at most two drains of either kind
 * are outstanding, completed oldest first, each by the end call of its kind
 * (the other returns PS_E_STATE and completes nothing).  A third begin
 * returns PS_E_STATE; an end with none outstanding and a begin before any run
 * return PS_E_NOTREADY; a topic or peer out of range returns PS_E_RANGE with
 * nothing enqueued and no slot taken; n == 0 is a valid drain (no list,
 * list_off = {0}); a multi-rank engine returns PS_E_STATE;
 * ps_drain_shared_end returns PS_E_STATE when the device-side check of the
 * window's tables failed. */
int ps_drain_shared_begin(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, size_t list_cap,
                          size_t id_cap);
int ps_drain_shared_end(ps_engine* e, const uint32_t** list_out, const uint64_t** list_off_out,
                        const uint32_t** msg_out, uint32_t* n_lists_out, uint64_t* total_out);
/* The sink: standing queries the engine drains itself behind EVERY window of
 * a run, into one answer per run (every read above answers for the last
 * window of the last run only; a run has several windows when a topic exceeds
 * msg_window or after ps_topic_drop).
 *   ps_sink_set registers the n queries (topic[q], peer[q]) -- repeats and any
 * order allowed, the arrays are copied; n == 0 clears the sink (the pointers
 * may be NULL).  A topic or peer out of range returns PS_E_RANGE and the
 * previous sink stays.  PS_E_STATE with a run in flight and on a multi-rank
 * engine; ps_dist_init* on an engine whose sink is set returns PS_E_STATE.
 * Setting or clearing discards results not yet taken, and replaces or clears
 * a topics sink too (ps_sink_set_topics below): an engine has one sink.
 *   While a sink is set, every window of every ps_run / ps_run_async enqueues
 * behind itself the shared drain of ps_drain_shared_begin for the standing
 * queries, resolved against the node space that window ran on, and the run's
 * windows accumulate: win_list[w * n + q] is query q's list in window w or
 * PS_NONE, the lists numbered run-wide in order of first use (window by
 * window, within a window as ps_drain_shared numbers them); list l is
 * msg[list_off[l] .. list_off[l + 1]), total = list_off[n_lists].  Window by
 * window this is entry for entry ps_drain_shared's answer for that window,
 * the list numbers shifted by the lists of the windows before, the ids dense.
 * Query q's deliveries of the run are its lists concatenated in window
 * order, which is arrival order.  Windows that run nothing do not count; a
 * run without a window gives n_windows = 0.
 *   Caps as ps_drain_shared_begin's, for the run: both zero selects the
 * engine's own, summed over the run's windows (a run whose answer may pass
 * 2^30 ids returns PS_E_RANGE from ps_run / ps_run_async, the messages left
 * pending).  When the answer exceeds a cap no further id is emitted and
 * ps_sink_take returns PS_E_RANGE; win_list, n_windows and n_lists are exact
 * then, list_off and total are exact if n_lists <= list_cap.
 *   ps_sink_take completes the oldest untaken run's result (one event wait)
 * and lends it from pinned memory; PS_E_NOTREADY with none outstanding,
 * PS_E_STATE when a window's device-side table check failed.  Two result
 * slots alternate: a view stays valid until the second run enqueued after
 * its own, the next ps_sink_set or ps_destroy; with both untaken, ps_run /
 * ps_run_async return PS_E_STATE before touching the pending messages.  A
 * run that fails gives up its slot; after a failed ps_wait that run's result
 * is unspecified.  The slots are the sink's own: ps_drain_begin and
 * ps_drain_shared_begin keep theirs. */
int ps_sink_set(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, size_t list_cap, size_t id_cap);
int ps_sink_take(ps_engine* e, const uint32_t** win_list_out, const uint64_t** list_off_out, const uint32_t** msg_out,
                 uint32_t* n_windows_out, uint32_t* n_lists_out, uint64_t* total_out);
/* A topic's whole audience, with no query per subscriber: who received what in
 * the last window of the last run, for the n distinct topics named.  Within a
 * window every reached subscriber of a topic holds the same list (the engine
 * checks this on the GPU, as ps_drain_shared does), so the answer per topic is
 * one list, the number of nodes that hold it, and the few that do not.
 *   Let Q be the peers of every non-root node of topic[i] in the node space
 * the window ran on, in ascending node (breadth-first) order, and A be
 * ps_drain_shared's answer for the queries (topic[i], Q).  Then n_nodes[i] =
 * |Q|; topic_list[i] is the list every message of the topic in the window, in
 * arrival order, or PS_NONE when no row holds it (an idle topic, a topic no
 * node of which was reached, a mesh topic whose window has several start
 * rounds); n_full[i] counts the queries of Q that A gives that list; the
 * others are the exceptions exc_off[i] .. exc_off[i+1], in Q's order:
 * exc_peer is the peer, exc_list is PS_NONE where A gives PS_NONE and else a
 * private list with the ids A gives.  A topic with no message in the window
 * has n_full = 0 and no exception (nothing was sent, nobody missed anything);
 * every other topic has n_full[i] + exc_off[i+1] - exc_off[i] == n_nodes[i].
 * Lists are numbered in request order, a topic's shared list (if any) before
 * the private lists of its exceptions in their order; list l is
 * msg[list_off[l] .. list_off[l+1]), total = list_off[n_lists].
 *   Subscribed peers that are not in the node space -- unattached peers and
 * orphans, for which ps_topic_get_parents gives PS_NONE -- are not part of the
 * answer, as in every other read.
 *   The call blocks and needs no sizing call: the arrays are lent from host
 * memory the engine owns, valid until the next ps_drain_topics or ps_destroy.
 * PS_E_INVAL for a NULL output, n > 0 without topic, or a topic named twice;
 * PS_E_RANGE with nothing written for a topic out of range, and when the
 * lists exceed what one drain call holds; PS_E_NOTREADY before any run;
 * PS_E_STATE on a multi-rank engine.  n == 0 is valid: exc_off = {0},
 * list_off = {0}. */
int ps_drain_topics(ps_engine* e, const uint32_t* topic, size_t n,
                    const uint32_t** topic_list_out,  /* [n]                 */
                    const uint64_t** n_nodes_out,     /* [n]                 */
                    const uint64_t** n_full_out,      /* [n]                 */
                    const uint64_t** exc_off_out,     /* [n + 1]             */
                    const uint32_t** exc_peer_out,    /* [exc_off[n]]        */
                    const uint32_t** exc_list_out,    /* [exc_off[n]]        */
                    const uint64_t** list_off_out,    /* [n_lists + 1]       */
                    const uint32_t** msg_out,         /* [total]             */
                    uint32_t* n_lists_out, uint64_t* total_out);
/* ps_drain_topics in two halves, for pipelined batches: ps_drain_topics'
 * answer for the window ps_drain_begin reads (the last window of the last run
 * enqueued, whether or not ps_wait has returned for it), enqueued behind that
 * run with no wait in between -- the per-topic totals and the list numbering
 * are computed on the GPU.  ps_drain_topics_end completes the oldest drain
 * begun and lends the ten outputs from pinned memory the engine owns, entry
 * for entry what ps_drain_topics returns for that window; they stay valid
 * until the next begin call of any kind, or ps_destroy.
 *   The view is sized by caps, since the host cannot know the counts without
 * waiting: at most exc_cap exception records, list_cap lists and id_cap ids.
 * A cap of zero selects the engine's own (all three zero: the engine's caps):
 * exc_cap = the non-root nodes of the named topics that have window messages,
 * 65,536 at most; list_cap = one list per named topic with window messages
 * plus one per non-root node of a named mesh topic whose window has several
 * start rounds; id_cap = those lists' window message counts, summed -- the
 * size of the answer while every reached row is full.  An id cap above 2^30
 * returns PS_E_RANGE, as does list_cap x the widest named topic's segments at
 * or above 2^31 - 1: use ps_drain_topics.  When the answer exceeds a cap
 * nothing is written past it, no id is emitted and ps_drain_topics_end
 * returns PS_E_RANGE; n_nodes, n_full and exc_off are exact then, whatever
 * the caps (retry with exc_cap = exc_off[n]), exc_peer and exc_list are exact
 * for the records below exc_cap, and *n_lists_out, list_off and *total_out are
 * exact when the exceptions and the lists fit.
 *   The two slots are ps_drain_begin's: at most two drains of any kind are
 * outstanding, completed oldest first, each by the end call of its kind (the
 * others return PS_E_STATE and complete nothing).  A third begin returns
 * PS_E_STATE; an end with none outstanding and a begin before any run return
 * PS_E_NOTREADY.  PS_E_INVAL for a NULL output, n > 0 without topic, or a
 * topic named twice; PS_E_RANGE for a topic out of range, with nothing
 * enqueued and no slot taken; PS_E_STATE on a multi-rank engine; n == 0 is a
 * valid drain; ps_drain_topics_end returns PS_E_STATE when the device-side
 * check of the window's tables failed. */
int ps_drain_topics_begin(ps_engine* e, const uint32_t* topic, size_t n, size_t exc_cap, size_t list_cap,
                          size_t id_cap);
int ps_drain_topics_end(ps_engine* e,
                        const uint32_t** topic_list_out,  /* [n]                 */
                        const uint64_t** n_nodes_out,     /* [n]                 */
                        const uint64_t** n_full_out,      /* [n]                 */
                        const uint64_t** exc_off_out,     /* [n + 1]             */
                        const uint32_t** exc_peer_out,    /* [min(exc_off[n], exc_cap)] */
                        const uint32_t** exc_list_out,    /* [min(exc_off[n], exc_cap)] */
                        const uint64_t** list_off_out,    /* [n_lists + 1]       */
                        const uint32_t** msg_out,         /* [total]             */
                        uint32_t* n_lists_out, uint64_t* total_out);
/* The audience sink: standing TOPICS the engine drains itself behind EVERY
 * window of a run, as ps_drain_topics does, into one answer per run -- what
 * ps_sink_set is to ps_drain_shared, for ps_drain_topics.
 *   ps_sink_set_topics registers the n distinct topics (copied; n == 0 clears
 * the sink, topic may be NULL then).  An engine has one sink, of one kind:
 * with n > 0 this call replaces a query sink and ps_sink_set replaces a
 * topics sink; either call discards results not yet taken, and either with
 * n == 0 clears whatever sink is set.  PS_E_INVAL for n > 0 without topic or a
 * topic named twice, PS_E_RANGE for a topic out of range (the previous sink
 * stays in both cases); PS_E_STATE with a run in flight and on a multi-rank
 * engine; ps_dist_init* on an engine whose sink is set returns PS_E_STATE.
 *   While the sink is set, every window of every ps_run / ps_run_async
 * enqueues behind itself ps_drain_topics_begin's passes over the standing
 * topics, against the node space that window ran on, and the run's windows
 * accumulate.  Entry (w, i) lies at index w * n + i: n_nodes, n_full and
 * topic_list are window w's values for topic[i], a topic_list entry shifted
 * by the lists of the windows before (PS_NONE stays).  exc_off is ONE
 * cumulative array over the run: the exceptions of (w, i) are records
 * exc_off[w * n + i] .. exc_off[w * n + i + 1], dense, in window order, then
 * request order, then node order; exc_list is shifted like topic_list.  Lists
 * are numbered run-wide, window by window, within a window as ps_drain_topics
 * numbers them; list l is msg[list_off[l] .. list_off[l + 1]), total =
 * list_off[n_lists].  A topic with no message in a window has n_full = 0, no
 * exception and PS_NONE in that window's row.  A topic's deliveries of the
 * run are its windows' lists in window order, which is arrival order.
 * Windows that run nothing do not count; a run without a window gives
 * n_windows = 0, exc_off = {0}, list_off = {0}.
 *   Caps as ps_drain_topics_begin's three, for the run: a cap of zero selects
 * the engine's own -- that call's own cap of each window, summed as the
 * windows come (exc_cap: the non-root nodes of the named topics with window
 * messages, 65,536 at most, per window).  ps_run / ps_run_async return
 * PS_E_RANGE before touching the pending messages when the engine's id cap
 * for the run may pass 2^30.  Overflow is sticky: from the first window whose
 * answer passes a cap no id is emitted and ps_sink_take_topics returns
 * PS_E_RANGE; n_windows, n_nodes, n_full and exc_off are exact then for every
 * window, whatever the caps (retry with exc_cap = exc_off[n_windows * n]);
 * exc_peer, exc_list, topic_list, n_lists, list_off and total are exact for
 * the windows before the first that overflowed and unspecified from there
 * on.  Nothing is stored past a cap.
 *   ps_sink_take_topics completes the oldest untaken run's result and lends
 * it from pinned memory.  The two result slots, the PS_E_STATE refusal of a
 * run with both untaken, the view lifetime and "a failed run gives up its
 * slot" are ps_sink_set's.  The take call of the other kind returns
 * PS_E_STATE and completes nothing.  PS_E_INVAL for a NULL output;
 * PS_E_NOTREADY with nothing outstanding; PS_E_STATE when a window's
 * device-side table check failed. */
int ps_sink_set_topics(ps_engine* e, const uint32_t* topic, size_t n, size_t exc_cap, size_t list_cap, size_t id_cap);
int ps_sink_take_topics(ps_engine* e,
                        const uint32_t** topic_list_out,  /* [n_windows * n]      */
                        const uint64_t** n_nodes_out,     /* [n_windows * n]      */
                        const uint64_t** n_full_out,      /* [n_windows * n]      */
                        const uint64_t** exc_off_out,     /* [n_windows * n + 1]  */
                        const uint32_t** exc_peer_out,    /* [min(exc_off[last], exc_cap)] */
                        const uint32_t** exc_list_out,    /* same                 */
                        const uint64_t** list_off_out,    /* [n_lists + 1]        */
                        const uint32_t** msg_out,         /* [total]              */
                        uint32_t* n_windows_out, uint32_t* n_lists_out, uint64_t* total_out);
/* Per-peer load: how much each peer carried, summed over the named topics (one
 * rank).  Per window and per topic t with c_t > 0 messages in
 * it, on the node space that window ran on: a non-root node of peer p whose
 * row holds k of t's window messages -- the k ids ps_drain_shared would list
 * for (t, p); 0 for a tree node the window did not reach -- adds k to recv[p]
 * and k * deg to sent[p], deg its children in the topic's tree (or mesh: a
 * mesh node forwards each message once, on first receipt).  The root is no
 * recipient: it adds nothing to recv and c_t * deg(root) to sent.  Children
 * count whether live or not: the parent writes to them, as forwardMessage
 * does.  A topic with no message in the window adds nothing; peers outside the
 * node space (unattached, orphans) get nothing, as in every other read.
 *   ps_peer_load answers for the last window of the last run, blocking, with
 * ps_drain_topics' window, stream-ordering and twin-join rules.  The n topics
 * are distinct; both arrays ([n_peers], either may be NULL) are written in
 * full: peers in no named topic read 0, and n == 0 gives all zeros.
 * PS_E_INVAL for a NULL engine, n > 0 without topic, both outputs NULL or a
 * topic named twice; PS_E_RANGE, nothing written, for a topic out of range;
 * PS_E_NOTREADY before any run; PS_E_STATE on a multi-rank engine.
 *   ps_load_track registers n standing topics (copied; n == 0 clears the
 * tracking and frees the totals).  PS_E_INVAL / PS_E_RANGE as above, the
 * previous tracking stays; PS_E_STATE with a run in flight and on a
 * multi-rank engine; ps_dist_init* on an engine that is tracking returns
 * PS_E_STATE.  Setting or clearing zeroes the totals.  Tracking is
 * independent of the sinks: an engine may have a sink and tracking at once.
 * While it is set, every window of every ps_run / ps_run_async that runs
 * something enqueues the pass behind itself -- the window is neither planned
 * nor launched differently -- and the pass adds into two totals on the
 * device, recv[n_peers] and sent[n_peers], in peer space: they survive
 * node-space rebuilds, joins, leaves and drops between windows.
 *   ps_load_take waits for the passes enqueued so far, copies the totals since
 * the last take or track call (each array may be NULL), zeroes them in front
 * of whatever runs next, sets *n_windows_out to the windows counted and
 * resets that count.  PS_E_NOTREADY when nothing is tracked; PS_E_STATE with
 * a run in flight (complete the runs with ps_wait first); PS_E_INVAL for a
 * NULL engine or n_windows_out.  After a failed ps_run / ps_wait the totals
 * are unspecified until the next take or track call. */
int ps_peer_load(ps_engine* e, const uint32_t* topic, size_t n,
                 uint64_t* recv_out, uint64_t* sent_out);          /* [n_peers] each, either may be NULL */
int ps_load_track(ps_engine* e, const uint32_t* topic, size_t n);
int ps_load_take(ps_engine* e, uint64_t* recv_out, uint64_t* sent_out, /* [n_peers], nullable */
                 uint64_t* n_windows_out);
/* Deliveries by hop per topic: how deep a topic's messages travel (one rank;
 * DESIGN.md 5.5j).  Per window and per named tree topic t with c_t > 0
 * messages in it, on the node space that window ran on: a non-root node u has
 * BFS level d(u) in [1, depth_t], and its row holds k(u) of t's window
 * messages -- ps_peer_load's k: 0 for a tree node the window did not reach.
 * Column h = min(d(u), PS_MAX_ROUNDS - 1) of the topic's row gets
 *   nodes[h] += 1, reached[h] += (k(u) > 0), deliv[h] += k(u).
 * On a tree the path is unique: every message a node receives arrives at hop
 * d(u), whatever its start round (ps_publish_at: hop = round - start), so
 * deliv[h] is the topic's deliveries at hop h.  Column 0 stays 0: the root is
 * no recipient.  The last column collects hop PS_MAX_ROUNDS - 1 and more, so
 * row sums stay exact for trees deeper than the array.  A topic with no
 * message in the window adds nothing, not even nodes; peers outside the node
 * space add nothing: both as in ps_peer_load.
 *   Mesh topics are refused: a mesh node's hop is its first-arrival round,
 * which no row records.  A tree topic that shares a window with a mesh is
 * answered as any other.
 *   ps_topic_hops answers for the last window of the last run, blocking, with
 * ps_peer_load's window, stream-ordering and twin-join rules.  The n topics
 * are distinct; row i of each array ([n * PS_MAX_ROUNDS]; any may be NULL, not
 * all three) belongs to topic[i] and is written in full: unused columns and
 * idle topics read 0.  n == 0 is valid and writes nothing.  PS_E_INVAL for a
 * NULL engine, n > 0 without topic, all three outputs NULL or a topic named
 * twice; PS_E_RANGE, nothing written, for a topic out of range; PS_E_NOTREADY
 * before any run; PS_E_STATE, nothing written, on a multi-rank engine, when a
 * named topic is a mesh in that window's node space, and for a topic that was
 * set anew over another kind since the window (its levels are gone: run first).
 *   ps_hops_track registers n standing topics (copied; n == 0 clears the
 * tracking and frees the totals).  PS_E_INVAL / PS_E_RANGE as above, and
 * PS_E_STATE for a topic whose child lists make a mesh: the previous tracking
 * stays.  PS_E_STATE with a run in flight and on a multi-rank engine;
 * ps_dist_init* on an engine that is tracking hops returns PS_E_STATE.
 * Setting or clearing zeroes the totals.  Tracking is independent of both
 * sinks and of ps_load_track: all three may be set at once.  While it is set,
 * every window of every ps_run / ps_run_async that runs something enqueues
 * the pass behind itself -- the window is neither planned nor launched
 * differently -- and the pass adds into three totals on the device,
 * [n][PS_MAX_ROUNDS] each, indexed by request position: they survive
 * node-space rebuilds, joins, leaves and drops between windows.  A tracked
 * topic that is a mesh in a window's node space adds nothing for that window;
 * each such (topic, window) pair is counted.
 *   ps_hops_take waits for the passes enqueued so far, copies the totals since
 * the last take or track call (each array may be NULL), zeroes them in front
 * of whatever runs next, sets *n_windows_out to the windows counted and
 * *n_skipped_out to the (mesh topic, window) pairs left out, and resets both
 * counts.  PS_E_NOTREADY when nothing is tracked; PS_E_STATE with a run in
 * flight (complete the runs with ps_wait first); PS_E_INVAL for a NULL engine
 * or count pointer.  After a failed ps_run / ps_wait the totals are
 * unspecified until the next take or track call. */
int ps_topic_hops(ps_engine* e, const uint32_t* topic, size_t n,
                  uint64_t* nodes_out, uint64_t* reached_out, uint64_t* deliv_out);
                  /* [n * PS_MAX_ROUNDS] each, row i = topic[i]; any may be NULL, not all three */
int ps_hops_track(ps_engine* e, const uint32_t* topic, size_t n);
int ps_hops_take(ps_engine* e, uint64_t* nodes_out, uint64_t* reached_out, uint64_t* deliv_out,
                 /* [n_tracked * PS_MAX_ROUNDS], nullable */
                 uint64_t* n_windows_out, uint64_t* n_skipped_out);
/* The audience behind each peer: how many subscribers hang below it, and how
 * many of the window's deliveries went through it and would have been lost
 * had it dropped (one rank).  Per window and per named tree
 * topic t with c_t > 0 messages in it, on the node space that window ran on:
 * every node v carries k(v), ps_peer_load's k -- the number of t's window
 * messages its row holds; 0 for a tree node the window did not reach -- and
 * k(root) counts as 0: the root is no recipient.  For every node u of peer p,
 * the root included:
 *   below[p]   += |{v : v a strict descendant of u}|
 *   carried[p] += the sum of k(v) over the strict descendants v of u.
 * Descendants count whether live or not, as children do in ps_peer_load: an
 * unreached subtree adds to below and nothing to carried.  A topic with no
 * message in the window adds nothing, not even to below; peers outside the
 * node space add nothing: both as in ps_peer_load and ps_topic_hops.
 *   Three identities follow.  carried[root_t] is topic t's deliveries of the
 * window, and below[root_t] is n_nodes - 1.  For one named topic, the sum of
 * below over the peers is the sum over h of h * nodes[h], and the sum of
 * carried is the sum over h of h * deliv[h], nodes and deliv being
 * ps_topic_hops' rows: a node at level h lies below h nodes.  The last two
 * hold while the tree is at most PS_MAX_ROUNDS - 2 levels deep, so that
 * ps_topic_hops' clamped last column is unused; below and carried themselves
 * are exact at any depth.
 *   Mesh topics are refused: a DAG has no subtrees.  A tree topic that shares
 * a window with a mesh is answered as any other.
 *   ps_peer_downstream answers for the last window of the last run, blocking,
 * with ps_peer_load's window, stream-ordering and twin-join rules.  The n
 * topics are distinct; both arrays ([n_peers], either may be NULL) are written
 * in full: peers in no named topic read 0, and n == 0 gives all zeros.
 * PS_E_INVAL for a NULL engine, n > 0 without topic, both outputs NULL or a
 * topic named twice; PS_E_RANGE, nothing written, for a topic out of range;
 * PS_E_NOTREADY before any run; PS_E_STATE, nothing written, on a multi-rank
 * engine, when a named topic is a mesh in that window's node space, and for a
 * topic that was set anew over another kind since the window (its levels are
 * gone: run first).
 *   ps_downstream_track registers n standing topics (copied; n == 0 clears the
 * tracking and frees the totals).  PS_E_INVAL / PS_E_RANGE as above, and
 * PS_E_STATE for a topic whose child lists make a mesh: the previous tracking
 * stays.  PS_E_STATE with a run in flight and on a multi-rank engine;
 * ps_dist_init* on an engine that is tracking downstream returns PS_E_STATE.
 * Setting or clearing zeroes the totals.  Tracking is independent of both
 * sinks, of ps_load_track and of ps_hops_track: all may be set at once.  While
 * it is set, every window of every ps_run / ps_run_async that runs something
 * enqueues the pass behind itself -- the window is neither planned nor
 * launched differently -- and the pass adds into two totals on the device,
 * below[n_peers] and carried[n_peers], in peer space: they survive node-space
 * rebuilds, joins, leaves and drops between windows.  Over several windows
 * below is a sum of per-window values: a peer with s nodes below it in each of
 * w windows reads w * s.  A tracked topic that is a mesh in a window's node
 * space adds nothing for that window; each such (topic, window) pair is
 * counted.
 *   ps_downstream_take waits for the passes enqueued so far, copies the totals
 * since the last take or track call (each array may be NULL), zeroes them in
 * front of whatever runs next, sets *n_windows_out to the windows counted and
 * *n_skipped_out to the (mesh topic, window) pairs left out, and resets both
 * counts.  PS_E_NOTREADY when nothing is tracked; PS_E_STATE with a run in
 * flight (complete the runs with ps_wait first); PS_E_INVAL for a NULL engine
 * or count pointer.  After a failed ps_run / ps_wait the totals are
 * unspecified until the next take or track call. */
int ps_peer_downstream(ps_engine* e, const uint32_t* topic, size_t n,
                       uint64_t* below_out, uint64_t* carried_out);   /* [n_peers] each, either may be NULL */
int ps_downstream_track(ps_engine* e, const uint32_t* topic, size_t n);
int ps_downstream_take(ps_engine* e, uint64_t* below_out, uint64_t* carried_out, /* [n_peers], nullable */
                       uint64_t* n_windows_out, uint64_t* n_skipped_out);
/* Losses blamed on their cut points: after a live mask, a drop or churn, what
 * was not delivered and at which peer the tree was cut (one rank; DESIGN.md
 * 5.5l).  Per window and per named tree topic t with c_t > 0 messages in it,
 * on the node space that window ran on: every node v carries k(v),
 * ps_peer_load's k -- the number of t's window messages its row holds; 0 for a
 * tree node the window did not reach -- and the root counts as full, k(root) =
 * c_t: it is the source.  miss(v) = c_t - k(v), 0 for the root.  A non-root
 * node u is a cut point when k(u) < c_t and its parent is full; T(u) is u
 * together with its strict descendants.  Four sums in peer space:
 *   missed[p]   += miss(v) for every node v of peer p: what p itself did not get
 *   cuts[p]     += 1 for every cut point u of p
 *   orphaned[p] += |T(u)| - 1 for every cut point u of p: the subscribers cut
 *                  off behind it, live or not, as in ps_peer_downstream's below
 *   lost[p]     += the sum of miss(v) over v in T(u) for every cut point u of
 *                  p, that is c_t * |T(u)| - the sum of k(v) over T(u): the
 *                  deliveries that did not happen because the tree was cut at
 *                  u, u's own included.
 * A topic with no message in the window adds nothing; peers outside the node
 * space add nothing: both as in ps_peer_load, ps_topic_hops and
 * ps_peer_downstream.
 *   Four identities follow.  (1) For the named topics, the sum of missed over
 * the peers is the sum over t of c_t * (n_nodes_t - 1) - deliveries_t.  (2) The
 * sum of lost equals the sum of missed: a tree node's row is a subset of its
 * parent's row, so every node with a miss lies in exactly one cut point's
 * T(u).  (3) In a window where every row is full or empty -- every tree window
 * of a healthy engine -- a cut point u of peer p, the only one of p in a single
 * named topic, gives lost[p] = c_t * (1 + orphaned[p]), orphaned[p] = below[p]
 * and carried[p] = 0, below and carried being ps_peer_downstream's.  (4) Under
 * an all-live mask all four arrays are zero.
 *   Mesh topics are refused: a DAG has no subtrees.  A tree topic that shares
 * a window with a mesh is answered as any other.
 *   ps_peer_cut answers for the last window of the last run, blocking, with
 * ps_peer_load's window, stream-ordering and twin-join rules.  The n topics
 * are distinct; the arrays ([n_peers] each, any may be NULL, not all four) are
 * written in full: peers in no named topic read 0, and n == 0 gives all zeros.
 * PS_E_INVAL for a NULL engine, n > 0 without topic, all outputs NULL or a
 * topic named twice; PS_E_RANGE, nothing written, for a topic out of range;
 * PS_E_NOTREADY before any run; PS_E_STATE, nothing written, on a multi-rank
 * engine, when a named topic is a mesh in that window's node space, and for a
 * topic that was set anew over another kind since the window (its levels are
 * gone: run first).
 *   ps_cut_track registers n standing topics (copied; n == 0 clears the
 * tracking and frees the totals).  PS_E_INVAL / PS_E_RANGE as above, and
 * PS_E_STATE for a topic whose child lists make a mesh: the previous tracking
 * stays.  PS_E_STATE with a run in flight and on a multi-rank engine;
 * ps_dist_init* on an engine that is tracking cut points returns PS_E_STATE.
 * Setting or clearing zeroes the totals.  Tracking is independent of both
 * sinks, of ps_load_track, of ps_hops_track and of ps_downstream_track: all
 * may be set at once.  While it is set, every window of every ps_run /
 * ps_run_async that runs something enqueues the pass behind itself -- the
 * window is neither planned nor launched differently -- and the pass adds into
 * four totals on the device, [n_peers] each, in peer space: they survive
 * node-space rebuilds, joins, leaves and drops between windows.  A tracked
 * topic that is a mesh in a window's node space adds nothing for that window;
 * each such (topic, window) pair is counted.
 *   ps_cut_take waits for the passes enqueued so far, copies the totals since
 * the last take or track call (each array may be NULL), zeroes them in front
 * of whatever runs next, sets *n_windows_out to the windows counted and
 * *n_skipped_out to the (mesh topic, window) pairs left out, and resets both
 * counts.  PS_E_NOTREADY when nothing is tracked; PS_E_STATE with a run in
 * flight (complete the runs with ps_wait first); PS_E_INVAL for a NULL engine
 * or count pointer.  After a failed ps_run / ps_wait the totals are
 * unspecified until the next take or track call. */
int ps_peer_cut(ps_engine* e, const uint32_t* topic, size_t n,
                uint64_t* missed_out, uint64_t* cuts_out,
                uint64_t* orphaned_out, uint64_t* lost_out);   /* [n_peers] each; any may be NULL, not all four */
int ps_cut_track(ps_engine* e, const uint32_t* topic, size_t n);
int ps_cut_take(ps_engine* e, uint64_t* missed_out, uint64_t* cuts_out,
                uint64_t* orphaned_out, uint64_t* lost_out,     /* [n_peers], nullable */
                uint64_t* n_windows_out, uint64_t* n_skipped_out);
/* Each missed subscriber and its cut point: "subscriber X did not get the
 * window's messages: where was its path cut, and how far up?" (one rank, tree
 * topics, the last window of the last run, blocking).
 * ps_drain_topics lists who missed, ps_peer_cut sums per cut point; these two
 * calls join a missed subscriber to the peer to blame.  Per named tree topic t
 * with c_t > 0 window messages, on the node space that window ran on: k(u) is
 * ps_peer_cut's k and the root counts as full; miss(u) = c_t - k(u), 0 for
 * the root; a cut point is a non-root node with k < c_t whose parent is full
 * -- ps_peer_cut's definition, word for word.  For a non-root node u with
 * miss(u) > 0, cut(u) is the nearest cut point on the path from u up to the
 * root, u itself included: u if its parent is full, and else cut(parent(u)).
 * This is well defined without assuming that a row is a subset of its
 * parent's: the walk ends at the root's child at the latest.  hop(u) is u's
 * BFS level, cut_hop(u) the level of cut(u): exact uint32_t values, with no
 * clamp at PS_MAX_ROUNDS.
 *   ps_topic_blame: the records of topic[i] are rec_off[i] .. rec_off[i+1],
 * total = rec_off[n]; one record per non-root node with miss > 0, in
 * ascending node (breadth-first) order -- for a tree topic entry for entry the
 * order and the set of ps_drain_topics' exceptions for the same request.  A
 * record holds the node's peer, the peer of cut(u), hop(u), cut_hop(u) and
 * miss(u).  A topic with no message in the window has no records.  The arrays
 * are lent from pinned memory the engine owns, as ps_drain_topics lends its
 * own, valid until the next ps_topic_blame or ps_destroy.  Any of the five
 * record pointers may be NULL: that array is neither copied nor lent.
 * rec_off_out and total_out are required.  PS_E_INVAL for a NULL engine,
 * rec_off_out or total_out NULL, n > 0 without topic, or a topic named twice;
 * PS_E_RANGE, nothing written, for a topic out of range; PS_E_NOTREADY before
 * any run; PS_E_STATE, nothing written, on a multi-rank engine, when a named
 * topic is a mesh in that window's node space, and for a topic that was set
 * anew over another kind since the window.  n == 0 is valid: rec_off = {0},
 * total 0.  Window, stream-ordering and twin-join rules as ps_peer_load's.
 *   ps_blame gives the same facts for n explicit (topic, peer) queries, which
 * may repeat and come in any order; the topics need not be distinct.  A query
 * whose peer is the root or holds a full row gets cut_peer = cut_hop =
 * PS_NONE, missed = 0 and hop = its level; so does every query of a topic
 * with no message in the window.  A peer outside the topic's node space
 * (unattached or orphan) gets PS_NONE in cut_peer, hop and cut_hop, and missed
 * = 0.  Any of the four outputs may be NULL, not all four; those given are
 * written in full.  Errors as ps_topic_blame's (repeats are no error), with
 * PS_E_RANGE, nothing written, for a topic or peer out of range and
 * PS_E_STATE if any queried topic is a mesh.
 *   ps_blame_track / ps_blame_take below give ps_topic_blame's records behind
 * every window of every run.  What remains missing is said of ps_blame's
 * explicit queries: There is no tracker and no _begin / _end form of them.
 * ps_topic_blame has no _begin / _end form either, and its tracker is for one
 * rank only. */
int ps_topic_blame(ps_engine* e, const uint32_t* topic, size_t n,
                   const uint64_t** rec_off_out,      /* [n + 1]          */
                   const uint32_t** rec_peer_out,     /* [total] each     */
                   const uint32_t** rec_cut_peer_out,
                   const uint32_t** rec_hop_out,
                   const uint32_t** rec_cut_hop_out,
                   const uint32_t** rec_missed_out,
                   uint64_t* total_out);
int ps_blame(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n,
             uint32_t* cut_peer_out, uint32_t* hop_out,
             uint32_t* cut_hop_out, uint32_t* missed_out);   /* [n] each */
/* ps_topic_blame's records behind every window, not the last one alone (one
 * rank).  ps_blame_track registers n standing tree topics
 * (distinct; the list is copied), as ps_cut_track registers its own: n == 0
 * clears the tracking and frees its buffers; PS_E_INVAL for a NULL engine,
 * n > 0 without topic or a topic named twice, PS_E_RANGE for a topic out of
 * range or rec_cap above 2^30, PS_E_STATE for a topic whose child lists make a
 * mesh, PS_E_NOMEM when the record arrays cannot be allocated -- the previous
 * tracking stays on each of these --, and PS_E_STATE with a run in flight and
 * on a multi-rank engine (ps_dist_init* on an engine that tracks returns
 * PS_E_STATE).  Setting or clearing discards what was not taken.  The tracking
 * is independent of both sinks and of the five other trackers; all may be set
 * at once.  From then on every window of every ps_run / ps_run_async that runs
 * something enqueues the blame pass behind itself -- the window is neither
 * planned nor launched differently -- and the pass appends its records on the
 * device, at a cursor that lives on the device: no host wait.
 *   For window w and request position i the records are rec_off[w*n + i] ..
 * rec_off[w*n + i + 1]; w counts the windows since the last take or track
 * call, across runs, in enqueue order; windows that run nothing do not count.
 * They are, field for field and in the same ascending node order, what
 * ps_topic_blame would have returned for topic[i] right after that window, on
 * the node space that window ran on: k, miss, cut point, cut(u), hop and
 * cut_hop are the ones defined above, word for word.  rec_off is one
 * cumulative array: rec_off[0] == 0, total = rec_off[n_windows * n].  A topic
 * idle in a window has an empty slice in that window's row; so has a tracked
 * topic that is a mesh in the window's node space, and each such (topic,
 * window) pair is counted once in n_skipped, as ps_cut_track counts it.
 *   rec_cap > 0: at most that many records are kept between two takes, in five
 * arrays (20 B a record) allocated by ps_blame_track.  rec_cap == 0: the
 * engine's own cap -- per window the non-root nodes of the tracked tree topics
 * that have window messages, 65536 at most, summed as the windows come; the
 * arrays grow with their contents kept.  Overflow is sticky and leaves a
 * prefix: records are stored densely in order, none at or past the cap in
 * effect, and from the first window that overflows no later record is stored;
 * stored is the number kept, and the arrays hold exactly the first `stored` of
 * the `total` records.  rec_off, n_windows, n_skipped and total are exact
 * whatever the cap; ps_blame_take then returns PS_E_RANGE with every output
 * set.  total == cap is no overflow.
 *   ps_blame_take waits for the passes enqueued so far and lends rec_off and
 * the arrays asked for from pinned memory the engine owns (a NULL record
 * pointer: that array is neither copied nor lent), valid until the next
 * ps_blame_take, ps_blame_track or ps_destroy; the view is separate from
 * ps_topic_blame's.  It resets the cursor in front of whatever runs next, and
 * the counts.  PS_E_NOTREADY when nothing is tracked; PS_E_STATE with a run in
 * flight; PS_E_INVAL for a NULL engine, rec_off_out or count pointer.  A take
 * with no window since the last one gives rec_off = {0} and zeros.  After a
 * failed ps_run / ps_wait the content is unspecified until the next take or
 * track call. */
int ps_blame_track(ps_engine* e, const uint32_t* topic, size_t n, size_t rec_cap);
int ps_blame_take(ps_engine* e,
                  const uint64_t** rec_off_out,      /* [n_windows * n + 1], cumulative */
                  const uint32_t** rec_peer_out,     /* [stored] each; any may be NULL  */
                  const uint32_t** rec_cut_peer_out,
                  const uint32_t** rec_hop_out,
                  const uint32_t** rec_cut_hop_out,
                  const uint32_t** rec_missed_out,
                  uint64_t* n_windows_out, uint64_t* n_skipped_out,
                  uint64_t* total_out, uint64_t* stored_out);

/* The four answers above from one pass: per-peer load, deliveries by hop, the
 * audience behind each peer and the losses blamed on their cut points, for an
 * operator who wants all of them every window (one rank).
 * `what` selects sections (PS_REPORT_*); a section's arrays are defined by the
 * comment of the call named beside it below, and this is the defining
 * property: on the same engine, the same window and the same distinct topics,
 * every array of a selected section is bit for bit what that call writes.  The
 * report runs one classify pass, one per-node kernel and one bottom-up sweep
 * where the four calls run four, four and two.
 *   ps_report is filled by the caller: eleven output pointers.  A pointer of
 * a section that is not selected is not touched; a NULL pointer inside a
 * selected section is skipped.  out_size is sizeof(ps_report) as the caller
 * compiled it (the struct is not among those ps_abi_check covers): a mismatch
 * is PS_E_INVAL.
 *   ps_peer_report answers for the last window of the last run, blocking, with
 * ps_peer_load's window, stream-ordering and twin-join rules.  PS_E_INVAL for
 * a NULL engine or out, a wrong out_size, what == 0 or bits outside
 * PS_REPORT_ALL, n > 0 without topic, a topic named twice, or a selected
 * section whose pointers are all NULL; PS_E_RANGE, nothing written, for a
 * topic out of range; PS_E_NOTREADY before any run; PS_E_STATE, nothing
 * written, on a multi-rank engine, and -- when what selects any section other
 * than PS_REPORT_LOAD -- when a named topic is a mesh in that window's node
 * space or was set anew over another kind since the window.  what ==
 * PS_REPORT_LOAD answers meshes, as ps_peer_load does.  n == 0 is valid: the
 * peer-space arrays read zero and the hop arrays are not written.
 *   ps_report_track / ps_report_take follow ps_cut_track / ps_cut_take rule
 * for rule, independent of both sinks and of the four trackers above: all may
 * be set at once.  ps_report_track returns PS_E_STATE for a topic whose child
 * lists make a mesh unless what == PS_REPORT_LOAD.  While it is set, every
 * window of every ps_run / ps_run_async that runs something enqueues the one
 * pass behind itself -- the window is neither planned nor launched
 * differently -- into totals on the device: peer space for the eight per-peer
 * arrays, [n][PS_MAX_ROUNDS] by request position for the three hop arrays.  A
 * tracked topic that is a mesh in a window's node space adds its load section
 * if that is selected and nothing to the others, and is counted once in
 * n_skipped for that (topic, window) when a section other than load is
 * selected.  Per section the totals are what that section's own tracker would
 * have accumulated.  ps_report_take copies the selected sections' totals,
 * zeroes them in front of whatever runs next and returns and resets the two
 * counts; PS_E_INVAL also for a NULL out or a wrong out_size. */
#define PS_REPORT_LOAD       0x1u   /* recv, sent                        (ps_peer_load)       */
#define PS_REPORT_HOPS       0x2u   /* nodes, reached, deliv             (ps_topic_hops)      */
#define PS_REPORT_DOWNSTREAM 0x4u   /* below, carried                    (ps_peer_downstream) */
#define PS_REPORT_CUT        0x8u   /* missed, cuts, orphaned, lost      (ps_peer_cut)        */
#define PS_REPORT_ALL        0xFu

typedef struct ps_report {          /* caller-filled: eleven nullable output pointers */
  uint64_t *recv, *sent;                       /* [n_peers]                          */
  uint64_t *nodes, *reached, *deliv;           /* [n * PS_MAX_ROUNDS], row i = topic[i] */
  uint64_t *below, *carried;                   /* [n_peers]                          */
  uint64_t *missed, *cuts, *orphaned, *lost;   /* [n_peers]                          */
} ps_report;

int ps_peer_report(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what,
                   const ps_report* out, size_t out_size);
int ps_report_track(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what);
int ps_report_take(ps_engine* e, const ps_report* out, size_t out_size,
                   uint64_t* n_windows_out, uint64_t* n_skipped_out);

/* This rank's share of ps_peer_report's load, hop and downstream sections, on
 * an engine of any rank count: the analytic read a sharded
 * engine answers.  The same ps_report struct; only the selected sections'
 * pointers are touched; the last window of the last run; blocking.
 *   A rank's share is what the nodes it owns contribute, on the node space the
 * window ran on.  For every named topic t with c_t > 0 window messages and
 * every node u of t this rank owns, with peer p and k(u) the window messages
 * u's row holds (c_t for a full row, 0 for a node the window did not reach):
 *   load        recv[p] += k(u) for a non-root u; sent[p] += k(u) * deg(u),
 *               deg counting every child, local or remote, live or not; on the
 *               root's owner sent[root] += c_t * deg(root);
 *   hops        for a non-root u at BFS level d, in row i = the topic's place
 *               in the request, column min(d, PS_MAX_ROUNDS - 1): nodes += 1,
 *               reached += (k(u) > 0), deliv += k(u);
 *   downstream  for every owned u, the root included, over its strict
 *               descendants on whatever rank they live: below[p] += their
 *               number, carried[p] += the sum of their k.
 * Summed over the ranks every array is, bit for bit, what ps_peer_report
 * writes on a one-rank engine for the same trees, live mask, publishes and
 * request; on a one-rank engine the call equals ps_peer_report itself (it runs
 * its own kernels, with nothing to exchange).
 *   With PS_REPORT_DOWNSTREAM selected on a multi-rank engine the call is
 * COLLECTIVE, as ps_run is: every rank calls it with the same topics in the
 * same order and the same `what`, after the same run; the sums cross ranks
 * through the transport's exchange, level by level.  PS_REPORT_LOAD and
 * PS_REPORT_HOPS alone exchange nothing: any rank may ask alone.
 *   PS_E_INVAL for a NULL engine or out, a wrong out_size, what == 0 or a bit
 * outside PS_REPORT_DIST (PS_REPORT_CUT is not answered across ranks), n > 0
 * without topic, a topic named twice, or a selected section whose pointers are
 * all NULL; PS_E_RANGE, nothing written, for a topic out of range;
 * PS_E_NOTREADY before any run; PS_E_STATE with a run in flight on a
 * multi-rank engine, for a topic set anew since the window, and -- unless what
 * == PS_REPORT_LOAD -- for a mesh topic (one-rank engines only: a multi-rank
 * engine holds none).  A failed exchange returns the transport's error
 * (PS_E_DEVICE) with the outputs unspecified; a rank that does not arrive
 * makes the others' exchange time out, as in ps_run.  n == 0 is valid: the
 * peer-space arrays read zero, the hop arrays are not written, nothing is
 * exchanged. */
#define PS_REPORT_DIST 0x7u   /* LOAD | HOPS | DOWNSTREAM: the sections ps_dist_report answers */
int ps_dist_report(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what,
                   const ps_report* out, size_t out_size);

/* This rank's share of ps_peer_cut, on an engine of any rank count (DESIGN.md
 * 5.5o): what was not delivered and at which peer each tree was cut, where
 * the subtree behind a cut point may lie on several ranks.  The last window of
 * the last run; blocking.
 *   For every named tree topic t with c_t > 0 window messages and every node u
 * of t this rank owns, with peer p and k(u) as in ps_dist_report (the root
 * counts as full, k(root) = c_t):
 *   missed[p] += c_t - k(u) for a non-root u;
 *   where u is a non-root with k(u) < c_t whose parent, on whatever rank, is
 *   full -- a cut point --, over T(u) = u and its strict descendants on
 *   whatever rank they live:
 *     cuts[p] += 1, orphaned[p] += |T(u)| - 1,
 *     lost[p] += c_t * |T(u)| - (the sum of k over T(u)).
 * The decision is made from the k values, seen from the child: a rank lacks
 * only the fullness of a remote parent, and one word per (remote parent, child
 * rank) pair brings it ahead of the bottom-up sweep.  Summed over the ranks
 * every array is, bit for bit, what ps_peer_cut writes on a one-rank engine for
 * the same trees, live mask, publishes and request; each rank's arrays are that
 * answer's per-node values masked to the nodes it owns; on a one-rank engine the
 * call equals ps_peer_cut itself (it runs its own kernels, with nothing to
 * exchange).  An idle topic and peers outside the node space add nothing.
 *   On a multi-rank engine the call is COLLECTIVE whenever n > 0, as ps_run
 * is: every rank calls it with the same topics in the same order, after the
 * same run.  Which of the four pointers are NULL does not change the pass and
 * may differ between the ranks.
 *   PS_E_INVAL for a NULL engine, n > 0 without topic, all four outputs NULL
 * or a topic named twice; PS_E_RANGE, nothing written, for a topic out of
 * range; PS_E_NOTREADY before any run; PS_E_STATE with a run in flight on a
 * multi-rank engine, for a topic set anew since the window or topics changed
 * since the run, and for a mesh topic (one-rank engines only).  A failed
 * exchange returns the transport's error (PS_E_DEVICE) with the outputs
 * unspecified.  n == 0 is valid: all zeros, nothing exchanged. */
int ps_dist_cut(ps_engine* e, const uint32_t* topic, size_t n,
                uint64_t* missed_out, uint64_t* cuts_out,
                uint64_t* orphaned_out, uint64_t* lost_out);  /* [n_peers] each; any may be NULL, not all four */

/* This rank's share of ps_topic_blame, on an engine of any rank count
 * (DESIGN.md 5.5r): each missed subscriber this rank owns and the peer where
 * its path was cut, where the cut point and every node on the way up to it may
 * live on any rank.  The last window of the last run; blocking.
 *   One record per non-root node u this rank owns (ps_partition_owner of its
 * peer) with miss(u) > 0, for every named tree topic with c_t > 0 window
 * messages.  k, miss, cut point and cut(u) are ps_topic_blame's, word for
 * word: k(u) the window messages u's row holds, miss(u) = c_t - k(u), a cut
 * point a non-root node with k < c_t under a full parent, cut(u) the nearest
 * cut point on the way from u up to the root, u included; the root counts as
 * full.  A record holds u's peer, the peer of cut(u), hop(u), cut_hop(u) --
 * exact BFS levels, with no clamp at PS_MAX_ROUNDS -- and miss(u).  The records
 * of topic[i] are rec_off[i] .. rec_off[i+1], total = rec_off[n], in the
 * rank's own ascending node order: within a topic rec_hop never decreases.
 *   Keyed by (request position, peer) the ranks' records together are, field
 * for field, the records ps_topic_blame gives on a one-rank engine for the
 * same trees, live mask, publishes and request; a rank returns exactly the
 * records whose node it owns; on a one-rank engine the call equals
 * ps_topic_blame entry for entry, order included (it runs its own kernels,
 * with nothing to exchange).
 *   The arrays are lent from pinned memory the engine owns, valid until the
 * next ps_dist_blame or ps_destroy; the view is separate from ps_topic_blame's.
 * Any of the five record pointers may be NULL: that array is neither written,
 * copied nor lent.  rec_off_out and total_out are required.
 *   On a multi-rank engine the call is COLLECTIVE whenever n > 0, as
 * ps_dist_cut is: every rank calls it with the same topics in the same order,
 * after the same run.  Which record pointers are NULL does not change the pass
 * and may differ between the ranks.
 *   PS_E_INVAL for a NULL engine, rec_off_out or total_out NULL, n > 0 without
 * topic, or a topic named twice; PS_E_RANGE, nothing written, for a topic out
 * of range; PS_E_NOTREADY before any run; PS_E_STATE with a run in flight on a
 * multi-rank engine, for a topic set anew since the window or topics changed
 * since the run, and for a mesh topic (one-rank engines only).  A failed
 * exchange returns the transport's error (PS_E_DEVICE) with the outputs
 * unspecified.  n == 0 is valid: rec_off = {0}, total 0, nothing exchanged.
 *   ps_topic_blame and ps_blame keep refusing multi-rank engines, and so does
 * ps_blame_track.  What remains missing on a sharded engine: there is no
 * sharded form of ps_blame, no tracker and no _begin / _end form -- a query's
 * peer may be owned by another rank than the one that asks, and a sharded
 * tracker needs collective exchanges inside the run: each its own piece of
 * work. */
int ps_dist_blame(ps_engine* e, const uint32_t* topic, size_t n,
                  const uint64_t** rec_off_out,      /* [n + 1]          */
                  const uint32_t** rec_peer_out,     /* [total] each     */
                  const uint32_t** rec_cut_peer_out,
                  const uint32_t** rec_hop_out,
                  const uint32_t** rec_cut_hop_out,
                  const uint32_t** rec_missed_out,
                  uint64_t* total_out);

/* Hops and duplicate copies, for mesh topics and tree topics alike (one rank;
 * DESIGN.md 5.5p): how deep a topic's messages travelled, and what the edges
 * beyond a tree cost, at which peers.  Per named topic t with c_t > 0 messages
 * in the window, on the node space that window ran on, with k(u) ps_peer_load's
 * k -- the number of t's window messages the row of node u holds (the
 * PSAMD_LOAD_COUNT=rows seam applies):
 *   Forwarders.  F is the root plus every non-root node with k(u) > 0;
 * k'(root) = c_t and k'(u) = k(u) otherwise.
 *   Hop.  h(root) = 0; for any other u in F, h(u) = 1 + min h(q) over the
 * child entries (q -> u) with q in F: the BFS distance from the root within F,
 * read from the rows and not from the live mask.  The flood is
 * level-synchronous and its seen test lets the first arrival win, so this is
 * the hop every message reached u at.
 *   Per topic row.  Column min(h(u), PS_MAX_ROUNDS - 1) gets reached += 1 and
 * deliv += k(u) for every non-root u in F that the BFS visits.  Column 0
 * stays 0; the last column collects the deeper hops, as in ps_topic_hops.
 *   unreached[i] counts the non-root nodes with k == 0, a peer once: where a
 * mesh parent lists a peer twice the node space holds a node for either
 * entry, and only the one the child entries name counts.  stranded[i] counts
 * the non-root nodes with k > 0 that the BFS never visits -- 0 on a healthy
 * engine, reported and not assumed.
 *   Per peer.  Every child entry (q -> u) with q in F, q visited and u in F
 * adds k'(q) to copies[peer(u)]: every forwarder sends each message once along
 * every child entry whose target received it.  Entries count with their
 * multiplicity; self-loops and entries naming the root are included -- the
 * root is no recipient, so everything sent to it is a duplicate.
 *   dup[p] = copies[p] - recv[p], recv ps_peer_load's for the same topics:
 * exact while every row is full or empty; computed modulo 2^64.
 * A topic with no message in the window adds nothing; peers outside the node
 * space add nothing.  On a tree reached / deliv equal ps_topic_hops' rows,
 * copies equals recv and dup is 0.
 *   ps_topic_spread answers for the last window of the last run, blocking, with
 * ps_peer_load's window, stream-ordering and twin-join rules.  The n topics
 * are distinct; row i of reached / deliv ([n * PS_MAX_ROUNDS]) and word i of
 * unreached / stranded ([n]) belong to topic[i]; copies / dup are [n_peers].
 * Any of the six may be NULL, not all; the arrays given are written in full.
 * n == 0 is valid: the peer arrays read zero and the others are not written.
 * PS_E_INVAL for a NULL engine, n > 0 without topic, all six outputs NULL or a
 * topic named twice; PS_E_RANGE, nothing written, for a topic out of range;
 * PS_E_NOTREADY before any run; PS_E_STATE on a multi-rank engine and for a
 * tree topic that was set anew over another kind since the window.
 *   There is no asynchronous form of this call: it reads the frontier count
 * between batches of level launches to find where the levels end.  The
 * tracker below needs no such read: behind a window that has been enqueued the
 * host knows its last round, which bounds every hop. */
int ps_topic_spread(ps_engine* e, const uint32_t* topic, size_t n,
                    uint64_t* reached_out, uint64_t* deliv_out,      /* [n * PS_MAX_ROUNDS], row i = topic[i] */
                    uint64_t* unreached_out, uint64_t* stranded_out, /* [n] */
                    uint64_t* copies_out, uint64_t* dup_out);        /* [n_peers] */
/* ps_topic_spread's answer behind every window, summed on the device (one
 * rank).  ps_spread_track registers n distinct standing
 * topics, meshes and trees alike -- nothing is refused or skipped for being a
 * mesh; n == 0 clears the tracking and frees the totals.  PS_E_INVAL for a
 * NULL engine, n > 0 without topic or a topic named twice; PS_E_RANGE for a
 * topic out of range; PS_E_STATE with a run in flight or on a multi-rank
 * engine; after a failure the previous tracking stays.  ps_dist_init* on an
 * engine that tracks spread returns PS_E_STATE.  Setting or clearing zeroes
 * the totals.  Independent of both sinks and of the six other trackers: all
 * may be set at once.
 *   While it is set, every window of every ps_run / ps_run_async that runs
 * something enqueues the pass behind itself on the engine's stream; the
 * window is neither planned nor launched differently, and nothing waits.  A
 * window ends with its last round r, which the host knows once the window is
 * enqueued; a node that holds a message received it at some round <= r over a
 * path of as many forwarders, so no hop lies beyond r and the pass enqueues
 * level launches 0 .. r whole, then checks on the device that the next
 * frontier is empty.  Each window adds into totals on the device; per window
 * and per standing topic the contribution is exactly ps_topic_spread's, on
 * the node space that window ran on (the PSAMD_LOAD_COUNT=rows seam
 * applies).  A topic idle in a window adds nothing.  stranded is the sum of
 * the windows' holders minus the sum of their visited nodes; dup is the sum
 * of copies minus the sum of recv, modulo 2^64.  The totals are indexed by
 * request position and survive rebuilds, joins, leaves and drops between
 * windows.  There is no n_skipped: nothing is skipped.
 *   ps_spread_take waits once for the passes enqueued so far and copies the
 * totals since the last take or track call; each array may be NULL, all six
 * too.  It zeroes the totals in front of whatever runs next and sets
 * *n_windows_out, and *n_truncated_out to the number of windows whose BFS
 * still had a frontier left behind its r + 1 launches -- 0 on a healthy
 * engine, reported and not assumed like stranded; such a window's late nodes
 * count as stranded and the copies they sent are missing.  Both counts start
 * again at 0.  PS_E_NOTREADY when nothing is tracked; PS_E_STATE with a run in
 * flight; PS_E_INVAL for a NULL engine or count pointer.  After a failed run
 * the totals are unspecified until the next take or track call.
 *   A/B only (PSAMD_AB=1): PSAMD_SPREAD_TRACK_LEVELS=n caps a tracked window's
 * level launches at n, to show that truncation is detected and counted. */
int ps_spread_track(ps_engine* e, const uint32_t* topic, size_t n);
int ps_spread_take(ps_engine* e,
                   uint64_t* reached_out, uint64_t* deliv_out,      /* [n_tracked * PS_MAX_ROUNDS], nullable */
                   uint64_t* unreached_out, uint64_t* stranded_out, /* [n_tracked], nullable */
                   uint64_t* copies_out, uint64_t* dup_out,         /* [n_peers], nullable */
                   uint64_t* n_windows_out, uint64_t* n_truncated_out);
/* Order-independent digest of the final seen state of the last window:
 * sum over (peer, topic, word < message words) of
 * mix64(mix64(peer << 32 | topic << 16 | word) ^ mix64(seen word)); a
 * multi-GPU engine sums its owned nodes (the ranks' digests add up). */
int ps_seen_digest(ps_engine* e, uint64_t* digest_out);

/* Pipelined windows (ps_run_async) whose leading launches ran beside the
 * previous window's last launches (no reference
 * counterpart: a scheduling diagnostic). */
int ps_overlapped_windows(ps_engine* e, uint64_t* count_out);

/* Chain launch slots (PS_K_CHAIN rounds) whose whole rows were written as a
 * reach pass plus a fill from the topic roots' rows instead of by the chain
 * kernel (a scheduling diagnostic, as above). */
int ps_chain_fill_launches(ps_engine* e, uint64_t* count_out);

/* ---- multi-GPU: one engine (process) per GPU --------------------------------
 * Every rank creates the same topics and memberships and publishes the same
 * messages; each owns a hash partition of every topic's tree nodes and ps_run
 * exchanges, each round, the deliveries addressed to other ranks' nodes
 * (stream-ordered all-to-allv over RCCL / xGMI).  Stats and ps_read_* cover
 * the owned nodes; sums over ranks give the job totals of deliveries,
 * duplicates, deliveries_per_round and the seen digest.  (A rank that owns
 * none of a topic's nodes answers ps_read_delivered for its messages with
 * zeros.)  The frontier counters are per reader, not per owner: in a level
 * run frontier_per_round[q] (and frontier_entries) of rank r counts, per
 * (topic, start group) the round writes, every reached parent of the level
 * above -- owned by r or read as a ghost record / row of another rank --
 * that has at least one child, live or not, owned by r.  A parent with
 * children on k ranks counts once on each, so the ranks' sum exceeds the
 * one-rank count by k - 1 for every such parent.
 *   PS_PART_PEER     owner(p) = splitmix64(p) mod world (the
 *                    default): every round ships each parent row whose
 *                    children live on other ranks once per such rank
 *   PS_PART_SUBTREE  a node below the split level belongs to the owner of its
 *                    ancestor at that level (the subtrees dealt largest first
 *                    to the least-loaded rank), so only edges out of the top
 *                    levels cross GPUs. */
#define PS_PART_PEER 0u
#define PS_PART_SUBTREE 1u
#define PS_UNIQUE_ID_BYTES 128

typedef struct ps_dist_config {
  int32_t rank;
  int32_t world;        /* <= 16 */
  uint32_t partition;   /* PS_PART_*                                    */
  uint32_t split_depth; /* PS_PART_SUBTREE: split level, 0 = automatic */
  uint32_t flags;       /* PS_DIST_F_*                                  */
  uint32_t reserved;
} ps_dist_config;
/* ps_dist_config.flags: the loopback transport copies every round's ghost
 * records into the receiver's buffer, the data path of the RCCL transport
 * (send parts, receive buffer, exchange stream), instead of reading them in
 * place (tests run the RCCL-shaped path on one GPU with it; RCCL: ignored) */
#define PS_DIST_F_COPY 0x1u
/* ps_dist_config.flags: ghost-fed nodes read their remote parents' rows in
 * the owner's own row set (no packed records, no shipping): the loopback's
 * ranks share one process; ps_dist_init_ipc's map each other's row sets
 * (across the GPUs of a node, xGMI peer reads).  Not with PS_DIST_F_COPY;
 * RCCL: refused. */
#define PS_DIST_F_INPLACE 0x2u

/* GPUs visible to this process (0 without one); a launcher decides from it
 * whether every rank gets a GPU of its own (RCCL) or ranks share (IPC) */
int ps_device_count(int32_t* out);
/* rank 0 creates the RCCL id; the caller ships it to every rank */
int ps_dist_unique_id(uint8_t id_out[PS_UNIQUE_ID_BYTES]);
int ps_dist_init(ps_engine* e, const ps_dist_config* dc, const uint8_t id[PS_UNIQUE_ID_BYTES]);
/* process-shared transport: one process per rank on one node -- their GPUs
 * map each other's memory (hipIpcGetMemHandle / hipIpcOpenMemHandle; several
 * ranks may share one GPU, which RCCL refuses).  Rank 0 calls ps_dist_ipc_id
 * (host only: a fresh POSIX shared-memory name) and the caller ships the id
 * to every rank, as with the RCCL id; ps_dist_init_ipc then meets the other
 * ranks there (host barriers in shared memory, 120 s timeout) and maps their
 * device flag blocks.  Each round is ordered by monotonic device flags in
 * IPC-mapped memory (a one-wave set kernel and a one-wave poll kernel with a
 * 30 s timeout, after which the next call fails with PS_E_DEVICE): no host
 * synchronisation with the GPU.  flags: PS_DIST_F_COPY copies the records
 * into the receive buffer (the RCCL data path), PS_DIST_F_INPLACE reads the
 * ghost parents' rows in their owner's row set, neither reads each sender's
 * records in place.  Replaces the cross-host child write subtree.go:333 and
 * the per-hop read client.go:104 for ranks that share a node. */
int ps_dist_ipc_id(uint8_t id_out[PS_UNIQUE_ID_BYTES]);
int ps_dist_init_ipc(ps_engine* e, const ps_dist_config* dc, const uint8_t id[PS_UNIQUE_ID_BYTES]);
/* in-process transport: `world` engines of one process (one thread each)
 * exchange through device copies -- runs the multi-GPU path on one GPU */
typedef struct ps_loopback ps_loopback;
int ps_loopback_create(int32_t world, ps_loopback** out);
void ps_loopback_destroy(ps_loopback* lb);
int ps_dist_init_loopback(ps_engine* e, const ps_dist_config* dc, ps_loopback* lb);
/* host-only: owner rank of every peer of a tree (parent array, PS_NONE =
 * absent) under a partition; -1 for peers outside the tree */
int ps_partition_owner(uint32_t n_peers, uint32_t root, const uint32_t* parent, uint32_t topic,
                       const ps_dist_config* dc, int32_t* owner_out);

/* ---- wire codec (host only, no engine needed) --------------------------------
 * The reference's stream framing, pubsub.go:122-153: writeMessage is
 * json.NewEncoder(s).Encode(m) and readMessage json.NewDecoder(r).Decode(m)
 * over
 *   type Message struct { Type MessageType; Data []byte `json:"data,omitempty"`;
 *     Peers []string `json:"parents,omitempty"`; TreeWidth, TreeMaxWidth,
 *     NumPeers int `json:"...,omitempty"` }
 * so a Go peer and this engine exchange byte-identical lines. */
#define PS_MSG_DATA 0   /* MessageType, pubsub.go:138-144 */
#define PS_MSG_JOIN 1
#define PS_MSG_PART 2
#define PS_MSG_UPDATE 3
#define PS_MSG_STATE 4

typedef struct ps_message {
  int32_t type;
  const uint8_t* data;      /* Data (base64 on the wire) */
  size_t data_len;
  const char* const* peers; /* Peers: NUL-terminated peer id strings */
  size_t n_peers;
  int64_t tree_width;
  int64_t tree_max_width;
  int64_t num_peers;
} ps_message;

/* decode target: caller-owned buffers; *_len / n_peers are always set, and
 * PS_E_RANGE is returned when data_cap / peers_cap is too small */
typedef struct ps_message_buf {
  int32_t type;
  int32_t reserved;
  uint8_t* data;
  size_t data_cap;
  size_t data_len;
  char* peers;              /* n_peers NUL-terminated strings, back to back */
  size_t peers_cap;
  size_t peers_len;
  size_t n_peers;
  int64_t tree_width;
  int64_t tree_max_width;
  int64_t num_peers;
} ps_message_buf;

/* one JSON line, '\n'-terminated; *len_out = bytes needed (PS_E_RANGE if cap
 * is short, nothing written) */
int ps_msg_encode(const ps_message* m, char* out, size_t cap, size_t* len_out);
/* one JSON value from in[0..len); *consumed = bytes up to the next value
 * (trailing whitespace included); PS_E_INVAL on malformed input */
int ps_msg_decode(const char* in, size_t len, ps_message_buf* out, size_t* consumed);

#ifdef __cplusplus
}
#endif
#endif /* PSENGINE_H */
