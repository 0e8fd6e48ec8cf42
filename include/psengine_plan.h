/*
 * psengine_plan.h -- host-only planner probe of libpsengine.so (tests).
 *
 * Not part of the drop-in boundary (include/psengine.h): these entry points
 * build one rank's node space and one window's launch plans on the host --
 * no device is touched -- so the planners (chunk cuts, round pairs, the
 * multi-GPU ghost exchange layout) are unit-tested on a machine without a GPU
 * (tests/test_plan_cpu.py replays the exchange from these tables with gloo
 * and checks the deliveries against the CPU restatement).
 */
#ifndef PSENGINE_PLAN_H
#define PSENGINE_PLAN_H

#include "psengine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A host-only engine of n_topics trees: parents[t * n_peers + p] (PS_NONE =
 * absent), roots[t]; dc (nullable) = this rank and the partition. */
int ps_plan_create(uint32_t n_peers, uint32_t n_topics, const uint32_t* roots, const uint32_t* parents,
                   const ps_dist_config* dc, ps_engine** out);
void ps_plan_destroy(ps_engine* e);
/* ps_config.msg_window of the probe (default 65536; PS_E_INVAL above 2^30) */
int ps_plan_set_msg_window(ps_engine* e, uint32_t msg_window);
/* Plans the first window of a batch (topic and start round per message; a
 * null start_round = all round 0), as ps_run would; flags: PS_F_* */
int ps_plan_window(ps_engine* e, const uint32_t* topic_of_msg, const uint32_t* start_round, size_t n_msgs,
                   uint32_t flags);

/* ps_plan_get(what, index): u64 values into out[0..cap), *n_out = how many
 * there are (PS_E_RANGE if cap is short). */
#define PS_PLAN_INFO 0        /* planned rounds, nodes, pull chunks, pair chunks, world, rank,
                                 send half words, recv words, ghost segments, level mode, ship entries */
#define PS_PLAN_NODES 1       /* per node: peer */
#define PS_PLAN_PARENT 2      /* per node: local parent node (PS_NONE: root or remote) */
#define PS_PLAN_GHOST_REF 3   /* per node: source rank << 27 | record index (PS_NONE: local parent) */
#define PS_PLAN_TOPIC 4       /* index = topic: nbase, n_nodes, depth, root_local, then level_off[0..depth+1],
                                 level_local[0..depth] */
#define PS_PLAN_LAYOUT 5      /* index = topic: W, wbase, flags, group count, then (start, w0, wn) per group */
#define PS_PLAN_ROUND_KIND 6  /* per round 0..planned+1: PS_K_* */
#define PS_PLAN_PULL 7        /* index = round: off, gsplit, end, then per chunk 13 values: node_begin,
                                 node_end, topic, W, row0, e_lo, e_hi, gin, gout, group, p_lo, p_hi,
                                 c_lo (pair launches: PS_NONE = a level-1 run of the second round) */
#define PS_PLAN_PAIR 8        /* index = round: lo, gsplit, hi, then the chunks as PS_PLAN_PULL */
#define PS_PLAN_XCHG 9        /* index = round: any, then per rank s_off, s_len, r_off, r_len (bytes) */
#define PS_PLAN_SEGS 10       /* per segment: topic, rw, rbase[world], sbase[world] */
#define PS_PLAN_SHIP 11       /* per ship entry: node, dst (rank << 27 | record index) */
#define PS_PLAN_PACK 12       /* index = round: per root segment e0, e1, gseg, W, row, unit0 */
#define PS_PLAN_CHAIN 13      /* index = round: rounds of the launch, then per chunk 17 values: node_begin,
                                 node_end, topic, W, row0, w0, S, levels, r0, group, first[0..6] */
#define PS_PLAN_SCHEDULE 14   /* the window's schedule, as a run enqueues it.  Ten header values: k_flood
                                 rounds (rounds 1..that many), prefix P (deep windows: rounds 1..P may run
                                 beside the previous window), partial counter slots, reach rows, PS_MODE_*,
                                 the window's row bytes, then the lengths nl, nw, nd, ns of the four tables
                                 that follow (nl = nw = nd = 0 outside level mode):
                                 lgrid[nl]    per round 0..planned: workgroups of the launch starting there
                                              (0: none, or a continuation round of a multi-round launch)
                                 woff[nw]     per round 0..planned+1: the round's first counter slot
                                 desc[nd]     (first slot, end slot, stride) per reduce row: rounds
                                              0..planned+1, then one row per reach row
                                 seed_off[ns] per start round 0..latest+1: seeds before that round */
#define PS_PLAN_FILL 15       /* index = round: the chain launch starting there as reach + fill (DESIGN.md
                                 5.1d).  0 alone: the launch has no fill segments.  Else segments ns, pieces
                                 np, reach blocks; then per segment 15 values: topic, W, row0, nbase, levels,
                                 first piece, first reach block, words per piece, first[0..6]; then per
                                 piece 4 values, in launch order: first word, words, the node holding the
                                 first word, that word's offset in the node's row */
int ps_plan_get(ps_engine* e, uint32_t what, uint32_t index, uint64_t* out, size_t cap, size_t* n_out);

/* ps_graph_get(what, index): the node space itself and which
 * build produced it, on a real engine or on the probe; values and *n_out as
 * ps_plan_get.  A real engine first brings its node space up to date exactly
 * as ps_run would (the rebuild after topology changes, the flags after
 * ps_set_live) and reads a GPU-built one back; it changes no later run.  If
 * the topology changed since the last run (a run's own repairs and prunes
 * count), that rebuild retires the last window's readbacks, as the next
 * ps_run or ps_topic_depth would: read hops and digests first.
 * PS_E_STATE while an asynchronous run or a drain is outstanding. */
#define PS_GRAPH_NODE_PEER 0    /* per node: peer */
#define PS_GRAPH_NODE_PARENT 1  /* per node: parent node (PS_NONE: root, or a parent on another rank) */
#define PS_GRAPH_NODE_TOPIC 2   /* per node: topic */
#define PS_GRAPH_NODE_FLAGS 3   /* per node: 1 live, 2 internal, 4 split */
#define PS_GRAPH_ROW_PTR 4      /* nodes + 1 entries: a node's children are col[row_ptr[u] .. row_ptr[u + 1]) */
#define PS_GRAPH_COL 5          /* per edge: child node */
#define PS_GRAPH_TOPIC 6        /* index = topic: exists, nbase, n_nodes, depth, max_deg, top_levels, then (a
                                   topic with nodes) level_off[0..depth+1], level_internal[0..depth] */
#define PS_GRAPH_BUILD 7        /* since creation: GPU builds, host builds, fall-backs to the host build by
                                   reason (stall, attempts, capacity, depth), repeated GPU attempts by reason
                                   (grid, order, depth growth); then the last build: kind (0 none, 1 GPU,
                                   2 host), GPU attempts */
int ps_graph_get(ps_engine* e, uint32_t what, uint32_t index, uint64_t* out, size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* PSENGINE_PLAN_H */
