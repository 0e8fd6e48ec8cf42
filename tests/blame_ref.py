"""The expected blame of every missed subscriber (ps_topic_blame / ps_blame,
DESIGN.md §5.5q) from the oracle alone.  No engine call, no GPU.

Per tree topic with c > 0 window messages:
  who receives comes from oracle.disseminate over the input child lists with
  the live mask (or from oracle.Tree under churn), as in cut_ref; membership
  and depth come from graph_check.reference (the peers whose parent chain
  reaches the root, live or not).  miss = c - recv for the non-root members, 0
  for the root: it is the source.  Blame is handed down level by level from
  the root: a member at depth d with miss > 0 is its own cut point, at hop d,
  where its parent is the root or has miss == 0, and else takes its parent's
  cut point and cut hop.  A member with miss == 0 has none.

In a tree topic each peer holds one node, so the answer is a table per peer
(Table below); records() lists it in the order of the engine's nodes.

Against cut_ref's four arrays (test_blame_cpu.py):
  bincount(cut_peer, weights = missed) == lost   and
  bincount(peer, weights = missed)     == missed
hold as stated.  #(peer == cut_peer) == cuts holds by definition.  The fourth,
#(cut_peer == p, peer != p) == orphaned[p], rests on every node behind a cut
point lacking a message -- a tree row is a subset of its parent's row, as
identity 2 of ps_peer_cut assumes: orphaned counts every node behind the cut
point, the blame only those with miss > 0.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import graph_check as GC
import oracle as O

NONE = 0xFFFFFFFF


class Table(NamedTuple):
    """Per peer, int64 [n_peers]; -1 where there is none."""
    member: np.ndarray    # bool: the peer holds a node of the topic (the root too)
    hop: np.ndarray       # the node's BFS level; -1 for a peer outside the node space
    miss: np.ndarray      # c - recv; 0 for the root and outside
    cut_peer: np.ndarray  # the cut point's peer; -1 where miss == 0
    cut_hop: np.ndarray   # its level; -1 where miss == 0


def from_parents(n_peers, root, parent, recv, c) -> Table:
    """The table of the tree `parent` under `root` whose members received
    `recv` of c messages each (the root's entry is ignored: it counts as full)."""
    par = np.asarray(parent, dtype=np.uint32).copy()
    par[root] = NONE
    depth_of = GC.reference(n_peers, [(root, par)], np.ones(n_peers, dtype=np.uint8))["topics"][0]["depth_of"]
    depth_of = np.asarray(depth_of, dtype=np.int64)
    member = depth_of >= 0
    miss = np.where(member, c - np.asarray(recv, dtype=np.int64), 0)
    miss[root] = 0
    assert (miss >= 0).all()
    cut_peer = np.full(n_peers, -1, dtype=np.int64)
    cut_hop = np.full(n_peers, -1, dtype=np.int64)
    for d in range(1, int(depth_of.max()) + 1):  # from the root down: the level above is settled
        at = np.nonzero(depth_of == d)[0]
        up = par[at].astype(np.int64)
        lacks = miss[at] > 0
        full_parent = miss[up] == 0  # (the root's miss is 0)
        cut_peer[at] = np.where(lacks, np.where(full_parent, at, cut_peer[up]), -1)
        cut_hop[at] = np.where(lacks, np.where(full_parent, d, cut_hop[up]), -1)
    return Table(member, np.where(member, depth_of, -1), miss, cut_peer, cut_hop)


def idle(n_peers, root, parent) -> Table:
    """A topic with no message in the window: levels, and nothing missed."""
    return from_parents(n_peers, root, parent, np.zeros(n_peers, dtype=np.int64), 0)


def topic_blame(n_peers, root, live, n_msgs, parent) -> Table:
    """The table of one tree topic's window of n_msgs messages.  parent: the
    tree's upstream array."""
    if n_msgs == 0:
        return idle(n_peers, root, parent)
    live = np.asarray(live, dtype=np.uint8)
    par = np.asarray(parent, dtype=np.uint32).copy()
    par[root] = NONE
    rp, cl = O.parents_to_csr(par)
    _, hops, _ = O.disseminate(rp, cl, root, live, n_msgs)
    got = hops != 0xFF
    got[:, root] = False
    return from_parents(n_peers, root, par, got.sum(axis=0), n_msgs)


def records(table: Table, node_peer):
    """ps_topic_blame's five arrays for one topic: node_peer lists the peers of
    its nodes in node order, the root's first (it is skipped: no record)."""
    q = np.asarray(node_peer, dtype=np.int64)[1:]
    q = q[table.miss[q] > 0]
    return tuple(x.astype(np.uint32) for x in (q, table.cut_peer[q], table.hop[q], table.cut_hop[q], table.miss[q]))


def queries(table: Table, peers):
    """ps_blame's four arrays (cut_peer, hop, cut_hop, missed) for `peers`, in
    their order; -1 reads NONE."""
    p = np.asarray(peers, dtype=np.int64)
    u32 = lambda x: (x & 0xFFFFFFFF).astype(np.uint32)
    return u32(table.cut_peer[p]), u32(table.hop[p]), u32(table.cut_hop[p]), table.miss[p].astype(np.uint32)
