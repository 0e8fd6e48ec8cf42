"""The expected audience behind each peer (ps_peer_downstream /
ps_downstream_track) from the oracle alone.  No engine call,
no GPU.

Per tree topic with c > 0 window messages:
  who receives comes from oracle.disseminate over the input child lists with
  the live mask, as in load_ref.topic_load; membership and depth come from
  graph_check.reference (the peers whose parent chain reaches the root, live
  or not).  Every member starts with (1, recv) -- the root with (1, 0): it is
  no recipient -- and adds its pair into its parent's, the deepest members
  first.  Then
    below[p]   = the members strictly below p   = w_n[p] - 1
    carried[p] = the messages delivered to them = w_k[p] - recv[p].
"""
from __future__ import annotations

import numpy as np

import graph_check as GC
import oracle as O

NONE = 0xFFFFFFFF


def from_parents(n_peers, root, parent, recv):
    """(below, carried), int64 [n_peers], of the tree `parent` under `root`
    whose members received `recv` messages each (the root's entry is ignored)."""
    par = np.asarray(parent, dtype=np.uint32).copy()
    par[root] = NONE
    depth_of = GC.reference(n_peers, [(root, par)], np.ones(n_peers, dtype=np.uint8))["topics"][0]["depth_of"]
    member = depth_of >= 0
    k = np.where(member, np.asarray(recv, dtype=np.int64), 0)
    k[root] = 0
    w_n = member.astype(np.int64)
    w_k = k.copy()
    for d in range(int(depth_of.max()), 0, -1):
        at = np.nonzero(depth_of == d)[0]
        np.add.at(w_n, par[at], w_n[at])
        np.add.at(w_k, par[at], w_k[at])
    return np.where(member, w_n - 1, 0), np.where(member, w_k - k, 0)


def topic_downstream(n_peers, root, live, n_msgs, parent):
    """(below, carried, oracle deliveries) of one tree topic's window of n_msgs
    messages; the arrays int64 [n_peers].  parent: the tree's upstream array."""
    if n_msgs == 0:
        return np.zeros(n_peers, dtype=np.int64), np.zeros(n_peers, dtype=np.int64), 0
    live = np.asarray(live, dtype=np.uint8)
    par = np.asarray(parent, dtype=np.uint32).copy()
    par[root] = NONE
    rp, cl = O.parents_to_csr(par)
    tot, hops, _ = O.disseminate(rp, cl, root, live, n_msgs)
    got = hops != 0xFF
    got[:, root] = False
    below, carried = from_parents(n_peers, root, par, got.sum(axis=0))
    return below, carried, tot


def window_downstream(n_peers, live, topics):
    """The sum over a window's topics: topics = [(root, n_msgs, parent), ...].
    Returns (below, carried, deliveries): uint64, uint64, int."""
    below = np.zeros(n_peers, dtype=np.int64)
    carried = np.zeros(n_peers, dtype=np.int64)
    total = 0
    for root, n_msgs, parent in topics:
        b, c, tot = topic_downstream(n_peers, root, live, n_msgs, parent)
        below += b
        carried += c
        total += tot
    return below.astype(np.uint64), carried.astype(np.uint64), total
