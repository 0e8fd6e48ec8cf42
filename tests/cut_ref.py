"""The expected losses and their cut points (ps_peer_cut / ps_cut_track,
DESIGN.md §5.5l) from the oracle alone.  No engine call, no GPU.

Per tree topic with c > 0 window messages:
  who receives comes from oracle.disseminate over the input child lists with
  the live mask (or from oracle.Tree under churn), as in downstream_ref;
  membership and depth come from graph_check.reference (the peers whose parent
  chain reaches the root, live or not).  miss = c - recv for the non-root
  members, 0 for the root: it is the source.  A cut point is a non-root member
  with miss > 0 whose parent is the root or has miss == 0.  Every member starts
  with (1, miss) and adds its pair into its parent's, the deepest members
  first: (|T(u)|, the misses in T(u)).  Then
    missed[p]   = miss[p]
    cuts[p]     = 1 where p is a cut point
    orphaned[p] = |T(p)| - 1 there
    lost[p]     = the misses in T(p) there.
"""
from __future__ import annotations

import numpy as np

import graph_check as GC
import oracle as O

NONE = 0xFFFFFFFF


def from_parents(n_peers, root, parent, recv, c):
    """(missed, cuts, orphaned, lost), int64 [n_peers], of the tree `parent`
    under `root` whose members received `recv` of c messages each (the root's
    entry is ignored: it counts as full)."""
    par = np.asarray(parent, dtype=np.uint32).copy()
    par[root] = NONE
    depth_of = GC.reference(n_peers, [(root, par)], np.ones(n_peers, dtype=np.uint8))["topics"][0]["depth_of"]
    member = depth_of >= 0
    miss = np.where(member, c - np.asarray(recv, dtype=np.int64), 0)
    miss[root] = 0
    assert (miss >= 0).all()
    w_n = member.astype(np.int64)
    w_m = miss.copy()
    for d in range(int(depth_of.max()), 0, -1):
        at = np.nonzero(depth_of == d)[0]
        np.add.at(w_n, par[at], w_n[at])
        np.add.at(w_m, par[at], w_m[at])
    up = np.where(member & (depth_of > 0), par, root).astype(np.int64)  # (the root's own entry is masked out below)
    cut = member & (depth_of > 0) & (miss > 0) & (miss[up] == 0)
    return miss, cut.astype(np.int64), np.where(cut, w_n - 1, 0), np.where(cut, w_m, 0)


def topic_cut(n_peers, root, live, n_msgs, parent):
    """(missed, cuts, orphaned, lost, oracle deliveries, members) of one tree
    topic's window of n_msgs messages; the arrays int64 [n_peers].  parent: the
    tree's upstream array."""
    z = np.zeros(n_peers, dtype=np.int64)
    if n_msgs == 0:
        return z, z.copy(), z.copy(), z.copy(), 0, 0
    live = np.asarray(live, dtype=np.uint8)
    par = np.asarray(parent, dtype=np.uint32).copy()
    par[root] = NONE
    rp, cl = O.parents_to_csr(par)
    tot, hops, _ = O.disseminate(rp, cl, root, live, n_msgs)
    got = hops != 0xFF
    got[:, root] = False
    depth_of = GC.reference(n_peers, [(root, par)], np.ones(n_peers, dtype=np.uint8))["topics"][0]["depth_of"]
    return from_parents(n_peers, root, par, got.sum(axis=0), n_msgs) + (tot, int((depth_of >= 0).sum()))


def window_cut(n_peers, live, topics):
    """The sum over a window's topics: topics = [(root, n_msgs, parent), ...].
    Returns (missed, cuts, orphaned, lost, deliveries, possible): four uint64
    arrays and two ints, possible = the sum of c_t * (n_nodes_t - 1)."""
    out = [np.zeros(n_peers, dtype=np.int64) for _ in range(4)]
    total = possible = 0
    for root, n_msgs, parent in topics:
        r = topic_cut(n_peers, root, live, n_msgs, parent)
        for o, x in zip(out, r[:4]):
            o += x
        total += r[4]
        possible += n_msgs * max(r[5] - 1, 0)
    return tuple(o.astype(np.uint64) for o in out) + (total, possible)
