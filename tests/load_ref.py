"""The expected per-peer load (ps_peer_load / ps_load_track)
from the oracle alone: who a topic's window messages are delivered to comes
from oracle.disseminate over the input child lists with the live mask, the
child counts from the input tree restricted to its members (peers whose
parent chain reaches the root: graph_check.reference's n_child).  No engine
call, no GPU.

Per topic with c > 0 window messages:
  recv[p] = the messages delivered to p (the root is no recipient: 0)
  sent[p] = recv[p] * children(p) for a non-root member, c * children(root)
            for the root; children count whether live or not.
"""
from __future__ import annotations

import numpy as np

import graph_check as GC
import oracle as O

NONE = 0xFFFFFFFF


def csr_members(rp, cl, root):
    """The peers reachable from the root over the child lists (the node space
    of a topic set by child lists), live or not."""
    n = len(rp) - 1
    member = np.zeros(n, dtype=bool)
    member[root] = True
    todo = [int(root)]
    while todo:
        p = todo.pop()
        for c in cl[int(rp[p]):int(rp[p + 1])]:
            if not member[c]:
                member[c] = True
                todo.append(int(c))
    return member


def topic_load(n_peers, root, live, n_msgs, parent=None, csr=None):
    """(recv, sent, oracle deliveries) of one topic's window of n_msgs
    messages, int64 [n_peers] each.  parent: a tree's upstream array; csr:
    (row_ptr, col) child lists (a mesh)."""
    recv = np.zeros(n_peers, dtype=np.int64)
    sent = np.zeros(n_peers, dtype=np.int64)
    if n_msgs == 0:
        return recv, sent, 0
    live = np.asarray(live, dtype=np.uint8)
    if csr is None:
        par = np.asarray(parent, dtype=np.uint32).copy()
        par[root] = NONE
        R = GC.reference(n_peers, [(root, par)], np.ones(n_peers, dtype=np.uint8))["topics"][0]
        member = R["depth_of"] >= 0
        n_child = R["n_child"]
        rp, cl = O.parents_to_csr(par)
    else:
        rp, cl = (np.asarray(x, dtype=np.uint32) for x in csr)
        member = csr_members(rp, cl, root)
        n_child = np.diff(rp.astype(np.int64))
    tot, hops, _ = O.disseminate(rp, cl, root, live, n_msgs)
    got = hops != 0xFF
    got[:, root] = False
    recv[:] = got.sum(axis=0)
    assert not recv[~member].any()
    sent[:] = np.where(member, recv * n_child, 0)
    sent[root] = n_msgs * n_child[root]
    return recv, sent, tot


def window_load(n_peers, live, topics):
    """The sum over a window's topics: topics = [(root, n_msgs, parent or
    None, csr or None), ...].  Returns (recv, sent, deliveries) as uint64 /
    uint64 / int."""
    recv = np.zeros(n_peers, dtype=np.int64)
    sent = np.zeros(n_peers, dtype=np.int64)
    total = 0
    for root, n_msgs, parent, csr in topics:
        r, s, tot = topic_load(n_peers, root, live, n_msgs, parent=parent, csr=csr)
        recv += r
        sent += s
        total += tot
    return recv.astype(np.uint64), sent.astype(np.uint64), total


def sent_live(n_peers, root, live, n_msgs, parent=None, csr=None):
    """sent counted over live children only: for a tree, what the children
    receive."""
    recv, _, _ = topic_load(n_peers, root, live, n_msgs, parent=parent, csr=csr)
    live = np.asarray(live).astype(bool)
    if csr is None:
        par = np.asarray(parent, dtype=np.uint32).copy()
        par[root] = NONE
        rp, cl = O.parents_to_csr(par)
    else:
        rp, cl = (np.asarray(x, dtype=np.uint32) for x in csr)
    member = csr_members(rp, cl, root)
    out = np.zeros(n_peers, dtype=np.int64)
    for p in np.nonzero(member)[0]:
        k = n_msgs if p == root else int(recv[p])
        out[p] = k * int(live[cl[int(rp[p]):int(rp[p + 1])]].sum())
    return out
