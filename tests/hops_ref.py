"""The expected deliveries by hop (ps_topic_hops / ps_hops_track, DESIGN.md
§5.5j) from the oracle alone.  No engine call, no GPU.

Per tree topic with c > 0 window messages, over columns h in [0, COLS):
  deliv[h]   = the entries of oracle.disseminate's hop table equal to h over
               non-root peers, hops of COLS - 1 and more in the last column;
  reached[h] = the peers with any entry at h;
  nodes[h]   = the members at BFS level h (graph_check.reference's depth_of),
               live or not: load_ref.py's convention for who is a node.
The oracle's hop table is a byte per entry and stops counting at 254; its hop
histogram does not (it is asked for 2 * COLS bins here).  So deliv comes from
the histogram, checked against the table below 254, and a peer the table
places at 254 stands at its BFS level: on a tree the path is unique and a
delivered peer's hop is its depth, which is asserted for every entry.
"""
from __future__ import annotations

import numpy as np

import graph_check as GC
import oracle as O

NONE = 0xFFFFFFFF
COLS = 256  # PS_MAX_ROUNDS
HOP_CAP = 254  # psoracle's hop bytes hold min(hop, 254)


def clamp_hist(by_level):
    """A per-level count as a row of COLS columns: the last one takes every
    level from COLS - 1 on."""
    by_level = np.asarray(by_level, dtype=np.int64)
    out = np.zeros(COLS, dtype=np.int64)
    k = min(by_level.size, COLS - 1)
    out[:k] = by_level[:k]
    out[COLS - 1] = by_level[COLS - 1:].sum()
    return out


def topic_hops(n_peers, root, live, n_msgs, parent):
    """(nodes, reached, deliv, oracle deliveries) of one tree topic's window of
    n_msgs messages; int64 [COLS] each.  parent: the tree's upstream array."""
    zero = np.zeros(COLS, dtype=np.int64)
    if n_msgs == 0:
        return zero, zero.copy(), zero.copy(), 0
    live = np.asarray(live, dtype=np.uint8)
    par = np.asarray(parent, dtype=np.uint32).copy()
    par[root] = NONE
    R = GC.reference(n_peers, [(root, par)], np.ones(n_peers, dtype=np.uint8))["topics"][0]
    depth_of = R["depth_of"]
    member = depth_of >= 0
    n_lvl = max(int(depth_of.max()) + 1, 2)
    rp, cl = O.parents_to_csr(par)
    tot, hops, hist = O.disseminate(rp, cl, root, live, n_msgs, hist_len=max(2 * COLS, n_lvl + 1))
    got = hops != 0xFF
    got[:, root] = False
    assert not got[:, ~member].any()
    # a tree: every delivery arrives at its peer's BFS level
    want_byte = np.minimum(depth_of, HOP_CAP)
    assert (hops[got] == np.broadcast_to(want_byte, hops.shape)[got]).all()
    hist = hist.astype(np.int64)
    assert hist[0] == 0 and hist.sum() == tot == got.sum()
    any_got = got.any(axis=0)
    nodes = np.bincount(depth_of[member], minlength=n_lvl)
    nodes[0] = 0  # the root is no recipient
    reached = np.bincount(depth_of[any_got], minlength=n_lvl)
    deliv = np.zeros(n_lvl, dtype=np.int64)
    np.add.at(deliv, depth_of[member], got.sum(axis=0)[member])
    assert np.array_equal(deliv, hist[:n_lvl]) and not hist[n_lvl:].any()
    return clamp_hist(nodes), clamp_hist(reached), clamp_hist(deliv), tot


def window_hops(n_peers, live, topics):
    """A window over several topics: topics = [(root, n_msgs, parent), ...].
    Returns (nodes, reached, deliv, deliveries): uint64 [len(topics), COLS]
    each, row i for topics[i], and the oracle's deliveries summed."""
    rows = [topic_hops(n_peers, root, live, n_msgs, parent) for root, n_msgs, parent in topics]
    out = tuple(np.array([r[k] for r in rows], dtype=np.int64).reshape(len(rows), COLS).astype(np.uint64) for k in range(3))
    return out + (sum(r[3] for r in rows),)
