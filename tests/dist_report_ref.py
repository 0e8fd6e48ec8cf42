"""The expected share of every rank in ps_dist_report: the
per-topic references' per-node values -- a topic has one node per peer, so a
per-peer array of one topic is per node -- masked to the nodes a rank owns and
summed over the request.  No engine call, no GPU, and no arithmetic of its own
beyond the masking and the per-level histogram of owned nodes.

  rank_reports(n_peers, live, topics, owners, world, what) -> [dict per rank]
    topics = [(root, n_msgs, parent), ...] in request order (trees only: a
    multi-rank engine holds no meshes); owners[i]: topic i's owner rank per
    peer, -1 outside its tree (dist_ref.owner_peer / owner_subtree)
    LOAD        recv, sent      load_ref.topic_load
    HOPS        nodes, reached, deliv   dist_ref.bfs_levels / reach_levels with
                                hops_ref.clamp_hist (row i: topics[i])
    DOWNSTREAM  below, carried  downstream_ref.topic_downstream
"""
from __future__ import annotations

import numpy as np

import dist_ref as DR
import downstream_ref as DSR
import hops_ref as HR
import load_ref as LR

LOAD, HOPS, DOWNSTREAM, DIST = 0x1, 0x2, 0x4, 0x7
SECTIONS = ((LOAD, ("recv", "sent")), (HOPS, ("nodes", "reached", "deliv")), (DOWNSTREAM, ("below", "carried")))


def names_of(what):
    """The arrays of the sections selected in `what`, in ps_report's order."""
    return tuple(k for sec, names in SECTIONS if what & sec for k in names)


def owners_of(trees, roots, world, subtree=False, split_depth=0):
    """Every topic's owner rank per peer, -1 outside its tree: the peer hash,
    or (subtree) the subtree partition with its split level."""
    out = []
    for parent, root in zip(trees, roots):
        par = np.asarray(parent, dtype=np.uint32).copy()
        par[root] = DR.NONE
        if subtree:
            out.append(DR.owner_subtree(par, root, world, split_depth))
        else:
            out.append(np.where(DR.bfs_levels(par, root) >= 0, DR.owner_peer(np.arange(par.shape[0]), world), -1))
    return out


def topic_values(n_peers, live, root, n_msgs, parent):
    """One topic's per-node values, int64 [n_peers] each: recv, sent, below,
    carried, the BFS level (-1 outside the tree) and whether the window
    reached the peer (the root: no)."""
    recv, sent, _ = LR.topic_load(n_peers, root, live, n_msgs, parent=parent)
    below, carried, _ = DSR.topic_downstream(n_peers, root, live, n_msgs, parent)
    par = np.asarray(parent, dtype=np.uint32).copy()
    par[root] = DR.NONE
    level = DR.bfs_levels(par, root)
    got = DR.reach_levels(par, root, live) >= 0
    got[root] = False
    return {"recv": recv, "sent": sent, "below": below, "carried": carried, "level": level, "got": got}


def rank_reports(n_peers, live, topics, owners, world, what=DIST, values=None):
    """Every rank's expected arrays: a list of `world` dicts of uint64 arrays,
    the peer-space ones [n_peers], the hop ones [len(topics), COLS].  values:
    topic_values of every topic where the caller has them already (they do not
    depend on the ranks)."""
    out = []
    for _ in range(world):
        d = {}
        for k in names_of(what):
            shape = (len(topics), HR.COLS) if k in ("nodes", "reached", "deliv") else (n_peers,)
            d[k] = np.zeros(shape, dtype=np.int64)
        out.append(d)
    for i, ((root, n_msgs, parent), own) in enumerate(zip(topics, owners)):
        if n_msgs == 0:
            continue
        v = values[i] if values is not None else topic_values(n_peers, live, root, n_msgs, parent)
        own = np.asarray(own)
        for r in range(world):
            sel = own == r
            for k in names_of(what & (LOAD | DOWNSTREAM)):
                out[r][k] += np.where(sel, v[k], 0)
            if what & HOPS:
                below_root = sel & (v["level"] >= 1)
                n_lvl = int(v["level"].max()) + 2
                nodes = np.bincount(v["level"][below_root], minlength=n_lvl)
                reached = np.bincount(v["level"][below_root & v["got"]], minlength=n_lvl)
                deliv = np.zeros(n_lvl, dtype=np.int64)  # load_ref's recv, by level
                np.add.at(deliv, v["level"][below_root], v["recv"][below_root])
                out[r]["nodes"][i] += HR.clamp_hist(nodes)
                out[r]["reached"][i] += HR.clamp_hist(reached)
                out[r]["deliv"][i] += HR.clamp_hist(deliv)
    return [{k: a.astype(np.uint64) for k, a in d.items()} for d in out]


def total(reports):
    """The ranks' arrays added up."""
    return {k: sum(r[k] for r in reports) for k in reports[0]}
