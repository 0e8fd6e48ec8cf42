"""The expected share of every rank in ps_dist_cut:
cut_ref.topic_cut's four per-peer arrays per topic -- a topic has one node per
peer, so a per-peer array of one topic is per node -- masked to the nodes a
rank owns (dist_report_ref.owners_of) and summed over the request.  No engine
call, no GPU, and no arithmetic of its own beyond the masking.

  rank_cuts(n_peers, live, topics, owners, world) -> [dict per rank]
    topics = [(root, n_msgs, parent), ...] in request order (trees only);
    owners[i]: topic i's owner rank per peer, -1 outside its tree
"""
from __future__ import annotations

import numpy as np

import cut_ref as CR

NAMES = ("missed", "cuts", "orphaned", "lost")


def topic_values(n_peers, live, root, n_msgs, parent):
    """One topic's per-node values: cut_ref.topic_cut's four arrays by name."""
    return dict(zip(NAMES, CR.topic_cut(n_peers, root, live, n_msgs, parent)[:4]))


def rank_cuts(n_peers, live, topics, owners, world, values=None):
    """Every rank's expected arrays: a list of `world` dicts of uint64
    [n_peers] arrays.  values: topic_values of every topic where the caller has
    them already (they do not depend on the ranks)."""
    out = [{k: np.zeros(n_peers, dtype=np.int64) for k in NAMES} for _ in range(world)]
    for i, ((root, n_msgs, parent), own) in enumerate(zip(topics, owners)):
        if n_msgs == 0:
            continue
        v = values[i] if values is not None else topic_values(n_peers, live, root, n_msgs, parent)
        own = np.asarray(own)
        for r in range(world):
            for k in NAMES:
                out[r][k] += np.where(own == r, v[k], 0)
    return [{k: a.astype(np.uint64) for k, a in d.items()} for d in out]


def total(shares):
    """The ranks' arrays added up."""
    return {k: sum(s[k] for s in shares) for k in NAMES}
