"""The expected share of every rank in ps_dist_blame:
blame_ref.topic_blame's table per topic -- a tree topic has one node per peer,
so the table is keyed by peer -- masked to the nodes a rank owns
(dist_report_ref.owners_of).  No engine call, no GPU, and no arithmetic of its
own beyond the masking.

A rank numbers its nodes in an order of its own, so a rank's records of one
topic are compared as a set keyed by peer (compare), plus the one rule the
order must keep: hop never decreases within a topic.

  share(table, own, r)  -> the five arrays of rank r's records of one topic,
                           by ascending peer
  keyed(records)        -> five arrays put in that order (peers are distinct)
  compare(got, table, own, r, what)
"""
from __future__ import annotations

import numpy as np

import blame_ref as BR

KEYS = ("peer", "cut_peer", "hop", "cut_hop", "missed")


def share(table: BR.Table, own, r):
    """Rank r's records of one topic: the peers it owns that miss messages
    (the root misses none), by ascending peer."""
    q = np.nonzero((np.asarray(own) == r) & (table.miss > 0))[0]
    return tuple(x.astype(np.uint32) for x in (q, table.cut_peer[q], table.hop[q], table.cut_hop[q], table.miss[q]))


def keyed(records):
    """Five record arrays by ascending peer; a peer appears once."""
    peer = np.asarray(records[0])
    assert np.unique(peer).size == peer.size, "a peer has two records in one topic"
    at = np.argsort(peer, kind="stable")
    return tuple(np.asarray(x)[at] for x in records)


def compare(got, table: BR.Table, own, r, what=""):
    """got: the five arrays of one rank's records of one topic, in the rank's
    order.  The set, field for field, and the order rule."""
    hop = np.asarray(got[2]).astype(np.int64)
    assert np.all(np.diff(hop) >= 0), f"{what}: hop decreases within the topic"
    want = share(table, own, r)
    have = keyed(got)
    for k, g, w in zip(KEYS, have, want):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{what} {k}: {bad.size} records differ, first peers {have[0][bad[:6]]} got {g[bad[:6]]} "
                                 f"want {w[bad[:6]]}")


def union(shares):
    """The ranks' records of one topic together, by ascending peer."""
    return keyed(tuple(np.concatenate([s[i] for s in shares]) for i in range(5)))
