"""The expected hops and duplicate copies (ps_topic_spread)
restated in plain numpy.  No engine call, no GPU.

Per topic with c > 0 window messages, over child lists (row_ptr, col) in peer
space, from the peers the window reached (`got`: a bool per peer, or the
messages each peer's row holds):
  node space  the peers the root reaches over the child lists, live or not
              (load_ref.csr_members);
  k(u)        the messages u's row holds: c where `got` is a reached flag;
  F           the root plus every other node with k > 0; k'(root) = c;
  h(u)        the BFS distance from the root within F, over child entries
              (q -> u) with q in F;
  reached[min(h, COLS - 1)] += 1 and deliv[...] += k(u) for every non-root u
              in F the BFS visits;
  unreached   the non-root nodes with k == 0;
  stranded    the non-root nodes with k > 0 the BFS never visits;
  copies[u]  += k'(q) for every child entry (q -> u) with q in F and visited
              and u in F, self-loops and entries naming the root included;
  dup         = copies - recv, recv[u] = k(u) for non-root nodes.
"""
from __future__ import annotations

import numpy as np

import load_ref as LR
import oracle as O

COLS = 256  # PS_MAX_ROUNDS
NONE = 0xFFFFFFFF


class Spread:
    """One topic's answer: level (int64 per peer, -1: not visited; the root
    0), reached / deliv (int64 [COLS]), unreached, stranded (int), copies /
    recv / dup (int64 [n_peers])."""


def topic_spread(row_ptr, col, root, got, c) -> Spread:
    rp = np.asarray(row_ptr, dtype=np.int64)
    cl = np.asarray(col, dtype=np.int64)
    n = rp.shape[0] - 1
    S = Spread()
    S.level = np.full(n, -1, dtype=np.int64)
    S.reached = np.zeros(COLS, dtype=np.int64)
    S.deliv = np.zeros(COLS, dtype=np.int64)
    S.copies = np.zeros(n, dtype=np.int64)
    S.recv = np.zeros(n, dtype=np.int64)
    S.unreached = S.stranded = 0
    if c == 0:
        S.dup = S.copies.copy()
        return S
    got = np.asarray(got)
    k = (got.astype(np.int64) * c) if got.dtype == bool else got.astype(np.int64).copy()
    assert k.shape[0] == n and k.min() >= 0 and k.max() <= c
    member = LR.csr_members(rp, cl, root)
    k[root] = 0
    assert not k[~member].any()  # nothing is delivered outside the node space
    in_f = k > 0
    in_f[root] = True
    kp = k.copy()
    kp[root] = c
    S.level[root] = 0
    cur, h = [int(root)], 0
    while cur:
        h += 1
        nxt = []
        for q in cur:
            for u in cl[rp[q]:rp[q + 1]]:
                if not in_f[u]:
                    continue
                S.copies[u] += kp[q]
                if S.level[u] < 0:
                    S.level[u] = h
                    nxt.append(int(u))
        cur = nxt
    nonroot = member.copy()
    nonroot[root] = False
    vis = nonroot & (S.level > 0)
    np.add.at(S.reached, np.minimum(S.level[vis], COLS - 1), 1)
    np.add.at(S.deliv, np.minimum(S.level[vis], COLS - 1), k[vis])
    S.unreached = int((nonroot & (k == 0)).sum())
    S.stranded = int((nonroot & (k > 0) & (S.level < 0)).sum())
    S.recv = np.where(nonroot, k, 0)
    S.dup = S.copies - S.recv
    return S


def tree_csr(parent, root):
    """A parent array's child lists (oracle.parents_to_csr), the root's own
    parent entry dropped."""
    par = np.asarray(parent, dtype=np.uint32).copy()
    par[root] = NONE
    return O.parents_to_csr(par)


def window_spread(n_peers, topics):
    """A request over several topics: topics = [(row_ptr, col, root, got, c),
    ...] (c == 0: an idle topic, the rest ignored).  Returns the six arrays as
    ps_topic_spread writes them: reached, deliv uint64 [n, COLS]; unreached,
    stranded uint64 [n]; copies, dup uint64 [n_peers] (dup modulo 2^64)."""
    n = len(topics)
    out = {"reached": np.zeros((n, COLS), dtype=np.uint64), "deliv": np.zeros((n, COLS), dtype=np.uint64),
           "unreached": np.zeros(n, dtype=np.uint64), "stranded": np.zeros(n, dtype=np.uint64)}
    copies = np.zeros(n_peers, dtype=np.int64)
    dup = np.zeros(n_peers, dtype=np.int64)
    for i, (rp, cl, root, got, c) in enumerate(topics):
        if c == 0:
            continue
        S = topic_spread(rp, cl, root, got, c)
        out["reached"][i] = S.reached.astype(np.uint64)
        out["deliv"][i] = S.deliv.astype(np.uint64)
        out["unreached"][i] = S.unreached
        out["stranded"][i] = S.stranded
        copies += S.copies
        dup += S.dup
    out["copies"] = copies.astype(np.uint64)
    out["dup"] = dup.astype(np.uint64)  # (two's complement: copies - recv modulo 2^64)
    return out
