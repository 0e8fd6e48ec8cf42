"""The expected totals of the spread tracker (ps_spread_track / ps_spread_take,
DESIGN.md §5.5t) restated in plain numpy: the sum of spread_ref.window_spread
over the windows between two takes.  No engine call, no GPU.

A window is what window_spread takes: a list of topics (row_ptr, col, root,
got, c), one per standing topic in request order (c == 0: the topic was idle
in that window).  stranded and dup are taken as the sums of their parts: a
window's holders minus its visited nodes, and its copies minus its recv
(modulo 2^64), summed.
"""
from __future__ import annotations

import numpy as np

import spread_ref as SR

NAMES = ("reached", "deliv", "unreached", "stranded", "copies", "dup")


def zeros(n_peers: int, n_topics: int) -> dict:
    """The totals after a take or a track call."""
    return {"reached": np.zeros((n_topics, SR.COLS), dtype=np.uint64), "deliv": np.zeros((n_topics, SR.COLS), dtype=np.uint64),
            "unreached": np.zeros(n_topics, dtype=np.uint64), "stranded": np.zeros(n_topics, dtype=np.uint64),
            "copies": np.zeros(n_peers, dtype=np.uint64), "dup": np.zeros(n_peers, dtype=np.uint64)}


def add(total: dict, part: dict) -> dict:
    """part (window_spread's arrays, or a blocking answer's) added into total,
    modulo 2^64 as the device adds."""
    with np.errstate(over="ignore"):
        for name in NAMES:
            total[name] += part[name].astype(np.uint64)
    return total


def windows_spread(n_peers: int, windows) -> dict:
    """The six arrays as ps_spread_take writes them after the windows
    `windows` (a list of window_spread topic lists of one length), with
    n_windows."""
    windows = list(windows)
    n_topics = len(windows[0]) if windows else 0
    total = zeros(n_peers, n_topics)
    for topics in windows:
        assert len(topics) == n_topics
        add(total, SR.window_spread(n_peers, topics))
    total["n_windows"] = len(windows)
    return total


def truncated(topic, cap: int) -> dict:
    """One topic's window cut short after `cap` level launches (launches 0 ..
    cap - 1): launch L gives hop L + 1, so the forwarders up to hop `cap` are
    visited and counted, those beyond are stranded, and only the forwarders
    up to hop cap - 1 have sent their copies.  Returns window_spread's arrays
    for the one-topic request, with `truncated`: the frontier launch `cap`
    would have read holds somebody."""
    rp, cl, root, got, c = topic
    S = SR.topic_spread(rp, cl, root, got, c)
    n = len(S.level)
    lvl = S.level
    out = zeros(n, 1)
    nonroot = np.ones(n, dtype=bool)
    nonroot[root] = False
    k = S.recv
    vis = nonroot & (lvl > 0) & (lvl <= cap)
    np.add.at(out["reached"][0], np.minimum(lvl[vis], SR.COLS - 1), 1)
    np.add.at(out["deliv"][0], np.minimum(lvl[vis], SR.COLS - 1), k[vis].astype(np.uint64))
    out["unreached"][0] = S.unreached
    out["stranded"][0] = S.stranded + int((nonroot & (lvl > cap)).sum())
    in_f = k > 0
    in_f[root] = True
    kp = k.copy()
    kp[root] = c
    copies = np.zeros(n, dtype=np.int64)
    rp64, cl64 = np.asarray(rp, dtype=np.int64), np.asarray(cl, dtype=np.int64)
    for q in np.flatnonzero((lvl >= 0) & (lvl < cap)):
        for u in cl64[rp64[q]:rp64[q + 1]]:
            if in_f[u]:
                copies[u] += kp[q]
    out["copies"] = copies.astype(np.uint64)
    out["dup"] = (copies - k).astype(np.uint64)
    out["truncated"] = bool((lvl == cap).any())
    return out
