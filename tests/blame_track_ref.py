"""The expected answer of ps_blame_take from the oracle alone:
blame_ref's records composed window by window into the cumulative rec_off and
the five record arrays.  No engine call, no GPU.

A window is a list with one entry per request position: blame_ref.records'
five arrays for the topic tracked there (blame_ref.topic_blame or from_parents
over the window's messages and mask, listed in the node order of the node space
the window ran on), or None where the position holds no record -- the topic is
idle in the window, or a mesh there and skipped.  compose() strings the windows
together in enqueue order; capped() cuts the answer down to what a cap keeps:
records are stored densely in order, none at or past the cap, and the counts
and offsets stay exact.
"""
from __future__ import annotations

import numpy as np

import blame_ref as BR

KEYS = ("peer", "cut_peer", "hop", "cut_hop", "missed")


def window(tables, orders):
    """One window's row: tables[i] is the blame_ref.Table of request position
    i (None: no record there), orders[i] the peers of its nodes in node order,
    the root's first."""
    return [None if t is None else BR.records(t, orders[i]) for i, t in enumerate(tables)]


def compose(windows, n, n_skipped=0) -> dict:
    """ps_blame_take's answer without a cap over `windows` (rows of n entries)."""
    off = [0]
    recs = [[] for _ in KEYS]
    for row in windows:
        assert len(row) == n
        for r in row:
            k = 0 if r is None else int(r[0].size)
            off.append(off[-1] + k)
            if k:
                for dst, a in zip(recs, r):
                    assert a.size == k
                    dst.append(np.asarray(a, dtype=np.uint32))
    out = {"rec_off": np.asarray(off, dtype=np.uint64)}
    for key, parts in zip(KEYS, recs):
        out[key] = np.concatenate(parts).astype(np.uint32) if parts else np.empty(0, dtype=np.uint32)
    out.update(n_windows=len(windows), n_skipped=n_skipped, total=off[-1], stored=off[-1])
    return out


def capped(full: dict, cap: int):
    """(answer, overflowed) under a cap of `cap` records: the prefix kept."""
    out = dict(full)
    stored = min(int(full["total"]), int(cap))
    for key in KEYS:
        out[key] = full[key][:stored]
    out["stored"] = stored
    return out, int(full["total"]) > int(cap)


def slice_of(res: dict, n: int, w: int, i: int):
    """The five arrays of window w, request position i (within what was stored)."""
    off = res["rec_off"].astype(np.int64)
    lo, hi = int(off[w * n + i]), int(off[w * n + i + 1])
    return tuple(res[k][lo:hi] for k in KEYS)
