"""The expected report (ps_peer_report / ps_report_track): the
four existing references composed per window, section by section.  No engine
call, no GPU, and no arithmetic of its own beyond the mesh rule: a topic given
by child lists (a mesh) feeds the load section alone.

  window_report(n_peers, live, topics, what) -> dict of the selected arrays
    topics = [(root, n_msgs, parent or None, csr or None), ...] in request order
    LOAD        recv, sent                      load_ref.window_load
    HOPS        nodes, reached, deliv           hops_ref.window_hops (row i: topics[i])
    DOWNSTREAM  below, carried                  downstream_ref.window_downstream
    CUT         missed, cuts, orphaned, lost    cut_ref.window_cut
"""
from __future__ import annotations

import numpy as np

import cut_ref as CR
import downstream_ref as DR
import hops_ref as HR
import load_ref as LR

LOAD, HOPS, DOWNSTREAM, CUT, ALL = 0x1, 0x2, 0x4, 0x8, 0xF
SECTIONS = ((LOAD, ("recv", "sent")), (HOPS, ("nodes", "reached", "deliv")), (DOWNSTREAM, ("below", "carried")),
            (CUT, ("missed", "cuts", "orphaned", "lost")))
NAMES = tuple(k for _, names in SECTIONS for k in names)


def names_of(what):
    """The arrays of the sections selected in `what`, in ps_report's order."""
    return tuple(k for sec, names in SECTIONS if what & sec for k in names)


def window_report(n_peers, live, topics, what=ALL):
    """One window's report over `topics` (request order).  A mesh topic (parent
    None, csr given) adds its load section and nothing else; its hop row stays
    zero."""
    out = {}
    trees = [(root, c, parent) for root, c, parent, csr in topics if csr is None]
    if what & LOAD:
        out["recv"], out["sent"], _ = LR.window_load(n_peers, live, topics)
    if what & HOPS:
        rows = [i for i, t in enumerate(topics) if t[3] is None]
        nodes, reached, deliv, _ = HR.window_hops(n_peers, live, trees)
        for k, a in (("nodes", nodes), ("reached", reached), ("deliv", deliv)):
            out[k] = np.zeros((len(topics), HR.COLS), dtype=np.uint64)
            out[k][rows] = a
    if what & DOWNSTREAM:
        out["below"], out["carried"], _ = DR.window_downstream(n_peers, live, trees)
    if what & CUT:
        out["missed"], out["cuts"], out["orphaned"], out["lost"] = CR.window_cut(n_peers, live, trees)[:4]
    return out


def add(total, part):
    """part's arrays added into total's (the same keys and shapes)."""
    for k, a in part.items():
        total[k] = total[k] + a if k in total else a.copy()
    return total
