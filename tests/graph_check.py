"""A plain numpy reference of the engine's node space and a
validator of the arrays ps_graph_get returns (include/psengine_plan.h).

reference() takes the topics as the caller defined them -- (root, parent
array) per topic slot -- and computes what any correct build must produce: the
member set, each member's depth, the level tables and the largest fan-out, by
a level-by-level numpy BFS that shares no code with the engine.  validate()
checks a node space against it, structure by structure, and raises GraphError
naming the first offending node.

Used by tests/test_graph_check_cpu.py (the host build through the planner
probe, and mutations the validator must reject) and tests/test_gpu_build.py
(the GPU rebuild, gbuild.hip).
"""
from __future__ import annotations

import numpy as np

import psengine as PE

NONE = 0xFFFFFFFF
ARRAYS = ("node_peer", "node_parent", "node_topic", "node_flags", "row_ptr", "col")
SIBLING_RULES = ("peer", "peer_upto_4096", "any")
SORTED_LIST_MAX = 4096  # the GPU build sorts child lists up to this length


class GraphError(AssertionError):
    pass


def read(eng) -> dict:
    """The six node arrays (int64) and every topic's table of an Engine or a
    plan.Plan."""
    g = {k: eng.graph(w).astype(np.int64) for k, w in zip(ARRAYS, range(6))}
    g["topics"] = [eng.graph_topic(t) for t in range(eng.n_topics)]
    return g


def copy(g: dict) -> dict:
    out = {k: g[k].copy() for k in ARRAYS}
    out["topics"] = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in T.items()} for T in g["topics"]]
    return out


def reference(n_peers: int, topics, live) -> dict:
    """topics[t] = None (never created, or closed) or (root, parent): parent[p]
    = p's upstream peer, NONE = none; the root's own entry is ignored.  A peer
    is a member iff its parent chain reaches the root."""
    live = np.asarray(live).astype(bool)
    assert live.shape == (n_peers,)
    out = []
    for item in topics:
        if item is None:
            out.append(None)
            continue
        root, parent = item
        par = np.asarray(parent, dtype=np.int64).copy()
        assert par.shape == (n_peers,)
        par[root] = NONE
        has_up = par != NONE
        up = np.where(has_up, par, 0)
        depth_of = np.full(n_peers, -1, dtype=np.int64)
        depth_of[root] = 0
        level_count = [1]
        d = 0
        while True:  # level d + 1 = the unplaced peers whose upstream sits at level d
            nxt = has_up & (depth_of == -1) & (depth_of[up] == d)
            k = int(nxt.sum())
            if k == 0:
                break
            d += 1
            depth_of[nxt] = d
            level_count.append(k)
        member = depth_of >= 0
        kid = member & has_up  # every member but the root
        n_child = np.bincount(par[kid], minlength=n_peers).astype(np.int64)
        level_internal = np.bincount(depth_of[member & (n_child > 0)], minlength=d + 1).astype(np.int64)
        out.append({"root": int(root), "parent": par, "depth_of": depth_of, "members": np.nonzero(member)[0],
                    "n_child": n_child, "depth": d, "level_count": np.array(level_count, dtype=np.int64),
                    "level_internal": level_internal, "max_deg": int(n_child[member].max())})
    return {"n_peers": n_peers, "live": live, "topics": out}


def _first(mask) -> int:
    return int(np.nonzero(mask)[0][0])


def validate(g: dict, ref: dict, sibling_rule: str = "peer") -> None:
    """Raises GraphError unless g (read()) is a node space of ref
    (reference()) on one rank, siblings ordered by sibling_rule: "peer" =
    ascending peer id under every parent; "peer_upto_4096" = ascending for
    lists of at most 4096 children, any order of the right children for longer
    ones; "any" = any order of the right children."""
    if sibling_rule not in SIBLING_RULES:
        raise ValueError(sibling_rule)
    peer, parent, topic, flags, row_ptr, col = (g[k] for k in ARRAYS)
    live = ref["live"]
    if len(g["topics"]) != len(ref["topics"]):
        raise GraphError(f"{len(g['topics'])} topic slots, reference has {len(ref['topics'])}")
    n_total = peer.shape[0]
    for k in ARRAYS[1:4]:
        if g[k].shape[0] != n_total:
            raise GraphError(f"{k} has {g[k].shape[0]} entries, node_peer {n_total}")
    if row_ptr.shape[0] != n_total + 1:
        raise GraphError(f"row_ptr has {row_ptr.shape[0]} entries for {n_total} nodes")
    # layout: the existing topics back to back from node 0, in topic order
    run = 0
    ebase = 0
    for t, (T, R) in enumerate(zip(g["topics"], ref["topics"])):
        if R is None:
            if T["exists"] or T["n_nodes"]:
                raise GraphError(f"topic {t} does not exist: exists {T['exists']}, {T['n_nodes']} nodes")
            if (topic == t).any():
                raise GraphError(f"topic {t} does not exist: node {_first(topic == t)} belongs to it")
            continue
        n = R["members"].shape[0]
        if not T["exists"]:
            raise GraphError(f"topic {t} exists in the reference only")
        if T["nbase"] != run:
            raise GraphError(f"topic {t}: nbase {T['nbase']}, its predecessors end at {run}")
        if T["n_nodes"] != n:
            raise GraphError(f"topic {t}: {T['n_nodes']} nodes, {n} members")
        nb = run
        run += n
        if run > n_total:
            raise GraphError(f"topic {t} ends at node {run} of {n_total}")
        sl = slice(nb, nb + n)
        if (topic[sl] != t).any():
            u = nb + _first(topic[sl] != t)
            raise GraphError(f"topic {t}: node {u} has node_topic {topic[u]}")
        # membership: each member once
        P = peer[sl]
        if (P < 0).any() or (P >= ref["n_peers"]).any():
            u = nb + _first((P < 0) | (P >= ref["n_peers"]))
            raise GraphError(f"topic {t}: node {u} holds peer {peer[u]}")
        if (R["depth_of"][P] < 0).any():
            u = nb + _first(R["depth_of"][P] < 0)
            raise GraphError(f"topic {t}: node {u} holds peer {peer[u]}, which is no member")
        seen_at = np.full(ref["n_peers"], -1, dtype=np.int64)
        seen_at[P[::-1]] = np.arange(nb + n - 1, nb - 1, -1)  # the first node of each peer
        dup = seen_at[P] != np.arange(nb, nb + n)
        if dup.any():
            u = nb + _first(dup)
            raise GraphError(f"topic {t}: node {u} repeats peer {peer[u]} of node {seen_at[peer[u]]}")
        node_of = seen_at  # (n distinct members in n nodes: every member is there)
        # parents
        if peer[nb] != R["root"] or parent[nb] != NONE:
            raise GraphError(f"topic {t}: node {nb} is peer {peer[nb]} with parent {parent[nb]}, not the root "
                             f"{R['root']}")
        want_par = node_of[R["parent"][P[1:]]]
        if (parent[nb + 1:nb + n] != want_par).any():
            u = nb + 1 + _first(parent[nb + 1:nb + n] != want_par)
            raise GraphError(f"topic {t}: node {u} (peer {peer[u]}) has parent node {parent[u]}, its upstream "
                             f"peer {R['parent'][peer[u]]} is node {want_par[u - nb - 1]}")
        # BFS order and the level tables
        dep = R["depth_of"][P]
        if (np.diff(dep) < 0).any():
            u = nb + 1 + _first(np.diff(dep) < 0)
            raise GraphError(f"topic {t}: node {u} at depth {dep[u - nb]} follows depth {dep[u - nb - 1]}")
        if n > 2 and (np.diff(parent[nb + 1:nb + n]) < 0).any():
            u = nb + 2 + _first(np.diff(parent[nb + 1:nb + n]) < 0)
            raise GraphError(f"topic {t}: node {u}'s parent {parent[u]} is below node {u - 1}'s {parent[u - 1]}")
        want_off = np.concatenate([[0], np.cumsum(R["level_count"])])
        if T["depth"] != R["depth"]:
            raise GraphError(f"topic {t}: depth {T['depth']}, reference {R['depth']}")
        if not np.array_equal(T["level_off"], want_off):
            raise GraphError(f"topic {t}: level_off {T['level_off'].tolist()[:12]}.., reference "
                             f"{want_off.tolist()[:12]}..")
        if not np.array_equal(T["level_internal"], R["level_internal"]):
            raise GraphError(f"topic {t}: level_internal {T['level_internal'].tolist()[:12]}.., reference "
                             f"{R['level_internal'].tolist()[:12]}..")
        if T["max_deg"] != R["max_deg"]:
            raise GraphError(f"topic {t}: max_deg {T['max_deg']}, reference {R['max_deg']}")
        # CSR: a node's children are row_ptr[u] .. row_ptr[u + 1], one
        # contiguous node range (col = the identity shifted by one per topic)
        deg = R["n_child"][P]
        want_rp = ebase + np.concatenate([[0], np.cumsum(deg)])
        if (row_ptr[nb:nb + n + 1] != want_rp).any():
            u = nb + _first(row_ptr[nb:nb + n + 1] != want_rp)
            raise GraphError(f"topic {t}: row_ptr[{u}] = {row_ptr[u]}, reference {want_rp[u - nb]}"
                             + (" (the topic's closing entry)" if u == nb + n else ""))
        if col.shape[0] < ebase + n - 1:
            raise GraphError(f"topic {t}: col has {col.shape[0]} entries, the topic's edges end at {ebase + n - 1}")
        C = col[ebase:ebase + n - 1]
        if (C != np.arange(nb + 1, nb + n)).any():
            k = ebase + _first(C != np.arange(nb + 1, nb + n))
            raise GraphError(f"topic {t}: col[{k}] = {col[k]}, reference {nb + 1 + k - ebase}")
        owner = np.repeat(np.arange(nb, nb + n), deg)
        if (parent[C] != owner).any():
            k = ebase + _first(parent[C] != owner)
            raise GraphError(f"topic {t}: col[{k}] = {col[k]} lies in node {owner[k - ebase]}'s list, its parent "
                             f"is {parent[col[k]]}")
        ebase += n - 1
        # flags: live from the mask (the root always), internal iff children
        want_fl = (live[P] * PE.NODE_LIVE) | ((deg > 0) * PE.NODE_INTERNAL)
        want_fl[0] |= PE.NODE_LIVE
        if (flags[sl] != want_fl).any():
            u = nb + _first(flags[sl] != want_fl)
            raise GraphError(f"topic {t}: node {u} (peer {peer[u]}, {deg[u - nb]} children) has flags "
                             f"{flags[u]}, reference {want_fl[u - nb]}")
        # sibling order
        if sibling_rule != "any" and n > 2:
            sib = parent[nb + 2:nb + n] == parent[nb + 1:nb + n - 1]  # node u and u - 1 share a parent
            bad = sib & (peer[nb + 2:nb + n] < peer[nb + 1:nb + n - 1])
            if sibling_rule == "peer_upto_4096":
                bad &= deg[parent[nb + 2:nb + n] - nb] <= SORTED_LIST_MAX
            if bad.any():
                u = nb + 2 + _first(bad)
                raise GraphError(f"topic {t}: siblings {u - 1}, {u} under node {parent[u]} hold peers "
                                 f"{peer[u - 1]}, {peer[u]}: not ascending")
    if run != n_total:
        raise GraphError(f"{n_total} nodes, the topics hold {run}")
    if col.shape[0] != ebase:
        raise GraphError(f"col has {col.shape[0]} entries, the topics hold {ebase} edges")
