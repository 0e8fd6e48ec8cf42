"""CPU: the node-space validator (tests/graph_check.py) on host-built node
spaces -- the planner probe's (ps_plan_create), read through ps_graph_get --
and proof that it bites: each mutation of a valid node space that the flood
kernels would index without noticing must be rejected."""
import numpy as np
import pytest

import graph_check as GC
import psengine as PE
from psengine import plan as PL

NONE = GC.NONE


def random_tree(n, rng, fan=4, members=1.0, perm=True):
    """A tree over a random subset of n peers with permuted labels: BFS slot i
    hangs below a random earlier slot within a window of about `fan`."""
    m = max(1, int(n * members))
    lab = rng.permutation(n)[:m] if perm else np.arange(m)
    parent = np.full(n, NONE, dtype=np.uint32)
    for i in range(1, m):
        parent[lab[i]] = lab[int(rng.integers(max(0, (i - 1) // fan - 1), (i - 1) // fan + 1))]
    return int(lab[0]), parent


def probe_case(name):
    if name == "lone_root":
        n = 5
        return n, [(3, np.full(n, NONE, dtype=np.uint32))]
    if name == "chain":
        n = 40
        par = np.full(n, NONE, dtype=np.uint32)
        par[1:] = np.arange(n - 1)
        return n, [(0, par)]
    if name == "star":
        n = 100
        par = np.zeros(n, dtype=np.uint32)
        par[0] = NONE
        return n, [(0, par)]
    if name == "random":
        return 700, [random_tree(700, np.random.default_rng(5))]
    if name == "partial_with_stray_cycle":
        n = 300
        root, par = random_tree(n, np.random.default_rng(6), members=0.6)
        out = np.nonzero((par == NONE) & (np.arange(n) != root))[0]
        par[out[0]], par[out[1]] = out[1], out[0]  # two outsiders pointing at each other: no members
        par[out[2]] = out[0]
        return n, [(root, par)]
    if name == "three_topics":
        n = 400
        return n, [random_tree(n, np.random.default_rng(7), fan=2),
                   (9, np.full(n, NONE, dtype=np.uint32)),
                   random_tree(n, np.random.default_rng(8), fan=9, members=0.5)]
    raise KeyError(name)


CASES = ("lone_root", "chain", "star", "random", "partial_with_stray_cycle", "three_topics")


def build_probe(n, topics):
    par = np.stack([p for _, p in topics])
    return PL.Plan(par, [r for r, _ in topics])


@pytest.mark.parametrize("name", CASES)
def test_host_build_validates(name):
    n, topics = probe_case(name)
    p = build_probe(n, topics)
    g = GC.read(p)
    ref = GC.reference(n, topics, np.ones(n, dtype=np.uint8))
    GC.validate(g, ref, "peer")
    GC.validate(g, ref, "peer_upto_4096")
    GC.validate(g, ref, "any")
    rep = p.build_report()
    assert (rep["gpu_builds"], rep["host_builds"], rep["last_kind"], rep["last_attempts"]) == (0, 1, "host", 0)
    assert rep["fallbacks"] == 0 and rep["redos"] == 0
    assert sum(len(R["members"]) for R in ref["topics"]) == g["node_peer"].shape[0]
    p.close()


def test_reference_by_hand():
    """The reference itself on a tree small enough to write down."""
    #        4
    #      / | \
    #     0  2  6      5 -> 7 -> 5 is a stray cycle, 1 hangs below it, 3 has no upstream
    #    / \     \
    #   8   9     10
    par = np.array([4, 5, 4, NONE, 0, 7, 4, 5, 0, 0, 6], dtype=np.uint32)  # (the root's own entry is ignored)
    R = GC.reference(11, [None, (4, par)], np.ones(11))["topics"]
    assert R[0] is None
    r = R[1]
    assert r["members"].tolist() == [0, 2, 4, 6, 8, 9, 10]
    assert r["depth_of"].tolist() == [1, -1, 1, -1, 0, -1, 1, -1, 2, 2, 2]
    assert (r["depth"], r["max_deg"]) == (2, 3)
    assert r["level_count"].tolist() == [1, 3, 3] and r["level_internal"].tolist() == [1, 2, 0]


def test_graph_get_conventions():
    n, topics = probe_case("random")
    p = build_probe(n, topics)
    L = PL.lib()
    import ctypes as C

    cnt = C.c_size_t()
    out = (C.c_uint64 * 4)()
    assert L.ps_graph_get(p._h, PE.G_NODE_PEER, 0, out, 4, C.byref(cnt)) == -7  # PS_E_RANGE, *n_out = the need
    assert cnt.value == n
    assert L.ps_graph_get(p._h, 99, 0, out, 4, C.byref(cnt)) == -1
    assert L.ps_graph_get(p._h, PE.G_TOPIC, 5, out, 4, C.byref(cnt)) == -7  # no such topic slot
    assert L.ps_graph_get(p._h, PE.G_BUILD, 0, None, 0, C.byref(cnt)) == -7 and cnt.value == len(PE.BUILD_FIELDS)
    # the older reader of the same arrays agrees
    assert np.array_equal(p.get(PL.NODES), p.graph(PE.G_NODE_PEER))
    assert np.array_equal(p.get(PL.PARENT), p.graph(PE.G_NODE_PARENT))
    p.close()


@pytest.fixture(scope="module")
def valid():
    """One valid node space of three topics (the middle one a lone root),
    10 % of the peers dead, for the mutations below."""
    n, topics = probe_case("three_topics")
    p = build_probe(n, topics)
    g = GC.read(p)
    p.close()
    # (the probe's flags are built with every peer live; validated so, then
    # the live bits rewritten for a mask with dead peers)
    GC.validate(g, GC.reference(n, topics, np.ones(n)), "peer")
    live = (np.random.default_rng(1).random(n) > 0.1).astype(np.uint8)
    for T, (root, _) in zip(g["topics"], topics):
        sl = slice(T["nbase"], T["nbase"] + T["n_nodes"])
        g["node_flags"][sl] = (g["node_flags"][sl] & ~PE.NODE_LIVE) | live[g["node_peer"][sl]]
        g["node_flags"][T["nbase"]] |= PE.NODE_LIVE
    ref = GC.reference(n, topics, live)
    GC.validate(g, ref, "peer")
    return g, ref


def sibling_leaves(g, ref):
    """Two adjacent sibling leaves of topic 0 with the same live bit."""
    T = g["topics"][0]
    fl, par = g["node_flags"], g["node_parent"]
    for u in range(T["nbase"] + 2, T["nbase"] + T["n_nodes"]):
        if par[u] == par[u - 1] and fl[u] == fl[u - 1] and not fl[u] & PE.NODE_INTERNAL:
            return u - 1, u
    raise AssertionError("no such pair")


def leaf(g, t=0):
    T = g["topics"][t]
    sl = slice(T["nbase"], T["nbase"] + T["n_nodes"])
    return T["nbase"] + int(np.nonzero((g["node_flags"][sl] & PE.NODE_INTERNAL) == 0)[0][0])


def mut_swap_siblings(g, ref):
    a, b = sibling_leaves(g, ref)
    g["node_peer"][[a, b]] = g["node_peer"][[b, a]]


def mut_duplicate_peer(g, ref):
    a, b = sibling_leaves(g, ref)
    g["node_peer"][b] = g["node_peer"][a]


def mut_level_off(g, ref):
    g["topics"][0]["level_off"][2] += 1


def mut_col(g, ref):
    g["col"][g["topics"][2]["nbase"] + 3] += 1


def mut_level_internal(g, ref):
    g["topics"][2]["level_internal"][1] -= 1


def mut_live_bit(g, ref):
    g["node_flags"][leaf(g, 2)] ^= PE.NODE_LIVE


def mut_internal_on_leaf(g, ref):
    g["node_flags"][leaf(g, 0)] |= PE.NODE_INTERNAL


def mut_max_deg(g, ref):
    g["topics"][0]["max_deg"] += 1


def mut_nbase(g, ref):
    g["topics"][2]["nbase"] += 1


def mut_row_ptr_closing(g, ref):
    T = g["topics"][0]
    g["row_ptr"][T["nbase"] + T["n_nodes"]] += 1


def mut_parent(g, ref):
    a, _ = sibling_leaves(g, ref)
    g["node_parent"][a] -= 1


def mut_node_topic(g, ref):
    g["node_topic"][g["topics"][2]["nbase"]] = 1


def mut_split_bit(g, ref):
    g["node_flags"][leaf(g, 0)] |= PE.NODE_SPLIT


def mut_lone_root_gets_depth(g, ref):
    g["topics"][1]["depth"] = 1


def mut_closed_topic_exists(g, ref):
    ref["topics"][1] = None  # (the reference says: no such topic; the node space still holds its root)


MUTATIONS = [mut_swap_siblings, mut_duplicate_peer, mut_level_off, mut_col, mut_level_internal, mut_live_bit,
             mut_internal_on_leaf, mut_max_deg, mut_nbase,
             # beyond the listed nine
             mut_row_ptr_closing, mut_parent, mut_node_topic, mut_split_bit, mut_lone_root_gets_depth,
             mut_closed_topic_exists]


@pytest.mark.parametrize("mutate", MUTATIONS, ids=lambda f: f.__name__[4:])
def test_validator_rejects(valid, mutate):
    g0, ref0 = valid
    g = GC.copy(g0)
    ref = dict(ref0, topics=list(ref0["topics"]))
    mutate(g, ref)
    with pytest.raises(GC.GraphError):
        GC.validate(g, ref, "peer")
    GC.validate(g0, ref0, "peer")  # (the shared node space is untouched)


def test_sibling_rules(valid):
    """Swapped siblings pass "any", fail "peer", and fail "peer_upto_4096"
    (their list is short); the membership and parent checks hold for all."""
    g0, ref = valid
    g = GC.copy(g0)
    mut_swap_siblings(g, ref)
    GC.validate(g, ref, "any")
    for rule in ("peer", "peer_upto_4096"):
        with pytest.raises(GC.GraphError, match="not ascending"):
            GC.validate(g, ref, rule)
    with pytest.raises(ValueError):
        GC.validate(g, ref, "none")
