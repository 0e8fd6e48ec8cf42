"""GPU: the rebuild of the node space on the device (csrc/gbuild.hip, driven
by gpu_build_graph in csrc/graph.cpp), checked structurally.

Every case reads the GPU-built node space back (ps_graph_get), validates it
against a plain numpy reference (tests/graph_check.py), asserts from the
engine's build report that the GPU build -- not the silent host fall-back --
produced it (and that the retry a case is about was counted), compares it
array for array with a host-built engine where both builds promise the same
numbering (set_tree topics whose child lists hold at most 4096), and then
floods 70 recorded messages over the same engine against the oracle.  Peer
labels are permuted everywhere, so the order in which children arrive in a
list is not their peer order.

The shapes sit on the kernels' own edges: child lists of 32 / 33 (k_kid_sort
-> k_kid_sort_big) and 4096 / 4097 (the LDS sort's capacity), more long lists
than k_kid_sort_big has blocks, parent levels of 512 / 513 (k_place_top ->
k_place_lb), of 256 / 257 (one look-back tile) and 16384 / 16385 (the first
64-tile look-back window), the host loop's retries, and chains around the
depth the level tables hold.
"""
import numpy as np
import pytest

import graph_check as GC
import oracle as O
import psengine as PE

pytestmark = pytest.mark.gpu

NONE = GC.NONE
N_MSGS = 70
FALLBACKS = ("fallback_stall", "fallback_attempts", "fallback_capacity", "fallback_depth")
REDOS = ("redo_grid", "redo_order", "redo_depth")


# ---- trees ------------------------------------------------------------------

def label(n_peers, slot_parent, rng):
    """(root, parent array) of the tree slot_parent (slot 0 = the root, every
    slot's parent an earlier slot) under a random labelling of its slots."""
    sp = np.asarray(slot_parent, dtype=np.int64)
    lab = rng.permutation(n_peers)[:sp.shape[0]]
    parent = np.full(n_peers, NONE, dtype=np.uint32)
    parent[lab[1:]] = lab[sp[1:]]
    return int(lab[0]), parent


def level_slots(sizes, maxfan, rng):
    """A tree whose level d holds sizes[d] nodes, each node of level d with at
    most maxfan[d] children (drawn at random, so some have none)."""
    sp = [np.array([-1])]
    start = 0
    for d in range(1, len(sizes)):
        assert sizes[d] <= sizes[d - 1] * maxfan[d - 1], (d, sizes)
        pool = np.repeat(np.arange(start, start + sizes[d - 1]), maxfan[d - 1])
        sp.append(np.sort(rng.permutation(pool)[:sizes[d]]))
        start += sizes[d - 1]
    return np.concatenate(sp)


def hang_below(sp, first, total, maxfan, rng):
    """Extends slot list sp to `total` slots: the slots from `first` on take
    0 .. maxfan children each, in turn."""
    sp = list(sp)
    at = first
    while len(sp) < total:
        k = int(rng.integers(0, maxfan + 1))
        if at == len(sp) - 1 and k == 0:
            k = 1  # (the last candidate: keep growing)
        sp.extend([at] * min(k, total - len(sp)))
        at += 1
    return np.array(sp)


def one_list(c, rng, total=2000):
    """The root's first child holds c children; about `total` peers in all
    hang below those with fan-out <= 3."""
    sp = [-1, 0, 0] + [1] * c
    return hang_below(sp, 3, max(total, c + 400), 3, rng)


# ---- the checks ---------------------------------------------------------------

def make(n, n_topics, gpu_build):
    return PE.Engine(n, n_topics, record_hops=True, plan={"gpu_build": int(gpu_build)})


def load(eng, topics, live=None):
    for t, item in enumerate(topics):
        if item is not None:
            eng.set_tree(t, item[0], item[1])
    if live is not None:
        eng.set_live(live)


def assert_no_fallback(rep):
    assert {k: rep[k] for k in FALLBACKS} == dict.fromkeys(FALLBACKS, 0), rep


def assert_gpu_built(rep, before=None):
    """The last build ran on the GPU, nothing ever fell back to the host
    build, and (before: an earlier report) exactly one build was added."""
    assert rep["last_kind"] == "gpu" and rep["last_attempts"] >= 1, rep
    assert rep["host_builds"] == 0, rep
    assert_no_fallback(rep)
    if before is not None:
        assert rep["gpu_builds"] == before["gpu_builds"] + 1, (before, rep)


def oracle_hops(item, live):
    root, parent = item
    par = np.array(parent, dtype=np.uint32)
    par[root] = NONE
    rp, cl = O.parents_to_csr(par)
    _, hops, _ = O.disseminate(rp, cl, root, live, 1)
    return hops[0]


def flood_check(eng, topics, live):
    """70 recorded messages over the existing topics: every hop the oracle's."""
    tt = [t for t, item in enumerate(topics) if item is not None]
    want = {t: oracle_hops(topics[t], live) for t in tt}
    msgs = np.array([tt[i % len(tt)] for i in range(N_MSGS)], dtype=np.uint32)
    first = eng.publish(msgs)
    st = eng.run()
    for m in range(N_MSGS):
        got = eng.hops(first + m)
        if not np.array_equal(got, want[int(msgs[m])]):
            bad = np.nonzero(got != want[int(msgs[m])])[0][:8]
            raise AssertionError(f"msg {m} topic {msgs[m]}: peers {bad} got {got[bad]} want "
                                 f"{want[int(msgs[m])][bad]}")
    assert st.deliveries == sum(int((want[int(t)] != 0xFF).sum()) for t in msgs)


def host_arrays(n, topics, live):
    with make(n, len(topics), 0) as h:
        load(h, topics, live)
        rep = h.build_report()
        assert (rep["last_kind"], rep["gpu_builds"], rep["host_builds"]) == ("host", 0, 1), rep
        return GC.read(h)


def assert_same_arrays(g, gh):
    for k in GC.ARRAYS:
        if not np.array_equal(g[k], gh[k]):
            i = int(np.nonzero(g[k] != gh[k])[0][0]) if g[k].shape == gh[k].shape else -1
            raise AssertionError(f"{k}: GPU and host builds differ at {i} ({g[k].shape} / {gh[k].shape})")
    for t, (a, b) in enumerate(zip(g["topics"], gh["topics"])):
        for k in ("exists", "n_nodes", "depth", "max_deg", "level_off", "level_internal"):
            assert np.array_equal(a[k], b[k]), (t, k)
        if a["exists"]:
            assert a["nbase"] == b["nbase"], t


def check_step(eng, n, topics, live, rule, before=None, host_equal=None):
    """One build on `eng` (already loaded): report, structure, host equality
    (by default wherever the rule is "peer"), flood.  Returns the report."""
    rep = eng.build_report()  # (brings the node space up to date: the build under test)
    assert_gpu_built(rep, before)
    g = GC.read(eng)
    GC.validate(g, GC.reference(n, topics, live), rule)
    if host_equal is None:
        host_equal = rule == "peer"
    if host_equal:
        assert_same_arrays(g, host_arrays(n, topics, live))
    flood_check(eng, topics, live)
    after = eng.build_report()
    assert after == rep, (rep, after)  # reading the node space and flooding it built nothing more
    return rep


def check_case(n, topics, live=None, rule="peer", host_equal=None):
    live = np.ones(n, dtype=np.uint8) if live is None else live
    with make(n, len(topics), 1) as eng:
        load(eng, topics, live)
        rep = check_step(eng, n, topics, live, rule, host_equal=host_equal)
        assert rep["gpu_builds"] == 1
        return rep


# ---- the reader itself --------------------------------------------------------

def test_reader_changes_no_run_and_refuses_while_busy():
    """ps_graph_get between topology changes and runs: deliveries, hops and
    the seen digest equal those of an engine that never called it; while an
    asynchronous run or a drain is outstanding it answers PS_E_STATE."""
    rng = np.random.default_rng(3)
    n = 1500
    item = label(n, level_slots([1, 3, 9, 27, 81, 243, 600], [3] * 7, rng), rng)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    out = []
    for peek in (False, True):
        with make(n, 1, 1) as e:
            load(e, [item], live)
            if peek:
                GC.read(e)
                e.build_report()
            first = e.publish(np.zeros(N_MSGS))
            if peek:
                GC.read(e)
            st = e.run()
            if peek:
                GC.read(e)
            out.append((st.deliveries, st.rounds, e.seen_digest(), e.hops(first + N_MSGS - 1).tobytes(),
                        e.depth(0)))
            if peek:
                e.publish(np.zeros(3))
                e.run_async()
                with pytest.raises(PE.EngineError) as ei:
                    e.graph(PE.G_NODE_PEER)
                assert ei.value.code == -3
                with pytest.raises(PE.EngineError):
                    e.build_report()
                e.wait()
                e.drain_begin(np.zeros(2, dtype=np.uint32), np.array([1, 2], dtype=np.uint32))
                with pytest.raises(PE.EngineError) as ei:
                    e.graph(PE.G_ROW_PTR)
                assert ei.value.code == -3
                e.drain_end()
                assert e.graph(PE.G_NODE_PEER).shape[0] == e.depth(0)[1]
    assert out[0] == out[1]


# ---- sort edges -----------------------------------------------------------------

@pytest.mark.parametrize("c", [1, 2, 32, 33, 64, 65, 1000, 4095, 4096, 4097, 5000])
def test_child_list_lengths(c):
    """One parent with c children under permuted labels: 32 is k_kid_sort's
    last list, 33 the first of k_kid_sort_big, 4096 its last (a full power of
    two), 4097 the first that keeps its arrival order."""
    rng = np.random.default_rng(c)
    sp = one_list(c, rng)
    n = sp.shape[0] + 37  # (some peers outside the tree)
    check_case(n, [label(n, sp, rng)], rule="peer" if c <= GC.SORTED_LIST_MAX else "peer_upto_4096")


def test_more_long_lists_than_sort_blocks():
    """100 parents of 40 children each, and the root's own list of 100: 101
    long lists for k_kid_sort_big's 64 grid-striding blocks."""
    rng = np.random.default_rng(100)
    sp = [-1] + [0] * 100 + list(np.repeat(np.arange(1, 101), 40))
    sp = hang_below(sp, 101, 6000, 2, rng)
    n = sp.shape[0] + 11
    rep = check_case(n, [label(n, sp, rng)])
    assert rep["redos"] == 0


def test_lists_of_33_4096_4097_side_by_side():
    """Three sibling parents with 33, 4096 and 4097 children: the two sorted
    lists are in peer order beside one that is not sorted at all."""
    rng = np.random.default_rng(33)
    sp = [-1, 0, 0, 0] + [1] * 33 + [2] * 4096 + [3] * 4097
    sp = hang_below(sp, 4, len(sp) + 700, 3, rng)
    n = sp.shape[0] + 5
    check_case(n, [label(n, sp, rng)], rule="peer_upto_4096")


# ---- placement hand-over ------------------------------------------------------

@pytest.mark.parametrize("x", [511, 512, 513])
def test_top_kernel_hand_over(x):
    """A level 1 of x nodes, each with 0 .. 3 children, two more levels
    below: 512 parents is the last level k_place_top places itself, 513 the
    first it leaves to k_place_lb (and every level below with it)."""
    rng = np.random.default_rng(x)
    sp = level_slots([1, x, x + x // 3, x, x // 2], [x, 3, 3, 3], rng)
    n = sp.shape[0] + 23
    rep = check_case(n, [label(n, sp, rng)])
    assert rep["redos"] == 0 and rep["last_attempts"] == 1


@pytest.mark.parametrize("w", [256, 257])
def test_look_back_one_and_two_tiles(w):
    """Below a level of 600 (so k_place_lb places everything from level 2
    on), a level of w parents with 0 .. 2 children each: one tile, or one
    tile and a tile of one parent."""
    rng = np.random.default_rng(w)
    sp = level_slots([1, 600, w, w, w // 2], [600, 2, 2, 2], rng)
    n = sp.shape[0] + 9
    check_case(n, [label(n, sp, rng)])


@pytest.mark.parametrize("w", [16384, 16385, 20000])
def test_look_back_windows(w):
    """A level of w parents with 0 .. 2 children each: 64 tiles end the
    look-back's first 64-tile window, the 65th tile reads past it; 20000
    parents (about 60,000 peers) is 79 tiles."""
    rng = np.random.default_rng(w)
    k1 = -(-w // 3500)
    sp = level_slots([1, k1, w, w, w - w // 20], [k1, 4096, 2, 2], rng)
    n = sp.shape[0] + 101
    rep = check_case(n, [label(n, sp, rng)])
    assert rep["redos"] == 0 and rep["last_attempts"] == 1


# ---- retries ------------------------------------------------------------------------

def deep_tree(depth, rng):
    """Depth `depth` with a level 1 of 600 nodes (k_place_lb places the
    levels below, launch by launch) and a thin tail."""
    sizes = [1, 600, 300, 100, 20] + [3] * (depth - 4)
    return level_slots(sizes, [600] + [2] * (len(sizes) - 2), rng)


def test_retry_depth_growth():
    """set_tree of the same topic again, deeper each time.  A fresh topic
    gets look-back launches for levels 1 .. 24, a built one for its last
    depth + 2: (a) depth 8 builds in one attempt; (b) depth 30 is redone
    with more levels; (c) depth 130 takes several doublings.  No step falls
    back."""
    rng = np.random.default_rng(8)
    n = 2500
    live = np.ones(n, dtype=np.uint8)
    with make(n, 1, 1) as eng:
        item = label(n, deep_tree(8, rng), rng)
        eng.set_tree(0, *item)
        a = check_step(eng, n, [item], live, "peer")
        assert a["redos"] == 0 and a["last_attempts"] == 1 and a["gpu_builds"] == 1
        assert eng.depth(0)[0] == 8
        item = label(n, deep_tree(30, rng), rng)
        eng.set_tree(0, *item)
        b = check_step(eng, n, [item], live, "peer", before=a)
        assert b["redo_depth"] >= a["redo_depth"] + 1 and b["last_attempts"] >= 2, b
        assert (b["redo_grid"], b["redo_order"]) == (0, 0)
        assert eng.depth(0)[0] == 30
        item = label(n, deep_tree(130, rng), rng)
        eng.set_tree(0, *item)
        c = check_step(eng, n, [item], live, "peer", before=b)
        assert c["redo_depth"] >= b["redo_depth"] + 2 and c["last_attempts"] >= 3, c
        assert (c["redo_grid"], c["redo_order"]) == (0, 0)
        assert eng.depth(0)[0] == 130


def test_retry_grid_redo_after_set_tree():
    """(d) A tree of depth 3 with a level of 2,400 parents by set_tree over a
    tree that had one node at that level: it outgrows the
    lb_tiles(1 + 0 + 2048) = 9-tile grid estimated from the last build
    (set_tree keeps the last build's level sizes) and is redone with full
    grids.  (The one-node levels had also all been the top kernel's, so the
    first attempt is an order redo.)"""
    rng = np.random.default_rng(2400)
    n = 6000
    live = np.ones(n, dtype=np.uint8)
    with make(n, 1, 1) as eng:
        item = label(n, level_slots([1, 1, 1, 1], [1, 1, 1], rng), rng)
        eng.set_tree(0, *item)
        a = check_step(eng, n, [item], live, "peer")
        item = label(n, level_slots([1, 3, 2400, 3000], [3, 4096, 2], rng), rng)
        eng.set_tree(0, *item)
        d = check_step(eng, n, [item], live, "peer", before=a)
        print("report:", d)
        assert d["redo_grid"] >= a["redo_grid"] + 1, d


def test_retry_order_redo_after_set_tree():
    """(e) A tree whose level 1 has 600 parents by set_tree over a tree
    whose levels 1 to 3 all had 512 or fewer: top_levels is stale, the
    look-back launches start below a level nobody placed (kBuildErrOrder)
    and the build is redone by look-back launches from level 1."""
    rng = np.random.default_rng(600)
    n = 3000
    live = np.ones(n, dtype=np.uint8)
    with make(n, 1, 1) as eng:
        item = label(n, level_slots([1, 100, 200, 300], [100, 3, 3], rng), rng)
        eng.set_tree(0, *item)
        a = check_step(eng, n, [item], live, "peer")
        item = label(n, level_slots([1, 600, 700, 300], [600, 3, 3], rng), rng)
        eng.set_tree(0, *item)
        e = check_step(eng, n, [item], live, "peer", before=a)
        print("report:", e)
        assert e["redo_order"] >= a["redo_order"] + 1, e


def join_step(eng, n, root, before=None):
    """One GPU build of join topic 0 (before: the report taken right before
    the topology changed): report, structure against the attached tree,
    flood."""
    live = np.ones(n, dtype=np.uint8)
    rep = eng.build_report()
    assert_gpu_built(rep, before)
    item = (root, eng.parents(0))
    GC.validate(GC.read(eng), GC.reference(n, [item], live), "peer_upto_4096")
    flood_check(eng, [item], live)
    return rep


def test_retry_grid_redo_join_topic():
    """A join topic keeps its last build's level sizes.  TreeWidth 3000: the
    root takes every joiner directly.  After a build with one node at level
    1, 2,999 more joiners make level 1 a level of 3,000 parents: 12 tiles
    for the 9-tile grid estimated from the one node -- kBuildErrGrid, and
    the build is redone with full grids."""
    rng = np.random.default_rng(12)
    n = 3200
    order = rng.permutation(n)
    root = int(order[0])
    with make(n, 1, 1) as eng:
        eng.topic_create(0, root, 3000, 3000)
        eng.join(0, order[1:2])
        a = join_step(eng, n, root)
        assert a["redos"] == 0 and eng.depth(0) == (1, 2)
        a = eng.build_report()  # (after any rebuild the run's lazy prune asked for)
        eng.join(0, order[2:3150])  # 3000 below the root, the rest one level down
        b = join_step(eng, n, root, before=a)
        assert eng.depth(0) == (2, 3150)
        # (the launches below the refused level find their parent level
        # unplaced, so the same attempt may report kBuildErrOrder as well)
        assert b["redo_grid"] == a["redo_grid"] + 1 and b["last_attempts"] == 2, b
        assert b["redo_depth"] == 0


def test_retry_order_redo_join_topic():
    """TreeWidth 600.  650 joiners give levels of 600 and 50; 150 childless
    level-1 peers leave, so the next build finds levels 1 and 2 both within
    k_place_top's 512 parents and notes it (top_levels).  150 new joiners
    fill level 1 up again: the top kernel stops above the level the
    look-back launches were to start from -- kBuildErrOrder, and every
    level is redone by look-back launches."""
    rng = np.random.default_rng(13)
    n = 1000
    order = rng.permutation(n)
    root = int(order[0])
    with make(n, 1, 1) as eng:
        eng.topic_create(0, root, 600, 600)
        eng.join(0, order[1:651])
        join_step(eng, n, root)
        par = eng.parents(0)
        lvl1 = np.nonzero(par == root)[0]
        assert lvl1.shape[0] == 600 and eng.depth(0) == (2, 651)
        childless = np.setdiff1d(lvl1, par[par != NONE])
        a = eng.build_report()
        eng.leave(0, childless[:150])
        join_step(eng, n, root, before=a)  # (its flood lets the root drop the 150 that left)
        assert int((eng.parents(0) == root).sum()) == 450
        b = eng.build_report()
        assert b["redos"] == 0 and eng.graph_topic(0)["top_levels"] == 3, b
        eng.join(0, order[651:801])
        c = join_step(eng, n, root, before=b)
        assert int((eng.parents(0) == root).sum()) == 600
        assert c["redo_order"] == b["redo_order"] + 1 and c["last_attempts"] >= 2, c


# ---- depth boundary ---------------------------------------------------------------

@pytest.mark.parametrize("depth,kind", [(252, "gpu"), (253, "gpu"), (254, "host"), (255, "host"), (256, "host")])
def test_depth_boundary(depth, kind):
    """Chains around the level tables' 255 entries: the GPU builds depths up
    to 253; from depth 254 on it cannot tell that the tree ends there and
    the host build takes over, counted as a depth fall-back.  Hops are the
    oracle's in every case (saturating at 254)."""
    rng = np.random.default_rng(depth)
    n = depth + 1 + 4
    item = label(n, np.arange(-1, depth), rng)
    live = np.ones(n, dtype=np.uint8)
    with make(n, 1, 1) as eng:
        eng.set_tree(0, *item)
        rep = eng.build_report()
        print("report:", rep)
        assert rep["last_kind"] == kind, rep
        if kind == "gpu":
            assert_gpu_built(rep)
            assert rep["gpu_builds"] == 1
        else:
            assert (rep["gpu_builds"], rep["host_builds"], rep["fallback_depth"]) == (0, 1, 1), rep
            assert (rep["fallback_stall"], rep["fallback_attempts"], rep["fallback_capacity"]) == (0, 0, 0), rep
        assert eng.depth(0) == (depth, depth + 1)
        g = GC.read(eng)
        GC.validate(g, GC.reference(n, [item], live), "peer")
        assert_same_arrays(g, host_arrays(n, [item], live))
        flood_check(eng, [item], live)
        want = oracle_hops(item, live)
        assert int(want[want != 0xFF].max()) == min(depth, 254)


# ---- topic bases ----------------------------------------------------------------------

def test_topic_bases_and_flags_pass():
    """Six topic slots over 3,000 peers: a lone root, a slot never created,
    a tree, a topic created and closed again, a tree sharing peers with the
    first, a root whose only child is dead.  10 % of the peers are dead,
    the first tree's root among them (its node stays live).  A second live
    mask without a tree change goes through k_node_flags alone: the flags
    equal the reference again and no build is counted."""
    rng = np.random.default_rng(6)
    n = 3000
    tree_a = label(n, level_slots([1, 4, 30, 200, 900, 1200], [4, 9, 9, 6, 3], rng), rng)
    tree_b = label(n, level_slots([1, 700, 650, 600], [700, 2, 2], rng), rng)
    closed = label(n, level_slots([1, 5, 20], [5, 5], rng), rng)
    lone = (int(rng.integers(n)), np.full(n, NONE, dtype=np.uint32))
    r5, c5 = (int(x) for x in rng.permutation(n)[:2])
    par5 = np.full(n, NONE, dtype=np.uint32)
    par5[c5] = r5
    topics = [lone, None, tree_a, None, tree_b, (r5, par5)]
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[tree_a[0]] = 0
    live[c5] = 0
    shared = np.intersect1d(GC.reference(n, [tree_a], live)["topics"][0]["members"],
                            GC.reference(n, [tree_b], live)["topics"][0]["members"])
    assert shared.shape[0] > 500
    with make(n, 6, 1) as eng:
        load(eng, topics, live)
        eng.set_tree(3, *closed)
        eng.topic_close(3)
        rep = check_step(eng, n, topics, live, "peer")
        assert rep["gpu_builds"] == 1
        t5 = eng.graph_topic(5)
        assert eng.graph(PE.G_NODE_FLAGS)[t5["nbase"] + 1] == 0  # the dead only child: neither live nor internal
        assert eng.graph(PE.G_NODE_FLAGS)[eng.graph_topic(2)["nbase"]] & PE.NODE_LIVE  # the dead root forwards
        live2 = (rng.random(n) > 0.3).astype(np.uint8)
        live2[tree_b[0]] = 0
        eng.set_live(live2)
        g = GC.read(eng)
        GC.validate(g, GC.reference(n, topics, live2), "peer")
        assert eng.build_report() == rep  # the flags pass is no build
        assert_same_arrays(g, host_arrays(n, topics, live2))
        flood_check(eng, topics, live2)
        assert eng.build_report() == rep


# ---- deltas ----------------------------------------------------------------------------

def test_set_tree_deltas():
    """set_tree on the same topic: 300 of 3,000 peers re-parented, 50
    detached (their subtrees leave the node space), 50 attached from
    outside; then the first tree again."""
    rng = np.random.default_rng(300)
    n = 3000
    m = 2900
    sp = hang_below([-1, 0, 0, 0], 0, m, 4, rng)
    lab = rng.permutation(n)
    live = (rng.random(n) > 0.1).astype(np.uint8)

    def tree(sp_of):
        parent = np.full(n, NONE, dtype=np.uint32)
        has = sp_of >= 0
        parent[lab[:sp_of.shape[0]][has]] = lab[sp_of[has]]
        return int(lab[0]), parent

    first = tree(np.concatenate([sp, np.full(n - m, -1)]))
    sp2 = np.concatenate([sp, np.full(n - m, -1)])
    moved = rng.choice(np.arange(1, m), size=350, replace=False)
    for s in moved[:300]:
        sp2[s] = int(rng.integers(0, s))  # an earlier slot: no cycle
    sp2[moved[300:]] = -1
    sp2[m:m + 50] = rng.integers(0, m, size=50)
    second = tree(sp2)
    ref1 = GC.reference(n, [first], live)["topics"][0]
    ref2 = GC.reference(n, [second], live)["topics"][0]
    assert 50 <= np.setdiff1d(ref1["members"], ref2["members"]).shape[0]  # the detached and their subtrees
    assert np.setdiff1d(ref2["members"], ref1["members"]).shape[0] >= 1
    with make(n, 1, 1) as eng:
        load(eng, [first], live)
        a = check_step(eng, n, [first], live, "peer")
        eng.set_tree(0, *second)
        b = check_step(eng, n, [second], live, "peer", before=a)
        eng.set_tree(0, *first)
        check_step(eng, n, [first], live, "peer", before=b)


@pytest.mark.parametrize("width,max_width", [(2, 5), (8, 20)])
def test_join_topic_deltas(width, max_width):
    """A join topic of 3,000 peers under 10 batches of joins, leaves and
    drops: after each batch the GPU-built node space is a node space of the
    attached tree with siblings in peer order, the host-built engine's one
    in the tree's own order; both flood alike, message by message: the first
    as the oracle floods the validated tree, the last as it floods the tree
    the run leaves behind (a run repairs around dropped hosts after its
    first message)."""
    rng = np.random.default_rng(width)
    n = 3000
    live = np.ones(n, dtype=np.uint8)
    root = int(rng.integers(n))
    engs = [make(n, 1, g) for g in (1, 0)]
    try:
        first_members = rng.permutation(np.setdiff1d(np.arange(n), [root]))[:n // 2]
        for e in engs:
            e.topic_create(0, root, width, max_width)
            e.join(0, first_members)
        members = {int(p) for p in first_members}
        prev = None
        for batch in range(10):
            outs = np.array(sorted(set(range(n)) - members - {root}))
            join = rng.choice(outs, size=40, replace=False)
            sts = [e.join(0, join, check=False) for e in engs]
            assert np.array_equal(sts[0], sts[1])
            members |= {int(p) for p, s in zip(join, sts[0]) if s == 0}
            leave = rng.choice(sorted(members), size=30, replace=False)
            drop = rng.choice(sorted(members - {int(p) for p in leave}), size=3, replace=False)
            for e in engs:
                for op, peers in ((e.leave, leave), (e.drop, drop)):
                    try:
                        op(0, peers)
                    except PE.EngineError:
                        pass
            members -= {int(p) for p in leave} | {int(p) for p in drop}
            rep = engs[0].build_report()
            assert_gpu_built(rep, prev)
            hrep = engs[1].build_report()
            assert hrep["last_kind"] == "host" and hrep["gpu_builds"] == 0
            par = engs[0].parents(0)
            assert np.array_equal(par, engs[1].parents(0)), batch
            ref = GC.reference(n, [(root, par)], live)
            GC.validate(GC.read(engs[0]), ref, "peer_upto_4096")
            GC.validate(GC.read(engs[1]), ref, "any")
            want = oracle_hops((root, par), live)
            firsts = [e.publish(np.zeros(N_MSGS)) for e in engs]
            sts = [e.run() for e in engs]
            assert sts[0].deliveries == sts[1].deliveries, batch
            # the first message floods the tree validated above; its failed
            # writes to dropped hosts are repaired before the next message
            # (subtrees re-attach), so the last one floods the tree the run
            # leaves behind; in between the two builds agree
            after = engs[0].parents(0)
            assert np.array_equal(after, engs[1].parents(0)), batch
            want_last = oracle_hops((root, after), live)
            for m in range(N_MSGS):
                got = [e.hops(f + m) for e, f in zip(engs, firsts)]
                assert np.array_equal(got[0], got[1]), (batch, m)
                if m == 0:
                    assert np.array_equal(got[0], want), batch
                if m == N_MSGS - 1:
                    assert np.array_equal(got[0], want_last), batch
            # (the run's lazy prune may have changed the tree: the next batch's report counts its build)
            prev = engs[0].build_report()
            assert_no_fallback(prev)
    finally:
        for e in engs:
            e.close()
