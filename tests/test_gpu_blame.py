"""GPU: each missed subscriber and its cut point (ps_topic_blame, ps_blame;
DESIGN.md §5.5q) -- per named tree topic the non-root nodes that lack window
messages, in node order, each with its peer, the peer of the nearest node on its
way up that lacks messages under a full parent, both BFS levels and the messages
it lacks; and the same facts for explicit (topic, peer) queries.

Every comparison is bit for bit and record for record against tests/blame_ref.py
(oracle.disseminate's deliveries, or oracle.Tree under churn, handed down level
by level over graph_check's depths), the tables ordered by the engine's
G_NODE_PEER.  Every case is cross-checked against calls that predate these two,
made on the same window: per named topic rec_peer equals ps_drain_topics'
exception slice, and the four bincount identities hold against ps_peer_cut.  And
on every case ps_blame over (t, every peer) -- the topic's peers, the unattached
ones and the root -- equals the reference and ps_topic_blame expanded.  The
seam (PSAMD_AB=1 PSAMD_LOAD_COUNT=rows) makes the weights kernel count full
rows from their words."""
import ctypes as C
import threading

import numpy as np
import pytest

import blame_ref as BR
import graph_check as GC
import oracle as O
import psengine as PE
from test_blame_cpu import FILL32, SENTINEL, lent, lent_untouched
from test_gpu_churn import assert_builds, make_engine
from test_gpu_cut import levels_of
from test_gpu_downstream import TOP_EDGE, fan_tree, path, star
from test_gpu_drain_batch import random_mesh2, random_tree
from test_gpu_drain_shared import one_topic
from test_gpu_drain_topics import kids_of, under
from test_gpu_load import heap_tree, seam, shared_topics
from test_gpu_sink import drop_engine

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
BLOCK = 256  # kDownBlock: the nodes of one work item
KEYS = ("peer", "cut_peer", "hop", "cut_hop", "missed")


# ---- helpers ------------------------------------------------------------------------

def node_order(eng, t):
    """The peers of topic t's nodes in node order, the root's first."""
    g = eng.graph_topic(int(t))
    if not g["exists"] or not g["n_nodes"]:
        return np.empty(0, dtype=np.int64)
    return eng.graph(PE.G_NODE_PEER)[g["nbase"]:g["nbase"] + g["n_nodes"]].astype(np.int64)


def same_arrays(got, want, names, what):
    for name, g, w in zip(names, got, want):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{what} {name}: {bad.size} entries differ, first {bad[:6]} got {g[bad[:6]]} want {w[bad[:6]]}")


def check(eng, topics, tables, what="", graph=True):
    """topic_blame(topics) and blame over every (t, peer) against the tables
    (topic -> blame_ref.Table), and against drain_topics and peer_cut on the
    same window.  Returns topic_blame's answer.  graph = False, where the tree
    may have changed since the window (a read of the node space would rebuild
    it and drop the window): the reference's records -- the same set, checked
    -- are put in the order of ps_drain_topics' exceptions."""
    topics = [int(t) for t in topics]
    n = eng.n_peers
    r = eng.topic_blame(topics)
    assert set(r) == {"rec_off", *KEYS} and r["rec_off"].dtype == np.uint64 and r["rec_off"].size == len(topics) + 1
    off = r["rec_off"].astype(np.int64)
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and all(r[k].size == off[-1] and r[k].dtype == np.uint32 for k in KEYS)
    dt = eng.drain_topics(topics)
    eo = dt["exc_off"].astype(np.int64)
    everyone = np.arange(n, dtype=np.uint32)
    for i, t in enumerate(topics):
        got = [r[k][off[i]:off[i + 1]] for k in KEYS]
        if graph:
            order = node_order(eng, t)
        else:
            exc = dt["exc_peer"][eo[i]:eo[i + 1]].astype(np.int64)
            assert sorted(exc.tolist()) == np.nonzero(tables[t].miss > 0)[0].tolist(), f"{what} topic {t}: the set"
            order = np.concatenate([[0], exc])  # (the first entry stands for the root: skipped)
        same_arrays(got, BR.records(tables[t], order), KEYS, f"{what} topic {t}")
        # the order and the set of ps_drain_topics' exceptions
        assert np.array_equal(got[0], dt["exc_peer"][eo[i]:eo[i + 1]]), f"{what} topic {t}: not drain_topics' exceptions"
        # the explicit queries: every peer of the engine, so the topic's own, the unattached ones and the root
        q = eng.blame(np.full(n, t, dtype=np.uint32), everyone)
        same_arrays(q, BR.queries(tables[t], everyone), ("cut_peer", "hop", "cut_hop", "missed"), f"{what} blame, topic {t}")
        # ... and ps_topic_blame expanded
        assert not np.delete(q[3], got[0]).any() and (np.delete(q[0], got[0]) == NONE).all()
        assert np.array_equal(q[0][got[0]], got[1]) and np.array_equal(q[1][got[0]], got[2])
        assert np.array_equal(q[2][got[0]], got[3]) and np.array_equal(q[3][got[0]], got[4])
    # the four identities against ps_peer_cut
    missed, cuts, orphaned, lost = eng.peer_cut(topics)
    w = r["missed"].astype(np.int64)
    own = r["peer"] == r["cut_peer"]
    u64 = lambda x: x.astype(np.uint64)
    assert np.array_equal(u64(np.bincount(r["cut_peer"], weights=w, minlength=n)), lost), f"{what}: lost"
    assert np.array_equal(u64(np.bincount(r["peer"], weights=w, minlength=n)), missed), f"{what}: missed"
    assert np.array_equal(u64(np.bincount(r["peer"][own], minlength=n)), cuts), f"{what}: cuts"
    assert np.array_equal(u64(np.bincount(r["cut_peer"][~own], minlength=n)), orphaned), f"{what}: orphaned"
    return r


def run_dead(parent, n_msgs, dead_sets, **kw):
    """One engine over a tree rooted at 0 whose peer ids name its nodes, one
    run per dead set: everything against the reference.  Returns the answers."""
    n = parent.size
    out = {}
    with PE.Engine(n, 1, **kw) as eng:
        eng.set_tree(0, 0, parent)
        assert np.array_equal(eng.graph(PE.G_NODE_PEER), np.arange(n))  # a peer id names a node
        for name, dead in dead_sets.items():
            live = np.ones(n, dtype=np.uint8)
            live[list(dead)] = 0
            assert live[0]
            eng.set_live(live)
            eng.publish(np.zeros(n_msgs))
            eng.run()
            r = check(eng, [0], {0: BR.topic_blame(n, 0, live, n_msgs, parent)}, f"{n} peers, dead {name}")
            assert (r["peer"].size > 0) == (len(dead) > 0), name
            if len(dead):
                assert set(r["cut_peer"].tolist()) <= set(dead)  # a healthy tree is cut at dead peers only
            out[name] = r
    return out


def raw_topic_blame(eng, topics, which=(True,) * 5, want_off=True, want_total=True):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    off, ptrs, total = lent()
    rc = eng._L.ps_topic_blame(eng._h, t.ctypes.data_as(U32P) if t.size else None, t.size, C.byref(off) if want_off else None,
                               *(C.byref(p) if w else None for p, w in zip(ptrs, which)),
                               C.byref(total) if want_total else None)
    return rc, off, ptrs, total


def raw_blame(eng, topics, peers, which=(True,) * 4):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    p = np.ascontiguousarray(peers, dtype=np.uint32)
    a = [np.full(max(t.size, 4), FILL32, dtype=np.uint32) for _ in range(4)]
    rc = eng._L.ps_blame(eng._h, t.ctypes.data_as(U32P), p.ctypes.data_as(U32P), t.size,
                         *(x.ctypes.data_as(U32P) if w else None for x, w in zip(a, which)))
    return rc, a


def untouched(a):
    return all((x == FILL32).all() for x in a)


# ---- 1. paths -----------------------------------------------------------------------

def test_cuts_on_a_path():
    """The cut at the first, a middle and the last node, and two cuts on one
    path: the closed forms."""
    n, c = 40, 3
    got = run_dead(path(n), c, {"first": [1], "middle": [20], "last": [39], "two": [5, 20], "none": []})
    for name, d in (("first", 1), ("middle", 20), ("last", 39), ("two", 5)):
        r = got[name]
        assert np.array_equal(r["peer"], np.arange(d, n)) and np.array_equal(r["hop"], r["peer"])
        assert (r["cut_peer"] == d).all() and (r["cut_hop"] == d).all() and (r["missed"] == c).all()


# ---- 2. work items ------------------------------------------------------------------

def wide_levels(w):
    """Root 0; level 1: w nodes; level 2: three children for level 1's first
    node and two for every other, so that the children of its 128th node are
    the 255th and 256th of their level; level 3: one child each.  Numbered
    level by level, siblings ascending: a peer id names a node."""
    parent = [NONE] + [0] * w
    l1 = list(range(1, 1 + w))
    for j, p in enumerate(l1):
        parent += [p] * (3 if j == 0 else 2)
    l2 = list(range(1 + w, 1 + w + 2 * w + 1))
    parent += l2
    return np.array(parent, dtype=np.uint32)


@pytest.mark.parametrize("w", [255, 256, 257])
def test_levels_around_a_work_item(w):
    """Levels of 255 / 256 / 257 nodes under the root: the level is the top
    kernel's or the first level launch's.  The 128th node's two children lie
    either side of a work item's edge: as a cut point it hands its words to
    both, and two blocks hand them on."""
    parent = wide_levels(w)
    lv = levels_of(parent)
    assert [x.size for x in lv] == [1, w, 2 * w + 1, 2 * w + 1]
    p = int(lv[1][127])
    kids = np.nonzero(parent == p)[0]
    assert (kids - lv[2][0]).tolist() == [BLOCK - 1, BLOCK]
    run_dead(parent, 2, {
        "straddling_parent": [p], "l1_first": [int(lv[1][0])], "l1_last": [int(lv[1][-1])],
        "l2_item_last": [int(kids[0])], "l2_item_next": [int(kids[1])], "l2_both": kids.tolist(),
        "parent_and_a_child": [p, int(kids[1])], "l1_255_256": [int(x) for x in lv[1][254:256]], "none": [],
    })


@pytest.mark.parametrize("shape", list(TOP_EDGE))
def test_block_edge_of_the_top_run(shape):
    """The handoff between the top run and the first level launch: the cut
    point at level top - 1, top and top + 1, at the level's first and last
    node -- in the last top level with its children in the first launch, and
    the other way round."""
    parent = TOP_EDGE[shape]()
    lv = levels_of(parent)
    depth = len(lv) - 1
    top = 0
    while top < depth and lv[top].size <= BLOCK:
        top += 1
    masks = {"none": []}
    for l in (top - 1, top, top + 1):
        if 1 <= l <= depth:
            masks[f"l{l}_first"] = [int(lv[l][0])]
            masks[f"l{l}_last"] = [int(lv[l][-1])]
            masks[f"l{l}_ends"] = sorted({int(lv[l][0]), int(lv[l][-1])})
    assert len(masks) >= 4
    run_dead(parent, 1, masks)


# ---- 3. strips ----------------------------------------------------------------------

@pytest.mark.parametrize("n", [2048, 2049, 2050, 4100])
def test_one_word_strips(n):
    """One message: one-word rows, 2,048 to a strip, so 2,047 / 2,048 / 2,049
    non-root nodes (and two strips and a bit): records at a strip's first and
    last node, alone and together."""
    masks = {"first_node": [1], "last_node": [n - 1], "none": [], "leaves": [n - 1, n - 2, n - 3]}
    if n - 1 >= 2048:
        masks["strip0_last"] = [2048]
    if n - 1 > 2048:
        masks["strip1_first"] = [2049]
        masks["strip_edge"] = [2048, 2049]
    run_dead(heap_tree(n), 1, masks)


@pytest.mark.parametrize("n", [16, 17, 32, 64])
def test_wide_row_strips(n):
    """8,300 messages: 130-word rows, 15 nodes to a strip."""
    masks = {"first_node": [1], "last_node": [n - 1], "strip0_last": [15], "none": []}
    if n > 16:
        masks["strip1_first"] = [16]
        masks["strip_edge"] = [15, 16]
    if n > 31:
        masks["strip1_last_strip2_first"] = [30, 31]
    run_dead(heap_tree(n), 8300, masks)


# ---- 4. wide fan-out ----------------------------------------------------------------

def test_star_of_3000():
    """The root's wave hands 3,000 children their words, a lane each 64: dead
    children at index 0, 63, 64, 65 and 2,999, one at a time and together."""
    idx = [0, 63, 64, 65, 2999]
    masks = {f"child{i}": [1 + i] for i in idx}
    masks["all_five"] = [1 + i for i in idx]
    masks["none"] = []
    got = run_dead(star(3001), 1, masks)
    r = got["all_five"]
    assert np.array_equal(r["peer"], r["cut_peer"]) and (r["hop"] == 1).all() and (r["cut_hop"] == 1).all()


@pytest.mark.parametrize("a,b", [(64, 65), (65, 64)])
def test_fan_out_64_and_65_at_an_inner_node(a, b):
    """Node 1 has a children, node 2 has b; each of those has one child.  With
    node 1 or 2 dead its children inherit its words: 64 through a lane's loop,
    65 through the wave's; with it live, its dead children blame themselves."""
    first1, last1, first2, last2 = 3, 2 + a, 3 + a, 2 + a + b
    got = run_dead(fan_tree(a, b), 2, {
        "node1": [1], "node2": [2], "both": [1, 2], "node1_and_its_last_child": [1, last1],
        "node2_and_its_first_child": [2, first2], "first_of_1": [first1], "last_of_2": [last2],
        "ends_of_both": [first1, last1, first2, last2], "every_child_of_2": list(range(first2, last2 + 1)), "none": [],
    })
    r = got["both"]
    assert r["peer"].size == 2 + 2 * (a + b) and set(r["cut_peer"].tolist()) == {1, 2} and (r["cut_hop"] == 1).all()
    assert sorted(set(r["hop"].tolist())) == [1, 2, 3]


# ---- 5. row widths ------------------------------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("n_msgs", [1, 4096, 4097, 8300])
def test_row_widths(n_msgs, rows, monkeypatch):
    """Rows of 1, 64, 65 and 130 words over one tree of 300 peers, ~10 %
    masked; under the seam every full row is counted word by word."""
    seam(monkeypatch, rows)
    n, root, parent, live = one_topic(n_msgs, n_msgs)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.publish(np.zeros(n_msgs))
        eng.run()
        r = check(eng, [0], {0: BR.topic_blame(n, root, live, n_msgs, parent)}, f"n_msgs {n_msgs}")
        assert r["peer"].size > 1 and (r["missed"] == n_msgs).all() and not live[r["cut_peer"]].any()


# ---- 6. start groups ----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["group_major", "group_major_rows", "aligned", "aligned_rows", "compact", "no_lazy_seen"])
def test_start_groups(kind, monkeypatch):
    """publish_at with start rounds 0..3: group-major rows (align_groups = 0),
    level-aligned rows, the compaction path and eager seen rows; plain and
    with every full row counted from its words."""
    seam(monkeypatch, kind.endswith("_rows"))
    rng = np.random.default_rng(33)
    n, root, n_msgs = 700, 11, 300
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    starts = rng.integers(0, 4, size=n_msgs)
    kw = {"group_major": {"plan": {"align_groups": 0}}, "group_major_rows": {"plan": {"align_groups": 0}},
          "compact": {"flags": PE.F_COMPACT}, "no_lazy_seen": {"flags": PE.F_NO_LAZY_SEEN}}.get(kind, {})
    topics = (np.arange(n_msgs) % 2).astype(np.uint32)
    c = [int((topics == t).sum()) for t in (0, 1)]
    with PE.Engine(n, 2, **kw) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        eng.publish(topics, starts)
        st = eng.run()
        assert st.windows == 1
        tables = {t: BR.topic_blame(n, root, live, c[t], parent) for t in (0, 1)}
        r = check(eng, [1, 0], tables, kind)
        assert r["peer"].size > 2 and np.array_equal(r["missed"][:int(r["rec_off"][1])], np.full(int(r["rec_off"][1]), c[1]))


# ---- 7. stale rows ------------------------------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("cut_first", [True, False])
def test_stale_rows(cut_first, rows, monkeypatch):
    """A window with a cut subtree and an all-live one, in either order, the
    first the wider: the all-live answer has no record whatever the rows held
    before, and the cut one counts nothing of the other run's rows."""
    seam(monkeypatch, rows)
    rng = np.random.default_rng(66)
    n, root = 500, 2
    parent = random_tree(rng, n, root)
    kids = kids_of(parent)
    cut = max((p for p in kids if p != root), key=lambda p: len(under(kids, p)))
    size = 1 + len(under(kids, cut))
    assert size >= 6
    dead = np.ones(n, dtype=np.uint8)
    dead[cut] = 0
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        for i, (is_cut, c0, c1) in enumerate(((cut_first, 300, 30), (not cut_first, 70, 0))):
            live = dead if is_cut else np.ones(n, dtype=np.uint8)
            eng.set_live(live)
            eng.publish(np.concatenate([np.zeros(c0), np.ones(c1)]).astype(np.uint32))  # five-word rows and one, then two
            eng.run()
            tables = {0: BR.topic_blame(n, root, live, c0, parent), 1: BR.topic_blame(n, root, live, c1, parent)}
            r = check(eng, [0, 1], tables, f"run {i}")
            if is_cut:
                assert r["rec_off"].tolist() == [0, size, size * (2 if c1 else 1)] and (r["cut_peer"] == cut).all()
            else:
                assert r["rec_off"].tolist() == [0, 0, 0]


# ---- 8. several topics sharing peers ------------------------------------------------

@pytest.mark.parametrize("order", [[0, 1, 2, 3], [3, 1, 2, 0], [1], [2, 3], []])
def test_several_topics(order):
    """A 1-word topic, a 130-word one rooted at a leaf of the first, an idle
    one and one created but empty, named in two orders and in subsets: a
    topic's records do not depend on what is named beside it, and the idle
    ones have none."""
    n, free, (r0, p0), (r1, p1), live = shared_topics()
    msgs = np.concatenate([np.full(10, 0), np.full(8300, 1)]).astype(np.uint32)
    none = np.full(n, NONE, dtype=np.uint32)
    tables = {0: BR.topic_blame(n, r0, live, 10, p0), 1: BR.topic_blame(n, r1, live, 8300, p1), 2: BR.idle(n, r0, p0),
              3: BR.idle(n, 7, none)}
    with PE.Engine(n, 4) as eng:
        eng.set_tree(0, r0, p0)
        eng.set_tree(1, r1, p1)
        eng.set_tree(2, r0, p0)
        eng.topic_create(3, 7)
        eng.set_live(live)
        eng.publish(msgs)
        eng.run()
        r = check(eng, order, tables, str(order))
        off = r["rec_off"].astype(np.int64)
        for i, t in enumerate(order):
            assert (off[i + 1] > off[i]) == (t in (0, 1)), (order, t)
        assert not np.isin(r["peer"], free).any()  # peers in no topic
        # queries that span the topics, repeated and shuffled: each as when asked alone
        rng = np.random.default_rng(len(order))
        qt = rng.integers(0, 4, size=3000).astype(np.uint32)
        qp = rng.integers(0, n, size=3000).astype(np.uint32)
        qp[:50] = qp[50:100]  # (repeats)
        qt[:50] = qt[50:100]
        got = eng.blame(qt, qp)
        for t in range(4):
            at = np.nonzero(qt == t)[0]
            want = BR.queries(tables[t], qp[at])
            for g, w in zip(got, want):
                assert np.array_equal(g[at], w), t
        assert (got[3] > 0).any() and (got[1] == NONE).any() and (got[1][qt == 2] != NONE).any()


def test_a_cut_point_in_one_topic_full_in_another():
    """Peer x is dead: in topic 0 it is an inner node and a cut point; of
    topic 1 it is the root, which counts as full -- a dead root still
    forwards -- so topic 1 has no record and x is blamed in topic 0 alone."""
    n, x, c0, c1 = 127, 5, 4, 70
    p0 = heap_tree(n)
    perm = np.arange(n)  # topic 1: the same heap, relabelled so that x is its root
    perm[[0, x]] = [x, 0]
    p1 = np.full(n, NONE, dtype=np.uint32)
    for i in range(1, n):
        p1[perm[i]] = perm[(i - 1) // 2]
    live = np.ones(n, dtype=np.uint8)
    live[x] = 0
    tables = {0: BR.topic_blame(n, 0, live, c0, p0), 1: BR.topic_blame(n, x, live, c1, p1)}
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, 0, p0)
        eng.set_tree(1, x, p1)
        eng.set_live(live)
        eng.publish(np.concatenate([np.zeros(c0), np.ones(c1)]).astype(np.uint32))
        eng.run()
        r = check(eng, [0, 1], tables, "both")
        assert r["rec_off"].tolist() == [0, 31, 31] and (r["cut_peer"] == x).all() and (r["cut_hop"] == 2).all()
        cut_peer, hop, cut_hop, missed = eng.blame([0, 1, 1], [x, x, 0])
        assert cut_peer.tolist() == [x, NONE, NONE] and hop.tolist() == [2, 0, 2] and missed.tolist() == [c0, 0, 0]
        assert cut_hop.tolist() == [2, NONE, NONE]
        assert check(eng, [1], tables, "topic 1 alone")["peer"].size == 0


# ---- 9. an all-live window ----------------------------------------------------------

def test_all_live_window_has_an_empty_view():
    n, root, parent, _ = one_topic(0, 5)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.publish(np.concatenate([np.zeros(70), np.ones(3)]).astype(np.uint32))
        eng.run()
        live = np.ones(n, dtype=np.uint8)
        r = check(eng, [0, 1], {t: BR.topic_blame(n, root, live, c, parent) for t, c in ((0, 70), (1, 3))}, "all live")
        assert r["rec_off"].tolist() == [0, 0, 0] and all(r[k].size == 0 for k in KEYS)
        rc, off, ptrs, total = raw_topic_blame(eng, [0, 1])
        assert rc == 0 and total.value == 0 and PE._view(off, 3, np.uint64).tolist() == [0, 0, 0]
        rc, off, ptrs, total = raw_topic_blame(eng, [])  # n == 0
        assert rc == 0 and total.value == 0 and PE._view(off, 1, np.uint64).tolist() == [0]
        rc, a = raw_blame(eng, [], [])  # n == 0: valid, nothing written
        assert rc == 0 and untouched(a)


# ---- 10. churn ----------------------------------------------------------------------

def tree_last_window(ot, n, k, dropped=False):
    """k messages over oracle.Tree ot as the engine runs them (the windows of
    test_gpu_cut.tree_window): the deliveries of all of them, the windows, and
    the last window's table."""
    left, windows, deliveries, table = k, 0, 0, None
    while left:
        par = ot.parents()
        hop = ot.message()
        c = 1 if dropped or not np.array_equal(ot.parents(), par) else left
        dropped = False
        for _ in range(c - 1):
            assert np.array_equal(ot.message(), hop)
        got = hop != 0xFF
        got[ot.root] = False
        table = BR.from_parents(n, ot.root, par, c * got, c)
        deliveries += c * int(got.sum())
        left -= c
        windows += 1
    return deliveries, windows, table


@pytest.mark.parametrize("gpu_build", [True, False])
def test_churn(gpu_build):
    """Joins, leaves and drops between runs, the node space rebuilt on the GPU
    or on the host every batch: each batch's last window follows the oracle's
    tree; orphans and leavers have no record and resolve to no node."""
    rng = np.random.default_rng(17)
    n, seed = 3000, 4  # (test_gpu_cut.test_churn's first six batches)
    eng = make_engine(n, gpu_build, seed=seed)
    ot = O.Tree(n, 0, 2, 5, PE.Engine.topic_seed(seed, 0))
    eng.topic_create(0, 0, 2, 5)
    eng.join(0, np.arange(1, n, 2))
    ot.join_all(range(1, n, 2))
    members = set(range(1, n, 2))
    built = records = 0
    with eng:
        for step in range(6):
            outs = [p for p in range(1, n) if p not in members]
            join = rng.choice(outs, size=20, replace=False)
            st = eng.join(0, join, check=False)
            for p, s in zip(join, st):
                assert ot.join(int(p)) == s
            members |= {int(p) for p, s in zip(join, st) if s == 0}
            leave = rng.choice(sorted(members), size=15, replace=False)
            for p in leave:
                assert ot.leave(int(p)) in (0, -3)
            try:
                eng.leave(0, leave)
            except PE.EngineError:
                pass
            members -= {int(p) for p in leave}
            if step % 3 == 1:
                p = int(rng.choice(sorted(members)))
                eng.drop(0, [p])
                assert ot.drop(p) == 0
                members.discard(p)
            k = int(rng.integers(2, 6))
            eng.publish(np.zeros(k))
            run = eng.run()
            d, kw, table = tree_last_window(ot, n, k, dropped=step % 3 == 1)
            assert run.deliveries == d and run.windows == kw, step
            # (the leaves are pruned by the run's messages: the node space is to be rebuilt, and is not read)
            r = check(eng, [0], {0: table}, f"step {step}, gpu_build {gpu_build}", graph=False)
            records += r["peer"].size
            assert np.array_equal(eng.parents(0), ot.parents()), step
            built = assert_builds(eng, gpu_build, built)
        # a live mask on top of the churned tree: something to blame
        live = (rng.random(n) > 0.05).astype(np.uint8)
        live[0] = 1
        eng.set_live(live)
        eng.publish(np.zeros(3))
        eng.run()
        built = assert_builds(eng, gpu_build, built, at_least=0)
        par = ot.parents()
        rp, cl = O.parents_to_csr(np.where(np.arange(n) == 0, NONE, par).astype(np.uint32))
        _, hops, _ = O.disseminate(rp, cl, 0, live, 3)
        got = hops != 0xFF
        got[:, 0] = False
        # nothing left or was dropped since the run before: the node space stands and is read
        r = check(eng, [0], {0: BR.from_parents(n, 0, par, got.sum(axis=0), 3)}, f"masked, gpu_build {gpu_build}")
        assert r["peer"].size > 0 and assert_builds(eng, gpu_build, built, at_least=0) == built


# ---- 11. asynchronous runs and windows ----------------------------------------------

def test_after_run_async_and_wait():
    n, root, parent, live = one_topic(0, 21)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.publish(np.zeros(9))
        eng.run_async()
        eng.wait()
        r = check(eng, [0], {0: BR.topic_blame(n, root, live, 9, parent)}, "after wait")
        assert r["peer"].size > 0


def test_a_run_split_into_windows_answers_the_last():
    """msg_window = 64: 150 + 70 messages run as windows of (64, 64), (64, 6)
    and (22, 0); the answer is the last window's: c = 22, and topic 1 idle."""
    n, root, parent, live = one_topic(0, 71)
    rng = np.random.default_rng(71)
    with PE.Engine(n, 2, msg_window=64) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        eng.publish(rng.permutation(np.concatenate([np.zeros(150), np.ones(70)])).astype(np.uint32))
        st = eng.run()
        assert st.windows == 3
        r = check(eng, [0, 1], {0: BR.topic_blame(n, root, live, 22, parent), 1: BR.idle(n, root, parent)}, "last window")
        assert r["peer"].size > 0 and (r["missed"] == 22).all() and r["rec_off"][1] == r["rec_off"][2]


def test_a_run_split_by_a_drop():
    """An interior peer dropped: topic 0's first message runs alone over the
    old tree, the rest over the repaired one; the last window is answered, on
    the node space it ran on."""
    n, seed = 60, 3
    topics = np.array([0] * 5 + [1] * 5, dtype=np.uint32)
    ots = [O.Tree(n, 0, 2, 5, PE.Engine.topic_seed(seed, t)) for t in (0, 1)]
    for ot in ots:
        ot.join_all(range(1, n))
    with drop_engine(n, seed) as eng:
        par = eng.parents(0)
        kids = kids_of(par)
        dead = max((p for p in kids if p != 0), key=lambda p: (len(kids[p]), len(under(kids, p))))
        eng.drop(0, [dead])
        assert ots[0].drop(dead) == 0
        eng.publish(topics)
        st = eng.run()
        assert st.windows >= 2
        (d0, k0, t0), (d1, k1, t1) = tree_last_window(ots[0], n, 5, dropped=True), tree_last_window(ots[1], n, 5)
        assert (k0, k1) == (2, 1) and d0 + d1 == st.deliveries
        # topic 1 ran in the first window alone: idle in the last
        r = check(eng, [0, 1], {0: t0, 1: BR.idle(n, 0, ots[1].parents())}, "drop", graph=False)
        assert r["peer"].size == 0
        assert eng.blame([0], [dead])[1][0] == NONE  # the dropped peer holds no node


# ---- 12. the rules ------------------------------------------------------------------

def test_rules():
    rng = np.random.default_rng(82)
    n, root = 300, 1
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        # before any run
        rc, off, ptrs, total = raw_topic_blame(eng, [0])
        assert rc == E_NOTREADY and lent_untouched(off, ptrs, total)
        rc, a = raw_blame(eng, [0], [5])
        assert rc == E_NOTREADY and untouched(a)
        eng.publish(np.zeros(10))
        eng.run()
        table = BR.topic_blame(n, root, live, 10, parent)
        full = check(eng, [0, 1], {0: table, 1: BR.idle(n, root, parent)}, "full")
        total_want = full["peer"].size
        assert total_want > 0
        # ps_topic_blame's arguments
        rc, off, ptrs, total = raw_topic_blame(eng, [0, 0])  # a topic named twice
        assert rc == E_INVAL and lent_untouched(off, ptrs, total)
        rc, off, ptrs, total = raw_topic_blame(eng, [0, 2])
        assert rc == E_RANGE and lent_untouched(off, ptrs, total)  # nothing written
        assert raw_topic_blame(eng, [0], want_off=False)[0] == E_INVAL
        assert raw_topic_blame(eng, [0], want_total=False)[0] == E_INVAL
        o, ps, tt = lent()
        assert eng._L.ps_topic_blame(eng._h, None, 1, C.byref(o), *(C.byref(p) for p in ps), C.byref(tt)) == E_INVAL
        assert lent_untouched(o, ps, tt)
        # every combination of the five record arrays: those asked for are lent, the others left alone
        for mask in range(32):
            which = tuple(bool(mask >> i & 1) for i in range(5))
            rc, off, ptrs, total = raw_topic_blame(eng, [0], which)
            assert rc == 0 and total.value == total_want, which
            assert PE._view(off, 2, np.uint64).tolist() == [0, total_want]
            for k, p, w in zip(KEYS, ptrs, which):
                if w:
                    assert np.array_equal(PE._view(p, total_want, np.uint32), full[k]), (which, k)
                else:
                    assert C.cast(p, C.c_void_p).value == SENTINEL, (which, k)
        # ps_blame's arguments
        rc, a = raw_blame(eng, [0, 2], [1, 1])
        assert rc == E_RANGE and untouched(a)  # a topic out of range: nothing written
        rc, a = raw_blame(eng, [0, 0], [1, n])
        assert rc == E_RANGE and untouched(a)  # a peer out of range
        assert raw_blame(eng, [0], [1], which=(False,) * 4)[0] == E_INVAL
        t1 = np.zeros(1, dtype=np.uint32)
        assert eng._L.ps_blame(eng._h, None, t1.ctypes.data_as(U32P), 1, t1.ctypes.data_as(U32P), None, None, None) == E_INVAL
        assert eng._L.ps_blame(eng._h, t1.ctypes.data_as(U32P), None, 1, t1.ctypes.data_as(U32P), None, None, None) == E_INVAL
        qp = np.concatenate([full["peer"][:5], [root, root], np.nonzero(live)[0][:5]]).astype(np.uint32)
        qt = np.zeros(qp.size, dtype=np.uint32)
        want = BR.queries(table, qp)
        for mask in range(1, 16):
            which = tuple(bool(mask >> i & 1) for i in range(4))
            rc, a = raw_blame(eng, qt, qp, which)
            assert rc == 0, which
            for x, w, f in zip(a, which, want):
                assert np.array_equal(x[:qp.size], f) if w else (x == FILL32).all(), which
        # the view stays valid across other calls until the next ps_topic_blame
        rc, off, ptrs, total = raw_topic_blame(eng, [1, 0])
        assert rc == 0 and total.value == total_want
        views = [PE._view(p, total_want, np.uint32) for p in ptrs]
        off_view = PE._view(off, 3, np.uint64)
        eng.peer_cut([0])
        eng.drain_topics([0, 1])
        eng.blame(qt, qp)
        eng.peer_downstream([0])
        eng.publish(np.zeros(3))
        eng.run()
        eng.blame(qt, qp)
        assert off_view.tolist() == [0, 0, total_want]
        for k, v in zip(KEYS, views):
            assert np.array_equal(v, full[k]), k
        r = eng.topic_blame([0])  # the next call: the new window
        assert (r["missed"] == 3).all() and np.array_equal(r["peer"], full["peer"])


def test_meshes_are_refused():
    """A mesh topic is refused by both calls, nothing written, also beside a
    tree topic of the same window -- which is then answered alone."""
    rng = np.random.default_rng(41)
    n, root = 400, 5
    rp, cl = random_mesh2(rng, n, root)
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_children(1, root, rp, cl)
        eng.set_live(live)
        eng.publish(np.concatenate([np.zeros(70), np.ones(70)]).astype(np.uint32))
        st = eng.run()
        assert st.windows == 1 and st.expand_mode == PE.MODE_COMPACT  # the tree runs beside the mesh: compaction path
        for named in ([1], [0, 1], [1, 0]):
            rc, off, ptrs, total = raw_topic_blame(eng, named)
            assert rc == E_STATE and lent_untouched(off, ptrs, total), named
            rc, a = raw_blame(eng, named, [3] * len(named))
            assert rc == E_STATE and untouched(a), named
        r = check(eng, [0], {0: BR.topic_blame(n, root, live, 70, parent)}, "a tree beside a mesh")
        assert r["peer"].size > 0


def test_a_topic_set_anew_since_the_window():
    """The levels are the last build's.  A parent array set over a parent
    array keeps them, and the last window is still answered; set over a join
    topic it starts the record afresh: PS_E_STATE, nothing written, until the
    next run."""
    rng = np.random.default_rng(83)
    n = 200
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[0] = 1
    p0, p1 = random_tree(rng, n, 0), random_tree(rng, n, 0)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, 0, p0)
        eng.topic_create(1, 0, 2, 5)
        eng.join(1, np.arange(1, n))
        eng.set_live(live)
        eng.publish(np.array([0] * 4 + [1] * 6, dtype=np.uint32))
        eng.run()
        before = eng.topic_blame([0, 1])
        only0 = check(eng, [0], {0: BR.topic_blame(n, 0, live, 4, p0)}, "topic 0")
        assert only0["peer"].size > 0 and before["rec_off"][2] > before["rec_off"][1] == only0["peer"].size
        eng.set_tree(0, 0, p1)  # over a parent array: the window's levels stay
        after = eng.topic_blame([0, 1])
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        eng.set_tree(1, 0, p1)  # over a join topic: its record starts afresh
        rc, off, ptrs, total = raw_topic_blame(eng, [0, 1])
        assert rc == E_STATE and lent_untouched(off, ptrs, total)
        rc, a = raw_blame(eng, [0, 1], [3, 3])
        assert rc == E_STATE and untouched(a)
        again = eng.topic_blame([0])  # the other topic alone
        for k in only0:
            assert np.array_equal(again[k], only0[k]), k
        eng.publish(np.array([0] * 3 + [1] * 2, dtype=np.uint32))
        eng.run()
        check(eng, [0, 1], {0: BR.topic_blame(n, 0, live, 3, p1), 1: BR.topic_blame(n, 0, live, 2, p1)}, "after the next run")


def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(2)]
    try:
        for r, e in enumerate(engines):
            e.dist_init_loopback(lb, r, PE.PART_PEER)
            e.set_tree(0, root, parent)
            e.publish(np.zeros(50))
        errs = []

        def go(e):
            try:
                e.run()
            except Exception as ex:  # noqa: BLE001
                errs.append(ex)

        th = [threading.Thread(target=go, args=(e,)) for e in engines]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in th) and not errs, errs
        for e in engines:
            rc, off, ptrs, total = raw_topic_blame(e, [0])
            assert rc == E_STATE and lent_untouched(off, ptrs, total)
            rc, a = raw_blame(e, [0], [7])
            assert rc == E_STATE and untouched(a)
    finally:
        for e in engines:
            e.close()
