"""GPU: the audience behind each peer (ps_peer_downstream, ps_downstream_track /
ps_downstream_take) -- per peer, over the named tree topics,
the nodes strictly below its nodes and the window messages delivered to them,
for the last window or accumulated behind every window of every run.

Every comparison is bit-exact, both arrays, against tests/downstream_ref.py
(oracle.disseminate's deliveries, or oracle.Tree under churn, added bottom-up
over graph_check's depths).  Where every topic is named, carried summed over
the roots equals the run's ps_stats.deliveries; where one tree topic of at
most 254 levels is named, sum(below) = sum(h * nodes[h]) and sum(carried) =
sum(h * deliv[h]) against Engine.topic_hops.  The seam (PSAMD_AB=1
PSAMD_LOAD_COUNT=rows) makes the weights kernel count full rows from their
words, the path a healthy tree's all-or-nothing rows never take otherwise."""
import ctypes as C
import threading

import numpy as np
import pytest

import downstream_ref as DR
import graph_check as GC
import hops_ref as HR
import load_ref as LR
import oracle as O
import psengine as PE
from psengine import workloads as WL
from test_gpu_churn import assert_builds, make_engine
from test_gpu_drain_batch import random_mesh2, random_tree
from test_gpu_drain_shared import one_topic
from test_gpu_drain_topics import kids_of, under
from test_gpu_load import heap_tree, seam, shared_topics, strip_masks
from test_gpu_sink import drop_engine, even_batches

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
COLS = PE.MAX_ROUNDS
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
FILL = 0xABABABABABABABAB
BLOCK = 256  # kDownBlock = kAudBlock: the nodes one block sums, a thread each


# ---- helpers ------------------------------------------------------------------------

def same(got, want, what=""):
    """(below, carried) against (below, carried), uint64, bit for bit."""
    for name, g, w in zip(("below", "carried"), got, want):
        w = np.asarray(w).astype(np.uint64)
        assert g.dtype == np.uint64 and g.shape == w.shape, (what, name)
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{what} {name}: {bad.size} peers differ, first {bad[:6]} got {g[bad[:6]]} "
                                 f"want {w[bad[:6]]}")


def add(a, b):
    return tuple(x + np.asarray(y).astype(np.uint64) for x, y in zip(a, b))


def zeros(n):
    return np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)


def identities(eng, t, got):
    """One named tree topic of at most 254 levels: a node at level h lies below
    h nodes, so the two sums are the hop rows' first moments."""
    nodes, _, deliv = eng.topic_hops([t])
    assert not nodes[0, COLS - 1]  # the clamped column is unused
    h = np.arange(COLS, dtype=np.uint64)
    assert got[0].sum() == (h * nodes[0]).sum(), "sum(below) != sum(h * nodes[h])"
    assert got[1].sum() == (h * deliv[0]).sum(), "sum(carried) != sum(h * deliv[h])"


def raw_down(eng, topics, below=True, carried=True):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    b = np.full(eng.n_peers, FILL, dtype=np.uint64)
    c = np.full(eng.n_peers, FILL, dtype=np.uint64)
    rc = eng._L.ps_peer_downstream(eng._h, t.ctypes.data_as(U32P), t.size, b.ctypes.data_as(U64P) if below else None,
                                   c.ctypes.data_as(U64P) if carried else None)
    return rc, b, c


def raw_track(eng, topics):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    return eng._L.ps_downstream_track(eng._h, t.ctypes.data_as(U32P), t.size)


def raw_take(eng):
    b = np.full(eng.n_peers, FILL, dtype=np.uint64)
    c = np.full(eng.n_peers, FILL, dtype=np.uint64)
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    rc = eng._L.ps_downstream_take(eng._h, b.ctypes.data_as(U64P), c.ctypes.data_as(U64P), C.byref(nw), C.byref(nsk))
    return rc, b, c, nw.value, nsk.value


def star(n):
    parent = np.zeros(n, dtype=np.uint32)
    parent[0] = NONE
    return parent


def path(n):
    parent = np.arange(-1, n - 1).astype(np.uint32)
    parent[0] = NONE
    return parent


def fan_tree(a, b):
    """Root 0 with the children 1 and 2; 1 has a children, 2 has b; each of
    those has one child.  Numbered level by level, siblings ascending: a peer
    id names a node."""
    parent = [NONE, 0, 0] + [1] * a + [2] * b
    parent += list(range(3, 3 + a + b))
    return np.array(parent, dtype=np.uint32)


def star_deep(k):
    """Root 0 with k children, each with one child of its own."""
    return np.array([NONE] + [0] * k + list(range(1, k + 1)), dtype=np.uint32)


# ---- 1. width edges -----------------------------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("n_msgs", [1, 63, 64, 65, 4097, 8300])
def test_width_edges(n_msgs, rows, monkeypatch):
    """Rows of 1 to 130 words over one tree of 300 peers, ~10 % masked; under
    the seam every full row is counted word by word."""
    seam(monkeypatch, rows)
    n, root, parent, live = one_topic(n_msgs, n_msgs)
    want = DR.topic_downstream(n, root, live, n_msgs, parent)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.publish(np.zeros(n_msgs))
        st = eng.run()
        got = eng.peer_downstream([0])
        same(got, want[:2], f"n_msgs {n_msgs}")
        assert got[1][root] == st.deliveries == want[2] and got[0][root] == n - 1
        identities(eng, 0, got)


# ---- 2. strips against levels, the block edge of the top run, live masks ---------------

def level_masks(parent):
    """The first and the last node of the widest level, and of the level above
    it (peer ids name nodes)."""
    n = parent.size
    d = GC.reference(n, [(0, parent)], np.ones(n, dtype=np.uint8))["topics"][0]["depth_of"]
    lvl = int(np.argmax(np.bincount(d[1:])))
    out = {}
    for name, l in (("level_ends", lvl), ("level_above_ends", lvl - 1)):
        at = np.nonzero(d == l)[0]
        if l >= 1:
            out[name] = sorted({int(at[0]), int(at[-1])})
    return out


def run_masks(parent, n_msgs, per):
    """One engine, one run per mask: strip_masks' dead sets (the first and the
    last node, either side of a strip bound, an inner node, everything but the
    root's children) and the ends of the widest level and of the one above."""
    n = parent.size
    masks = strip_masks(n - 1, per)
    masks.update(level_masks(parent))
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        assert np.array_equal(eng.graph(PE.G_NODE_PEER), np.arange(n))  # a peer id names a node
        for name, dead in masks.items():
            live = np.ones(n, dtype=np.uint8)
            live[dead] = 0
            eng.set_live(live)
            eng.publish(np.zeros(n_msgs))
            st = eng.run()
            want = DR.topic_downstream(n, 0, live, n_msgs, parent)
            got = eng.peer_downstream([0])
            same(got, want[:2], f"{n} peers, mask {name}")
            assert got[1][0] == st.deliveries == want[2] and got[0][0] == n - 1, name
            identities(eng, 0, got)  # (none of these shapes is deeper than 40 levels)


ONE_WORD = {"heap2047": lambda: heap_tree(2047), "heap2048": lambda: heap_tree(2048), "heap2049": lambda: heap_tree(2049),
            "heap4100": lambda: heap_tree(4100), "star3000": lambda: star(3001), "fan65_64": lambda: fan_tree(65, 64),
            "path40": lambda: path(40)}


@pytest.mark.parametrize("shape", list(ONE_WORD))
def test_strips_against_levels_one_word_rows(shape):
    """One message: one-word rows, 2,048 to a strip.  Heap trees in which a
    level bound falls inside a strip and a strip bound inside a level; a star
    whose one level is wider than a block and is summed by the root's wave; an
    inner node with 65 children (its wave sums them) beside one with 64 (its
    lane does); a path that the top kernel walks alone."""
    run_masks(ONE_WORD[shape](), 1, 2048)


@pytest.mark.parametrize("shape", ["heap15", "heap16", "heap17", "heap33", "heap64", "path40"])
def test_strips_against_levels_wide_rows(shape):
    """8,300 messages: 130-word rows, 15 to a strip, so levels of 8, 16 and 32
    nodes start and end inside strips."""
    parent = path(40) if shape == "path40" else heap_tree(int(shape[4:]))
    run_masks(parent, 8300, 16384 // (130 * 8))


TOP_EDGE = {
    # level 9 holds 256 nodes: every level fits the block, the top kernel walks them all
    "heap767": lambda: heap_tree(767),
    # level 9 holds 257: the first level wider than the block is the last one (leaves: no level launch)
    "heap768": lambda: heap_tree(768),
    # level 9 holds 512 and is the level before the last: one level launch of two blocks, then the top
    "heap1028": lambda: heap_tree(1028),
    "root256": lambda: star(257), "root257": lambda: star(258),
    # a level of 256 / 257 inner nodes directly under the root: one block, and two of which the second holds one node
    "root256_deep": lambda: star_deep(256), "root257_deep": lambda: star_deep(257),
}


@pytest.mark.parametrize("shape", list(TOP_EDGE))
def test_block_edge_of_the_top_run(shape):
    parent = TOP_EDGE[shape]()
    d = GC.reference(parent.size, [(0, parent)], np.ones(parent.size, dtype=np.uint8))["topics"][0]["depth_of"]
    width = np.bincount(d)
    want = {"heap767": [BLOCK, BLOCK], "heap768": [BLOCK, BLOCK + 1], "heap1028": [2 * BLOCK, 5], "root256": [1, BLOCK],
            "root257": [1, BLOCK + 1], "root256_deep": [BLOCK, BLOCK], "root257_deep": [BLOCK + 1, BLOCK + 1]}[shape]
    assert width[-2:].tolist() == want  # the two deepest levels
    run_masks(parent, 1, 2048)


def test_dead_nodes_keep_below_and_cut_carried():
    """A dead leaf, a dead inner node and a dead child of the root: below is
    the all-live answer in each case; carried is 0 at and beneath the dead
    node and shrinks by its subtree's share above it."""
    n, n_msgs = 255, 3
    parent = heap_tree(n)
    kids = kids_of(parent)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        eng.publish(np.zeros(n_msgs))
        eng.run()
        full = eng.peer_downstream([0])
        same(full, DR.topic_downstream(n, 0, np.ones(n, dtype=np.uint8), n_msgs, parent)[:2], "all live")
        assert np.array_equal(full[1], n_msgs * full[0])
        for dead in (254, 5, 1):  # a leaf, an inner node, a child of the root
            live = np.ones(n, dtype=np.uint8)
            live[dead] = 0
            eng.set_live(live)
            eng.publish(np.zeros(n_msgs))
            st = eng.run()
            got = eng.peer_downstream([0])
            same(got, DR.topic_downstream(n, 0, live, n_msgs, parent)[:2], f"dead {dead}")
            sub = sorted(under(kids, dead))
            assert np.array_equal(got[0], full[0])
            assert not got[1][[dead] + sub].any()
            lost = n_msgs * (1 + len(sub))
            assert got[1][0] == full[1][0] - lost == st.deliveries
            p = int(parent[dead])
            assert got[1][p] == full[1][p] - lost
            identities(eng, 0, got)


# ---- 3. start groups ----------------------------------------------------------------

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
    want = DR.window_downstream(n, live, [(root, c[1], parent), (root, c[0], parent)])
    with PE.Engine(n, 2, **kw) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        eng.publish(topics, starts)
        st = eng.run()
        assert st.windows == 1
        got = eng.peer_downstream([1, 0])
        same(got, want[:2], kind)
        assert got[1][root] == st.deliveries == want[2]
        one = eng.peer_downstream([1])
        same(one, DR.topic_downstream(n, root, live, c[1], parent)[:2], kind + " topic 1")
        identities(eng, 1, one)


# ---- 4. several topics sharing peers ------------------------------------------------

@pytest.mark.parametrize("order", [[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [1], [0], [2, 3], [0, 2], []])
def test_several_topics(order):
    """A 1-word topic, a 130-word one rooted at a leaf of the first, an idle
    one and one created but empty, named in several orders and subsets: the
    sums in peer space, nothing from the idle ones, nothing at peers in no
    topic."""
    n, free, (r0, p0), (r1, p1), live = shared_topics()
    msgs = np.concatenate([np.full(10, 0), np.full(8300, 1)]).astype(np.uint32)
    per = {0: DR.topic_downstream(n, r0, live, 10, p0), 1: DR.topic_downstream(n, r1, live, 8300, p1)}
    with PE.Engine(n, 4) as eng:
        eng.set_tree(0, r0, p0)
        eng.set_tree(1, r1, p1)
        eng.set_tree(2, r0, p0)
        eng.topic_create(3, 7)
        eng.set_live(live)
        eng.publish(msgs)
        st = eng.run()
        want = zeros(n)
        for t in order:
            if t in per:
                want = add(want, per[t][:2])
        got = eng.peer_downstream(order)
        same(got, want, str(order))
        assert not got[0][free].any() and not got[1][free].any()  # peers in no topic
        if {0, 1} <= set(order):
            assert per[0][1][r0] + per[1][1][r1] == st.deliveries == per[0][2] + per[1][2]
        if 1 in order:  # topic 1's root is a leaf of topic 0: everything behind it is topic 1's
            assert per[0][0][r1] == 0 and got[0][r1] == per[1][0][r1] == 200 and got[1][r1] == per[1][2]
        for t in order:
            if t in per:
                identities(eng, t, eng.peer_downstream([t]))


# ---- 5. meshes ----------------------------------------------------------------------

def test_meshes():
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
        assert raw_track(eng, [0, 1]) == E_STATE and raw_track(eng, [1]) == E_STATE  # a mesh is not tracked
        eng.downstream_track([0])
        eng.publish(np.concatenate([np.zeros(70), np.ones(70)]).astype(np.uint32))
        st = eng.run()
        assert st.windows == 1 and st.expand_mode == PE.MODE_COMPACT  # the tree runs beside the mesh: compaction path
        for named in ([1], [0, 1], [1, 0]):
            rc, b, c = raw_down(eng, named)
            assert rc == E_STATE and (b == FILL).all() and (c == FILL).all(), named
        want = DR.topic_downstream(n, root, live, 70, parent)
        got = eng.peer_downstream([0])
        same(got, want[:2], "a tree beside a mesh")
        assert 0 < got[1][root] == want[2] < st.deliveries
        identities(eng, 0, got)
        # the tracked tree becomes a mesh: that window adds nothing and is counted
        eng.set_children(0, root, rp, cl)
        eng.publish(np.zeros(5))
        st2 = eng.run()
        assert st2.deliveries > 0
        assert raw_down(eng, [0])[0] == E_STATE
        t = eng.downstream_take()
        same(t[:2], want[:2], "before the topic became a mesh")
        assert t[2:] == (2, 1)
        # ... and a tree again
        eng.set_tree(0, root, parent)
        eng.publish(np.zeros(3))
        eng.run()
        t = eng.downstream_take()
        same(t[:2], DR.topic_downstream(n, root, live, 3, parent)[:2], "a tree again")
        assert t[2:] == (1, 0)


# ---- 6. stale rows ------------------------------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
def test_stale_rows(rows, monkeypatch):
    """A wider first window over two topics, then a second run that publishes
    to one of them below a cut subtree: nothing of the first run's rows is
    counted, and the idle topic adds nothing, not even to below."""
    seam(monkeypatch, rows)
    rng = np.random.default_rng(66)
    n, root = 500, 2
    parent = random_tree(rng, n, root)
    kids = kids_of(parent)
    cut = max((p for p in kids if p != root), key=lambda p: len(under(kids, p)))
    assert len(under(kids, cut)) >= 5
    live = np.ones(n, dtype=np.uint8)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.publish(np.concatenate([np.zeros(300), np.ones(30)]).astype(np.uint32))  # five-word rows, then two
        st = eng.run()
        got = eng.peer_downstream([0, 1])
        same(got, DR.window_downstream(n, live, [(root, 300, parent), (root, 30, parent)])[:2], "first run")
        assert got[1][root] == st.deliveries
        live[cut] = 0
        eng.set_live(live)
        eng.publish(np.zeros(70))
        st = eng.run()
        want = DR.window_downstream(n, live, [(root, 70, parent), (root, 0, parent)])
        got = eng.peer_downstream([0, 1])
        same(got, want[:2], "second run")
        assert got[1][root] == st.deliveries == want[2] == 70 * (n - 2 - len(under(kids, cut)))
        assert got[0][root] == n - 1 and not eng.peer_downstream([1])[0].any()
        assert not got[1][[cut] + sorted(under(kids, cut))].any()


# ---- 7. deep trees ------------------------------------------------------------------

def test_deep_path_on_the_host_build():
    """A path of 300 peers: 300 levels of one node, all in the top kernel.
    Peer space has no column to clamp: every value is exact."""
    n = 300
    parent = path(n)
    live = np.ones(n, dtype=np.uint8)
    with make_engine(n, False) as eng:
        eng.set_tree(0, 0, parent)
        eng.publish(np.zeros(3))
        st = eng.run()
        assert_builds(eng, False)
        got = eng.peer_downstream([0])
        same(got, DR.topic_downstream(n, 0, live, 3, parent)[:2], "path 300")
        assert np.array_equal(got[0], (n - 1 - np.arange(n)).astype(np.uint64)) and got[1][0] == st.deliveries == 3 * 299
        live[280] = 0
        eng.set_live(live)
        eng.publish(np.zeros(3))
        st = eng.run()
        got = eng.peer_downstream([0])
        same(got, DR.topic_downstream(n, 0, live, 3, parent)[:2], "path 300, cut at 280")
        assert got[1][0] == st.deliveries == 3 * 279 and got[0][0] == n - 1 and not got[1][279:].any()


# ---- 8. tracking against the blocking call -----------------------------------------

def test_tracking_windows_runs_and_takes():
    """msg_window = 64: a run of three windows, two more runs, takes between:
    the totals equal the sum of downstream_ref per window and of
    peer_downstream per single-window run; below counts once per window."""
    n, root, parent, live = one_topic(0, 71)
    rng = np.random.default_rng(71)
    p1 = random_tree(rng, n, 9)

    def ref(c0, c1):
        return DR.window_downstream(n, live, [(root, c0, parent), (9, c1, p1)])

    with PE.Engine(n, 2, msg_window=64) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, 9, p1)
        eng.set_live(live)
        eng.downstream_track([1, 0])
        b, c, nw, nsk = eng.downstream_take()  # nothing has run
        assert (nw, nsk) == (0, 0) and not b.any() and not c.any()
        # 150 + 70 messages: windows of (64, 64), (64, 6), (22, 0)
        msgs = rng.permutation(np.concatenate([np.zeros(150), np.ones(70)])).astype(np.uint32)
        eng.publish(msgs)
        st = eng.run()
        assert st.windows == 3
        want = zeros(n)
        total = 0
        for c0, c1 in ((64, 64), (64, 6), (22, 0)):
            w = ref(c0, c1)
            want = add(want, w[:2])
            total += w[2]
        assert total == st.deliveries
        same(eng.peer_downstream([0, 1]), ref(22, 0)[:2], "last window")  # while the totals stand
        blocking = zeros(n)
        for c0, c1 in ((10, 3), (0, 64)):
            eng.publish(np.concatenate([np.zeros(c0), np.ones(c1)]).astype(np.uint32))
            st2 = eng.run()
            assert st2.windows == 1
            total += st2.deliveries
            want = add(want, ref(c0, c1)[:2])
            blocking = add(blocking, eng.peer_downstream([0, 1]))
        b, c, nw, nsk = eng.downstream_take()
        assert (nw, nsk) == (5, 0)
        same((b, c), want, "five windows")
        # below is a sum of per-window values: each topic had messages in four of the five windows
        b0, b1 = DR.topic_downstream(n, root, live, 1, parent)[0], DR.topic_downstream(n, 9, live, 1, p1)[0]
        assert np.array_equal(b, (4 * b0 + 4 * b1).astype(np.uint64))
        assert c[root] >= blocking[1][root] > 0  # topic 0's root carries that topic's deliveries of every window
        # a second take: zeros and no window
        b, c, nw, nsk = eng.downstream_take()
        assert (nw, nsk) == (0, 0) and not b.any() and not c.any()
        # take, run, take: the new run alone, equal to the blocking call's answer
        eng.publish(np.zeros(40))
        st3 = eng.run()
        b, c, nw, nsk = eng.downstream_take()
        assert (nw, nsk) == (1, 0) and c[root] == st3.deliveries
        same((b, c), ref(40, 0)[:2], "the new run")
        same((b, c), eng.peer_downstream([1, 0]), "the new run, blocking")
        # setting again zeroes the totals; a subset tracked: topic 1 is not counted
        eng.publish(np.zeros(5))
        eng.run()
        eng.downstream_track([0])
        b, c, nw, nsk = eng.downstream_take()
        assert (nw, nsk) == (0, 0) and not b.any() and not c.any()
        eng.publish(np.concatenate([np.zeros(7), np.ones(9)]).astype(np.uint32))
        eng.run()
        b, c, nw, nsk = eng.downstream_take()
        assert (nw, nsk) == (1, 0)
        same((b, c), ref(7, 0)[:2], "topic 0 alone")


def tree_window(ot, n, k, dropped=False):
    """k messages over oracle.Tree ot as the engine runs them: (below, carried)
    summed, the deliveries, the windows, and the last window's pair alone; a
    window per tree the messages met: the first message after a drop runs
    alone (it is lost below the failed edge, whether or not a repair then
    moves anybody), as does one that changes the tree; the rest run over the
    tree it left.  Every window adds its tree's below."""
    out = [np.zeros(n, dtype=np.int64) for _ in range(2)]
    last = None
    left, windows, deliveries = k, 0, 0
    while left:
        par = ot.parents()
        hop = ot.message()
        c = 1 if dropped or not np.array_equal(ot.parents(), par) else left
        dropped = False
        for _ in range(c - 1):
            assert np.array_equal(ot.message(), hop)
        got = hop != 0xFF
        got[ot.root] = False
        last = DR.from_parents(n, ot.root, par, c * got)
        assert last[1][ot.root] == c * got.sum()
        for o, w in zip(out, last):
            o += w
        deliveries += c * int(got.sum())
        left -= c
        windows += 1
    return tuple(out), deliveries, windows, last


def test_tracking_a_run_split_by_a_drop():
    """An interior peer dropped: topic 0's first message runs alone over the
    old tree, the rest over the repaired one (a rebuilt node space between two
    windows of one run); the totals are in peer space."""
    n, seed = 60, 3
    topics = np.array([0] * 5 + [1] * 5, dtype=np.uint32)
    ots = [O.Tree(n, 0, 2, 5, PE.Engine.topic_seed(seed, t)) for t in (0, 1)]
    for ot in ots:
        ot.join_all(range(1, n))
    with drop_engine(n, seed) as eng:
        par = eng.parents(0)
        assert np.array_equal(par, ots[0].parents())
        kids = kids_of(par)
        dead = max((p for p in kids if p != 0), key=lambda p: (len(kids[p]), len(under(kids, p))))
        eng.drop(0, [dead])
        assert ots[0].drop(dead) == 0
        eng.downstream_track([0, 1])
        eng.publish(topics)
        st = eng.run()
        assert st.windows >= 2
        (w0, d0, k0, l0), (w1, d1, k1, l1) = tree_window(ots[0], n, 5, dropped=True), tree_window(ots[1], n, 5)
        assert (k0, k1) == (2, 1) and d0 + d1 == st.deliveries
        b, c, nw, nsk = eng.downstream_take()
        assert (nw, nsk) == (st.windows, 0)
        same((b, c), add(tuple(x.astype(np.uint64) for x in w0), w1), "drop")
        assert c[0] == st.deliveries  # peer 0 is the root of both
        # the blocking call answers for the last window: topic 0's four messages
        # over the repaired tree, topic 1's five in that same window
        same(eng.peer_downstream([0, 1]), add(tuple(x.astype(np.uint64) for x in l0), l1), "drop, last window")


# ---- 9. churn -----------------------------------------------------------------------

@pytest.mark.parametrize("gpu_build", [True, False])
def test_churn(gpu_build):
    """Joins, leaves and drops between runs, the node space rebuilt on the GPU
    or on the host every batch: the subtrees move from window to window, and
    the totals over all batches, and the blocking answer for each batch's last
    window, follow the oracle's trees."""
    rng = np.random.default_rng(17)
    n, seed = 3000, 4
    eng = make_engine(n, gpu_build, seed=seed)
    ot = O.Tree(n, 0, 2, 5, PE.Engine.topic_seed(seed, 0))
    eng.topic_create(0, 0, 2, 5)
    eng.join(0, np.arange(1, n, 2))
    ot.join_all(range(1, n, 2))
    members = set(range(1, n, 2))
    eng.downstream_track([0])
    want = zeros(n)
    windows = deliveries = built = 0
    shapes = set()
    with eng:
        for step in range(10):
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
            w, d, kw, last = tree_window(ot, n, k, dropped=step % 3 == 1)
            assert run.deliveries == d and run.windows == kw, step
            want = add(want, w)
            windows += run.windows
            deliveries += run.deliveries
            blocking = eng.peer_downstream([0])
            same(blocking, last, f"step {step}, the batch's last window")
            identities(eng, 0, blocking)
            shapes.add(int(blocking[0].sum()))
            assert np.array_equal(eng.parents(0), ot.parents()), step
            built = assert_builds(eng, gpu_build, built)
        b, c, nw, nsk = eng.downstream_take()
        assert (nw, nsk) == (windows, 0)
        same((b, c), want, f"churn gpu_build {gpu_build}")
        assert c[0] == deliveries
        assert len(shapes) > 1  # the subtrees changed between windows


# ---- 10. pipelined ------------------------------------------------------------------

def tracked_blocking(e, batches):
    stats = []
    for b in batches:
        e.publish(b)
        stats.append(e.run())
    return e.downstream_take(), stats


def tracked_pipelined(e, batches):
    stats = []
    for i, b in enumerate(batches):
        e.publish(b)
        e.run_async()
        if i:
            stats.append(e.wait())
    rc, b, c, nw, nsk = raw_take(e)  # a run in flight: refused, nothing changes
    assert rc == E_STATE and nw == 0xCCCC and nsk == 0xDDDD and (b == FILL).all() and (c == FILL).all()
    stats.append(e.wait())
    return e.downstream_take(), stats


@pytest.mark.parametrize("shape", ["deep", "twin"])
def test_pipelined(shape):
    """Six run_async over a shape whose windows overlap their predecessors
    (deep: alternating row sets and overlapped prefixes; twin: whole windows
    side by side), then the waits and one take: the totals of the same six
    batches run one after the other."""
    if shape == "deep":
        wl = WL.cfg3(200_000, 16, 5000)
        live = (np.random.default_rng(11).random(wl.n_peers) >= 0.03).astype(np.uint8)
        live[[ts.root for ts in wl.topics]] = 1
        batches, plan = even_batches(len(wl.topics), 6, 52), {"overlap_min_bytes": 0}
    else:
        wl = WL.cfg3(60_000, 16, 4000)
        live = np.ones(wl.n_peers, dtype=np.uint8)
        batches, plan = even_batches(len(wl.topics), 6, 51), {"flood": 0}
    order = np.arange(len(wl.topics), dtype=np.uint32)[::-1].copy()

    def make():
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=64, plan=plan)
        WL.build_engine_topics(e, wl)
        e.set_live(live)
        e.downstream_track(order)
        return e

    with make() as e:
        t0, st0 = tracked_blocking(e, batches)
        last = e.peer_downstream(order)
    with make() as e:
        t1, st1 = tracked_pipelined(e, batches)
        over = e.overlapped_windows()
        same(e.peer_downstream(order), last, shape + " last window")
    print("pipelined", shape, "overlapped", over)
    assert over > 0
    assert t0[2] == t1[2] == sum(s.windows for s in st0) == 12 and t0[3] == t1[3] == 0
    same(t1[:2], t0[:2], shape)
    assert sum(s.deliveries for s in st1) == sum(s.deliveries for s in st0) > 0
    assert (t1[1] <= 64 * t1[0]).all()  # at most a window's messages to each node below
    if shape == "twin":  # all live: every node below holds every message of its window
        assert np.array_equal(t1[1], 64 * t1[0])
    assert np.array_equal(t1[0], 12 * last[0])  # below: the same node space in each of the 12 windows


# ---- 11. beside a sink, load tracking and hop tracking --------------------------------

def test_with_a_sink_load_and_hops_tracking():
    """A topics sink, load tracking, hop tracking and downstream tracking at
    once: each answer as with that one alone, and equal to its reference."""
    n, root, parent, live = one_topic(0, 91)
    rng = np.random.default_rng(91)
    msgs = [rng.integers(0, 2, size=150).astype(np.uint32), np.zeros(70, dtype=np.uint32)]

    def go(sink, load, hops, down):
        with PE.Engine(n, 2, msg_window=64) as e:
            e.set_tree(0, root, parent)
            e.set_tree(1, root, parent)
            e.set_live(live)
            if sink:
                e.sink_set_topics([0, 1])
            if load:
                e.load_track([0, 1])
            if hops:
                e.hops_track([0, 1])
            if down:
                e.downstream_track([0, 1])
            views = []
            for m in msgs:
                e.publish(m)
                e.run()
                if sink:
                    views.append(e.sink_take_topics())
            return (views, e.load_take() if load else None, e.hops_take() if hops else None,
                    e.downstream_take() if down else None)

    all4, only_sink, only_load = go(True, True, True, True), go(True, False, False, False), go(False, True, False, False)
    only_hops, only_down = go(False, False, True, False), go(False, False, False, True)
    same(all4[3][:2], only_down[3][:2], "downstream beside a sink, load and hop tracking")
    assert all4[3][2:] == only_down[3][2:] == (sum(v["n_windows"] for v in all4[0]), 0)
    # each against its own reference: the first batch runs as two windows of (64, 64) and the rest, the second as (64, 0), (6, 0)
    c = [int((msgs[0] == t).sum()) for t in (0, 1)]
    assert 64 < min(c) and max(c) <= 128
    wins = [(64, 64), (c[0] - 64, c[1] - 64), (64, 0), (6, 0)]
    want_d, want_l, want_h = zeros(n), zeros(n), None
    for c0, c1 in wins:
        want_d = add(want_d, DR.window_downstream(n, live, [(root, c0, parent), (root, c1, parent)])[:2])
        want_l = add(want_l, LR.window_load(n, live, [(root, c0, parent, None), (root, c1, parent, None)])[:2])
        h = HR.window_hops(n, live, [(root, c0, parent), (root, c1, parent)])[:3]
        want_h = h if want_h is None else tuple(a + b for a, b in zip(want_h, h))
    assert all4[3][2] == len(wins)
    same(all4[3][:2], want_d, "downstream against its reference")
    for a, b, w in zip(all4[1][:2], only_load[1][:2], want_l):
        assert np.array_equal(a, b) and np.array_equal(a, w)
    for a, b, w in zip(all4[2][:3], only_hops[2][:3], want_h):
        assert np.array_equal(a, b) and np.array_equal(a, w)
    assert all4[1][2] == only_load[1][2] and all4[2][3:] == only_hops[2][3:]
    assert all4[3][1][root] == all4[1][0].sum() == all4[2][2].sum() > 0  # deliveries, three ways
    for a, b in zip(all4[0], only_sink[0]):
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


# ---- 12. the rules ------------------------------------------------------------------

def test_rules():
    rng = np.random.default_rng(82)
    n, root = 300, 1
    parent = random_tree(rng, n, root)
    live = np.ones(n, dtype=np.uint8)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        # before any run
        rc, b, c = raw_down(eng, [0])
        assert rc == E_NOTREADY and (b == FILL).all() and (c == FILL).all()
        rc, b, c, nw, nsk = raw_take(eng)
        assert rc == E_NOTREADY and nw == 0xCCCC and nsk == 0xDDDD and (b == FILL).all() and (c == FILL).all()
        eng.publish(np.zeros(10))
        eng.run()
        # the arguments
        assert raw_down(eng, [0, 0])[0] == E_INVAL  # a topic named twice
        rc, b, c = raw_down(eng, [0, 2])
        assert rc == E_RANGE and (b == FILL).all() and (c == FILL).all()  # nothing written
        assert raw_down(eng, [0], below=False, carried=False)[0] == E_INVAL
        assert eng._L.ps_peer_downstream(eng._h, None, 1, b.ctypes.data_as(U64P), None) == E_INVAL
        # either output alone; no topic: zeros; an idle topic: zeros
        full = eng.peer_downstream([0, 1])
        same(full, DR.window_downstream(n, live, [(root, 10, parent), (root, 0, parent)])[:2], "full")
        rc, b, c = raw_down(eng, [0], carried=False)
        assert rc == 0 and np.array_equal(b, full[0]) and (c == FILL).all()
        rc, b, c = raw_down(eng, [0], below=False)
        assert rc == 0 and np.array_equal(c, full[1]) and (b == FILL).all()
        rc, b, c = raw_down(eng, [])
        assert rc == 0 and not b.any() and not c.any()
        b, c = eng.peer_downstream([1])
        assert not b.any() and not c.any()
        # tracking: a refused call leaves the previous tracking
        eng.downstream_track([0])
        assert raw_track(eng, [1, 1]) == E_INVAL and raw_track(eng, [0, 5]) == E_RANGE
        assert eng._L.ps_downstream_track(eng._h, None, 2) == E_INVAL
        eng.publish(np.zeros(3))
        eng.run()
        b, c, nw, nsk = eng.downstream_take()
        assert (nw, nsk) == (1, 0) and c[root] == 3 * (n - 1) and b[root] == n - 1
        assert eng._L.ps_downstream_take(eng._h, None, None, None, None) == E_INVAL
        # NULL arrays are allowed: the take still clears
        eng.publish(np.zeros(2))
        eng.run()
        nwc, nskc = C.c_uint64(), C.c_uint64()
        assert eng._L.ps_downstream_take(eng._h, None, None, C.byref(nwc), C.byref(nskc)) == 0 and nwc.value == 1
        assert eng.downstream_take()[2] == 0
        # a run in flight
        eng.publish(np.zeros(4))
        eng.run_async()
        assert raw_track(eng, [1]) == E_STATE
        rc, b, c, nw, nsk = raw_take(eng)
        assert rc == E_STATE and nw == 0xCCCC and (b == FILL).all() and (c == FILL).all()
        eng.wait()
        b, c, nw, nsk = eng.downstream_take()
        assert (nw, nsk) == (1, 0) and c[root] == 4 * (n - 1)
        # setting again and clearing zero the totals
        eng.publish(np.zeros(1))
        eng.run()
        eng.downstream_track([1, 0])
        b, c, nw, nsk = eng.downstream_take()
        assert (nw, nsk) == (0, 0) and not b.any() and not c.any()
        eng.downstream_track([])
        rc, _, _, nw, _ = raw_take(eng)
        assert rc == E_NOTREADY and nw == 0xCCCC
        eng.publish(np.zeros(1))
        eng.run()  # nothing is tracked: the run is as ever
        assert eng.peer_downstream([0])[1][root] == n - 1


def test_a_topic_set_anew_since_the_window():
    """The levels are the last build's.  A parent array set over a parent
    array keeps them, and the last window is still answered; set over a join
    topic it starts the record afresh: PS_E_STATE, nothing written, until the
    next run."""
    rng = np.random.default_rng(83)
    n = 200
    live = np.ones(n, dtype=np.uint8)
    p0, p1 = random_tree(rng, n, 0), random_tree(rng, n, 0)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, 0, p0)
        eng.topic_create(1, 0, 2, 5)
        eng.join(1, np.arange(1, n))
        eng.publish(np.array([0] * 4 + [1] * 6, dtype=np.uint32))
        eng.run()
        before = eng.peer_downstream([0, 1])
        only0 = eng.peer_downstream([0])
        same(only0, DR.topic_downstream(n, 0, live, 4, p0)[:2], "topic 0")
        assert before[1][0] == 4 * (n - 1) + 6 * (n - 1)
        eng.set_tree(0, 0, p1)  # over a parent array: the window's levels stay
        same(eng.peer_downstream([0, 1]), before, "after set_tree over a parent array")
        eng.set_tree(1, 0, p1)  # over a join topic: its record starts afresh
        rc, b, c = raw_down(eng, [0, 1])
        assert rc == E_STATE and (b == FILL).all() and (c == FILL).all()
        same(eng.peer_downstream([0]), only0, "the other topic alone")
        eng.publish(np.array([0] * 3 + [1] * 2, dtype=np.uint32))
        eng.run()
        same(eng.peer_downstream([0, 1]), DR.window_downstream(n, live, [(0, 3, p1), (0, 2, p1)])[:2], "after the next run")


def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(3)]
    try:
        # an engine that is tracking takes no ranks
        engines[2].downstream_track([0])
        with pytest.raises(PE.EngineError) as ei:
            engines[2].dist_init_loopback(lb, 0, PE.PART_PEER)
        assert ei.value.code == E_STATE
        for r, e in enumerate(engines[:2]):
            e.dist_init_loopback(lb, r, PE.PART_PEER)
            e.set_tree(0, root, parent)
            assert raw_track(e, [0]) == E_STATE  # one rank only
            e.publish(np.zeros(50))
        errs = []

        def go(e):
            try:
                e.run()
            except Exception as ex:  # noqa: BLE001
                errs.append(ex)

        th = [threading.Thread(target=go, args=(e,)) for e in engines[:2]]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in th) and not errs, errs
        for e in engines[:2]:
            rc, b, c = raw_down(e, [0])
            assert rc == E_STATE and (b == FILL).all() and (c == FILL).all()
            assert raw_take(e)[0] == E_NOTREADY
    finally:
        for e in engines:
            e.close()
