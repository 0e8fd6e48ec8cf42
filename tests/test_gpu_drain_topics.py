"""GPU: a topic's whole audience (ps_drain_topics / Engine.drain_topics) --
one list per topic, the number of nodes that hold it, and the nodes that do
not.  The reference is the existing API: Q_t, the peers of the topic's
non-root nodes in node order, read from the node space (G_NODE_PEER and the
topic's node range), goes to Engine.drain_shared as explicit queries and the
two answers are compared: per peer the expanded ids, bit-exact; n_nodes, the
count identity, the exceptions' order; and that sharing happens where
drain_shared shares (one shared list per topic with a full row, named by every
full query and by no exception).

The kernel's strips: a run of nodes of one topic holding at most 16 KiB of
rows, a row of up to 64 mask words counted at the power of two at or above its
words and a wider one at its words.  So a 1-word row gives strips of 2048
nodes (N - 1 non-root nodes = 2047, 2048, 2049 for N = 2048, 2049, 2050) and a
130-word row (8300 messages) strips of 15 nodes (N = 15, 16, 17).
"""
import ctypes as C
import threading

import numpy as np
import pytest

import psengine as PE
from test_gpu_drain_batch import oracle_lists, random_mesh2, random_tree, tree_hops
from test_gpu_drain_shared import one_topic, run_tree_case, shared

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NARROW_STRIP, WIDE_STRIP = 2048, 15  # nodes per strip: 1-word rows, 130-word rows


def audience(eng, topics):
    """Q_t of every topic: the peers of its non-root nodes, in node order."""
    node_peer = eng.graph(PE.G_NODE_PEER)
    out = []
    for t in topics:
        g = eng.graph_topic(int(t))
        lo, hi = g["nbase"] + 1, g["nbase"] + g["n_nodes"]
        out.append(node_peer[lo:hi].astype(np.uint32) if g["exists"] and hi > lo else np.empty(0, dtype=np.uint32))
    return out


def well_formed(r, n):
    assert r["topic_list"].dtype == np.uint32 and r["exc_peer"].dtype == np.uint32 and r["exc_list"].dtype == np.uint32
    assert r["n_nodes"].dtype == np.uint64 and r["n_full"].dtype == np.uint64 and r["ids"].dtype == np.uint32
    assert r["exc_off"].dtype == np.uint64 and r["list_off"].dtype == np.uint64
    assert r["topic_list"].size == n and r["n_nodes"].size == n and r["n_full"].size == n and r["exc_off"].size == n + 1
    eo, lo = r["exc_off"].astype(np.int64), r["list_off"].astype(np.int64)
    assert eo[0] == 0 and np.all(np.diff(eo) >= 0) and eo[-1] == r["exc_peer"].size == r["exc_list"].size
    assert lo[0] == 0 and np.all(np.diff(lo) >= 0) and lo[-1] == r["ids"].size
    # numbered in request order: a topic's shared list, then its exceptions' private lists
    k = 0
    for i in range(n):
        if r["topic_list"][i] != NONE:
            assert r["topic_list"][i] == k
            k += 1
        for l in r["exc_list"][eo[i]:eo[i + 1]]:
            if l != NONE:
                assert l == k
                k += 1
    assert k == lo.size - 1


def check(eng, topics, window=None, sharing=True):
    """drain_topics(topics) against drain_shared over (t, Q_t).  window: topic
    -> its window messages in arrival order, where the caller knows them ([]:
    none).  sharing: full rows share (False under the private seam).  Returns
    the answer and, per entry, Q_t."""
    topics = [int(t) for t in topics]
    r = eng.drain_topics(topics)
    well_formed(r, len(topics))
    Q = audience(eng, topics)
    qt = np.concatenate([np.full(q.size, t, dtype=np.uint32) for t, q in zip(topics, Q)] + [np.empty(0, dtype=np.uint32)])
    qp = np.concatenate(Q + [np.empty(0, dtype=np.uint32)])
    a_list, a_off, a_ids = shared(eng, qt, qp)
    ours = lambda l: r["ids"][int(r["list_off"][l]):int(r["list_off"][l + 1])]
    theirs = lambda l: a_ids[int(a_off[l]):int(a_off[l + 1])]
    same = {}  # (our list, drain_shared's list) -> equal, compared once

    def equal(lo, la):
        if (lo, la) not in same:
            same[(lo, la)] = np.array_equal(ours(lo), theirs(la))
        return same[(lo, la)]

    pos = 0
    for i, t in enumerate(topics):
        q = Q[i]
        assert r["n_nodes"][i] == q.size
        assert len(set(q.tolist())) == q.size
        mine = a_list[pos:pos + q.size]
        pos += q.size
        e0, e1 = int(r["exc_off"][i]), int(r["exc_off"][i + 1])
        tl = int(r["topic_list"][i])
        if window is not None and t in window and not window[t]:  # nothing was sent: nobody missed anything
            assert (r["n_full"][i], e1 - e0, tl) == (0, 0, NONE) and np.all(mine == NONE)
            continue
        if np.all(mine == NONE) and e1 == e0:  # (no message in the window: drain_shared cannot tell)
            assert r["n_full"][i] == 0 and tl == NONE and (window is None or t not in window)
            continue
        assert r["n_full"][i] + (e1 - e0) == q.size  # the count identity
        k = e0
        full_lists = set()
        n_full = 0
        counts = np.bincount(mine[mine != NONE]) if np.any(mine != NONE) else np.zeros(1, dtype=np.int64)
        for j, p in enumerate(q.tolist()):
            la = int(mine[j])
            if k < e1 and r["exc_peer"][k] == p:  # an exception, in Q_t order
                le = int(r["exc_list"][k])
                assert (le == NONE) == (la == NONE), (t, p)
                if le != NONE:
                    assert le != tl and equal(le, la), (t, p)
                    assert counts[la] == 1, (t, p)  # a list drain_shared shares is no exception's
                    if sharing and window is not None and t in window:
                        assert ours(le).tolist() != window[t], (t, p)  # a row that holds everything is full
                k += 1
            else:  # on the topic's shared list
                assert tl != NONE and la != NONE and equal(tl, la), (t, p)
                full_lists.add(la)
                n_full += 1
        assert k == e1  # every exception was met, in order
        assert n_full == r["n_full"][i]
        if tl == NONE:
            assert n_full == 0
        else:
            assert sharing and n_full > 0 and len(full_lists) == 1  # one shared list, and somebody holds it
            if window is not None and t in window:
                assert ours(tl).tolist() == window[t]
    assert pos == qt.size
    return r, Q


def per_peer(r, Q, i):
    """Entry i expanded: peer -> ids (numpy), for the oracle comparisons."""
    ids = lambda l: r["ids"][int(r["list_off"][l]):int(r["list_off"][l + 1])]
    e0, e1 = int(r["exc_off"][i]), int(r["exc_off"][i + 1])
    exc = {int(p): int(l) for p, l in zip(r["exc_peer"][e0:e1], r["exc_list"][e0:e1])}
    out = {}
    for p in Q[i].tolist():
        l = exc.get(p, int(r["topic_list"][i]))
        out[p] = ids(l) if l != NONE else np.empty(0, dtype=np.uint32)
    return out


# ---- widths ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n_msgs", [1, 63, 64, 65, 129, 1000, 4095, 4096, 4097, 8300])
def test_width_edges(n_msgs):
    """Rows of 1, 2, 3, 16 and 64 words (lane groups of 1, 2, 4, 16 and 64),
    the pad word, 65 and 130 words (the wide path: two and three loads a
    node); 300 peers, a tenth masked."""
    n, root, parent, live = one_topic(n_msgs, n_msgs)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        first = eng.publish(np.zeros(n_msgs))
        eng.run()
        window = {0: list(range(first, first + n_msgs))}
        r, Q = check(eng, [0], window)
        hop = tree_hops(parent, root, live)
        got = per_peer(r, Q, 0)
        peers = sorted(got)
        exp = oracle_lists(np.zeros(len(peers)), peers, np.zeros(n_msgs), None, first, hop, root)
        for p, x in zip(peers, exp):
            assert got[p].tolist() == x, p
        reached = sum(1 for x in exp if x)
        assert 0 < reached < len(peers)
        assert r["n_full"][0] == reached and r["exc_peer"].size == len(peers) - reached
        assert np.all(r["exc_list"] == NONE) and r["list_off"].size - 1 == 1


# ---- node counts ----------------------------------------------------------------------------

@pytest.mark.parametrize("n,n_msgs", [(2, 1), (3, 1), (64, 1), (65, 1), (66, 1), (NARROW_STRIP, 1), (NARROW_STRIP + 1, 1),
                                      (NARROW_STRIP + 2, 1), (4097, 1), (70_001, 1), (WIDE_STRIP, 8300),
                                      (WIDE_STRIP + 1, 8300), (WIDE_STRIP + 2, 8300), (4097, 8300)])
def test_node_count_edges(n, n_msgs):
    """All peers in one tree, none masked: every count at its maximum.  One
    node below, at and above a 64-node load and a strip boundary, for a narrow
    and a wide row; many strips; a partly filled last strip."""
    rng = np.random.default_rng(n + n_msgs)
    root = n // 2
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        first = eng.publish(np.zeros(n_msgs))
        eng.run()
        r, Q = check(eng, [0], {0: list(range(first, first + n_msgs))})
        assert r["n_nodes"][0] == n - 1 and r["n_full"][0] == n - 1 and r["exc_peer"].size == 0
        assert sorted(Q[0].tolist()) == [p for p in range(n) if p != root]
        assert r["topic_list"][0] == 0 and r["ids"].tolist() == list(range(first, first + n_msgs))


# ---- exceptions -----------------------------------------------------------------------------

def kids_of(parent):
    kids = {}
    for p, q in enumerate(parent.tolist()):
        if q != NONE:
            kids.setdefault(q, []).append(p)
    return kids


def under(kids, p):
    out, todo = set(), list(kids.get(p, []))
    while todo:
        x = todo.pop()
        out.add(x)
        todo += kids.get(x, [])
    return out


@pytest.mark.parametrize("n,n_msgs,strip", [(5000, 3, NARROW_STRIP), (100, 8300, WIDE_STRIP)])
def test_exceptions_at_the_edges(n, n_msgs, strip):
    """Masked by node index: the first non-root node, the last node, the two
    nodes either side of the first strip boundary, and an interior node with
    a subtree: PS_NONE for each and for everything below it."""
    rng = np.random.default_rng(n)
    root = 1
    parent = random_tree(rng, n, root)
    kids = kids_of(parent)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        nodes = audience(eng, [0])[0]  # node u's peer is nodes[u - 1]
        assert nodes.size == n - 1
        edges = {int(nodes[0]), int(nodes[-1]), int(nodes[strip - 1]), int(nodes[strip])}
        inner = [int(p) for p in nodes[1:-1] if int(p) not in edges and len(under(kids, int(p))) >= 2]
        masked = edges | {inner[len(inner) // 2]}
        assert len(masked) == 5
        live = np.ones(n, dtype=np.uint8)
        live[list(masked)] = 0
        eng.set_live(live)
        first = eng.publish(np.zeros(n_msgs))
        eng.run()
        r, Q = check(eng, [0], {0: list(range(first, first + n_msgs))})
        assert np.array_equal(Q[0], nodes)  # (a live mask moves no node)
        cut = set(masked)
        for p in masked:
            cut |= under(kids, p)
        assert set(r["exc_peer"].tolist()) == cut and np.all(r["exc_list"] == NONE)
        assert r["n_full"][0] == n - 1 - len(cut) > 0
        assert r["exc_peer"][0] == nodes[0] and r["exc_peer"][-1] == nodes[-1]


def test_all_but_the_roots_children_cut():
    rng = np.random.default_rng(17)
    n, root = 3000, 0
    parent = random_tree(rng, n, root)
    first_level = [p for p in range(n) if parent[p] == root]
    live = np.zeros(n, dtype=np.uint8)
    live[[root] + first_level] = 1
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        first = eng.publish(np.zeros(70))
        eng.run()
        r, Q = check(eng, [0], {0: list(range(first, first + 70))})
        assert r["n_full"][0] == len(first_level) and r["exc_peer"].size == n - 1 - len(first_level)
        assert set(Q[0].tolist()) - set(r["exc_peer"].tolist()) == set(first_level)
        assert np.all(r["exc_list"] == NONE)


# ---- layouts --------------------------------------------------------------------------------

def windows_of(qt, exp):
    """topic -> its window messages: the longest expected list of its queries."""
    return {t: max((x for q, x in zip(qt, exp) if q == t), key=len) for t in set(int(q) for q in qt)}


@pytest.mark.parametrize("kind", ["unpaced", "paced0", "paced1", "compact"])
def test_tree_layouts(kind):
    """Node-major rows, group-major blocks, level-aligned rows, the compaction
    path, two topics each."""
    eng, qt, qp, topics, hop, root, exp = run_tree_case(kind)
    with eng:
        window = windows_of(qt, exp)
        r, Q = check(eng, [0, 1], window)
        for i in (0, 1):
            reached = sum(1 for p in Q[i].tolist() if hop[p] != 0xFF)
            assert r["n_full"][i] == reached > 100
            assert len(window[i]) == int(np.sum(np.asarray(topics) == i))
        r2, _ = check(eng, [1, 0], window)
        assert r2["topic_list"].tolist() == [0, 1] and r2["n_full"].tolist() == r["n_full"][::-1].tolist()


@pytest.mark.parametrize("paced", [False, True])
def test_mesh(paced):
    """Two parents per node.  Unpaced: a mask-layout table, no generation
    test, one shared list.  Paced: the arrival-order table -- every node takes
    a private list and the topic has no shared one."""
    rng = np.random.default_rng(41 + paced)
    n, root, n_msgs = 800, 5, 300
    rp, cl = random_mesh2(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    starts = rng.integers(0, 5, size=n_msgs) if paced else None
    with PE.Engine(n, 1) as eng:
        eng.set_children(0, root, rp, cl)
        eng.set_live(live)
        first = eng.publish(np.zeros(n_msgs), starts)
        eng.run()
        if paced:
            r, Q = check(eng, [0], None)
            assert r["topic_list"][0] == NONE and r["n_full"][0] == 0
            assert r["exc_peer"].size == Q[0].size and np.array_equal(r["exc_peer"], Q[0])
            assert np.all(r["exc_list"] != NONE) and r["list_off"].size - 1 == Q[0].size
            assert r["ids"].size > n_msgs
        else:
            r, Q = check(eng, [0], {0: list(range(first, first + n_msgs))})
            assert r["topic_list"][0] == 0 and r["n_full"][0] > 100 and r["exc_peer"].size > 0


def test_private_seam(monkeypatch):
    """PSAMD_AB=1 PSAMD_DRAIN_SHARED=private: no row is full, every reached
    node takes a list of its own; the same ids per peer."""
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_DRAIN_SHARED", "private")
    eng, qt, qp, topics, hop, root, exp = run_tree_case("unpaced")
    with eng:
        r, Q = check(eng, [0, 1], windows_of(qt, exp), sharing=False)
        assert r["n_full"].tolist() == [0, 0] and r["topic_list"].tolist() == [NONE, NONE]
        reached = sum(1 for q in Q for p in q.tolist() if hop[p] != 0xFF)
        assert reached > 200 and r["list_off"].size - 1 == reached == int(np.sum(r["exc_list"] != NONE))
        assert r["exc_peer"].size == Q[0].size + Q[1].size


def test_dead_subtree_stale_rows():
    """The cut-subtree scenario of test_gpu_drain_shared.py: the rows below the
    cut keep the first window's bits under a stale generation."""
    rng = np.random.default_rng(51)
    n, root = 600, 0
    parent = random_tree(rng, n, root)
    kids = kids_of(parent)
    cut = max((p for p in range(n) if parent[p] == root), key=lambda p: len(under(kids, p)))
    below = under(kids, cut)
    assert len(below) >= 10
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        first = eng.publish(np.zeros(200))
        eng.run()
        r, _ = check(eng, [0], {0: list(range(first, first + 200))})
        assert r["n_full"][0] == n - 1 and r["exc_peer"].size == 0
        live = np.ones(n, dtype=np.uint8)
        live[cut] = 0
        eng.set_live(live)
        first = eng.publish(np.zeros(150))
        eng.run()
        r, _ = check(eng, [0], {0: list(range(first, first + 150))})
        assert set(r["exc_peer"].tolist()) == below | {cut} and np.all(r["exc_list"] == NONE)
        assert r["n_full"][0] == n - 2 - len(below)


# ---- several topics -------------------------------------------------------------------------

@pytest.mark.parametrize("order", [[0, 1, 2, 3], [3, 2, 1, 0], [1], [2, 0]])
def test_several_topics(order):
    """A 1-word and a 130-word topic, an idle one and a created-but-empty one;
    drain_shared's answer is the same before and after (the tables are shared)."""
    n, root, parent, live = one_topic(0, 77)
    topics = np.concatenate([np.zeros(10), np.ones(8300)]).astype(np.uint32)
    with PE.Engine(n, 4) as eng:
        for t in range(3):
            eng.set_tree(t, root, parent)
        eng.topic_create(3, root)
        eng.set_live(live)
        first = eng.publish(topics)
        eng.run()
        qt = np.tile([0, 1, 2, 3], n).astype(np.uint32)
        qp = np.repeat(np.arange(n), 4).astype(np.uint32)
        before = shared(eng, qt, qp)
        window = {0: list(range(first, first + 10)), 1: list(range(first + 10, first + 8310)), 2: [], 3: []}
        r, Q = check(eng, order, window)
        after = shared(eng, qt, qp)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        hop = tree_hops(parent, root, live)
        reached = sum(1 for p in range(n) if p != root and hop[p] != 0xFF)
        for i, t in enumerate(order):
            assert r["n_nodes"][i] == (0 if t == 3 else n - 1)
            assert r["n_full"][i] == (reached if t < 2 else 0)
            assert (r["topic_list"][i] == NONE) == (t >= 2)
            assert r["exc_off"][i + 1] - r["exc_off"][i] == (n - 1 - reached if t < 2 else 0)
        assert r["ids"].size == sum(len(window[t]) for t in order)


# ---- churn ----------------------------------------------------------------------------------

def test_after_churn():
    """Join, leave and drop, then runs: the answer follows the new node
    space, a dropped peer and the peers it orphaned are absent, and the node
    space was rebuilt on the GPU.  (Two runs: the first repairs the tree
    between its windows and prunes the peers that left behind its messages,
    which leaves the node space to be rebuilt; reading the graph then would
    rebuild it and drop the window.  The second runs on the rebuilt one.)"""
    n, joined, seed = 400, 300, 3
    with PE.Engine(n, 1, seed=seed) as eng:
        eng.topic_create(0, 0, 2, 5)
        eng.join(0, np.arange(1, joined))
        eng.publish(np.zeros(20))
        eng.run()
        r, Q = check(eng, [0])
        assert r["n_nodes"][0] == joined - 1 == r["n_full"][0]
        par = eng.parents(0)
        kids = kids_of(par)
        dead = max((p for p in kids if p != 0), key=lambda p: (len(kids[p]), len(under(kids, p))))
        assert len(kids[dead]) >= 2
        childless = [p for p in range(1, joined) if p not in kids and p != dead][:10]
        eng.leave(0, childless)
        eng.join(0, np.arange(joined, joined + 40))
        eng.drop(0, [dead])
        eng.publish(np.zeros(5))
        st = eng.run()  # the drop's repair, and behind the messages the prune of the peers that left
        assert st.windows >= 2
        first = eng.publish(np.zeros(5))
        eng.run()  # over the node space rebuilt after that prune
        r, Q = check(eng, [0])
        rep = eng.build_report()
        assert rep["last_kind"] == "gpu" and rep["fallbacks"] == 0, rep
        after = eng.parents(0)
        members = set(Q[0].tolist())
        assert dead not in members and dead not in r["exc_peer"].tolist()
        connected, orphan_roots = set(), set()
        for p in range(1, n):
            q = p
            while q != 0 and after[q] != NONE:
                q = int(after[q])
            if q == 0:
                connected.add(p)
            elif after[p] == NONE and p < joined + 40 and p != dead and p not in childless:
                orphan_roots.add(p)
        assert not (orphan_roots & members)
        assert connected <= members and connected & set(range(joined, joined + 40))
        full = members - set(r["exc_peer"].tolist())
        assert full and full <= connected
        last = r["ids"][int(r["list_off"][0]):int(r["list_off"][1])].tolist()
        assert r["topic_list"][0] == 0 and last == list(range(first, first + 5))


# ---- rules ----------------------------------------------------------------------------------

U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def raw(eng, topics):
    """The bare call: (rc, pointers, n_lists, total); the pointers start NULL,
    the counts at a sentinel."""
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    p32 = [U32P() for _ in range(4)]  # topic_list, exc_peer, exc_list, msg
    p64 = [U64P() for _ in range(4)]  # n_nodes, n_full, exc_off, list_off
    n_lists, total = C.c_uint32(0xBBBB), C.c_uint64(0xCCCC)
    rc = eng._L.ps_drain_topics(eng._h, t.ctypes.data_as(U32P), t.size, C.byref(p32[0]), C.byref(p64[0]), C.byref(p64[1]),
                                C.byref(p64[2]), C.byref(p32[1]), C.byref(p32[2]), C.byref(p64[3]), C.byref(p32[3]),
                                C.byref(n_lists), C.byref(total))
    return rc, p32, p64, n_lists.value, total.value


def untouched(res):
    rc, p32, p64, n_lists, total = res
    return not any(bool(p) for p in p32 + p64) and n_lists == 0xBBBB and total == 0xCCCC


def test_rules_and_views():
    rng = np.random.default_rng(81)
    n, root = 300, 0
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        res = raw(eng, [0])
        assert res[0] == -8 and untouched(res)  # PS_E_NOTREADY: no run yet
        first = eng.publish(np.arange(100) % 2)
        eng.run()
        r = eng.drain_topics([])  # n == 0
        assert r["exc_off"].tolist() == [0] and r["list_off"].tolist() == [0]
        assert r["topic_list"].size == 0 and r["ids"].size == 0 and r["exc_peer"].size == 0
        res = raw(eng, [0, 1, 0])
        assert res[0] == -1 and untouched(res)  # a topic named twice
        res = raw(eng, [0, 2])
        assert res[0] == -7 and untouched(res)  # out of range: nothing written
        # the views of one call stay readable until the next
        rc, p32, p64, n_lists, total = raw(eng, [1, 0])
        assert rc == 0 and n_lists == 2 and total == 100
        want = eng.drain_shared([0, 1], [5, 5])  # (another drain in between)
        assert want[2].size == 100
        assert np.ctypeslib.as_array(p32[0], shape=(2,)).tolist() == [0, 1]
        assert np.ctypeslib.as_array(p64[0], shape=(2,)).tolist() == [n - 1, n - 1]
        assert np.ctypeslib.as_array(p64[1], shape=(2,)).tolist() == [n - 1, n - 1]
        assert np.ctypeslib.as_array(p64[2], shape=(3,)).tolist() == [0, 0, 0]
        assert np.ctypeslib.as_array(p64[3], shape=(3,)).tolist() == [0, 50, 100]
        assert np.ctypeslib.as_array(p32[3], shape=(100,)).tolist() == (
            list(range(first + 1, first + 100, 2)) + list(range(first, first + 100, 2)))
        check(eng, [0, 1])


def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(2)]
    try:
        for k, e in enumerate(engines):
            e.dist_init_loopback(lb, k, PE.PART_PEER)
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
            res = raw(e, [0])
            assert res[0] == -3 and untouched(res)  # PS_E_STATE
    finally:
        for e in engines:
            e.close()
        lb.close()


def test_after_async_runs():
    rng = np.random.default_rng(101)
    n, root = 2000, 0
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1, plan={"flood": 0}) as eng:
        eng.set_tree(0, root, parent)
        eng.publish(np.zeros(1000))
        eng.run_async()
        first = eng.publish(np.zeros(1000))
        eng.run_async()
        eng.wait()
        eng.wait()
        r, _ = check(eng, [0], {0: list(range(first, first + 1000))})
        assert r["n_full"][0] == n - 1 and r["exc_peer"].size == 0


def test_last_window_only():
    rng = np.random.default_rng(61)
    n, root = 400, 2
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1, msg_window=128) as eng:
        eng.set_tree(0, root, parent)
        first = eng.publish(np.zeros(300))
        st = eng.run()
        assert st.windows == 3
        r, _ = check(eng, [0])
        ids = r["ids"]
        assert r["list_off"].size - 1 == 1 and 0 < ids.size <= 128
        assert ids.tolist() == list(range(int(ids[0]), first + 300))  # one window, ending with the run's last message
        assert r["n_full"][0] == n - 1
