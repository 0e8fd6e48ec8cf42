"""GPU: per-peer load (ps_peer_load, ps_load_track / ps_load_take; DESIGN.md
§5.5i) -- how many messages each peer received and how many copies it wrote
to its children, summed over the named topics, for the last window or
accumulated behind every window of every run.

Every comparison is bit-exact, both arrays, against tests/load_ref.py: the
oracle's deliveries (oracle.disseminate, or oracle.Tree under churn) times the
child counts of the input tree restricted to its members.  Where every topic
is named, recv.sum() equals the run's ps_stats.deliveries.  The seam
(PSAMD_AB=1 PSAMD_LOAD_COUNT=rows) makes the kernel count full rows from their
words, the path a healthy tree's all-or-nothing rows never take otherwise."""
import ctypes as C
import threading

import numpy as np
import pytest

import graph_check as GC
import load_ref as LR
import oracle as O
import psengine as PE
from psengine import workloads as WL
from test_gpu_churn import assert_builds, make_engine
from test_gpu_drain_batch import random_mesh2, random_tree
from test_gpu_drain_shared import one_topic
from test_gpu_drain_topics import kids_of, under
from test_gpu_sink import drop_engine, even_batches, window_chunks

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
FILL = 0xABABABABABABABAB


# ---- helpers ------------------------------------------------------------------------

def seam(monkeypatch, on=True):
    """Read at ps_create: set before the engine is made."""
    if on:
        monkeypatch.setenv("PSAMD_AB", "1")
        monkeypatch.setenv("PSAMD_LOAD_COUNT", "rows")


def same(got, want, what=""):
    """(recv, sent) against (recv, sent), uint64, bit for bit."""
    for name, g, w in zip(("recv", "sent"), got, want):
        assert g.dtype == np.uint64 and g.shape == w.shape, (what, name)
        if not np.array_equal(g, w.astype(np.uint64)):
            bad = np.nonzero(g != w.astype(np.uint64))[0]
            raise AssertionError(f"{what} {name}: {bad.size} peers differ, first {bad[:6]} got {g[bad[:6]]} "
                                 f"want {w[bad[:6]]}")


def add(a, b):
    return a[0] + b[0], a[1] + b[1]


def zeros(n):
    return np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)


def heap_tree(n):
    """Peer p's upstream is (p - 1) // 2, root 0: BFS order with ascending
    siblings numbers the nodes as the peers, so a peer id names a node."""
    parent = ((np.arange(n, dtype=np.int64) - 1) // 2).astype(np.uint32)
    parent[0] = NONE
    return parent


def raw_load(eng, topics, recv=True, sent=True):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    r = np.full(eng.n_peers, FILL, dtype=np.uint64)
    s = np.full(eng.n_peers, FILL, dtype=np.uint64)
    rc = eng._L.ps_peer_load(eng._h, t.ctypes.data_as(U32P), t.size, r.ctypes.data_as(U64P) if recv else None,
                             s.ctypes.data_as(U64P) if sent else None)
    return rc, r, s


def raw_track(eng, topics):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    return eng._L.ps_load_track(eng._h, t.ctypes.data_as(U32P), t.size)


def raw_take(eng):
    r = np.full(eng.n_peers, FILL, dtype=np.uint64)
    s = np.full(eng.n_peers, FILL, dtype=np.uint64)
    nw = C.c_uint64(0xCCCC)
    rc = eng._L.ps_load_take(eng._h, r.ctypes.data_as(U64P), s.ctypes.data_as(U64P), C.byref(nw))
    return rc, r, s, nw.value


# ---- 1. width edges -----------------------------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("n_msgs", [1, 63, 64, 65, 129, 1000, 4095, 4096, 4097, 8300])
def test_width_edges(n_msgs, rows, monkeypatch):
    """Rows of 1 to 130 words over one tree of 300 peers, ~10 % masked; under
    the seam every full row is counted word by word, the last word partly
    filled at 65, 129 and 4097 messages."""
    seam(monkeypatch, rows)
    n, root, parent, live = one_topic(n_msgs, n_msgs)
    want = LR.topic_load(n, root, live, n_msgs, parent=parent)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.publish(np.zeros(n_msgs))
        st = eng.run()
        got = eng.peer_load([0])
        same(got, want[:2], f"n_msgs {n_msgs}")
        assert got[0].sum() == st.deliveries == want[2]
        assert got[0][root] == 0 and got[1][root] > 0


# ---- 2. strip edges -----------------------------------------------------------------

def strip_masks(n_nodes, per):
    """Live masks by name over heap_tree(n_nodes + 1), `per` nodes to a strip:
    the first and the last non-root node, either side of the first strip
    boundary, an interior subtree, everything but the root's children."""
    n = n_nodes + 1
    out = {"none": []}
    out["first"] = [1]
    out["last"] = [n - 1]
    if n_nodes > per:
        out["before_boundary"] = [per]      # node per: the first strip's last
        out["after_boundary"] = [per + 1]   # the second strip's first
    if n > 8:
        out["interior"] = [3]
    out["all_but_roots_children"] = list(range(3, n))
    return out


@pytest.mark.parametrize("n_nodes,n_msgs", [(2048, 1), (2049, 1), (2050, 1), (15, 8300), (16, 8300), (17, 8300), (32, 8300),
                                            (33, 8300)])
def test_strip_edges(n_nodes, n_msgs):
    """One-word rows go 2,048 to a strip, 130-word rows 15: node counts at a
    strip's end, one and two past it, with the masked node at the strip's
    edges.  One engine per size, one run per mask."""
    n = n_nodes + 1
    per = 2048 if n_msgs == 1 else 16384 // (130 * 8)
    parent = heap_tree(n)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        assert np.array_equal(eng.graph(PE.G_NODE_PEER), np.arange(n))  # a peer id names a node
        for name, dead in strip_masks(n_nodes, per).items():
            live = np.ones(n, dtype=np.uint8)
            live[dead] = 0
            eng.set_live(live)
            eng.publish(np.zeros(n_msgs))
            st = eng.run()
            want = LR.topic_load(n, 0, live, n_msgs, parent=parent)
            got = eng.peer_load([0])
            same(got, want[:2], f"{n_nodes} nodes, mask {name}")
            assert got[0].sum() == st.deliveries == want[2], name


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
    want = LR.window_load(n, live, [(root, int((topics == t).sum()), parent, None) for t in (0, 1)])
    with PE.Engine(n, 2, **kw) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        eng.publish(topics, starts)
        st = eng.run()
        assert st.windows == 1
        got = eng.peer_load([1, 0])
        same(got, want[:2], kind)
        assert got[0].sum() == st.deliveries == want[2]
        one = eng.peer_load([1])
        same(one, LR.topic_load(n, root, live, int((topics == 1).sum()), parent=parent)[:2], kind + " topic 1")


# ---- 4. meshes ----------------------------------------------------------------------

@pytest.mark.parametrize("paced,n_msgs", [(False, 70), (True, 70), (True, 8300)])
def test_mesh(paced, n_msgs):
    """Two parents per node.  One start round: mask rows, partial where a
    parent is masked.  Several: the arrival-order table (kDrainGather), every
    row counted by the wave."""
    rng = np.random.default_rng(41 + paced)
    n, root = 400, 5
    rp, cl = random_mesh2(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    starts = rng.integers(0, 4, size=n_msgs) if paced else None
    want = LR.topic_load(n, root, live, n_msgs, csr=(rp, cl))
    with PE.Engine(n, 1) as eng:
        eng.set_children(0, root, rp, cl)
        eng.set_live(live)
        eng.publish(np.zeros(n_msgs), starts)
        st = eng.run()
        assert st.windows == 1
        got = eng.peer_load([0])
        same(got, want[:2], f"mesh paced {paced}")
        assert got[0].sum() == st.deliveries == want[2]
        if not paced:
            # a mesh node forwards once: what is written to live children arrives or is a duplicate
            assert LR.sent_live(n, root, live, n_msgs, csr=(rp, cl)).sum() == st.deliveries + st.duplicates


# ---- 5. several topics sharing peers ------------------------------------------------

def shared_topics():
    """Four topics over 400 peers of which 40 are in none: a 1-word topic, a
    130-word one rooted at a leaf of the first, an idle one, and one created
    but empty."""
    rng = np.random.default_rng(55)
    n = 400
    free = np.arange(360, 400)
    p0 = random_tree(rng, 360, 3)
    p0 = np.concatenate([p0, np.full(40, NONE, dtype=np.uint32)])
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[3] = 1
    reached = LR.topic_load(n, 3, live, 1, parent=p0)[0] > 0
    leaves = np.setdiff1d(np.arange(360), np.append(p0[p0 != NONE], 3))
    leaf = int(leaves[reached[leaves]][0])  # a leaf of topic 0 that its messages reach
    sub =np.sort(rng.choice(np.setdiff1d(np.arange(360), [leaf]), 200, replace=False))
    order = np.concatenate([[leaf], rng.permutation(sub)])
    p1 = np.full(n, NONE, dtype=np.uint32)
    for i in range(1, order.size):
        p1[order[i]] = order[rng.integers(0, i)]
    return n, free, (3, p0), (leaf, p1), live


@pytest.mark.parametrize("order", [[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [1], [0], [2, 3], [0, 2], []])
def test_several_topics(order):
    n, free, (r0, p0), (r1, p1), live = shared_topics()
    msgs = np.concatenate([np.full(10, 0), np.full(8300, 1)]).astype(np.uint32)
    per = {0: LR.topic_load(n, r0, live, 10, parent=p0), 1: LR.topic_load(n, r1, live, 8300, parent=p1)}
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
                want = add(want, tuple(x.astype(np.uint64) for x in per[t][:2]))
        got = eng.peer_load(order)
        same(got, want, str(order))
        assert not got[0][free].any() and not got[1][free].any()  # peers in no topic
        if {0, 1} <= set(order):
            assert got[0].sum() == st.deliveries == per[0][2] + per[1][2]
        if 1 in order:  # topic 1's root is a leaf of topic 0: it receives there alone, and sends here alone
            assert got[0][r1] == (10 if 0 in order else 0) and per[0][0][r1] == 10 and per[0][1][r1] == 0
            assert got[1][r1] == per[1][1][r1] >= 8300


# ---- 6. stale rows ------------------------------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
def test_stale_rows(rows, monkeypatch):
    """Two runs, a subtree cut in the second: the second window's answer holds
    nothing of the first window's bits below the cut."""
    seam(monkeypatch, rows)
    rng = np.random.default_rng(66)
    n, root = 500, 2
    parent = random_tree(rng, n, root)
    kids = kids_of(parent)
    cut = max((p for p in kids if p != root), key=lambda p: len(under(kids, p)))
    assert len(under(kids, cut)) >= 5
    live = np.ones(n, dtype=np.uint8)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.publish(np.zeros(100))
        eng.run()
        same(eng.peer_load([0]), LR.topic_load(n, root, live, 100, parent=parent)[:2], "first run")
        live[cut] = 0
        eng.set_live(live)
        eng.publish(np.zeros(70))
        st = eng.run()
        want = LR.topic_load(n, root, live, 70, parent=parent)
        got = eng.peer_load([0])
        same(got, want[:2], "second run")
        assert got[0].sum() == st.deliveries
        assert not got[0][[cut] + sorted(under(kids, cut))].any()


# ---- 7. tracking against the blocking call -----------------------------------------

def test_tracking_windows_runs_and_takes():
    """msg_window = 64: a run of three windows, two more runs, takes between:
    the totals equal the sum of load_ref per window and of peer_load per
    single-window run."""
    n, root, parent, live = one_topic(0, 71)
    rng = np.random.default_rng(71)
    p1 = random_tree(rng, n, 9)

    def ref(c0, c1):
        return LR.window_load(n, live, [(root, c0, parent, None), (9, c1, p1, None)])

    with PE.Engine(n, 2, msg_window=64) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, 9, p1)
        eng.set_live(live)
        eng.load_track([1, 0])
        r, s, nw = eng.load_take()  # nothing has run
        assert nw == 0 and not r.any() and not s.any()
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
        # the last window alone, from the blocking call, while the totals stand
        same(eng.peer_load([0, 1]), ref(22, 0)[:2], "last window")
        # two more runs of one window each
        blocking = zeros(n)
        for c0, c1 in ((10, 3), (0, 64)):
            eng.publish(np.concatenate([np.zeros(c0), np.ones(c1)]).astype(np.uint32))
            st2 = eng.run()
            assert st2.windows == 1
            total += st2.deliveries
            want = add(want, ref(c0, c1)[:2])
            blocking = add(blocking, eng.peer_load([0, 1]))
        r, s, nw = eng.load_take()
        assert nw == 5
        same((r, s), want, "five windows")
        assert r.sum() == total == st.deliveries + int(blocking[0].sum())
        # a second take: zeros and no window
        r, s, nw = eng.load_take()
        assert nw == 0 and not r.any() and not s.any()
        # take, run, take: the new run alone, equal to the blocking call's answer
        eng.publish(np.zeros(40))
        st3 = eng.run()
        r, s, nw = eng.load_take()
        assert nw == 1 and r.sum() == st3.deliveries
        same((r, s), ref(40, 0)[:2], "the new run")
        same((r, s), eng.peer_load([1, 0]), "the new run, blocking")
        # setting again zeroes the totals
        eng.publish(np.zeros(5))
        eng.run()
        eng.load_track([0])
        r, s, nw = eng.load_take()
        assert nw == 0 and not r.any() and not s.any()
        # a subset tracked: topic 1's traffic is not counted
        eng.publish(np.concatenate([np.zeros(7), np.ones(9)]).astype(np.uint32))
        eng.run()
        r, s, nw = eng.load_take()
        assert nw == 1
        same((r, s), ref(7, 0)[:2], "topic 0 alone")


def tree_window(ot, n, k):
    """k messages over oracle.Tree ot as the engine runs them: (recv, sent,
    deliveries) summed, a window per tree the messages met (a message that
    repairs the tree runs alone, the rest over the repaired tree)."""
    recv = np.zeros(n, dtype=np.int64)
    sent = np.zeros(n, dtype=np.int64)
    left = k
    while left:
        par = ot.parents()
        hop = ot.message()
        c = 1 if not np.array_equal(ot.parents(), par) else left
        for _ in range(c - 1):
            assert np.array_equal(ot.message(), hop)
        R = GC.reference(n, [(ot.root, par)], np.ones(n, dtype=np.uint8))["topics"][0]
        got = hop != 0xFF
        got[ot.root] = False
        assert not got[R["depth_of"] < 0].any()
        recv += c * got
        sent += c * got * R["n_child"]
        sent[ot.root] += c * R["n_child"][ot.root]
        left -= c
    return recv, sent, int(recv.sum())


def test_tracking_a_run_split_by_a_drop():
    """An interior peer dropped: topic 0's first message runs alone over the
    old tree, the rest over the repaired one (a rebuilt node space between
    two windows of one run); the totals are in peer space."""
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
        eng.load_track([0, 1])
        eng.publish(topics)
        st = eng.run()
        assert st.windows >= 2
        w0, w1 = tree_window(ots[0], n, 5), tree_window(ots[1], n, 5)
        r, s, nw = eng.load_take()
        assert nw == st.windows
        same((r, s), add(w0[:2], w1[:2]), "drop")
        assert r.sum() == st.deliveries
        # the dropped host carries nothing in topic 0; it still stands in topic 1
        assert w0[0][dead] == 0 and w0[1][dead] == 0 and r[dead] == w1[0][dead] == 5


# ---- 8. churn -----------------------------------------------------------------------

@pytest.mark.parametrize("gpu_build", [True, False])
def test_churn(gpu_build):
    """Joins, leaves and drops between runs, the node space rebuilt on the GPU
    or on the host every batch: the totals over all batches, and each batch's
    blocking answer, against the oracle's trees."""
    rng = np.random.default_rng(17)
    n, seed = 3000, 4
    eng = make_engine(n, gpu_build, seed=seed)
    ot = O.Tree(n, 0, 2, 5, PE.Engine.topic_seed(seed, 0))
    eng.topic_create(0, 0, 2, 5)
    eng.join(0, np.arange(1, n, 2))
    ot.join_all(range(1, n, 2))
    members = set(range(1, n, 2))
    eng.load_track([0])
    want = (np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64))
    windows = deliveries = built = 0
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
            w = tree_window(ot, n, k)
            assert run.deliveries == w[2], step
            want = add(want, w[:2])
            windows += run.windows
            deliveries += run.deliveries
            assert np.array_equal(eng.parents(0), ot.parents()), step
            built = assert_builds(eng, gpu_build, built)
        r, s, nw = eng.load_take()
        assert nw == windows
        same((r, s), want, f"churn gpu_build {gpu_build}")
        assert r.sum() == deliveries


# ---- 9. pipelined -------------------------------------------------------------------

def tracked_blocking(e, batches):
    stats = []
    for b in batches:
        e.publish(b)
        stats.append(e.run())
    return e.load_take(), stats


def tracked_pipelined(e, batches):
    stats = []
    for i, b in enumerate(batches):
        e.publish(b)
        e.run_async()
        if i:
            stats.append(e.wait())
    rc, _, _, nw = raw_take(e)  # a run in flight: refused, nothing changes
    assert rc == E_STATE and nw == 0xCCCC
    stats.append(e.wait())
    return e.load_take(), stats


@pytest.mark.parametrize("shape", ["deep", "twin"])
def test_pipelined(shape):
    """Six run_async over a shape whose windows overlap their predecessors
    (deep: alternating row sets and overlapped prefixes; twin: whole windows
    side by side), then six waits and one take: the totals of the same six
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
    order = np.arange(len(wl.topics), dtype=np.uint32)

    def make():
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=64, plan=plan)
        WL.build_engine_topics(e, wl)
        e.set_live(live)
        e.load_track(order)
        return e

    with make() as e:
        (r0, s0, nw0), st0 = tracked_blocking(e, batches)
    with make() as e:
        (r1, s1, nw1), st1 = tracked_pipelined(e, batches)
        over = e.overlapped_windows()
    print("pipelined", shape, "overlapped", over)
    assert over > 0
    assert nw0 == nw1 == sum(s.windows for s in st0) == 12
    same((r1, s1), (r0, s0), shape)
    assert r1.sum() == sum(s.deliveries for s in st1) == sum(s.deliveries for s in st0)
    # the root of a topic receives nothing in it; every reached peer sends to its children
    assert s1.sum() >= r1.sum() > 0


# ---- 10. with a sink ----------------------------------------------------------------

def test_with_a_sink():
    """A topics sink and tracking at once: both answers as with each alone."""
    n, root, parent, live = one_topic(0, 91)
    rng = np.random.default_rng(91)
    msgs = [rng.integers(0, 2, size=150).astype(np.uint32), np.zeros(70, dtype=np.uint32)]

    def go(sink, track):
        with PE.Engine(n, 2, msg_window=64) as e:
            e.set_tree(0, root, parent)
            e.set_tree(1, root, parent)
            e.set_live(live)
            if sink:
                e.sink_set_topics([0, 1])
            if track:
                e.load_track([0, 1])
            views = []
            for m in msgs:
                e.publish(m)
                e.run()
                if sink:
                    views.append(e.sink_take_topics())
            return views, e.load_take() if track else None

    both, alone_sink, alone_track = go(True, True), go(True, False), go(False, True)
    same(both[1][:2], alone_track[1][:2], "tracking beside a sink")
    assert both[1][2] == alone_track[1][2] == sum(v["n_windows"] for v in both[0])
    for a, b in zip(both[0], alone_sink[0]):
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


# ---- 11. the rules ------------------------------------------------------------------

def test_rules():
    rng = np.random.default_rng(82)
    n, root = 300, 1
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        # before any run
        rc, r, s = raw_load(eng, [0])
        assert rc == E_NOTREADY and (r == FILL).all() and (s == FILL).all()
        rc, r, s, nw = raw_take(eng)
        assert rc == E_NOTREADY and nw == 0xCCCC and (r == FILL).all()
        eng.publish(np.zeros(10))
        eng.run()
        # the arguments
        assert raw_load(eng, [0, 0])[0] == E_INVAL  # a topic named twice
        rc, r, s = raw_load(eng, [0, 2])
        assert rc == E_RANGE and (r == FILL).all() and (s == FILL).all()  # nothing written
        assert raw_load(eng, [0], recv=False, sent=False)[0] == E_INVAL
        assert eng._L.ps_peer_load(eng._h, None, 1, r.ctypes.data_as(U64P), None) == E_INVAL
        # either output alone; no topic: zeros
        full = eng.peer_load([0])
        rc, r, s = raw_load(eng, [0], sent=False)
        assert rc == 0 and np.array_equal(r, full[0]) and (s == FILL).all()
        rc, r, s = raw_load(eng, [0], recv=False)
        assert rc == 0 and np.array_equal(s, full[1]) and (r == FILL).all()
        rc, r, s = raw_load(eng, [])
        assert rc == 0 and not r.any() and not s.any()
        assert not eng.peer_load([1])[0].any()  # a topic with no message in the window
        # tracking: a refused call leaves the previous tracking
        eng.load_track([0])
        assert raw_track(eng, [1, 1]) == E_INVAL and raw_track(eng, [0, 5]) == E_RANGE
        assert eng._L.ps_load_track(eng._h, None, 2) == E_INVAL
        eng.publish(np.zeros(3))
        eng.run()
        r, s, nw = eng.load_take()
        assert nw == 1 and r.sum() == 3 * (n - 1)
        assert eng._L.ps_load_take(eng._h, None, None, None) == E_INVAL
        # NULL arrays are allowed: the take still clears
        eng.publish(np.zeros(2))
        eng.run()
        nwc = C.c_uint64()
        assert eng._L.ps_load_take(eng._h, None, None, C.byref(nwc)) == 0 and nwc.value == 1
        assert eng.load_take()[2] == 0
        # a run in flight
        eng.publish(np.zeros(4))
        eng.run_async()
        assert raw_track(eng, [1]) == E_STATE
        rc, r, s, nw = raw_take(eng)
        assert rc == E_STATE and nw == 0xCCCC and (r == FILL).all() and (s == FILL).all()
        eng.wait()
        r, s, nw = eng.load_take()
        assert nw == 1 and r.sum() == 4 * (n - 1)
        # clearing, then taking
        eng.load_track([])
        rc, _, _, nw = raw_take(eng)
        assert rc == E_NOTREADY and nw == 0xCCCC
        eng.publish(np.zeros(1))
        eng.run()  # nothing is tracked: the run is as ever
        assert eng.peer_load([0])[0].sum() == n - 1


def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(3)]
    try:
        # an engine that is tracking takes no ranks
        engines[2].load_track([0])
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
            assert raw_load(e, [0])[0] == E_STATE
            assert raw_take(e)[0] == E_NOTREADY
    finally:
        for e in engines:
            e.close()
