"""GPU: deliveries by hop per topic (ps_topic_hops, ps_hops_track /
ps_hops_take) -- per tree topic and BFS level, the nodes, the
nodes the window reached and the messages they hold, for the last window or
accumulated behind every window of every run.

Every comparison is bit-exact, all three arrays, against tests/hops_ref.py
(oracle.disseminate's hops, or oracle.Tree under churn, and graph_check's
depths).  Where every topic is named, deliv.sum() equals the run's
ps_stats.deliveries; in a window of one start round the column sums equal
ps_stats.deliveries_per_round.  The seam (PSAMD_AB=1 PSAMD_LOAD_COUNT=rows)
makes the kernel count full rows from their words, the path a healthy tree's
all-or-nothing rows never take otherwise."""
import ctypes as C
import threading

import numpy as np
import pytest

import graph_check as GC
import hops_ref as HR
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
NAMES = ("nodes", "reached", "deliv")


# ---- helpers ------------------------------------------------------------------------

def same(got, want, what=""):
    """(nodes, reached, deliv) against the same, uint64 [n, COLS], bit for bit."""
    for name, g, w in zip(NAMES, got, want):
        w = np.asarray(w).astype(np.uint64).reshape(-1, COLS)
        assert g.dtype == np.uint64 and g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what} {name}: {len(bad)} bins differ, first (row, hop) {bad[:6].tolist()} got "
                                 f"{[int(g[tuple(b)]) for b in bad[:6]]} want {[int(w[tuple(b)]) for b in bad[:6]]}")


def ref(n, live, topics):
    """hops_ref.window_hops as (the three arrays, deliveries)."""
    w = HR.window_hops(n, live, topics)
    return w[:3], w[3]


def zeros(rows):
    return tuple(np.zeros((rows, COLS), dtype=np.uint64) for _ in range(3))


def add(a, b):
    return tuple(x + np.asarray(y).astype(np.uint64).reshape(x.shape) for x, y in zip(a, b))


def against_stats(got, st, single_start=True):
    """All topics named: the row sums are the run's deliveries; a window of one
    start round delivers hop h in round h."""
    deliv = got[2]
    assert deliv.sum() == st.deliveries
    assert not got[0][:, 0].any() and not got[1][:, 0].any() and not deliv[:, 0].any()  # the root is no recipient
    assert (got[1] <= got[0]).all()
    if single_start and st.windows == 1:
        per_round = np.array(list(st.deliveries_per_round), dtype=np.uint64)
        assert np.array_equal(deliv.sum(axis=0), per_round), (deliv.sum(axis=0)[:12], per_round[:12])


def raw_hops(eng, topics, which=(True, True, True)):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    a = [np.full((max(t.size, 1), COLS), FILL, dtype=np.uint64) for _ in range(3)]
    rc = eng._L.ps_topic_hops(eng._h, t.ctypes.data_as(U32P), t.size,
                              *(x.ctypes.data_as(U64P) if w else None for x, w in zip(a, which)))
    return rc, a


def raw_track(eng, topics):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    return eng._L.ps_hops_track(eng._h, t.ctypes.data_as(U32P), t.size)


def raw_take(eng, rows):
    a = [np.full((rows, COLS), FILL, dtype=np.uint64) for _ in range(3)]
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    rc = eng._L.ps_hops_take(eng._h, *(x.ctypes.data_as(U64P) for x in a), C.byref(nw), C.byref(nsk))
    return rc, a, nw.value, nsk.value


def star(n):
    parent = np.zeros(n, dtype=np.uint32)
    parent[0] = NONE
    return parent


def path(n):
    parent = np.arange(-1, n - 1).astype(np.uint32)
    parent[0] = NONE
    return parent


# ---- 1. width edges -----------------------------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("n_msgs", [1, 64, 65, 4096, 4097, 8300])
def test_width_edges(n_msgs, rows, monkeypatch):
    """Rows of 1 to 130 words over one tree of 300 peers, ~10 % masked; under
    the seam every full row is counted word by word."""
    seam(monkeypatch, rows)
    n, root, parent, live = one_topic(n_msgs, n_msgs)
    want, tot = ref(n, live, [(root, n_msgs, parent)])
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.publish(np.zeros(n_msgs))
        st = eng.run()
        got = eng.topic_hops([0])
        same(got, want, f"n_msgs {n_msgs}")
        assert st.deliveries == tot
        against_stats(got, st)


# ---- 2. strips against levels -------------------------------------------------------

def level_mask(parent):
    """The first and the last node of the widest level (peer ids name nodes)."""
    n = parent.size
    d = GC.reference(n, [(0, parent)], np.ones(n, dtype=np.uint8))["topics"][0]["depth_of"]
    lvl = int(np.argmax(np.bincount(d[1:])))
    at = np.nonzero(d == lvl)[0]
    return sorted({int(at[0]), int(at[-1])})


def run_masks(parent, n_msgs, per):
    """One engine, one run per mask: strip_masks' dead sets and one that kills
    the first and the last node of a level."""
    n = parent.size
    masks = strip_masks(n - 1, per)
    masks["level_ends"] = level_mask(parent)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        assert np.array_equal(eng.graph(PE.G_NODE_PEER), np.arange(n))  # a peer id names a node
        for name, dead in masks.items():
            live = np.ones(n, dtype=np.uint8)
            live[dead] = 0
            eng.set_live(live)
            eng.publish(np.zeros(n_msgs))
            st = eng.run()
            want, tot = ref(n, live, [(0, n_msgs, parent)])
            got = eng.topic_hops([0])
            same(got, want, f"{n} peers, mask {name}")
            assert st.deliveries == tot, name
            against_stats(got, st)


ONE_WORD = {"heap2049": lambda: heap_tree(2049), "heap2050": lambda: heap_tree(2050), "heap4097": lambda: heap_tree(4097),
            "heap4100": lambda: heap_tree(4100), "star3000": lambda: star(3001), "path40": lambda: path(40)}


@pytest.mark.parametrize("shape", list(ONE_WORD))
def test_strips_against_levels_one_word_rows(shape):
    """One message: one-word rows, 2,048 to a strip.  Heap trees whose last
    levels end at, one past and far past a strip's end; a star whose one level
    spans two strips; a path whose one strip spans 39 levels."""
    run_masks(ONE_WORD[shape](), 1, 2048)


@pytest.mark.parametrize("shape", ["heap15", "heap16", "heap17", "heap32", "heap33", "heap64", "path40"])
def test_strips_against_levels_wide_rows(shape):
    """8,300 messages: 130-word rows, 15 to a strip, so levels of 8, 16 and 32
    nodes start and end inside strips."""
    parent = path(40) if shape == "path40" else heap_tree(int(shape[4:]) + 1)
    run_masks(parent, 8300, 16384 // (130 * 8))


# ---- 3. start groups ----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["group_major", "group_major_rows", "aligned", "aligned_rows", "compact", "no_lazy_seen"])
def test_start_groups(kind, monkeypatch):
    """publish_at with start rounds 0..3: the hop columns do not move with the
    start round, whatever the row layout."""
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
    want, tot = ref(n, live, [(root, c[1], parent), (root, c[0], parent)])
    with PE.Engine(n, 2, **kw) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        eng.publish(topics, starts)
        st = eng.run()
        assert st.windows == 1 and st.deliveries == tot
        got = eng.topic_hops([1, 0])
        same(got, want, kind)
        against_stats(got, st, single_start=False)
        same(eng.topic_hops([1]), tuple(w[:1] for w in want), kind + " topic 1")


# ---- 4. several topics sharing peers ------------------------------------------------

@pytest.mark.parametrize("order", [[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [1], [0], [2, 3], [0, 2]])
def test_several_topics(order):
    """A 1-word topic, a 130-word one rooted at a leaf of the first, an idle
    one and one created but empty: rows in request order, the idle ones zero
    in nodes as well, a single topic's row as in the full request."""
    n, free, (r0, p0), (r1, p1), live = shared_topics()
    msgs = np.concatenate([np.full(10, 0), np.full(8300, 1)]).astype(np.uint32)
    per = {0: (r0, 10, p0), 1: (r1, 8300, p1), 2: (r0, 0, p0), 3: (7, 0, np.full(n, NONE, dtype=np.uint32))}
    with PE.Engine(n, 4) as eng:
        eng.set_tree(0, r0, p0)
        eng.set_tree(1, r1, p1)
        eng.set_tree(2, r0, p0)
        eng.topic_create(3, 7)
        eng.set_live(live)
        eng.publish(msgs)
        st = eng.run()
        want, _ = ref(n, live, [per[t] for t in order])
        got = eng.topic_hops(order)
        same(got, want, str(order))
        for i, t in enumerate(order):
            if t >= 2:
                assert not any(a[i].any() for a in got)
            else:
                same(eng.topic_hops([t]), tuple(a[i:i + 1] for a in got), f"topic {t} alone")
        if {0, 1} <= set(order):
            against_stats(got, st)


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
        eng.hops_track([0])
        eng.publish(np.concatenate([np.zeros(70), np.ones(70)]).astype(np.uint32))
        st = eng.run()
        assert st.windows == 1 and st.expand_mode == PE.MODE_COMPACT  # the tree runs beside the mesh: compaction path
        for named in ([1], [0, 1], [1, 0]):
            rc, a = raw_hops(eng, named)
            assert rc == E_STATE and all((x == FILL).all() for x in a), named
        want, tot = ref(n, live, [(root, 70, parent)])
        got = eng.topic_hops([0])
        same(got, want, "a tree beside a mesh")
        assert 0 < got[2].sum() == tot < st.deliveries
        # the tracked tree becomes a mesh: that window adds nothing and is counted
        eng.set_children(0, root, rp, cl)
        eng.publish(np.zeros(5))
        st2 = eng.run()
        assert st2.deliveries > 0
        assert raw_hops(eng, [0])[0] == E_STATE
        t = eng.hops_take()
        same(t[:3], want, "before the topic became a mesh")
        assert t[3:] == (2, 1)
        # ... and a tree again
        eng.set_tree(0, root, parent)
        eng.publish(np.zeros(3))
        eng.run()
        t = eng.hops_take()
        same(t[:3], ref(n, live, [(root, 3, parent)])[0], "a tree again")
        assert t[3:] == (1, 0)


# ---- 6. stale rows ------------------------------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
def test_stale_rows(rows, monkeypatch):
    """A second run that publishes to one topic of two, below a cut subtree:
    nothing of the first run's rows is counted."""
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
        eng.publish(np.concatenate([np.zeros(100), np.ones(30)]).astype(np.uint32))
        st = eng.run()
        got = eng.topic_hops([0, 1])
        same(got, ref(n, live, [(root, 100, parent), (root, 30, parent)])[0], "first run")
        against_stats(got, st)
        live[cut] = 0
        eng.set_live(live)
        eng.publish(np.zeros(70))
        st = eng.run()
        want, tot = ref(n, live, [(root, 70, parent), (root, 0, parent)])
        got = eng.topic_hops([0, 1])
        same(got, want, "second run")
        assert not got[0][1].any() and st.deliveries == tot == 70 * (n - 2 - len(under(kids, cut)))
        against_stats(got, st)


# ---- 7. the depth clamp -------------------------------------------------------------

def test_depth_clamp():
    """A path of 300 peers: levels 255 .. 299 share the last column, and the
    row sums stay exact."""
    n = 300
    parent = path(n)
    live = np.ones(n, dtype=np.uint8)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        eng.publish(np.zeros(3))
        st = eng.run()
        assert st.deliveries == 3 * 299
        got = eng.topic_hops([0])
        same(got, ref(n, live, [(0, 3, parent)])[0], "path 300")
        assert got[0][0, 255] == 45 and got[2][0, 255] == 135 and got[2].sum() == st.deliveries
        live[280] = 0
        eng.set_live(live)
        eng.publish(np.zeros(3))
        st = eng.run()
        got = eng.topic_hops([0])
        same(got, ref(n, live, [(0, 3, parent)])[0], "path 300, cut at 280")
        assert got[1][0, 255] == 25 and got[2].sum() == st.deliveries == 3 * 279


# ---- 8. tracking against the blocking call -----------------------------------------

def test_tracking_windows_runs_and_takes():
    """msg_window = 64: a run of three windows, two more runs, takes between:
    the totals equal the sum of hops_ref per window and of topic_hops per
    single-window run."""
    n, root, parent, live = one_topic(0, 71)
    rng = np.random.default_rng(71)
    p1 = random_tree(rng, n, 9)

    def want(c0, c1):  # request order [1, 0]
        return ref(n, live, [(9, c1, p1), (root, c0, parent)])

    with PE.Engine(n, 2, msg_window=64) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, 9, p1)
        eng.set_live(live)
        eng.hops_track([1, 0])
        t = eng.hops_take()  # nothing has run
        assert t[3:] == (0, 0) and not any(a.any() for a in t[:3]) and t[0].shape == (2, COLS)
        # 150 + 70 messages: windows of (64, 64), (64, 6), (22, 0)
        msgs = rng.permutation(np.concatenate([np.zeros(150), np.ones(70)])).astype(np.uint32)
        eng.publish(msgs)
        st = eng.run()
        assert st.windows == 3
        total, deliveries = zeros(2), 0
        for c0, c1 in ((64, 64), (64, 6), (22, 0)):
            w, tot = want(c0, c1)
            total = add(total, w)
            deliveries += tot
        assert deliveries == st.deliveries
        same(eng.topic_hops([1, 0]), want(22, 0)[0], "last window")  # while the totals stand
        blocking = zeros(2)
        for c0, c1 in ((10, 3), (0, 64)):
            eng.publish(np.concatenate([np.zeros(c0), np.ones(c1)]).astype(np.uint32))
            st2 = eng.run()
            assert st2.windows == 1
            deliveries += st2.deliveries
            total = add(total, want(c0, c1)[0])
            b = eng.topic_hops([1, 0])
            against_stats(b, st2)
            blocking = add(blocking, b)
        t = eng.hops_take()
        assert t[3:] == (5, 0)
        same(t[:3], total, "five windows")
        assert t[2].sum() == deliveries == st.deliveries + int(blocking[2].sum())
        t = eng.hops_take()  # a second take: zeros and no window
        assert t[3:] == (0, 0) and not any(a.any() for a in t[:3])
        eng.publish(np.zeros(40))
        st3 = eng.run()
        t = eng.hops_take()
        assert t[3:] == (1, 0) and t[2].sum() == st3.deliveries
        same(t[:3], want(40, 0)[0], "the new run")
        same(t[:3], eng.topic_hops([1, 0]), "the new run, blocking")
        # setting again zeroes the totals; a subset tracked: topic 1 is not counted
        eng.publish(np.zeros(5))
        eng.run()
        eng.hops_track([0])
        t = eng.hops_take()
        assert t[3:] == (0, 0) and not any(a.any() for a in t[:3]) and t[0].shape == (1, COLS)
        eng.publish(np.concatenate([np.zeros(7), np.ones(9)]).astype(np.uint32))
        eng.run()
        t = eng.hops_take()
        assert t[3:] == (1, 0)
        same(t[:3], ref(n, live, [(root, 7, parent)])[0], "topic 0 alone")


def tree_window(ot, n, k, dropped=False):
    """k messages over oracle.Tree ot as the engine runs them: (nodes, reached,
    deliv) [COLS] summed, the windows, and the last window's three alone; a
    window per tree the messages met:
    the first message after a drop runs alone (it is lost below the failed
    edge, whether or not a repair then moves anybody), as does one that
    changes the tree; the rest run over the tree it left.  Every window adds
    its tree's nodes.  A delivered peer's hop is its depth in the tree the
    message met."""
    out = [np.zeros(COLS, dtype=np.int64) for _ in range(3)]
    last = None
    left, windows = k, 0
    while left:
        par = ot.parents()
        hop = ot.message()
        c = 1 if dropped or not np.array_equal(ot.parents(), par) else left
        dropped = False
        for _ in range(c - 1):
            assert np.array_equal(ot.message(), hop)
        d = GC.reference(n, [(ot.root, par)], np.ones(n, dtype=np.uint8))["topics"][0]["depth_of"]
        got = hop != 0xFF
        got[ot.root] = False
        assert (hop[got] == d[got]).all() and d.max() < 254
        member = d > 0
        reached = np.bincount(d[got], minlength=COLS)
        last = (np.bincount(d[member], minlength=COLS), reached, c * reached)
        for o, w in zip(out, last):
            o += w
        left -= c
        windows += 1
    return tuple(out), windows, last


def test_tracking_a_run_split_by_a_drop():
    """An interior peer dropped: topic 0's first message runs alone over the
    old tree, the rest over the repaired one (a rebuilt node space between two
    windows of one run); the totals are indexed by request position."""
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
        eng.hops_track([0, 1])
        eng.publish(topics)
        st = eng.run()
        assert st.windows >= 2
        (w0, k0, l0), (w1, k1, l1) = tree_window(ots[0], n, 5, dropped=True), tree_window(ots[1], n, 5)
        assert (k0, k1) == (2, 1)
        t = eng.hops_take()
        assert t[3:] == (st.windows, 0)
        same(t[:3], tuple(np.stack([a, b]) for a, b in zip(w0, w1)), "drop")
        assert t[2].sum() == st.deliveries
        # the blocking call answers for the last window: topic 0's four messages
        # over the repaired tree, topic 1's five in that same window
        same(eng.topic_hops([0, 1]), tuple(np.stack([a, b]) for a, b in zip(l0, l1)), "drop, last window")


# ---- 9. churn -----------------------------------------------------------------------

@pytest.mark.parametrize("gpu_build", [True, False])
def test_churn(gpu_build):
    """Joins, leaves and drops between runs, the node space rebuilt on the GPU
    or on the host every batch: the depth profile moves from window to window,
    and the totals over all batches, and the blocking answer for each batch's
    last window, follow the oracle's trees."""
    rng = np.random.default_rng(17)
    n, seed = 3000, 4
    eng = make_engine(n, gpu_build, seed=seed)
    ot = O.Tree(n, 0, 2, 5, PE.Engine.topic_seed(seed, 0))
    eng.topic_create(0, 0, 2, 5)
    eng.join(0, np.arange(1, n, 2))
    ot.join_all(range(1, n, 2))
    members = set(range(1, n, 2))
    eng.hops_track([0])
    want = zeros(1)
    windows = deliveries = built = 0
    profiles = set()
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
            w, kw, last = tree_window(ot, n, k, dropped=step % 3 == 1)
            assert run.deliveries == w[2].sum() and run.windows == kw, step
            want = add(want, w)
            windows += run.windows
            deliveries += run.deliveries
            blocking = eng.topic_hops([0])
            same(blocking, last, f"step {step}, the batch's last window")
            profiles.add(tuple(blocking[0][0, :40].tolist()))
            assert np.array_equal(eng.parents(0), ot.parents()), step
            built = assert_builds(eng, gpu_build, built)
        t = eng.hops_take()
        assert t[3:] == (windows, 0)
        same(t[:3], want, f"churn gpu_build {gpu_build}")
        assert t[2].sum() == deliveries
        assert len(profiles) > 1  # the depth profile changed between windows


# ---- 10. pipelined ------------------------------------------------------------------

def tracked_blocking(e, batches):
    stats = []
    for b in batches:
        e.publish(b)
        stats.append(e.run())
    return e.hops_take(), stats


def tracked_pipelined(e, batches, rows):
    stats = []
    for i, b in enumerate(batches):
        e.publish(b)
        e.run_async()
        if i:
            stats.append(e.wait())
    rc, a, nw, nsk = raw_take(e, rows)  # a run in flight: refused, nothing changes
    assert rc == E_STATE and nw == 0xCCCC and nsk == 0xDDDD and all((x == FILL).all() for x in a)
    stats.append(e.wait())
    return e.hops_take(), stats


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
        e.hops_track(order)
        return e

    with make() as e:
        t0, st0 = tracked_blocking(e, batches)
        last = e.topic_hops(order)
    with make() as e:
        t1, st1 = tracked_pipelined(e, batches, order.size)
        over = e.overlapped_windows()
        same(e.topic_hops(order), last, shape + " last window")
    print("pipelined", shape, "overlapped", over)
    assert over > 0
    assert t0[3] == t1[3] == sum(s.windows for s in st0) == 12 and t0[4] == t1[4] == 0
    same(t1[:3], t0[:3], shape)
    assert t1[2].sum() == sum(s.deliveries for s in st1) == sum(s.deliveries for s in st0) > 0
    assert (t1[1] <= t1[0]).all() and not t1[0][:, 0].any()
    if shape == "twin":  # all live: every node reached, every message delivered
        assert np.array_equal(t1[0], t1[1])


# ---- 11. beside a sink and load tracking --------------------------------------------

def test_with_a_sink_and_load_tracking():
    """A topics sink, load tracking and hop tracking at once: each answer as
    with that one alone."""
    n, root, parent, live = one_topic(0, 91)
    rng = np.random.default_rng(91)
    msgs = [rng.integers(0, 2, size=150).astype(np.uint32), np.zeros(70, dtype=np.uint32)]

    def go(sink, load, hops):
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
            views = []
            for m in msgs:
                e.publish(m)
                e.run()
                if sink:
                    views.append(e.sink_take_topics())
            return views, e.load_take() if load else None, e.hops_take() if hops else None

    all3, only_sink, only_load, only_hops = go(True, True, True), go(True, False, False), go(False, True, False), \
        go(False, False, True)
    same(all3[2][:3], only_hops[2][:3], "hops beside a sink and load tracking")
    assert all3[2][3:] == only_hops[2][3:] == (sum(v["n_windows"] for v in all3[0]), 0)
    assert all3[2][2].sum() == all3[1][0].sum() > 0  # deliveries by hop = deliveries by peer
    for a, b in zip(all3[1][:2], only_load[1][:2]):
        assert np.array_equal(a, b)
    assert all3[1][2] == only_load[1][2]
    for a, b in zip(all3[0], only_sink[0]):
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
        rc, a = raw_hops(eng, [0])
        assert rc == E_NOTREADY and all((x == FILL).all() for x in a)
        rc, a, nw, nsk = raw_take(eng, 1)
        assert rc == E_NOTREADY and nw == 0xCCCC and nsk == 0xDDDD and all((x == FILL).all() for x in a)
        eng.publish(np.zeros(10))
        eng.run()
        # the arguments
        assert raw_hops(eng, [0, 0])[0] == E_INVAL  # a topic named twice
        rc, a = raw_hops(eng, [0, 2])
        assert rc == E_RANGE and all((x == FILL).all() for x in a)  # nothing written
        assert raw_hops(eng, [0], which=(False, False, False))[0] == E_INVAL
        assert eng._L.ps_topic_hops(eng._h, None, 1, a[0].ctypes.data_as(U64P), None, None) == E_INVAL
        # each output alone; no topic: nothing written
        full = eng.topic_hops([0, 1])
        same(full, ref(n, live, [(root, 10, parent), (root, 0, parent)])[0], "full")
        for k in range(3):
            rc, a = raw_hops(eng, [0, 1], which=tuple(j == k for j in range(3)))
            assert rc == 0 and np.array_equal(a[k], full[k])
            assert all((a[j] == FILL).all() for j in range(3) if j != k)
        rc, a = raw_hops(eng, [])
        assert rc == 0 and all((x == FILL).all() for x in a)
        # tracking: a refused call leaves the previous tracking
        eng.hops_track([0])
        assert raw_track(eng, [1, 1]) == E_INVAL and raw_track(eng, [0, 5]) == E_RANGE
        assert eng._L.ps_hops_track(eng._h, None, 2) == E_INVAL
        eng.publish(np.zeros(3))
        eng.run()
        t = eng.hops_take()
        assert t[3:] == (1, 0) and t[2].sum() == 3 * (n - 1) and t[0].sum() == n - 1
        assert eng._L.ps_hops_take(eng._h, None, None, None, None, None) == E_INVAL
        # NULL arrays are allowed: the take still clears
        eng.publish(np.zeros(2))
        eng.run()
        nw, nsk = C.c_uint64(), C.c_uint64()
        assert eng._L.ps_hops_take(eng._h, None, None, None, C.byref(nw), C.byref(nsk)) == 0 and nw.value == 1
        assert eng.hops_take()[3] == 0
        # a run in flight
        eng.publish(np.zeros(4))
        eng.run_async()
        assert raw_track(eng, [1]) == E_STATE
        rc, a, nw, nsk = raw_take(eng, 1)
        assert rc == E_STATE and nw == 0xCCCC and all((x == FILL).all() for x in a)
        eng.wait()
        t = eng.hops_take()
        assert t[3:] == (1, 0) and t[2].sum() == 4 * (n - 1)
        # setting again and clearing zero the totals
        eng.publish(np.zeros(1))
        eng.run()
        eng.hops_track([1, 0])
        t = eng.hops_take()
        assert t[3:] == (0, 0) and not any(x.any() for x in t[:3])
        eng.hops_track([])
        rc, _, nw, _ = raw_take(eng, 1)
        assert rc == E_NOTREADY and nw == 0xCCCC
        eng.publish(np.zeros(1))
        eng.run()  # nothing is tracked: the run is as ever
        assert eng.topic_hops([0])[2].sum() == n - 1


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
        before = eng.topic_hops([0, 1])
        same(tuple(a[:1] for a in before), ref(n, live, [(0, 4, p0)])[0], "topic 0")
        assert before[2][1].sum() == 6 * (n - 1)
        eng.set_tree(0, 0, p1)  # over a parent array: the window's levels stay
        same(eng.topic_hops([0, 1]), before, "after set_tree over a parent array")
        eng.set_tree(1, 0, p1)  # over a join topic: its record starts afresh
        rc, a = raw_hops(eng, [0, 1])
        assert rc == E_STATE and all((x == FILL).all() for x in a)
        same(eng.topic_hops([0]), tuple(a[:1] for a in before), "the other topic alone")
        eng.publish(np.array([0] * 3 + [1] * 2, dtype=np.uint32))
        eng.run()
        same(eng.topic_hops([0, 1]), ref(n, live, [(0, 3, p1), (0, 2, p1)])[0], "after the next run")


def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(3)]
    try:
        # an engine that is tracking takes no ranks
        engines[2].hops_track([0])
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
            assert raw_hops(e, [0])[0] == E_STATE
            assert raw_take(e, 1)[0] == E_NOTREADY
    finally:
        for e in engines:
            e.close()
