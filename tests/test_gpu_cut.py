"""GPU: losses blamed on their cut points (ps_peer_cut, ps_cut_track /
ps_cut_take) -- per peer, over the named tree topics, what
its nodes missed, its cut points, the nodes behind them and the deliveries lost
at and behind them, for the last window or accumulated behind every window of
every run.

Every comparison is bit-exact, all four arrays, against tests/cut_ref.py
(oracle.disseminate's deliveries, or oracle.Tree under churn, added bottom-up
over graph_check's depths).  Every case asserts identity 1 (sum(missed) = the
possible deliveries minus the oracle's) and identity 2 (sum(lost) =
sum(missed): a tree row is a subset of its parent's row); the single-topic
cases assert identity 3 against Engine.peer_downstream.  The seam (PSAMD_AB=1
PSAMD_LOAD_COUNT=rows) makes the weights kernel count full rows from their
words."""
import ctypes as C
import threading

import numpy as np
import pytest

import cut_ref as CR
import downstream_ref as DR
import graph_check as GC
import hops_ref as HR
import load_ref as LR
import oracle as O
import psengine as PE
from psengine import workloads as WL
from test_gpu_churn import assert_builds, make_engine
from test_gpu_downstream import TOP_EDGE, fan_tree, path, star
from test_gpu_drain_batch import random_mesh2, random_tree
from test_gpu_drain_shared import one_topic
from test_gpu_drain_topics import kids_of, under
from test_gpu_load import heap_tree, seam, shared_topics
from test_gpu_sink import drop_engine, even_batches

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
FILL = 0xABABABABABABABAB
BLOCK = 256  # kDownBlock: the nodes of one work item
NAMES = ("missed", "cuts", "orphaned", "lost")


# ---- helpers ------------------------------------------------------------------------

def same(got, want, what=""):
    """(missed, cuts, orphaned, lost) against the same, uint64, bit for bit."""
    assert len(got) == len(want) == 4, what
    for name, g, w in zip(NAMES, got, want):
        w = np.asarray(w).astype(np.uint64)
        assert g.dtype == np.uint64 and g.shape == w.shape, (what, name)
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{what} {name}: {bad.size} peers differ, first {bad[:6]} got {g[bad[:6]]} "
                                 f"want {w[bad[:6]]}")


def add(a, b):
    return tuple(x + np.asarray(y).astype(np.uint64) for x, y in zip(a, b))


def zeros(n):
    return tuple(np.zeros(n, dtype=np.uint64) for _ in range(4))


def sums(got, possible, deliveries, what=""):
    """Identities 1 and 2."""
    assert int(got[0].sum()) == possible - deliveries, f"{what}: sum(missed) != possible - deliveries"
    assert int(got[3].sum()) == int(got[0].sum()), f"{what}: sum(lost) != sum(missed)"


def identity3(eng, t, c, got, what=""):
    """One named topic in a window of full or empty rows: each peer holds one
    node, so a peer with a cut point has exactly that one."""
    below, carried = eng.peer_downstream([t])
    at = np.nonzero(got[1])[0]
    assert (got[1][at] == 1).all(), what
    assert np.array_equal(got[3][at], np.uint64(c) * (1 + got[2][at])), f"{what}: lost != c * (1 + orphaned)"
    assert np.array_equal(got[2][at], below[at]), f"{what}: orphaned != below"
    assert not carried[at].any(), f"{what}: carried != 0 at a cut point"
    rest = np.setdiff1d(np.arange(got[1].size), at)
    assert not got[2][rest].any() and not got[3][rest].any(), what


def check_topic(eng, t, root, live, c, parent, st=None, what=""):
    """Topic t alone against the reference, with all three identities."""
    n = eng.n_peers
    want = CR.topic_cut(n, root, live, c, parent)
    got = eng.peer_cut([t])
    same(got, want[:4], what)
    sums(got, c * max(want[5] - 1, 0), want[4], what)
    if st is not None:
        assert st.deliveries == want[4], what
    identity3(eng, t, c, got, what)
    return got, want


def raw_cut(eng, topics, which=(True, True, True, True)):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    a = [np.full(eng.n_peers, FILL, dtype=np.uint64) for _ in range(4)]
    rc = eng._L.ps_peer_cut(eng._h, t.ctypes.data_as(U32P), t.size,
                            *(x.ctypes.data_as(U64P) if w else None for x, w in zip(a, which)))
    return rc, a


def raw_track(eng, topics):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    return eng._L.ps_cut_track(eng._h, t.ctypes.data_as(U32P), t.size)


def raw_take(eng):
    a = [np.full(eng.n_peers, FILL, dtype=np.uint64) for _ in range(4)]
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    rc = eng._L.ps_cut_take(eng._h, *(x.ctypes.data_as(U64P) for x in a), C.byref(nw), C.byref(nsk))
    return rc, a, nw.value, nsk.value


def untouched(a):
    return all((x == FILL).all() for x in a)


def levels_of(parent):
    """The peers of each BFS level of a tree rooted at 0 whose peer ids name its nodes."""
    n = parent.size
    d = GC.reference(n, [(0, parent)], np.ones(n, dtype=np.uint8))["topics"][0]["depth_of"]
    return [np.nonzero(d == l)[0] for l in range(int(d.max()) + 1)]


def run_dead(parent, n_msgs, dead_sets):
    """One engine over a tree rooted at 0 whose peer ids name its nodes, one
    run per dead set: everything against the reference."""
    n = parent.size
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        assert np.array_equal(eng.graph(PE.G_NODE_PEER), np.arange(n))  # a peer id names a node
        for name, dead in dead_sets.items():
            live = np.ones(n, dtype=np.uint8)
            live[list(dead)] = 0
            assert live[0]
            eng.set_live(live)
            eng.publish(np.zeros(n_msgs))
            st = eng.run()
            got, want = check_topic(eng, 0, 0, live, n_msgs, parent, st, f"{n} peers, dead {name}")
            if not len(dead):
                assert not any(x.any() for x in got)  # identity 4
            else:
                assert got[1].sum() >= 1


# ---- 1. row widths ------------------------------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("n_msgs", [1, 63, 64, 65, 4097, 8300])
def test_row_widths(n_msgs, rows, monkeypatch):
    """Rows of 1 to 130 words over one tree of 300 peers, ~10 % masked; under
    the seam every full row is counted word by word."""
    seam(monkeypatch, rows)
    n, root, parent, live = one_topic(n_msgs, n_msgs)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.publish(np.zeros(n_msgs))
        st = eng.run()
        got, want = check_topic(eng, 0, root, live, n_msgs, parent, st, f"n_msgs {n_msgs}")
        assert got[1].sum() > 1 and not got[0][root]
        assert not live[np.nonzero(got[1])[0]].any()  # a healthy tree is cut at dead peers only


# ---- 2. where the cut point sits ----------------------------------------------------

def test_where_the_cut_point_sits():
    """A heap tree of 255 (levels 0..7), 3 messages.  A deepest-level leaf is
    found by its parent's lane (no launch covers its level); a child of the
    root by level 0, whose stored k is 0; nested dead nodes count once."""
    parent = heap_tree(255)
    run_dead(parent, 3, {
        "none": [], "deepest_leaf": [254], "inner": [5], "roots_child": [1], "roots_children": [1, 2],
        "level_first": [63], "level_last": [126], "deepest_first": [127], "level_ends": [31, 62],
        "dead_under_dead": [5, 11], "dead_leaf_under_dead_parent": [62, 125], "three_deep": [1, 3, 7, 127],
        "siblings_and_a_nephew": [3, 4, 12],
    })


def test_closed_forms_on_a_path():
    n, c = 40, 3
    parent = path(n)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        for j in (1, 20, 38, 39):
            live = np.ones(n, dtype=np.uint8)
            live[j] = 0
            eng.set_live(live)
            eng.publish(np.zeros(c))
            eng.run()
            missed, cuts, orphaned, lost = eng.peer_cut([0])
            assert cuts.sum() == 1 and cuts[j] == 1 and orphaned[j] == n - 1 - j and lost[j] == c * (n - j)
            assert orphaned.sum() == orphaned[j] and lost.sum() == lost[j] == missed.sum()
            assert not missed[:j].any() and (missed[j:] == c).all()


# ---- 3. work-item, strip and block edges ------------------------------------------------

def edge_masks(parent, per=2048):
    """Dead sets at the first and the last node of every 256-node work item's
    edge of the levels wider than a block, of the first strip bound, and a
    pair that straddles two work items under one parent item."""
    n = parent.size
    out = {"none": []}
    for l, at in enumerate(levels_of(parent)):
        if at.size <= BLOCK:
            continue
        lo, hi = int(at[0]), int(at[-1])
        out[f"l{l}_first"] = [lo]
        out[f"l{l}_item_last"] = [lo + BLOCK - 1]
        out[f"l{l}_item_next"] = [lo + BLOCK] if lo + BLOCK <= hi else [hi]
        out[f"l{l}_straddle"] = [x for x in (lo + BLOCK - 1, lo + BLOCK) if x <= hi]
        out[f"l{l}_last"] = [hi]
    if n - 1 > per:
        out["strip_last"] = [per]
        out["strip_next"] = [per + 1]
    return out


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4100])
def test_work_item_and_strip_edges(n):
    """One message: one-word rows, 2,048 to a strip.  Heap trees whose last
    levels are cut into several work items: the parents of one item have
    their children in two."""
    parent = heap_tree(n)
    masks = edge_masks(parent)
    assert any(k.endswith("_straddle") for k in masks)
    run_dead(parent, 1, masks)


@pytest.mark.parametrize("shape", list(TOP_EDGE))
def test_block_edge_of_the_top_run(shape):
    """The shapes in which the first level wider than a block is the last one
    or the one before it, and a root with 256 / 257 children: the cut point
    at level top - 1, top and top + 1, at the level's first and last node."""
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
    assert len(masks) >= 3
    run_dead(parent, 1, masks)


# ---- 4. wide fan-out ----------------------------------------------------------------

def test_star_of_3000():
    """The root's wave walks 3,000 children, a lane each 64: dead children at
    index 0, 63, 64, 65 and 2,999, one at a time and together."""
    idx = [0, 63, 64, 65, 2999]
    masks = {f"child{i}": [1 + i] for i in idx}
    masks["all_five"] = [1 + i for i in idx]
    masks["none"] = []
    run_dead(star(3001), 1, masks)


@pytest.mark.parametrize("a,b", [(64, 65), (65, 64)])
def test_fan_out_64_and_65_at_an_inner_node(a, b):
    """Node 1 has a children (3 .. 2 + a), node 2 has b; each of those has one
    child: 64 children are walked by a lane, 65 by the wave."""
    first1, last1, first2, last2 = 3, 2 + a, 3 + a, 2 + a + b
    run_dead(fan_tree(a, b), 2, {
        "first_of_1": [first1], "last_of_1": [last1], "first_of_2": [first2], "last_of_2": [last2],
        "ends_of_both": [first1, last1, first2, last2],
        "every_child_of_1": list(range(first1, last1 + 1)), "every_child_of_2": list(range(first2, last2 + 1)),
        "every_child": list(range(first1, last2 + 1)), "none": [],
    })


# ---- 5. 130-word rows ---------------------------------------------------------------

@pytest.mark.parametrize("shape", ["heap15", "heap16", "heap17", "heap33", "heap64", "path40"])
def test_wide_rows(shape):
    """8,300 messages: 130-word rows, 15 to a strip; a level's first and last
    node masked, level by level."""
    parent = path(40) if shape == "path40" else heap_tree(int(shape[4:]))
    lv = levels_of(parent)
    pick = range(1, len(lv)) if shape != "path40" else (1, 15, 16, 39)
    masks = {f"l{l}_ends": sorted({int(lv[l][0]), int(lv[l][-1])}) for l in pick}
    masks["none"] = []
    run_dead(parent, 8300, masks)


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
    want = CR.window_cut(n, live, [(root, c[1], parent), (root, c[0], parent)])
    with PE.Engine(n, 2, **kw) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        eng.publish(topics, starts)
        st = eng.run()
        assert st.windows == 1
        got = eng.peer_cut([1, 0])
        same(got, want[:4], kind)
        sums(got, want[5], want[4], kind)
        assert st.deliveries == want[4]
        check_topic(eng, 1, root, live, c[1], parent, None, kind + " topic 1")


# ---- 7. several topics sharing peers ------------------------------------------------

@pytest.mark.parametrize("order", [[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [1], [0], [2, 3], [0, 2], []])
def test_several_topics(order):
    """A 1-word topic, a 130-word one rooted at a leaf of the first, an idle
    one and one created but empty, named in several orders and subsets: the
    sums in peer space, nothing from the idle ones, nothing at peers in no
    topic."""
    n, free, (r0, p0), (r1, p1), live = shared_topics()
    msgs = np.concatenate([np.full(10, 0), np.full(8300, 1)]).astype(np.uint32)
    per = {0: CR.topic_cut(n, r0, live, 10, p0), 1: CR.topic_cut(n, r1, live, 8300, p1)}
    both = np.nonzero((per[0][1] > 0) & (per[1][1] > 0))[0]
    assert both.size  # a peer that is a cut point in both topics: its sums add
    with PE.Engine(n, 4) as eng:
        eng.set_tree(0, r0, p0)
        eng.set_tree(1, r1, p1)
        eng.set_tree(2, r0, p0)
        eng.topic_create(3, 7)
        eng.set_live(live)
        eng.publish(msgs)
        st = eng.run()
        want, possible, deliveries = zeros(n), 0, 0
        for t in order:
            if t in per:
                want = add(want, per[t][:4])
                possible += (10, 8300)[t] * (per[t][5] - 1)
                deliveries += per[t][4]
        got = eng.peer_cut(order)
        same(got, want, str(order))
        sums(got, possible, deliveries, str(order))
        assert not any(x[free].any() for x in got)  # peers in no topic
        if {0, 1} <= set(order):
            assert st.deliveries == deliveries
            assert (got[1][both] == 2).all() and np.array_equal(got[3][both], (per[0][3] + per[1][3])[both].astype(np.uint64))
        for t in order:
            if t in per:
                check_topic(eng, t, (r0, r1)[t], live, (10, 8300)[t], (p0, p1)[t], None, f"topic {t} alone")


def test_a_cut_point_in_one_topic_full_in_another():
    """Peer x is dead: in topic 0 it is an inner node and a cut point; of
    topic 1 it is the root, which counts as full -- a dead root still
    forwards -- so topic 1 adds nothing at x."""
    n, x, c0, c1 = 127, 5, 4, 70
    p0 = heap_tree(n)
    perm = np.arange(n)  # topic 1: the same heap, relabelled so that x is its root
    perm[[0, x]] = [x, 0]
    p1 = np.full(n, NONE, dtype=np.uint32)
    for i in range(1, n):
        p1[perm[i]] = perm[(i - 1) // 2]
    live = np.ones(n, dtype=np.uint8)
    live[x] = 0
    a, b = CR.topic_cut(n, 0, live, c0, p0), CR.topic_cut(n, x, live, c1, p1)
    assert a[1][x] == 1 and a[3][x] == c0 * 31 and not any(v.any() for v in b[:4]) and b[4] == c1 * (n - 1)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, 0, p0)
        eng.set_tree(1, x, p1)
        eng.set_live(live)
        eng.publish(np.concatenate([np.zeros(c0), np.ones(c1)]).astype(np.uint32))
        st = eng.run()
        assert st.deliveries == a[4] + b[4]
        got = eng.peer_cut([0, 1])
        same(got, add(a[:4], b[:4]), "both")
        sums(got, c0 * (n - 1) + c1 * (n - 1), a[4] + b[4])
        assert got[1].sum() == 1 and got[1][x] == 1 and got[0][x] == c0
        one = eng.peer_cut([1])
        assert not any(v.any() for v in one)


# ---- 8. meshes ----------------------------------------------------------------------

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
        eng.cut_track([0])
        eng.publish(np.concatenate([np.zeros(70), np.ones(70)]).astype(np.uint32))
        st = eng.run()
        assert st.windows == 1 and st.expand_mode == PE.MODE_COMPACT  # the tree runs beside the mesh: compaction path
        for named in ([1], [0, 1], [1, 0]):
            rc, a = raw_cut(eng, named)
            assert rc == E_STATE and untouched(a), named
        got, want = check_topic(eng, 0, root, live, 70, parent, None, "a tree beside a mesh")
        assert 0 < want[4] < st.deliveries and got[1].sum() > 0
        # the tracked tree becomes a mesh: that window adds nothing and is counted
        eng.set_children(0, root, rp, cl)
        eng.publish(np.zeros(5))
        eng.run()
        assert raw_cut(eng, [0])[0] == E_STATE
        t = eng.cut_take()
        same(t[:4], want[:4], "before the topic became a mesh")
        assert t[4:] == (2, 1)
        # ... and a tree again
        eng.set_tree(0, root, parent)
        eng.publish(np.zeros(3))
        eng.run()
        t = eng.cut_take()
        same(t[:4], CR.topic_cut(n, root, live, 3, parent)[:4], "a tree again")
        assert t[4:] == (1, 0)


# ---- 9. stale rows ------------------------------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("cut_first", [True, False])
def test_stale_rows(cut_first, rows, monkeypatch):
    """A window with a cut subtree and an all-live one, in either order, the
    first the wider: the all-live answer is all zeros whatever the rows held
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
            st = eng.run()
            want = CR.window_cut(n, live, [(root, c0, parent), (root, c1, parent)])
            got = eng.peer_cut([0, 1])
            same(got, want[:4], f"run {i}")
            sums(got, want[5], want[4], f"run {i}")
            assert st.deliveries == want[4]
            if is_cut:
                assert got[1].sum() == got[1][cut] == (2 if c1 else 1) and got[2][cut] == got[1][cut] * (size - 1)
                assert got[3][cut] == (c0 + c1) * size
            else:
                assert not any(x.any() for x in got)
            check_topic(eng, 0, root, live, c0, parent, None, f"run {i}, topic 0")
            assert c1 or not any(x.any() for x in eng.peer_cut([1]))  # the idle topic adds nothing


# ---- 10. deep trees -----------------------------------------------------------------

def test_deep_path_on_the_host_build():
    """A path of 300 peers: 300 levels of one node, all in the top kernel; the
    dead node at depth 150."""
    n, c, j = 300, 3, 150
    parent = path(n)
    live = np.ones(n, dtype=np.uint8)
    with make_engine(n, False) as eng:
        eng.set_tree(0, 0, parent)
        eng.publish(np.zeros(c))
        st = eng.run()
        assert_builds(eng, False)
        got, _ = check_topic(eng, 0, 0, live, c, parent, st, "path 300")
        assert not any(x.any() for x in got)
        live[j] = 0
        eng.set_live(live)
        eng.publish(np.zeros(c))
        st = eng.run()
        got, _ = check_topic(eng, 0, 0, live, c, parent, st, "path 300, cut at 150")
        assert got[1].sum() == got[1][j] == 1 and got[2][j] == n - 1 - j and got[3][j] == c * (n - j)
        assert st.deliveries == c * (j - 1)


# ---- 11. tracking against the blocking call ----------------------------------------

def test_tracking_windows_runs_and_takes():
    """msg_window = 64: a run of three windows, then runs under two other
    masks, takes between: the totals equal the sum of cut_ref per window and
    of peer_cut per single-window run."""
    n, root, parent, live = one_topic(0, 71)
    rng = np.random.default_rng(71)
    p1 = random_tree(rng, n, 9)
    live[9] = 1
    live2 = (rng.random(n) > 0.2).astype(np.uint8)
    live2[[root, 9]] = 1
    all_live = np.ones(n, dtype=np.uint8)

    def ref(lv, c0, c1):
        return CR.window_cut(n, lv, [(root, c0, parent), (9, c1, p1)])

    with PE.Engine(n, 2, msg_window=64) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, 9, p1)
        eng.set_live(live)
        eng.cut_track([1, 0])
        t = eng.cut_take()  # nothing has run
        assert t[4:] == (0, 0) and not any(x.any() for x in t[:4])
        # 150 + 70 messages: windows of (64, 64), (64, 6), (22, 0)
        msgs = rng.permutation(np.concatenate([np.zeros(150), np.ones(70)])).astype(np.uint32)
        eng.publish(msgs)
        st = eng.run()
        assert st.windows == 3
        want, possible, total = zeros(n), 0, 0
        for c0, c1 in ((64, 64), (64, 6), (22, 0)):
            w = ref(live, c0, c1)
            want = add(want, w[:4])
            possible += w[5]
            total += w[4]
        assert total == st.deliveries
        same(eng.peer_cut([0, 1]), ref(live, 22, 0)[:4], "last window")  # while the totals stand
        blocking = zeros(n)
        for lv, c0, c1 in ((live2, 10, 3), (all_live, 0, 64), (live2, 5, 0)):
            eng.set_live(lv)
            eng.publish(np.concatenate([np.zeros(c0), np.ones(c1)]).astype(np.uint32))
            st2 = eng.run()
            assert st2.windows == 1
            w = ref(lv, c0, c1)
            assert st2.deliveries == w[4]
            total += w[4]
            possible += w[5]
            want = add(want, w[:4])
            blocking = add(blocking, eng.peer_cut([0, 1]))
        t = eng.cut_take()
        assert t[4:] == (6, 0)
        same(t[:4], want, "six windows")
        sums(t[:4], possible, total, "six windows")
        assert (t[1] >= blocking[1]).all() and blocking[1].sum() > 0
        # a second take: zeros and no window
        t = eng.cut_take()
        assert t[4:] == (0, 0) and not any(x.any() for x in t[:4])
        # take, run, take: the new run alone, equal to the blocking call's answer
        eng.set_live(live)
        eng.publish(np.zeros(40))
        eng.run()
        t = eng.cut_take()
        assert t[4:] == (1, 0)
        same(t[:4], ref(live, 40, 0)[:4], "the new run")
        same(t[:4], eng.peer_cut([1, 0]), "the new run, blocking")
        # setting again zeroes the totals; a subset tracked: topic 1 is not counted
        eng.publish(np.zeros(5))
        eng.run()
        eng.cut_track([0])
        t = eng.cut_take()
        assert t[4:] == (0, 0) and not any(x.any() for x in t[:4])
        eng.publish(np.concatenate([np.zeros(7), np.ones(9)]).astype(np.uint32))
        eng.run()
        t = eng.cut_take()
        assert t[4:] == (1, 0)
        same(t[:4], ref(live, 7, 0)[:4], "topic 0 alone")


def tree_window(ot, n, k, dropped=False):
    """k messages over oracle.Tree ot as the engine runs them (the windows of
    test_gpu_downstream.tree_window): the four arrays summed, the deliveries,
    the possible deliveries, the windows, and the last window's arrays alone."""
    out = [np.zeros(n, dtype=np.int64) for _ in range(4)]
    last = None
    left, windows, deliveries, possible = k, 0, 0, 0
    while left:
        par = ot.parents()
        hop = ot.message()
        c = 1 if dropped or not np.array_equal(ot.parents(), par) else left
        dropped = False
        for _ in range(c - 1):
            assert np.array_equal(ot.message(), hop)
        got = hop != 0xFF
        got[ot.root] = False
        last = CR.from_parents(n, ot.root, par, c * got, c)
        p = np.asarray(par, dtype=np.uint32).copy()
        p[ot.root] = NONE
        members = int((GC.reference(n, [(ot.root, p)], np.ones(n, dtype=np.uint8))["topics"][0]["depth_of"] >= 0).sum())
        for o, w in zip(out, last):
            o += w
        deliveries += c * int(got.sum())
        possible += c * (members - 1)
        left -= c
        windows += 1
    return tuple(out), deliveries, possible, windows, last


def test_tracking_a_run_split_by_a_drop():
    """An interior peer dropped: topic 0's first message runs alone over the
    old tree and is lost below the dead host, the rest over the repaired one
    (a rebuilt node space between two windows of one run).  The dropped peer
    has left the node space and those it took down are orphans until the
    repair: neither is a node, so nothing is missed and nothing is cut."""
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
        eng.cut_track([0, 1])
        eng.publish(topics)
        st = eng.run()
        assert st.windows >= 2
        (w0, d0, p0, k0, l0), (w1, d1, p1, k1, l1) = tree_window(ots[0], n, 5, dropped=True), tree_window(ots[1], n, 5)
        assert (k0, k1) == (2, 1) and d0 + d1 == st.deliveries
        t = eng.cut_take()
        assert t[4:] == (st.windows, 0)
        want = add(tuple(x.astype(np.uint64) for x in w0), w1)
        same(t[:4], want, "drop")
        sums(t[:4], p0 + p1, d0 + d1, "drop")
        assert not any(x.any() for x in t[:4]) and p0 + p1 == d0 + d1  # every node of every window was reached
        same(eng.peer_cut([0, 1]), add(tuple(x.astype(np.uint64) for x in l0), l1), "drop, last window")


# ---- 12. churn ----------------------------------------------------------------------

@pytest.mark.parametrize("gpu_build", [True, False])
def test_churn(gpu_build):
    """Joins, leaves and drops between runs, the node space rebuilt on the GPU
    or on the host every batch: the totals over all batches, and the blocking
    answer for each batch's last window, follow the oracle's trees; orphans
    add nothing."""
    rng = np.random.default_rng(17)
    n, seed = 3000, 4
    eng = make_engine(n, gpu_build, seed=seed)
    ot = O.Tree(n, 0, 2, 5, PE.Engine.topic_seed(seed, 0))
    eng.topic_create(0, 0, 2, 5)
    eng.join(0, np.arange(1, n, 2))
    ot.join_all(range(1, n, 2))
    members = set(range(1, n, 2))
    eng.cut_track([0])
    want = zeros(n)
    windows = deliveries = possible = built = 0
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
            w, d, poss, kw, last = tree_window(ot, n, k, dropped=step % 3 == 1)
            assert run.deliveries == d and run.windows == kw, step
            want = add(want, w)
            windows += run.windows
            deliveries += run.deliveries
            possible += poss
            blocking = eng.peer_cut([0])
            same(blocking, last, f"step {step}, the batch's last window")
            assert int(blocking[3].sum()) == int(blocking[0].sum())
            assert np.array_equal(eng.parents(0), ot.parents()), step
            built = assert_builds(eng, gpu_build, built)
        t = eng.cut_take()
        assert t[4:] == (windows, 0)
        same(t[:4], want, f"churn gpu_build {gpu_build}")
        sums(t[:4], possible, deliveries, "churn")
        assert not any(x[sorted(set(range(n)) - members - {0})].any() for x in t[:4])  # peers outside the topic


# ---- 13. pipelined ------------------------------------------------------------------

def tracked_blocking(e, batches):
    stats = []
    for b in batches:
        e.publish(b)
        stats.append(e.run())
    return e.cut_take(), stats


def tracked_pipelined(e, batches):
    stats = []
    for i, b in enumerate(batches):
        e.publish(b)
        e.run_async()
        if i:
            stats.append(e.wait())
    rc, a, nw, nsk = raw_take(e)  # a run in flight: refused, nothing changes
    assert rc == E_STATE and nw == 0xCCCC and nsk == 0xDDDD and untouched(a)
    stats.append(e.wait())
    return e.cut_take(), stats


@pytest.mark.parametrize("shape", ["deep", "twin"])
def test_pipelined(shape):
    """Six run_async over a shape whose windows overlap their predecessors
    (deep: alternating row sets and overlapped prefixes; twin: whole windows
    side by side), under a mask with 3 % dead, then the waits and one take:
    the totals of the same six batches run one after the other."""
    if shape == "deep":
        wl = WL.cfg3(200_000, 16, 5000)
        batches, plan = even_batches(len(wl.topics), 6, 52), {"overlap_min_bytes": 0}
    else:
        wl = WL.cfg3(60_000, 16, 4000)
        batches, plan = even_batches(len(wl.topics), 6, 51), {"flood": 0}
    live = (np.random.default_rng(11).random(wl.n_peers) >= 0.03).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    order = np.arange(len(wl.topics), dtype=np.uint32)[::-1].copy()

    def make():
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=64, plan=plan)
        WL.build_engine_topics(e, wl)
        e.set_live(live)
        e.cut_track(order)
        return e

    with make() as e:
        t0, st0 = tracked_blocking(e, batches)
        last = e.peer_cut(order)
    with make() as e:
        t1, st1 = tracked_pipelined(e, batches)
        over = e.overlapped_windows()
        same(e.peer_cut(order), last, shape + " last window")
    print("pipelined", shape, "overlapped", over)
    assert over > 0
    assert t0[4] == t1[4] == sum(s.windows for s in st0) == 12 and t0[5] == t1[5] == 0
    same(t1[:4], t0[:4], shape)
    assert sum(s.deliveries for s in st1) == sum(s.deliveries for s in st0) > 0
    assert int(t1[3].sum()) == int(t1[0].sum()) > 0 and t1[1].sum() > 0  # identity 2 over the run
    for a, b in zip(t1[:4], last):  # the same node space and mask in each of the 12 windows
        assert np.array_equal(a, 12 * b)


# ---- 14. beside a sink, load, hop and downstream tracking --------------------------------

def test_with_a_sink_and_the_other_trackers():
    """A topics sink and load, hop, downstream and cut tracking at once: each
    answer as with that one alone, and equal to its reference."""
    n, root, parent, live = one_topic(0, 91)
    rng = np.random.default_rng(91)
    msgs = [rng.integers(0, 2, size=150).astype(np.uint32), np.zeros(70, dtype=np.uint32)]

    def go(sink, load, hops, down, cut):
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
            if cut:
                e.cut_track([0, 1])
            views = []
            for m in msgs:
                e.publish(m)
                e.run()
                if sink:
                    views.append(e.sink_take_topics())
            return (views, e.load_take() if load else None, e.hops_take() if hops else None,
                    e.downstream_take() if down else None, e.cut_take() if cut else None)

    all5 = go(True, True, True, True, True)
    only_sink, only_load = go(True, False, False, False, False), go(False, True, False, False, False)
    only_hops, only_down = go(False, False, True, False, False), go(False, False, False, True, False)
    only_cut = go(False, False, False, False, True)
    same(all5[4][:4], only_cut[4][:4], "cut beside a sink and the other trackers")
    assert all5[4][4:] == only_cut[4][4:] == (sum(v["n_windows"] for v in all5[0]), 0)
    # each against its own reference: the first batch runs as two windows of (64, 64) and the rest, the second as (64, 0), (6, 0)
    c = [int((msgs[0] == t).sum()) for t in (0, 1)]
    assert 64 < min(c) and max(c) <= 128
    wins = [(64, 64), (c[0] - 64, c[1] - 64), (64, 0), (6, 0)]
    want_c, want_d, want_l, want_h = zeros(n), zeros(n)[:2], zeros(n)[:2], None
    possible = total = 0
    for c0, c1 in wins:
        tl = [(root, c0, parent), (root, c1, parent)]
        w = CR.window_cut(n, live, tl)
        want_c = add(want_c, w[:4])
        total += w[4]
        possible += w[5]
        want_d = add(want_d, DR.window_downstream(n, live, tl)[:2])
        want_l = add(want_l, LR.window_load(n, live, [(root, c0, parent, None), (root, c1, parent, None)])[:2])
        h = HR.window_hops(n, live, tl)[:3]
        want_h = h if want_h is None else tuple(a + b for a, b in zip(want_h, h))
    assert all5[4][4] == len(wins)
    same(all5[4][:4], want_c, "cut against its reference")
    sums(all5[4][:4], possible, total, "four windows")
    for a, b, w in zip(all5[3][:2], only_down[3][:2], want_d):
        assert np.array_equal(a, b) and np.array_equal(a, w)
    for a, b, w in zip(all5[1][:2], only_load[1][:2], want_l):
        assert np.array_equal(a, b) and np.array_equal(a, w)
    for a, b, w in zip(all5[2][:3], only_hops[2][:3], want_h):
        assert np.array_equal(a, b) and np.array_equal(a, w)
    assert all5[1][2] == only_load[1][2] and all5[2][3:] == only_hops[2][3:] and all5[3][2:] == only_down[3][2:]
    assert all5[3][1][root] == all5[1][0].sum() == all5[2][2].sum() == total > 0  # deliveries, three ways
    for a, b in zip(all5[0], only_sink[0]):
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


# ---- 15. the rules ------------------------------------------------------------------

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
        rc, a = raw_cut(eng, [0])
        assert rc == E_NOTREADY and untouched(a)
        rc, a, nw, nsk = raw_take(eng)
        assert rc == E_NOTREADY and nw == 0xCCCC and nsk == 0xDDDD and untouched(a)
        eng.publish(np.zeros(10))
        eng.run()
        # the arguments
        assert raw_cut(eng, [0, 0])[0] == E_INVAL  # a topic named twice
        rc, a = raw_cut(eng, [0, 2])
        assert rc == E_RANGE and untouched(a)  # nothing written
        assert raw_cut(eng, [0], which=(False,) * 4)[0] == E_INVAL
        assert eng._L.ps_peer_cut(eng._h, None, 1, a[0].ctypes.data_as(U64P), None, None, None) == E_INVAL
        # each output alone and every pair; no topic: zeros; an idle topic: zeros
        full = eng.peer_cut([0, 1])
        same(full, CR.window_cut(n, live, [(root, 10, parent), (root, 0, parent)])[:4], "full")
        assert full[1].sum() > 0
        for mask in range(1, 16):
            which = tuple(bool(mask >> i & 1) for i in range(4))
            rc, a = raw_cut(eng, [0], which)
            assert rc == 0, which
            for x, w, f in zip(a, which, full):
                assert np.array_equal(x, f) if w else (x == FILL).all(), which
        rc, a = raw_cut(eng, [])
        assert rc == 0 and not any(x.any() for x in a)
        assert not any(x.any() for x in eng.peer_cut([1]))
        # tracking: a refused call leaves the previous tracking
        eng.cut_track([0])
        assert raw_track(eng, [1, 1]) == E_INVAL and raw_track(eng, [0, 5]) == E_RANGE
        assert eng._L.ps_cut_track(eng._h, None, 2) == E_INVAL
        eng.publish(np.zeros(3))
        eng.run()
        w3 = CR.topic_cut(n, root, live, 3, parent)
        t = eng.cut_take()
        assert t[4:] == (1, 0)
        same(t[:4], w3[:4], "three messages")
        assert eng._L.ps_cut_take(eng._h, None, None, None, None, None, None) == E_INVAL
        # NULL arrays are allowed: the take still clears
        eng.publish(np.zeros(2))
        eng.run()
        nwc, nskc = C.c_uint64(), C.c_uint64()
        assert eng._L.ps_cut_take(eng._h, None, None, None, None, C.byref(nwc), C.byref(nskc)) == 0 and nwc.value == 1
        t = eng.cut_take()
        assert t[4] == 0 and not any(x.any() for x in t[:4])
        # a run in flight
        eng.publish(np.zeros(3))
        eng.run_async()
        assert raw_track(eng, [1]) == E_STATE
        rc, a, nw, nsk = raw_take(eng)
        assert rc == E_STATE and nw == 0xCCCC and untouched(a)
        eng.wait()
        t = eng.cut_take()
        assert t[4:] == (1, 0)
        same(t[:4], w3[:4], "three messages, asynchronous")
        # setting again and clearing zero the totals
        eng.publish(np.zeros(1))
        eng.run()
        eng.cut_track([1, 0])
        t = eng.cut_take()
        assert t[4:] == (0, 0) and not any(x.any() for x in t[:4])
        eng.cut_track([])
        rc, _, nw, _ = raw_take(eng)
        assert rc == E_NOTREADY and nw == 0xCCCC
        eng.publish(np.zeros(3))
        eng.run()  # nothing is tracked: the run is as ever
        same(eng.peer_cut([0]), w3[:4], "untracked")


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
        before = eng.peer_cut([0, 1])
        only0 = eng.peer_cut([0])
        same(only0, CR.topic_cut(n, 0, live, 4, p0)[:4], "topic 0")
        assert only0[1].sum() > 0
        eng.set_tree(0, 0, p1)  # over a parent array: the window's levels stay
        same(eng.peer_cut([0, 1]), before, "after set_tree over a parent array")
        eng.set_tree(1, 0, p1)  # over a join topic: its record starts afresh
        rc, a = raw_cut(eng, [0, 1])
        assert rc == E_STATE and untouched(a)
        same(eng.peer_cut([0]), only0, "the other topic alone")
        eng.publish(np.array([0] * 3 + [1] * 2, dtype=np.uint32))
        eng.run()
        same(eng.peer_cut([0, 1]), CR.window_cut(n, live, [(0, 3, p1), (0, 2, p1)])[:4], "after the next run")


def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(3)]
    try:
        # an engine that is tracking takes no ranks
        engines[2].cut_track([0])
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
            rc, a = raw_cut(e, [0])
            assert rc == E_STATE and untouched(a)
            assert raw_take(e)[0] == E_NOTREADY
    finally:
        for e in engines:
            e.close()
