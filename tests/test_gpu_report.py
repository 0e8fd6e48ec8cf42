"""GPU: the four answers from one pass (ps_peer_report, ps_report_track /
ps_report_take) -- per-peer load, deliveries by hop, the
audience behind each peer and the losses blamed on their cut points, the
sections selected in `what`, for the last window or accumulated behind every
window of every run.

Every comparison is bit-exact, against tests/report_ref.py (the four
references composed) and against the engine's own four calls on the same
window -- ps_peer_load, ps_topic_hops, ps_peer_downstream, ps_peer_cut, and
their trackers.  Those are the yardsticks: the report is never checked against
itself.  The seam (PSAMD_AB=1 PSAMD_LOAD_COUNT=rows) makes k_report_nodes count
every full row from its words."""
import ctypes as C
import threading

import numpy as np
import pytest

import graph_check as GC
import oracle as O
import psengine as PE
import report_ref as RR
from psengine import workloads as WL
from test_gpu_churn import assert_builds, make_engine
from test_gpu_cut import tree_window as cut_tree_window
from test_gpu_downstream import TOP_EDGE, fan_tree, path, star
from test_gpu_drain_batch import random_mesh2, random_tree
from test_gpu_drain_shared import one_topic
from test_gpu_load import heap_tree, seam, shared_topics
from test_gpu_sink import drop_engine, even_batches

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
FILL = 0xABABABABABABABAB
BLOCK = 256  # kDownBlock: the nodes of one work item
ALL = PE.REPORT_ALL
SIZE = C.sizeof(PE.Report)
MASKS = list(range(1, 16))


# ---- helpers ------------------------------------------------------------------------

def same(got, want, what=""):
    """A dict of arrays against another: the same keys, uint64, bit for bit."""
    assert tuple(got) == tuple(want), (what, tuple(got), tuple(want))
    for k in got:
        g, w = got[k], np.asarray(want[k]).astype(np.uint64)
        assert g.dtype == np.uint64 and g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what} {k}: {len(bad)} words differ, first {bad[:6].tolist()} got "
                                 f"{g[g != w][:6]} want {w[g != w][:6]}")


def four_calls(eng, topics, what=ALL):
    """The engine's own answers for the last window, as the report names them."""
    out = {}
    if what & PE.REPORT_LOAD:
        out["recv"], out["sent"] = eng.peer_load(topics)
    if what & PE.REPORT_HOPS:
        out["nodes"], out["reached"], out["deliv"] = eng.topic_hops(topics)
    if what & PE.REPORT_DOWNSTREAM:
        out["below"], out["carried"] = eng.peer_downstream(topics)
    if what & PE.REPORT_CUT:
        out["missed"], out["cuts"], out["orphaned"], out["lost"] = eng.peer_cut(topics)
    return out


def four_tracks(eng, topics):
    eng.load_track(topics)
    eng.hops_track(topics)
    eng.downstream_track(topics)
    eng.cut_track(topics)


def four_takes(eng, what=ALL):
    """The four trackers' totals as the report names them, and their counts."""
    out, counts = {}, {}
    if what & PE.REPORT_LOAD:
        out["recv"], out["sent"], counts["load"] = eng.load_take()
    if what & PE.REPORT_HOPS:
        out["nodes"], out["reached"], out["deliv"], *counts["hops"] = eng.hops_take()
    if what & PE.REPORT_DOWNSTREAM:
        out["below"], out["carried"], *counts["down"] = eng.downstream_take()
    if what & PE.REPORT_CUT:
        out["missed"], out["cuts"], out["orphaned"], out["lost"], *counts["cut"] = eng.cut_take()
    return out, counts


def check(eng, topics, ref=None, what=ALL, tag=""):
    """peer_report(topics, what) against the four calls and, where given, the
    reference (a dict of all eleven arrays, or of what's)."""
    got = eng.peer_report(topics, what)
    assert tuple(got) == RR.names_of(what), tag
    same(got, four_calls(eng, topics, what), f"{tag} what {what:#x} against the four calls")
    if ref is not None:
        same(got, {k: ref[k] for k in got}, f"{tag} what {what:#x} against the reference")
    return got


def filled(eng, n_topics, skip=()):
    """Eleven filled arrays and the ps_report over them; skip: names that get a NULL pointer."""
    arrays = {k: np.full((n_topics, PE.MAX_ROUNDS) if k in ("nodes", "reached", "deliv") else eng.n_peers, FILL, dtype=np.uint64)
              for k in RR.NAMES}
    rep = PE.Report()
    for k, a in arrays.items():
        if k not in skip:
            setattr(rep, k, a.ctypes.data_as(U64P))
    return arrays, rep


def raw_report(eng, topics, what, skip=()):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    arrays, rep = filled(eng, t.size, skip)
    rc = eng._L.ps_peer_report(eng._h, t.ctypes.data_as(U32P) if t.size else None, t.size, what, C.byref(rep), SIZE)
    return rc, arrays


def raw_track(eng, topics, what=ALL):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    return eng._L.ps_report_track(eng._h, t.ctypes.data_as(U32P), t.size, what)


def raw_take(eng, n_topics=1):
    arrays, rep = filled(eng, n_topics)
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    rc = eng._L.ps_report_take(eng._h, C.byref(rep), SIZE, C.byref(nw), C.byref(nsk))
    return rc, arrays, nw.value, nsk.value


def untouched(arrays):
    return all((a == FILL).all() for a in arrays.values())


def zero(d):
    return not any(a.any() for a in d.values())


def levels_of(parent):
    """The peers of each BFS level of a tree rooted at 0 whose peer ids name its nodes."""
    n = parent.size
    d = GC.reference(n, [(0, parent)], np.ones(n, dtype=np.uint8))["topics"][0]["depth_of"]
    return [np.nonzero(d == l)[0] for l in range(int(d.max()) + 1)]


def run_dead(parent, n_msgs, dead_sets, whats=(ALL,)):
    """One engine over a tree rooted at 0 whose peer ids name its nodes, one run
    per dead set: the report against the four calls and the reference."""
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
            ref = RR.window_report(n, live, [(0, n_msgs, parent, None)])
            got = check(eng, [0], ref, ALL, f"{n} peers, dead {name}")
            for what in whats:
                if what != ALL:
                    check(eng, [0], ref, what, f"{n} peers, dead {name}")
            assert int(got["recv"].sum()) == st.deliveries == int(got["deliv"].sum())
            assert (got["cuts"].sum() >= 1) == bool(len(dead))


# ---- 1. every mask ------------------------------------------------------------------

def test_every_mask():
    """A 31-peer heap tree with a dead inner node, 70 messages (two-word rows):
    each of the 15 masks writes its sections and leaves the other pointers'
    arrays alone; a NULL pointer inside a selected section is skipped."""
    n, c = 31, 70
    parent = heap_tree(n)
    live = np.ones(n, dtype=np.uint8)
    live[5] = 0
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        eng.set_live(live)
        eng.publish(np.zeros(c))
        eng.run()
        ref = RR.window_report(n, live, [(0, c, parent, None)])
        yard = four_calls(eng, [0])
        same(yard, ref, "the four calls against the reference")
        assert yard["cuts"][5] == 1 and yard["lost"][5] == c * 7 and yard["below"][5] == 6
        for what in MASKS:
            check(eng, [0], ref, what)
            rc, a = raw_report(eng, [0], what)
            assert rc == 0, what
            on = RR.names_of(what)
            for k in RR.NAMES:
                if k in on:
                    assert np.array_equal(a[k].reshape(yard[k].shape), yard[k]), (what, k)
                else:
                    assert (a[k] == FILL).all(), (what, k)
        # one NULL pointer inside a selected section, each array in turn; then all but one of each section
        for k in RR.NAMES:
            rc, a = raw_report(eng, [0], ALL, skip=(k,))
            assert rc == 0 and (a[k] == FILL).all(), k
            assert all(np.array_equal(a[j].reshape(yard[j].shape), yard[j]) for j in RR.NAMES if j != k), k
        keep = ("sent", "deliv", "below", "orphaned")
        rc, a = raw_report(eng, [0], ALL, skip=tuple(k for k in RR.NAMES if k not in keep))
        assert rc == 0
        for k in RR.NAMES:
            assert np.array_equal(a[k].reshape(yard[k].shape), yard[k]) if k in keep else (a[k] == FILL).all(), k


# ---- 2. row widths ------------------------------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("n_msgs", [1, 63, 64, 65, 8300])
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
        ref = RR.window_report(n, live, [(root, n_msgs, parent, None)])
        for what in (ALL, PE.REPORT_LOAD, PE.REPORT_HOPS, PE.REPORT_DOWNSTREAM, PE.REPORT_CUT, 0x6, 0x9):
            check(eng, [0], ref, what, f"n_msgs {n_msgs} rows {rows}")
        got = eng.peer_report([0])
        assert int(got["recv"].sum()) == st.deliveries and got["cuts"].sum() > 1


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("shape", ["heap15", "heap16", "heap17", "heap64", "path40"])
def test_wide_rows(shape, rows, monkeypatch):
    """8,300 messages: 130-word rows, 15 to a strip, so that strips end inside
    levels and levels inside strips; a level's first and last node masked."""
    seam(monkeypatch, rows)
    parent = path(40) if shape == "path40" else heap_tree(int(shape[4:]))
    lv = levels_of(parent)
    pick = (1, len(lv) - 1) if shape != "path40" else (15, 16)
    masks = {f"l{l}_ends": sorted({int(lv[l][0]), int(lv[l][-1])}) for l in pick}
    masks["none"] = []
    run_dead(parent, 8300, masks)


# ---- 3. strip and work-item edges ---------------------------------------------------

def edge_masks(parent, per=2048):
    """Dead sets at the first and the last node of the 256-node work items of
    the levels wider than a block, a pair that straddles two items, and the
    last node of the first strip and the first of the second."""
    n = parent.size
    out = {"none": []}
    for l, at in enumerate(levels_of(parent)):
        if at.size <= BLOCK:
            continue
        lo, hi = int(at[0]), int(at[-1])
        out[f"l{l}_item_ends"] = sorted({lo, lo + BLOCK - 1, hi})
        out[f"l{l}_straddle"] = [x for x in (lo + BLOCK - 1, lo + BLOCK) if x <= hi]
    if n - 1 > per:
        out["strip_last"] = [per]
        out["strip_next"] = [per + 1]
        out["strip_both"] = [per, per + 1]
    return out


@pytest.mark.parametrize("n", [2047, 2049, 4100])
def test_strip_and_work_item_edges(n):
    """One message: one-word rows, 2,048 to a strip -- a strip spans every
    level of the 2,047-peer tree, and a level boundary lies inside the strips
    of the others.  The last levels are cut into several work items."""
    parent = heap_tree(n)
    masks = edge_masks(parent)
    assert any(k.endswith("_straddle") for k in masks) and (n < 2050 or "strip_both" in masks)
    run_dead(parent, 1, masks, whats=(ALL, 0xC, 0x3))


@pytest.mark.parametrize("shape", list(TOP_EDGE))
def test_top_edge(shape):
    """The shapes in which the first level wider than a block is the last one
    or the one before it: the cut at level top - 1, top and top + 1."""
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
    idx = [0, 63, 64, 65, 2999]
    masks = {f"child{i}": [1 + i] for i in idx}
    masks["all_five"] = [1 + i for i in idx]
    masks["none"] = []
    run_dead(star(3001), 1, masks)


@pytest.mark.parametrize("a,b", [(64, 65), (65, 64)])
def test_fan_out_64_and_65_at_an_inner_node(a, b):
    """Node 1 has a children (3 .. 2 + a), node 2 has b; each of those has one
    child: 64 children are walked by a lane, 65 by the wave with the parent's
    fullness broadcast."""
    first1, last1, first2, last2 = 3, 2 + a, 3 + a, 2 + a + b
    run_dead(fan_tree(a, b), 2, {
        "first_of_each": [first1, first2], "last_of_each": [last1, last2],
        "every_child_of_1": list(range(first1, last1 + 1)), "every_child_of_2": list(range(first2, last2 + 1)),
        "every_child": list(range(first1, last2 + 1)), "a_dead_wide_parent": [1, 2, first1, last2], "none": [],
    })


# ---- 5. depth -----------------------------------------------------------------------

def test_deep_path_on_the_host_build():
    """A path of 300 peers on the host's node-space build, cut at depth 150:
    the hop arrays' clamped last column, below and lost."""
    n, c, j = 300, 3, 150
    parent = path(n)
    live = np.ones(n, dtype=np.uint8)
    live[j] = 0
    with make_engine(n, False) as eng:
        eng.set_tree(0, 0, parent)
        eng.set_live(live)
        eng.publish(np.zeros(c))
        st = eng.run()
        assert_builds(eng, False)
        got = check(eng, [0], RR.window_report(n, live, [(0, c, parent, None)]), ALL, "path 300, cut at 150")
        hops = eng.topic_hops([0])
        assert np.array_equal(got["nodes"][:, 255], hops[0][:, 255]) and got["nodes"][0, 255] == n - 255
        assert not got["reached"][0, 255] and got["reached"][0, 149] == 1 and not got["reached"][0, 150]
        assert np.array_equal(got["below"], np.arange(n - 1, -1, -1).astype(np.uint64))
        assert got["lost"].sum() == got["lost"][j] == c * (n - j) and st.deliveries == c * (j - 1)
        check(eng, [0], None, 0xE)


# ---- 6. start groups ----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["group_major", "group_major_rows", "aligned", "aligned_rows", "compact", "no_lazy_seen"])
def test_start_groups(kind, monkeypatch):
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
        got = check(eng, [1, 0], RR.window_report(n, live, [(root, c[1], parent, None), (root, c[0], parent, None)]), ALL, kind)
        assert int(got["recv"].sum()) == st.deliveries
        check(eng, [1], None, 0xA, kind)


# ---- 7. several topics --------------------------------------------------------------

@pytest.mark.parametrize("order", [[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [2, 1], [3], []])
def test_several_topics(order):
    """A 1-word topic, a 130-word one rooted at a leaf of the first, an idle one
    and one that is its root alone, in several orders and subsets: the sums in
    peer space, hop row i for order[i]."""
    n, free, (r0, p0), (r1, p1), live = shared_topics()
    msgs = np.concatenate([np.full(10, 0), np.full(8300, 1), np.full(3, 3)]).astype(np.uint32)
    defs = {0: (r0, 10, p0, None), 1: (r1, 8300, p1, None), 2: (r0, 0, p0, None),
            3: (7, 3, np.full(n, NONE, dtype=np.uint32), None)}
    with PE.Engine(n, 4) as eng:
        eng.set_tree(0, r0, p0)
        eng.set_tree(1, r1, p1)
        eng.set_tree(2, r0, p0)
        eng.topic_create(3, 7)
        eng.set_live(live)
        eng.publish(msgs)
        eng.run()
        ref = RR.window_report(n, live, [defs[t] for t in order])
        for what in (ALL, 0x2, 0x7, 0xC):
            check(eng, order, ref, what, str(order))
        got = eng.peer_report(order)
        assert zero({k: got[k][free] for k in got if got[k].ndim == 1})  # peers in no topic
        for i, t in enumerate(order):
            alone = eng.topic_hops([t])
            for k, a in zip(("nodes", "reached", "deliv"), alone):
                assert np.array_equal(got[k][i], a[0]), (order, t, k)
            assert got["nodes"][i].any() == (t in (0, 1))
        if not order:
            assert zero(got) and got["nodes"].shape == (0, PE.MAX_ROUNDS)


def test_a_cut_point_in_one_topic_the_root_of_another():
    n, x, c0, c1 = 127, 5, 4, 70
    p0 = heap_tree(n)
    perm = np.arange(n)  # topic 1: the same heap, relabelled so that x is its root
    perm[[0, x]] = [x, 0]
    p1 = np.full(n, NONE, dtype=np.uint32)
    for i in range(1, n):
        p1[perm[i]] = perm[(i - 1) // 2]
    live = np.ones(n, dtype=np.uint8)
    live[x] = 0
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, 0, p0)
        eng.set_tree(1, x, p1)
        eng.set_live(live)
        eng.publish(np.concatenate([np.zeros(c0), np.ones(c1)]).astype(np.uint32))
        eng.run()
        ref = RR.window_report(n, live, [(0, c0, p0, None), (x, c1, p1, None)])
        got = check(eng, [0, 1], ref, ALL, "both")
        assert got["cuts"].sum() == 1 and got["cuts"][x] == 1 and got["missed"][x] == c0
        assert got["sent"][x] == 2 * c1 and got["below"][x] == 30 + n - 1  # a dead root still forwards
        check(eng, [1, 0], None, 0xE, "the other order")


# ---- 8. stale rows ------------------------------------------------------------------

@pytest.mark.parametrize("first", [0x5, 0xA])
def test_stale_rows(first):
    """Two windows over the same row set, the first the wider, under different
    masks and different sections, in both orders: nothing of the other window's
    rows, verdicts, partials or weights is counted."""
    rng = np.random.default_rng(66)
    n, root = 500, 2
    parent = random_tree(rng, n, root)
    dead = (rng.random(n) > 0.1).astype(np.uint8)
    dead[root] = 1
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        for i, (live, c0, c1, what) in enumerate(((dead, 300, 30, first), (np.ones(n, dtype=np.uint8), 70, 0, ALL & ~first),
                                                  (dead, 5, 0, ALL))):
            eng.set_live(live)
            eng.publish(np.concatenate([np.zeros(c0), np.ones(c1)]).astype(np.uint32))
            eng.run()
            ref = RR.window_report(n, live, [(root, c0, parent, None), (root, c1, parent, None)])
            check(eng, [0, 1], ref, what, f"run {i}")
            check(eng, [0, 1], ref, ALL, f"run {i}")
            if i == 1:
                got = eng.peer_report([0, 1], PE.REPORT_CUT)
                assert zero(got)  # all live: nothing is missed, whatever the rows held before


# ---- 9. meshes ----------------------------------------------------------------------

def test_meshes():
    rng = np.random.default_rng(41)
    n, root = 400, 5
    rp, cl = random_mesh2(rng, n, root)
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    tree, mesh = (root, 70, parent, None), (root, 70, None, (rp, cl))
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_children(1, root, rp, cl)
        eng.set_live(live)
        for what in MASKS:  # a mesh is tracked for its load alone
            assert raw_track(eng, [0, 1], what) == (0 if what == PE.REPORT_LOAD else E_STATE), what
        assert raw_track(eng, [], ALL) == 0
        eng.report_track([0])
        eng.publish(np.concatenate([np.zeros(70), np.ones(70)]).astype(np.uint32))
        st = eng.run()
        assert st.windows == 1
        # the load section alone answers both topics
        for named, defs in (([0, 1], [tree, mesh]), ([1, 0], [mesh, tree]), ([1], [mesh])):
            got = check(eng, named, RR.window_report(n, live, defs, PE.REPORT_LOAD), PE.REPORT_LOAD, str(named))
            for what in MASKS[1:]:
                rc, a = raw_report(eng, named, what)
                assert rc == E_STATE and untouched(a), (named, what)
        assert int(eng.peer_report([0, 1], PE.REPORT_LOAD)["recv"].sum()) == st.deliveries
        want = RR.window_report(n, live, [tree])
        check(eng, [0], want, ALL, "a tree beside a mesh")
        # the tracked tree becomes a mesh: its load keeps adding, the rest does not, one skip a window
        eng.set_children(0, root, rp, cl)
        eng.publish(np.zeros(5))
        eng.run()
        assert raw_report(eng, [0], ALL)[0] == E_STATE
        as_mesh = RR.window_report(n, live, [(root, 5, None, (rp, cl))])
        same({k: as_mesh[k] for k in ("recv", "sent")}, four_calls(eng, [0], PE.REPORT_LOAD), "the mesh's load")
        assert zero({k: as_mesh[k] for k in RR.NAMES[2:]})
        got, nw, nsk = eng.report_take()
        same(got, RR.add(dict(want), as_mesh), "a tree, then a mesh")
        assert (nw, nsk) == (2, 1)
        # ... and a tree again
        eng.set_tree(0, root, parent)
        eng.publish(np.zeros(3))
        eng.run()
        got, nw, nsk = eng.report_take()
        same(got, RR.window_report(n, live, [(root, 3, parent, None)]), "a tree again")
        assert (nw, nsk) == (1, 0)
        # the load section alone: nothing is skipped
        eng.report_track([0, 1], PE.REPORT_LOAD)
        eng.set_children(0, root, rp, cl)
        eng.publish(np.array([0, 0, 1], dtype=np.uint32))
        eng.run()
        got, nw, nsk = eng.report_take()
        same(got, RR.window_report(n, live, [(root, 2, None, (rp, cl)), (root, 1, None, (rp, cl))], PE.REPORT_LOAD), "load of two meshes")
        same(got, four_calls(eng, [0, 1], PE.REPORT_LOAD), "load of two meshes, blocking")
        assert (nw, nsk) == (1, 0)


# ---- 10. tracking -------------------------------------------------------------------

@pytest.mark.parametrize("what", [ALL, 0x6, 0x9, 0x1])
def test_tracking_windows_runs_and_takes(what):
    """msg_window = 64: a run of three windows, then runs under two other
    masks, takes between: the totals equal the reference per window summed, and
    what the four trackers, set beside, accumulate."""
    n, root, parent, live = one_topic(0, 71)
    rng = np.random.default_rng(71)
    p1 = random_tree(rng, n, 9)
    live[9] = 1
    live2 = (rng.random(n) > 0.2).astype(np.uint8)
    live2[[root, 9]] = 1
    all_live = np.ones(n, dtype=np.uint8)

    def ref(lv, c0, c1):
        return RR.window_report(n, lv, [(9, c1, p1, None), (root, c0, parent, None)], what)

    with PE.Engine(n, 2, msg_window=64) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, 9, p1)
        eng.set_live(live)
        eng.report_track([1, 0], what)
        four_tracks(eng, [1, 0])
        got, nw, nsk = eng.report_take()  # nothing has run
        assert (nw, nsk) == (0, 0) and zero(got) and tuple(got) == RR.names_of(what)
        # 150 + 70 messages: windows of (64, 64), (64, 6), (22, 0)
        msgs = rng.permutation(np.concatenate([np.zeros(150), np.ones(70)])).astype(np.uint32)
        eng.publish(msgs)
        st = eng.run()
        assert st.windows == 3
        want = {}
        for c0, c1 in ((64, 64), (64, 6), (22, 0)):
            RR.add(want, ref(live, c0, c1))
        check(eng, [1, 0], ref(live, 22, 0), what, "last window")  # while the totals stand
        for lv, c0, c1 in ((live2, 10, 3), (all_live, 0, 64), (live2, 5, 0)):
            eng.set_live(lv)
            eng.publish(np.concatenate([np.zeros(c0), np.ones(c1)]).astype(np.uint32))
            assert eng.run().windows == 1
            RR.add(want, ref(lv, c0, c1))
        got, nw, nsk = eng.report_take()
        assert (nw, nsk) == (6, 0)
        same(got, want, "six windows")
        same(got, four_takes(eng, what)[0], "six windows, the four trackers")
        # a second take: zeros and no window
        got, nw, nsk = eng.report_take()
        assert (nw, nsk) == (0, 0) and zero(got)
        # take, run, take: the new run alone, equal to the blocking calls' answers
        eng.set_live(live)
        eng.publish(np.zeros(40))
        eng.run()
        got, nw, nsk = eng.report_take()
        assert (nw, nsk) == (1, 0)
        same(got, ref(live, 40, 0), "the new run")
        same(got, four_calls(eng, [1, 0], what), "the new run, blocking")


def test_tracking_a_run_split_by_a_drop():
    """An interior peer dropped: topic 0's first message runs alone over the old
    tree, the rest over the repaired one (a rebuilt node space between two
    windows of one run).  The totals are the four trackers', and the cut
    section the oracle trees'."""
    n, seed = 60, 3
    topics = np.array([0] * 5 + [1] * 5, dtype=np.uint32)
    ots = [O.Tree(n, 0, 2, 5, PE.Engine.topic_seed(seed, t)) for t in (0, 1)]
    for ot in ots:
        ot.join_all(range(1, n))
    with drop_engine(n, seed) as eng:
        par = eng.parents(0)
        kids = {}
        for p, q in enumerate(par):
            if q != NONE:
                kids.setdefault(int(q), []).append(p)
        dead = max((p for p in kids if p != 0), key=lambda p: len(kids[p]))
        eng.drop(0, [dead])
        assert ots[0].drop(dead) == 0
        eng.report_track([0, 1])
        four_tracks(eng, [0, 1])
        eng.publish(topics)
        st = eng.run()
        assert st.windows >= 2
        (w0, d0, _, k0, _), (w1, d1, _, k1, _) = cut_tree_window(ots[0], n, 5, dropped=True), cut_tree_window(ots[1], n, 5)
        got, nw, nsk = eng.report_take()
        assert (nw, nsk) == (st.windows, 0) and d0 + d1 == st.deliveries == int(got["recv"].sum())
        yard, counts = four_takes(eng)
        same(got, yard, "drop")
        assert counts["load"] == st.windows and counts["cut"] == [st.windows, 0]
        for k, a, b in zip(("missed", "cuts", "orphaned", "lost"), w0, w1):
            assert np.array_equal(got[k], (a + b).astype(np.uint64)), k
        check(eng, [0, 1], None, ALL, "drop, last window")


@pytest.mark.parametrize("gpu_build", [True, False])
def test_churn(gpu_build):
    """Joins, leaves and drops between runs, the node space rebuilt on the GPU
    or on the host every batch: the totals are the four trackers', the cut
    section follows the oracle's trees, and orphans add nothing."""
    rng = np.random.default_rng(17)
    n, seed = 3000, 4
    eng = make_engine(n, gpu_build, seed=seed)
    ot = O.Tree(n, 0, 2, 5, PE.Engine.topic_seed(seed, 0))
    eng.topic_create(0, 0, 2, 5)
    eng.join(0, np.arange(1, n, 2))
    ot.join_all(range(1, n, 2))
    members = set(range(1, n, 2))
    eng.report_track([0])
    four_tracks(eng, [0])
    want = [np.zeros(n, dtype=np.int64) for _ in range(4)]
    windows = deliveries = built = 0
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
            w, d, _, kw, _ = cut_tree_window(ot, n, k, dropped=step % 3 == 1)
            assert run.deliveries == d and run.windows == kw, step
            want = [a + b for a, b in zip(want, w)]
            windows += run.windows
            deliveries += run.deliveries
            check(eng, [0], None, ALL, f"step {step}, the batch's last window")
            built = assert_builds(eng, gpu_build, built)
        got, nw, nsk = eng.report_take()
        assert (nw, nsk) == (windows, 0)
        same(got, four_takes(eng)[0], f"churn gpu_build {gpu_build}")
        for k, a in zip(("missed", "cuts", "orphaned", "lost"), want):
            assert np.array_equal(got[k], a.astype(np.uint64)), k
        assert int(got["recv"].sum()) == deliveries == int(got["deliv"].sum())
        outside = sorted(set(range(n)) - members - {0})
        assert zero({k: got[k][outside] for k in ("missed", "cuts", "orphaned", "lost")})  # peers outside the topic


# ---- 11. pipelined ------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["deep", "twin"])
def test_pipelined(shape):
    """Six run_async over a shape whose windows overlap their predecessors,
    under a mask with 3 % dead, then the waits and one take: the totals of the
    four trackers over the same six batches run one after the other."""
    if shape == "deep":
        wl = WL.cfg3(200_000, 16, 5000)
        batches, plan = even_batches(len(wl.topics), 6, 52), {"overlap_min_bytes": 0}
    else:
        wl = WL.cfg3(60_000, 16, 4000)
        batches, plan = even_batches(len(wl.topics), 6, 51), {"flood": 0}
    live = (np.random.default_rng(11).random(wl.n_peers) >= 0.03).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    order = np.arange(len(wl.topics), dtype=np.uint32)[::-1].copy()

    def make(report):
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=64, plan=plan)
        WL.build_engine_topics(e, wl)
        e.set_live(live)
        if report:
            e.report_track(order)
        else:
            four_tracks(e, order)
        return e

    with make(False) as e:
        stats = []
        for b in batches:
            e.publish(b)
            stats.append(e.run())
        yard, counts = four_takes(e)
        last = four_calls(e, order)
    with make(True) as e:
        for i, b in enumerate(batches):
            e.publish(b)
            e.run_async()
            if i:
                e.wait()
        rc, a, nw, nsk = raw_take(e, len(order))  # a run in flight: refused, nothing changes
        assert rc == E_STATE and nw == 0xCCCC and nsk == 0xDDDD and untouched(a)
        e.wait()
        got, nw, nsk = e.report_take()
        over = e.overlapped_windows()
        same(e.peer_report(order), last, shape + " last window")
    print("pipelined", shape, "overlapped", over)
    assert over > 0
    assert nw == counts["load"] == sum(s.windows for s in stats) == 12 and nsk == 0
    same(got, yard, shape)
    assert int(got["lost"].sum()) == int(got["missed"].sum()) > 0 and got["cuts"].sum() > 0
    for k in got:  # the same node space and mask in each of the 12 windows
        assert np.array_equal(got[k], 12 * last[k]), k


# ---- 12. beside a sink and the four trackers ------------------------------------------

def test_with_a_sink_and_all_four_trackers():
    n, root, parent, live = one_topic(0, 91)
    rng = np.random.default_rng(91)
    msgs = [rng.integers(0, 2, size=150).astype(np.uint32), np.zeros(70, dtype=np.uint32)]

    def go(trackers):
        with PE.Engine(n, 2, msg_window=64) as e:
            e.set_tree(0, root, parent)
            e.set_tree(1, root, parent)
            e.set_live(live)
            e.sink_set_topics([0, 1])
            if trackers:
                e.report_track([1, 0])
                four_tracks(e, [1, 0])
            views = []
            for m in msgs:
                e.publish(m)
                e.run()
                views.append(e.sink_take_topics())
            return views, (e.report_take() if trackers else None), (four_takes(e) if trackers else None)

    views, (got, nw, nsk), (yard, counts) = go(True)
    plain = go(False)[0]
    same(got, yard, "the report beside the four trackers")
    assert nw == counts["load"] == sum(v["n_windows"] for v in views) == 4 and nsk == 0
    assert counts["hops"] == counts["down"] == counts["cut"] == [4, 0]
    c = [int((msgs[0] == t).sum()) for t in (0, 1)]
    want = {}
    for c0, c1 in ((64, 64), (c[0] - 64, c[1] - 64), (64, 0), (6, 0)):
        RR.add(want, RR.window_report(n, live, [(root, c1, parent, None), (root, c0, parent, None)]))
    same(got, want, "the report against its reference")
    for a, b in zip(views, plain):  # the sink's answer as without trackers
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


# ---- 13. the rules ------------------------------------------------------------------

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
        # before any run; nothing tracked
        for what in (ALL, PE.REPORT_LOAD):
            rc, a = raw_report(eng, [0], what)
            assert rc == E_NOTREADY and untouched(a)
        rc, a, nw, nsk = raw_take(eng)
        assert rc == E_NOTREADY and nw == 0xCCCC and nsk == 0xDDDD and untouched(a)
        eng.publish(np.zeros(10))
        eng.run()
        # the arguments
        assert raw_report(eng, [0, 0], ALL)[0] == E_INVAL  # a topic named twice
        for what in (ALL, PE.REPORT_LOAD):
            rc, a = raw_report(eng, [0, 2], what)
            assert rc == E_RANGE and untouched(a)  # nothing written
        assert raw_report(eng, [0], 0)[0] == E_INVAL and raw_report(eng, [0], 0x10)[0] == E_INVAL
        rc, a = raw_report(eng, [0], ALL, skip=("below", "carried"))
        assert rc == E_INVAL and untouched(a)  # a selected section without a pointer
        rep = PE.Report()
        assert eng._L.ps_peer_report(eng._h, None, 1, ALL, C.byref(rep), SIZE) == E_INVAL
        assert eng._L.ps_peer_report(eng._h, None, 0, ALL, C.byref(rep), SIZE - 8) == E_INVAL
        # no topic: zeros, the hop arrays not written; an idle topic: zeros
        rc, a = raw_report(eng, [], ALL)
        assert rc == 0 and zero({k: a[k] for k in a if a[k].ndim == 1})
        ref = RR.window_report(n, live, [(root, 0, parent, None), (root, 10, parent, None)])
        check(eng, [1, 0], ref, ALL, "an idle topic first")
        assert zero(eng.peer_report([1]))
        # tracking: a refused call leaves the previous tracking
        eng.report_track([0], 0xC)
        assert raw_track(eng, [1, 1]) == E_INVAL and raw_track(eng, [0, 5]) == E_RANGE
        assert raw_track(eng, [1], 0) == E_INVAL and raw_track(eng, [1], 0x1F) == E_INVAL
        assert eng._L.ps_report_track(eng._h, None, 2, ALL) == E_INVAL
        eng.publish(np.zeros(3))
        eng.run()
        w3 = RR.window_report(n, live, [(root, 3, parent, None)])
        got, nw, nsk = eng.report_take()
        assert (nw, nsk) == (1, 0)
        same(got, {k: w3[k] for k in RR.names_of(0xC)}, "three messages")
        # pointers of sections that are not tracked are not touched; the take clears
        eng.publish(np.zeros(2))
        eng.run()
        rc, a, nw, nsk = raw_take(eng)
        assert rc == 0 and (nw, nsk) == (1, 0) and untouched({k: a[k] for k in RR.names_of(0x3)})
        assert a["missed"].any() and not (a["missed"] == FILL).any()
        got, nw, nsk = eng.report_take()
        assert nw == 0 and zero(got)
        # a run in flight
        eng.publish(np.zeros(3))
        eng.run_async()
        assert raw_track(eng, [1]) == E_STATE
        rc, a, nw, nsk = raw_take(eng)
        assert rc == E_STATE and nw == 0xCCCC and untouched(a)
        eng.wait()
        got, nw, nsk = eng.report_take()
        assert (nw, nsk) == (1, 0)
        same(got, {k: w3[k] for k in RR.names_of(0xC)}, "three messages, asynchronous")
        # setting again and clearing zero the totals
        eng.publish(np.zeros(1))
        eng.run()
        eng.report_track([1, 0])
        got, nw, nsk = eng.report_take()
        assert (nw, nsk) == (0, 0) and zero(got)
        eng.report_track([])
        rc, _, nw, _ = raw_take(eng)
        assert rc == E_NOTREADY and nw == 0xCCCC
        eng.publish(np.zeros(3))
        eng.run()  # nothing is tracked: the run is as ever
        check(eng, [0], w3, ALL, "untracked")


def test_a_topic_set_anew_since_the_window():
    """Set over a join topic, a parent array starts the topic's record afresh:
    PS_E_STATE, nothing written, for every mask but the load section alone."""
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
        before = check(eng, [0, 1], None, ALL, "before")
        eng.set_tree(1, 0, p1)  # over a join topic: its record starts afresh
        for what in MASKS[1:]:
            rc, a = raw_report(eng, [0, 1], what)
            assert rc == E_STATE and untouched(a), what
        check(eng, [0, 1], None, PE.REPORT_LOAD, "the load section")
        check(eng, [0], RR.window_report(n, live, [(0, 4, p0, None)]), ALL, "the other topic alone")
        eng.publish(np.array([0] * 3 + [1] * 2, dtype=np.uint32))
        eng.run()
        check(eng, [0, 1], RR.window_report(n, live, [(0, 3, p0, None), (0, 2, p1, None)]), ALL, "after the next run")
        assert before["cuts"].sum() > 0


def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(3)]
    try:
        # an engine that is tracking takes no ranks
        engines[2].report_track([0], PE.REPORT_LOAD)
        with pytest.raises(PE.EngineError) as ei:
            engines[2].dist_init_loopback(lb, 0, PE.PART_PEER)
        assert ei.value.code == E_STATE
        for r, e in enumerate(engines[:2]):
            e.dist_init_loopback(lb, r, PE.PART_PEER)
            e.set_tree(0, root, parent)
            assert raw_track(e, [0]) == E_STATE and raw_track(e, [0], PE.REPORT_LOAD) == E_STATE  # one rank only
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
            for what in (ALL, PE.REPORT_LOAD):
                rc, a = raw_report(e, [0], what)
                assert rc == E_STATE and untouched(a)
            assert raw_take(e)[0] == E_NOTREADY
    finally:
        for e in engines:
            e.close()
