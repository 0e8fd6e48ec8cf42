"""GPU: the sink (ps_sink_set / ps_sink_take) -- standing
queries drained behind every window of a run, the windows accumulated on the
device into one result per run.  Two independent references:
 (a) a stepping engine: same topology and seed, fed the same messages one
     window's worth per run, Engine.drain_shared after each run;
 (b) the closed form the drain tests use (oracle_lists over the tree hops and
     the live mask)."""
import ctypes as C
import threading

import numpy as np
import pytest

import psengine as PE
from psengine import workloads as WL
from test_gpu_drain_async import per_peer, stats_key, vary
from test_gpu_drain_batch import drain_lists, random_mesh2, random_tree, split, tree_hops
from test_gpu_drain_shared import NONE, expand, shared, tree_case

pytestmark = pytest.mark.gpu

U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_STATE, E_RANGE, E_NOTREADY = -3, -7, -8


# ---- helpers ------------------------------------------------------------------------

def window_chunks(topics, cap):
    """The message indices of every window of one phase: window k holds each
    topic's messages k * cap .. (k + 1) * cap - 1, in publish order."""
    topics = np.asarray(topics)
    rank = np.zeros(topics.size, dtype=np.int64)
    for t in np.unique(topics):
        idx = np.nonzero(topics == t)[0]
        rank[idx] = np.arange(idx.size)
    k = rank // cap
    return [np.nonzero(k == w)[0] for w in range(int(k.max()) + 1)]


def stepped(eng, chunks, topics, starts, qt, qp, first=0):
    """Reference (a) on a second engine: one run per chunk, drain_shared after
    each, the ids mapped back to the numbering of a run that publishes
    everything at once (first + index)."""
    topics = np.asarray(topics)
    out = []
    for idx in chunks:
        f = eng.publish(topics[idx], None if starts is None else np.asarray(starts)[idx])
        eng.run()
        lists, off, ids = shared(eng, qt, qp)
        out.append((lists, off, (first + idx[ids.astype(np.int64) - f]).astype(np.uint32)))
    return out


def check_windows(res, ref):
    """The sink's result against reference (a), window by window, entry for
    entry: list numbers shifted by the lists before, ids dense."""
    wl, off, ids = res
    assert wl.dtype == np.uint32 and off.dtype == np.uint64 and ids.dtype == np.uint32
    assert wl.shape[0] == len(ref), (wl.shape, len(ref))
    assert off[0] == 0 and off[-1] == ids.size
    base = 0
    for w, (lists, o, i) in enumerate(ref):
        nl = o.size - 1
        want = np.where(lists == NONE, NONE, lists + np.uint32(base)).astype(np.uint32)
        assert np.array_equal(wl[w], want), w
        seg = off[base:base + nl + 1]
        assert np.array_equal(seg - seg[0], o), w
        assert np.array_equal(ids[int(seg[0]):int(seg[-1])], i), w
        base += nl
    assert off.size - 1 == base


def per_query(res):
    """Query q's deliveries of the run: its lists concatenated in window order."""
    wl, off, ids = res
    out = []
    for q in range(wl.shape[1]):
        got = []
        for w in range(wl.shape[0]):
            l = int(wl[w, q])
            if l != NONE:
                got += ids[int(off[l]):int(off[l + 1])].tolist()
        out.append(got)
    return out


def closed_form(qt, qp, chunks, topics, starts, first, hop, root):
    """Reference (b): per window, a topic's messages in (start round, publish)
    order, held by every reached non-root subscriber."""
    topics = np.asarray(topics)
    starts = np.zeros(topics.size, dtype=np.int64) if starts is None else np.asarray(starts)
    out = [[] for _ in qt]
    for idx in chunks:
        for q, (t, p) in enumerate(zip(qt, qp)):
            if p == root or hop[p] == 0xFF:
                continue
            mine = [int(m) for m in idx if topics[m] == t]
            out[q] += [first + m for m in sorted(mine, key=lambda m: (int(starts[m]), m))]
    return out


def raw_take(eng, n):
    """(rc, win_list copy, list_off pointer, ids pointer, n_windows, n_lists, total)."""
    wp, op, mp = U32P(), U64P(), U32P()
    n_windows, n_lists, total = C.c_uint32(0xAAAA), C.c_uint32(0xBBBB), C.c_uint64(0xCCCC)
    rc = eng._L.ps_sink_take(eng._h, C.byref(wp), C.byref(op), C.byref(mp), C.byref(n_windows), C.byref(n_lists),
                             C.byref(total))
    nw = n_windows.value if wp else 0
    wl = np.ctypeslib.as_array(wp, shape=(nw, n)).copy() if nw and n else np.empty((0, n), dtype=np.uint32)
    return rc, wl, op, mp, n_windows.value, n_lists.value, total.value


def raw_set(eng, qt, qp, list_cap=0, id_cap=0):
    qt = np.ascontiguousarray(qt, dtype=np.uint32)
    qp = np.ascontiguousarray(qp, dtype=np.uint32)
    return eng._L.ps_sink_set(eng._h, qt.ctypes.data_as(U32P), qp.ctypes.data_as(U32P), qt.size, list_cap, id_cap)


def same(got, want):
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


# ---- 1. window split --------------------------------------------------------------------

def test_window_split():
    """300 messages at msg_window = 128 (the shape of test_last_window_only):
    three windows, and every reached subscriber holds all 300 in order."""
    rng = np.random.default_rng(61)
    n, root = 400, 2
    parent = random_tree(rng, n, root)
    topics = np.zeros(300, dtype=np.uint32)
    qp = np.arange(n)
    qt = np.zeros(n, dtype=np.uint32)
    chunks = window_chunks(topics, 128)
    with PE.Engine(n, 1, msg_window=128) as eng, PE.Engine(n, 1, msg_window=128) as ref:
        eng.set_tree(0, root, parent)
        ref.set_tree(0, root, parent)
        eng.sink_set(qt, qp)
        first = eng.publish(topics)
        st = eng.run()
        assert st.windows == 3
        res = eng.sink_take()
        assert res[0].shape == (3, n)
        got = per_query(res)
        hop = tree_hops(parent, root, np.ones(n, dtype=np.uint8))
        for p in range(n):
            assert got[p] == ([] if p == root or hop[p] == 0xFF else list(range(first, first + 300))), p
        assert sum(1 for g in got if g) == n - 1
        check_windows(res, stepped(ref, chunks, topics, None, qt, qp, first))
        assert got == closed_form(qt, qp, chunks, topics, None, first, hop, root)
        # one shared list per window: 128 + 128 + 44 ids
        assert res[1].tolist() == [0, 128, 256, 300]


# ---- 2. uneven topics -------------------------------------------------------------------

def test_uneven_topics():
    """130 / 64 / 1 messages at msg_window = 64: topic 0 runs three windows,
    topics 1 and 2 one; a repeated query, the root, a peer outside the tree and
    a peer masked off among the queries."""
    rng = np.random.default_rng(62)
    n, root, outside = 300, 4, 299
    parent = random_tree(rng, n, root)
    parent[parent == outside] = root
    parent[outside] = 0xFFFFFFFF
    live = np.ones(n, dtype=np.uint8)
    off_peer = int(np.nonzero((parent == root) & (np.arange(n) != root))[0][0])  # a child of the root, masked off
    live[off_peer] = 0
    topics = rng.permutation(np.concatenate([np.full(c, t) for t, c in enumerate((130, 64, 1))])).astype(np.uint32)
    hop = tree_hops(parent, root, live)
    some = [int(p) for p in rng.choice(n, 60, replace=False)]
    peers = some + [some[3], root, outside, off_peer, some[3]]
    qt = np.tile([0, 1, 2], len(peers)).astype(np.uint32)
    qp = np.repeat(peers, 3).astype(np.uint32)
    chunks = window_chunks(topics, 64)
    assert len(chunks) == 3
    with PE.Engine(n, 3, msg_window=64) as eng, PE.Engine(n, 3, msg_window=64) as ref:
        for e in (eng, ref):
            for t in range(3):
                e.set_tree(t, root, parent)
            e.set_live(live)
        eng.sink_set(qt, qp)
        first = eng.publish(topics)
        eng.run()
        res = eng.sink_take()
        check_windows(res, stepped(ref, chunks, topics, None, qt, qp, first))
        got = per_query(res)
        assert got == closed_form(qt, qp, chunks, topics, None, first, hop, root)
        wl = res[0]
        assert np.all(wl[1:, qt != 0] == NONE)  # topics 1 and 2 are idle after the first window
        assert np.all(wl[:, qp == root] == NONE) and np.all(wl[:, qp == outside] == NONE)
        assert np.all(wl[:, qp == off_peer] == NONE)
        assert sum(len(g) for g in got) > 0


# ---- 3. drop ------------------------------------------------------------------------------

def drop_engine(n, seed):
    e = PE.Engine(n, 2, seed=seed)
    e.topic_create(0, 0, 2, 5)
    e.join(0, np.arange(1, n))
    e.topic_create(1, 0, 2, 5)
    e.join(1, np.arange(1, n))
    return e


@pytest.mark.parametrize("which", ["one_child", "widest"])
def test_drop(which):
    """An interior peer dropped: the topic's first message runs alone over the
    old tree and is lost below the dead host, the rest over the repaired tree.
    The repair re-attaches the children the dead host's parent knows of -- as
    in the reference, the one that joined it last (subtree.go:356-377, the
    State message names one peer).  one_child: the dropped peer has a single
    child, so everyone below it is re-attached.  widest: it has several, and
    the subtrees of the others are left without a parent: they hold nothing."""
    n, seed = 60, 3
    topics = np.array([0] * 5 + [1] * 5, dtype=np.uint32)
    with drop_engine(n, seed) as eng, drop_engine(n, seed) as ref:
        par = eng.parents(0)
        kids = {}
        for p in range(1, n):
            kids.setdefault(int(par[p]), []).append(p)

        def under(p):
            out, todo = set(), list(kids.get(p, []))
            while todo:
                x = todo.pop()
                out.add(x)
                todo += kids.get(x, [])
            return out

        interior = [p for p in kids if p != 0]
        if which == "one_child":
            dead = max((p for p in interior if len(kids[p]) == 1), key=lambda p: len(under(p)))
        else:
            dead = max(interior, key=lambda p: (len(kids[p]), len(under(p))))
            assert len(kids[dead]) >= 2
        below = under(dead)
        assert below
        qp = np.tile(np.arange(n), 2).astype(np.uint32)
        qt = np.repeat([0, 1], n).astype(np.uint32)
        for e in (eng, ref):
            e.drop(0, [dead])
        eng.sink_set(qt, qp)
        first = eng.publish(topics)
        st = eng.run()
        assert st.windows >= 2
        res = eng.sink_take()
        assert res[0].shape[0] >= 2
        got = per_query(res)
        t0 = list(range(first, first + 5))
        t1 = list(range(first + 5, first + 10))
        chunks = [np.array([0]), np.arange(1, 10)]
        check_windows(res, stepped(ref, chunks, topics, None, qt, qp, first))
        after = ref.parents(0)  # the repaired tree: who below the dead host has a way to the root again
        orphaned = set()
        for p in below:
            q = p
            while q != 0 and after[q] != 0xFFFFFFFF:
                q = int(after[q])
            if q != 0:
                orphaned.add(p)
        assert below - orphaned
        if which == "one_child":
            assert not orphaned
        for p in range(1, n):
            if p == dead:
                assert np.all(res[0][1:, p] == NONE)  # no row once the tree is repaired
                assert got[p] == []
            elif p in orphaned:
                assert got[p] == [], p
            elif p in below:
                assert got[p] == t0[1:], p
            else:
                assert got[p] == t0, p
            assert got[n + p] == t1, p  # the untouched topic
        assert got[0] == [] and got[n] == []


# ---- 4. kernel edges ------------------------------------------------------------------------

def test_edge_unaligned_base_multi_segment():
    """(i) 65 join topics with a dropped peer each: the first window carries
    one message of each -- 65 lists of one id -- and the second a list of
    4097 ids, two segments, from id 65 on: a base that is a multiple of
    neither 64 ids nor 256 bytes."""
    nt, per = 65, 8
    n = nt * per
    topics = np.concatenate([np.arange(nt), np.zeros(4097)]).astype(np.uint32)

    def make():
        e = PE.Engine(n, nt, msg_window=8192, seed=5)
        for t in range(nt):
            e.topic_create(t, t * per, 2, 5)
            e.join(t, np.arange(t * per + 1, (t + 1) * per))
            e.drop(t, [t * per + 1])
        return e

    qt = np.repeat(np.arange(nt), 3).astype(np.uint32)
    qp = (qt * per + np.tile([2, 3, 7], nt)).astype(np.uint32)
    with make() as eng, make() as ref:
        eng.sink_set(qt, qp)
        first = eng.publish(topics)
        st = eng.run()
        assert st.windows == 2
        res = eng.sink_take()
        wl, off, ids = res
        assert off[65] == 65 and off.size - 1 == 66 and int(off[66]) - int(off[65]) == 4097
        assert ids[65:].tolist() == list(range(first + nt, first + nt + 4097))
        check_windows(res, stepped(ref, [np.arange(nt), np.arange(nt, nt + 4097)], topics, None, qt, qp, first))


@pytest.mark.parametrize("total", [4095, 4096, 4097])
def test_edge_segment_totals_then_a_window(total):
    """(ii) A first window of 4095 / 4096 / 4097 ids in all, then one more.
    (msg_window counts in whole row words of 64 messages: the totals are made
    of 64 topics of 64 messages, the last of them 63, or a 65th of one.)"""
    rng = np.random.default_rng(total)
    n, root, nt = 300, 3, 65
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    counts = [64] * 63 + [total - 4032 if total < 4097 else 64, 1 if total == 4097 else 0]
    assert sum(counts) == total
    topics = np.concatenate([np.full(c, t) for t, c in enumerate(counts)] + [np.zeros(10)]).astype(np.uint32)
    hop = tree_hops(parent, root, live)
    reached = [p for p in range(n) if p != root and hop[p] != 0xFF]
    peers = reached[:4] + [root]
    qt = np.repeat(np.arange(nt), len(peers)).astype(np.uint32)
    qp = np.tile(peers, nt).astype(np.uint32)
    with PE.Engine(n, nt, msg_window=64) as eng, PE.Engine(n, nt, msg_window=64) as ref:
        for e in (eng, ref):
            for t in range(nt):
                e.set_tree(t, root, parent)
            e.set_live(live)
        eng.sink_set(qt, qp)
        first = eng.publish(topics)
        st = eng.run()
        assert st.windows == 2
        res = eng.sink_take()
        n1 = sum(1 for c in counts if c)  # a list per topic in the first window, one in the second
        assert res[1].size - 1 == n1 + 1 and res[1][n1] == total and res[1][n1 + 1] == total + 10
        assert res[2][total:].tolist() == list(range(first + total, first + total + 10))
        chunks = window_chunks(topics, 64)
        check_windows(res, stepped(ref, chunks, topics, None, qt, qp, first))
        assert per_query(res) == closed_form(qt, qp, chunks, topics, None, first, hop, root)


def test_edge_many_lists_through_the_seam(monkeypatch):
    """(iii) PSAMD_AB=1 PSAMD_DRAIN_SHARED=private: a list per reached query,
    257 queries over three windows."""
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_DRAIN_SHARED", "private")
    rng = np.random.default_rng(63)
    n, root = 400, 1
    parent = random_tree(rng, n, root)
    topics = np.zeros(150, dtype=np.uint32)
    qp = rng.integers(0, n, size=257).astype(np.uint32)
    qp[11] = root
    qt = np.zeros(257, dtype=np.uint32)
    chunks = window_chunks(topics, 64)
    with PE.Engine(n, 1, msg_window=64) as eng, PE.Engine(n, 1, msg_window=64) as ref:
        eng.set_tree(0, root, parent)
        ref.set_tree(0, root, parent)
        eng.sink_set(qt, qp)
        first = eng.publish(topics)
        eng.run()
        res = eng.sink_take()
        n_reached = int(np.sum(qp != root))
        assert res[1].size - 1 == 3 * n_reached and res[2].size == 150 * n_reached
        check_windows(res, stepped(ref, chunks, topics, None, qt, qp, first))
        hop = tree_hops(parent, root, np.ones(n, dtype=np.uint8))
        assert per_query(res) == closed_form(qt, qp, chunks, topics, None, first, hop, root)


def test_edge_single_window_equals_drain_shared():
    """(iv) One window: the result is drain_shared's of that window exactly."""
    rng = np.random.default_rng(64)
    n, root = 500, 9
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.2).astype(np.uint8)
    live[root] = 1
    qp = rng.integers(0, n, size=333).astype(np.uint32)
    qt = (np.arange(333) % 2).astype(np.uint32)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        eng.sink_set(qt, qp)
        eng.publish(np.arange(200) % 2)
        eng.run()
        wl, off, ids = eng.sink_take()
        assert wl.shape == (1, 333)
        same((wl[0], off, ids), shared(eng, qt, qp))


def test_edge_nothing_resolves():
    """(v) Only the root and a peer outside the tree are asked for."""
    rng = np.random.default_rng(65)
    n, root, outside = 200, 0, 199
    parent = random_tree(rng, n, root)
    parent[parent == outside] = root
    parent[outside] = 0xFFFFFFFF
    with PE.Engine(n, 1, msg_window=64) as eng:
        eng.set_tree(0, root, parent)
        eng.sink_set([0, 0, 0], [root, outside, root])
        eng.publish(np.zeros(150))
        eng.run()
        wl, off, ids = eng.sink_take()
        assert wl.shape == (3, 3) and np.all(wl == NONE)
        assert off.tolist() == [0] and ids.size == 0


# ---- 5. layouts ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["unpaced", "paced0", "paced1", "compact"])
def test_tree_layouts(kind):
    kw, n, root, parent, live, topics, starts, peers = tree_case(kind)
    kw = dict(kw, msg_window=64)
    topics = np.asarray(topics, dtype=np.uint32)
    qt = np.repeat([0, 1], len(peers)).astype(np.uint32)
    qp = np.tile(peers, 2).astype(np.uint32)
    chunks = window_chunks(topics, 64)
    assert len(chunks) >= 2
    with PE.Engine(n, 2, **kw) as eng, PE.Engine(n, 2, **kw) as ref:
        for e in (eng, ref):
            e.set_tree(0, root, parent)
            e.set_tree(1, root, parent)
            e.set_live(live)
        eng.sink_set(qt, qp)
        first = eng.publish(topics, starts)
        st = eng.run()
        assert st.windows == len(chunks)
        res = eng.sink_take()
        check_windows(res, stepped(ref, chunks, topics, starts, qt, qp, first))
        hop = tree_hops(parent, root, live)
        got = per_query(res)
        assert got == closed_form(qt, qp, chunks, topics, starts, first, hop, root)
        assert sum(len(g) for g in got) > 0


@pytest.mark.parametrize("paced", [False, True])
def test_mesh(paced):
    """Two parents per node; paced: the arrival-order table, a private list
    per query with a row in every window (the gather lists)."""
    rng = np.random.default_rng(41 + paced)
    n, root, n_msgs = 800, 5, 300
    rp, cl = random_mesh2(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    starts = rng.integers(0, 5, size=n_msgs) if paced else None
    topics = np.zeros(n_msgs, dtype=np.uint32)
    chunks = window_chunks(topics, 128)
    qp = np.arange(n)
    qt = np.zeros(n, dtype=np.uint32)
    with PE.Engine(n, 1, msg_window=128) as eng, PE.Engine(n, 1, msg_window=128) as ref:
        for e in (eng, ref):
            e.set_children(0, root, rp, cl)
            e.set_live(live)
        eng.sink_set(qt, qp)
        first = eng.publish(topics, starts)
        eng.run()
        res = eng.sink_take()
        assert res[0].shape[0] == 3
        check_windows(res, stepped(ref, chunks, topics, starts, qt, qp, first))
        n_reached = int(np.sum(res[0][0] != NONE))
        assert n_reached > 100
        if paced:
            assert res[1].size - 1 == 3 * n_reached  # private lists
        else:
            assert res[1].size - 1 == 3 and res[2].size == n_msgs


# ---- 6. caps ---------------------------------------------------------------------------------

def test_caps():
    """600 queries over two topics, two windows: the engine's caps are four
    lists and 200 ids; either cap one short gives PS_E_RANGE with the exact
    fields; the exact caps pass."""
    rng = np.random.default_rng(81)
    n, root = 300, 0
    parent = random_tree(rng, n, root)
    qp = np.tile(np.arange(n), 2)
    qt = np.repeat([1, 0], n).astype(np.uint32)
    topics = (np.arange(200) % 2).astype(np.uint32)
    with PE.Engine(n, 2, msg_window=64) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.sink_set(qt, qp)
        f0 = eng.publish(topics)
        eng.run()
        want = eng.sink_take()
        n_lists, total = want[1].size - 1, want[2].size
        assert want[0].shape == (2, 600) and n_lists == 4 and total == 200
        assert want[1].tolist() == [0, 64, 128, 164, 200]

        def again(list_cap, id_cap):
            assert raw_set(eng, qt, qp, list_cap, id_cap) == 0
            f = eng.publish(topics)
            eng.run()
            return f, raw_take(eng, qt.size)

        f, (rc, wl, op, mp, nw, nl, tot) = again(n_lists - 1, total)
        assert rc == E_RANGE and nw == 2 and nl == n_lists and np.array_equal(wl, want[0])
        f, (rc, wl, op, mp, nw, nl, tot) = again(n_lists, total - 1)
        assert rc == E_RANGE and nw == 2 and nl == n_lists and tot == total and np.array_equal(wl, want[0])
        assert [op[i] for i in range(n_lists + 1)] == want[1].tolist()
        # (the first window fits and was emitted before the overflow)
        assert [mp[i] for i in range(128)] == (want[2][:128] - f0 + f).tolist()
        f, (rc, wl, op, mp, nw, nl, tot) = again(n_lists, total)
        assert rc == 0 and nw == 2 and nl == n_lists and tot == total and np.array_equal(wl, want[0])
        assert [op[i] for i in range(n_lists + 1)] == want[1].tolist()
        assert [mp[i] for i in range(total)] == (want[2] - f0 + f).tolist()
        eng.sink_set(qt, qp)  # the engine's own again
        f = eng.publish(topics)
        eng.run()
        got = eng.sink_take()
        same((got[0], got[1], got[2] - np.uint32(f - f0)), want)


# ---- 7. pipelined -----------------------------------------------------------------------------

def splitting_window(batches):
    """A msg_window (whole row words of 64) that splits at least one topic of every batch."""
    most = min(int(np.bincount(b).max()) for b in batches)
    assert most > 64
    return (most - 1) // 64 * 64


def even_batches(n_topics, n_batches, seed):
    """Every topic with 128 messages per batch, interleaved at random: at
    msg_window = 64 each batch is two windows of one shape, so the plan stays
    on the device and the windows may run beside each other.  (A batch that
    splits only some of its topics alternates between two window shapes, and
    no window overlaps its predecessor then -- with or without a sink: the
    `uneven` cases check the results alone.)"""
    rng = np.random.default_rng(seed)
    return [rng.permutation(np.repeat(np.arange(n_topics, dtype=np.uint32), 128)) for _ in range(n_batches)]


def sink_pipelined(e, batches):
    """publish; run_async; (wait; sink_take of the previous)."""
    views, res, over = [], [], 0
    for i, b in enumerate(batches):
        e.publish(b)
        e.run_async()
        if i:
            st = e.wait()
            res.append(stats_key(st))
            over += st.overlapped
            views.append(e.sink_take())
    st = e.wait()
    res.append(stats_key(st))
    over += st.overlapped
    views.append(e.sink_take())
    return views, res, over


def sink_blocking(e, batches):
    views, res = [], []
    for b in batches:
        e.publish(b)
        res.append(stats_key(e.run()))
        views.append(e.sink_take())
    return views, res


def compare_sink_runs(out, n_batches):
    assert sum(v[2].size for v in out[0][0]) > 0
    for i in range(n_batches):
        assert out[0][0][i][0].shape[0] >= 2  # the batch was split
        same(out[1][0][i], out[0][0][i])
    assert out[1][1] == out[0][1]
    assert out[1][2] == out[0][2]


def step_check(make, batches, which, cap, qt, qp, views):
    """Reference (a) for the batches `which`: a stepping engine fed every batch
    before, then that batch window by window."""
    with make() as ref:
        first = 0
        for i, b in enumerate(batches):
            if i in which:
                check_windows(views[i], stepped(ref, window_chunks(b, cap), b, None, qt, qp, first))
            else:
                ref.publish(b)
                ref.run()
            first += b.size
            if i == max(which):
                break


@pytest.mark.parametrize("kind", ["even", "uneven"])
def test_pipelined_twin_windows(kind):
    wl = WL.cfg3(60_000, 16, 4000)
    if kind == "even":
        batches, cap = even_batches(len(wl.topics), 12, 51), 64
    else:
        batches = [vary(wl.msg_topics, i, 5) for i in range(12)]
        cap = splitting_window(batches)
    rng = np.random.default_rng(5)
    qt = np.arange(300, dtype=np.uint32) % len(wl.topics)
    qp = np.array([rng.choice(wl.topics[int(t)].join_order) for t in qt], dtype=np.uint32)

    def make():
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=cap, plan={"flood": 0})
        WL.build_engine_topics(e, wl)
        return e

    out = []
    for mode in ("blocking", "pipelined"):
        with make() as e:
            e.sink_set(qt, qp)
            if mode == "blocking":
                views, res = sink_blocking(e, batches)
            else:
                views, res, over = sink_pipelined(e, batches)
                print("twin windows:", kind, "overlapped", over)
                if kind == "even":
                    assert over >= 6, over  # windows ran as twins
            out.append((views, res, e.seen_digest()))
    compare_sink_runs(out, 12)
    step_check(make, batches, {0, 7}, cap, qt, qp, out[1][0])


@pytest.mark.parametrize("kind", ["even", "uneven"])
def test_pipelined_deep_overlapped_windows(kind):
    wl = WL.cfg3(200_000, 16, 5000)
    rng = np.random.default_rng(11)
    live = (rng.random(wl.n_peers) >= 0.03).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    if kind == "even":
        batches, cap = even_batches(len(wl.topics), 8, 52), 64
    else:
        batches = [vary(wl.msg_topics, i, 7) for i in range(8)]
        cap = splitting_window(batches)

    def make():
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=cap, plan={"overlap_min_bytes": 0})
        WL.build_engine_topics(e, wl)
        e.set_live(live)
        return e

    out = []
    qt = qp = None
    for mode in ("blocking", "pipelined"):
        with make() as e:
            if qt is None:
                # each topic's root's children and the depth-2 nodes (the rows a
                # successor's prefix rewrites first), then random subscribers
                ts_, ps_ = [], []
                for t, spec in enumerate(wl.topics):
                    par = e.parents(t)
                    kids = np.nonzero(par == spec.root)[0]
                    kids = kids[kids != spec.root]
                    deep2 = np.nonzero(np.isin(par, kids))[0][:8]
                    some = rng.choice(spec.join_order, 6)
                    for p in list(kids) + list(deep2) + list(some):
                        ts_.append(t)
                        ps_.append(int(p))
                qt = np.array(ts_, dtype=np.uint32)
                qp = np.array(ps_, dtype=np.uint32)
            e.sink_set(qt, qp)
            if mode == "blocking":
                views, res = sink_blocking(e, batches)
                assert res[-1][2] >= 12  # a deep window (rounds)
            else:
                views, res, _ = sink_pipelined(e, batches)
                print("deep windows:", kind, "overlapped", e.overlapped_windows())
                if kind == "even":
                    assert e.overlapped_windows() >= 5
            out.append((views, res, e.seen_digest()))
    compare_sink_runs(out, 8)
    step_check(make, batches, {1, 6}, cap, qt, qp, out[1][0])


# ---- 8. rules -----------------------------------------------------------------------------------

def test_rules():
    rng = np.random.default_rng(82)
    n, root = 2000, 0
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1, msg_window=512, plan={"flood": 0}) as eng:
        eng.set_tree(0, root, parent)
        with pytest.raises(PE.EngineError) as ei:
            eng.sink_take()
        assert ei.value.code == E_NOTREADY  # no sink, no run
        qp = rng.choice(n, 300, replace=False)
        qp[7] = root
        qt = np.zeros(300, dtype=np.uint32)
        eng.sink_set(qt, qp)
        with pytest.raises(PE.EngineError) as ei:
            eng.sink_take()
        assert ei.value.code == E_NOTREADY  # no run yet
        firsts = []
        for _ in range(2):  # two runs enqueued and not taken
            firsts.append(eng.publish(np.zeros(1000)))
            eng.run_async()
        third = eng.publish(np.zeros(700))
        with pytest.raises(PE.EngineError) as ei:
            eng.run_async()  # the third: refused, its messages stay pending
        assert ei.value.code == E_STATE
        assert raw_set(eng, qt, qp) == E_STATE  # runs in flight
        eng.wait()
        eng.wait()
        with pytest.raises(PE.EngineError) as ei:
            eng.run()  # still both untaken
        assert ei.value.code == E_STATE
        with pytest.raises(PE.EngineError) as ei:
            eng.run_async()
        assert ei.value.code == E_STATE
        for first in firsts:
            wl, off, ids = eng.sink_take()
            assert wl.shape == (2, 300) and off.tolist() == [0, 512, 1000]
            assert ids.tolist() == list(range(first, first + 1000))
            assert np.array_equal(wl[0] == NONE, qp == root) and np.array_equal(wl[1] == NONE, qp == root)
        st = eng.run()  # the same messages, after a take
        assert st.windows == 2 and st.deliveries == 700 * (n - 1)
        wl, off, ids = eng.sink_take()
        assert off.tolist() == [0, 512, 700] and ids.tolist() == list(range(third, third + 700))
        # a range error keeps the old sink
        assert raw_set(eng, [0, 0], [5, n]) == E_RANGE
        assert raw_set(eng, [0, 1], [5, 5]) == E_RANGE
        first = eng.publish(np.zeros(100))
        eng.run()
        wl, off, ids = eng.sink_take()
        assert wl.shape == (1, 300) and ids.tolist() == list(range(first, first + 100))
        # setting discards what was not taken; clearing ends the sink
        eng.publish(np.zeros(100))
        eng.run()
        eng.sink_set(qt[:10], qp[:10])
        with pytest.raises(PE.EngineError) as ei:
            eng.sink_take()
        assert ei.value.code == E_NOTREADY
        eng.sink_set([], [])
        eng.publish(np.zeros(100))
        eng.run()
        with pytest.raises(PE.EngineError) as ei:
            eng.sink_take()
        assert ei.value.code == E_NOTREADY
        # a run without a message: a valid, empty result
        eng.sink_set(qt, qp)
        eng.run()
        wl, off, ids = eng.sink_take()
        assert wl.shape == (0, 300) and off.tolist() == [0] and ids.size == 0


def test_view_lifetime():
    wl = WL.cfg3(60_000, 16, 4000)
    batches = [vary(wl.msg_topics, i, 5) for i in range(4)]
    rng = np.random.default_rng(6)
    qt = np.arange(200, dtype=np.uint32) % len(wl.topics)
    qp = np.array([rng.choice(wl.topics[int(t)].join_order) for t in qt], dtype=np.uint32)
    with PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=splitting_window(batches),
                   plan={"flood": 0}) as e:
        WL.build_engine_topics(e, wl)
        e.sink_set(qt, qp)
        for i in range(3):
            e.publish(batches[i])
            e.run_async()
            e.wait()
            view = e.sink_take(copy=False)
            kept = [x.copy() for x in view]
            assert kept[2].size > 0 and kept[0].shape[0] >= 2
            e.publish(batches[i + 1])
            e.run_async()  # the first run after its own: the view stays
            same(view, kept)
            e.wait()
            same(view, kept)
            e.sink_take()


def test_mixed_with_last_window_reads():
    """The sink beside drain_shared_begin / _end, drain and peer_messages of
    the last window: all agree, and the drains' slots are their own."""
    rng = np.random.default_rng(91)
    n, root = 2000, 4
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    qp = rng.choice(n, 250, replace=False)
    qt = np.zeros(250, dtype=np.uint32)
    with PE.Engine(n, 1, msg_window=256, plan={"flood": 0}) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.sink_set(qt, qp)
        first = eng.publish(np.zeros(700))
        eng.run_async()
        eng.drain_shared_begin(qt, qp)
        eng.drain_begin(qt, qp)
        last = drain_lists(eng, qt, qp)
        assert per_peer(eng, qt[:40], qp[:40]) == last[:40]
        sync = shared(eng, qt, qp)
        eng.wait()
        res = eng.sink_take()
        assert res[0].shape == (3, 250)
        wl, off, ids = res
        base = (off.size - 1) - (sync[1].size - 1)  # the lists of the windows before the last
        assert np.array_equal(wl[2], np.where(sync[0] == NONE, NONE, sync[0] + np.uint32(base)))
        assert np.array_equal(off[base:] - off[base], sync[1]) and np.array_equal(ids[int(off[base]):], sync[2])
        same(eng.drain_shared_end(), sync)
        assert split(*eng.drain_end()) == last
        assert expand(*sync) == last
        hop = tree_hops(parent, root, live)
        topics = np.zeros(700, dtype=np.uint32)
        assert per_query(res) == closed_form(qt, qp, window_chunks(topics, 256), topics, None, first, hop, root)


def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(3)]
    try:
        # an engine whose sink is set takes no ranks
        engines[2].sink_set([0], [5])
        with pytest.raises(PE.EngineError) as ei:
            engines[2].dist_init_loopback(lb, 0, PE.PART_PEER)
        assert ei.value.code == E_STATE
        for r, e in enumerate(engines[:2]):
            e.dist_init_loopback(lb, r, PE.PART_PEER)
            e.set_tree(0, root, parent)
            assert raw_set(e, [0, 0], [5, 6]) == E_STATE  # one rank only
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
            rc, _, _, _, nw, nl, tot = raw_take(e, 2)
            assert rc == E_NOTREADY and nw == 0xAAAA and nl == 0xBBBB and tot == 0xCCCC
    finally:
        for e in engines:
            e.close()
        lb.close()
