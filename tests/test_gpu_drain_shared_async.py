"""GPU: the shared drain in two halves (ps_drain_shared_begin /
ps_drain_shared_end) -- ps_drain_shared's answer enqueued
behind a run that may still execute, its lists numbered and laid out on the
device.  The comparison is always the triple (list_of_query, list_off, ids)
against Engine.drain_shared of the same window, entry for entry: on a quiet
engine the same engine's, in the pipelined cases a second, blocking
engine's.  Where a case has an oracle, the expanded lists are compared with
Engine.drain and the oracle as well, as test_gpu_drain_shared.py does."""
import ctypes as C
import threading

import numpy as np
import pytest

import psengine as PE
from psengine import workloads as WL
from test_gpu_drain_async import per_peer, stats_key, vary
from test_gpu_drain_batch import drain_lists, oracle_lists, random_mesh2, random_tree, split, tree_hops
from test_gpu_drain_shared import NONE, check_sharing, expand, run_tree_case, shared

pytestmark = pytest.mark.gpu

U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_STATE, E_RANGE, E_NOTREADY = -3, -7, -8


def same(got, want):
    """The triple, entry for entry."""
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def shared_async(eng, qt, qp, list_cap=0, id_cap=0):
    eng.drain_shared_begin(qt, qp, list_cap, id_cap)
    return eng.drain_shared_end()


def raw_begin(eng, qt, qp, list_cap=0, id_cap=0):
    qt = np.ascontiguousarray(qt, dtype=np.uint32)
    qp = np.ascontiguousarray(qp, dtype=np.uint32)
    return eng._L.ps_drain_shared_begin(eng._h, qt.ctypes.data_as(U32P), qp.ctypes.data_as(U32P), qt.size, list_cap,
                                        id_cap)


def raw_end(eng, n):
    """(rc, list_of_query copy, list_off pointer, n_lists, total)."""
    lp, op, mp = U32P(), U64P(), U32P()
    n_lists, total = C.c_uint32(0xBBBB), C.c_uint64(0xCCCC)
    rc = eng._L.ps_drain_shared_end(eng._h, C.byref(lp), C.byref(op), C.byref(mp), C.byref(n_lists), C.byref(total))
    lists = np.ctypeslib.as_array(lp, shape=(n,)).copy() if lp and n else np.empty(0, dtype=np.uint32)
    return rc, lists, op, n_lists.value, total.value


def check_quiet(eng, qt, qp, exp=None):
    """The asynchronous call first (it builds the window's tables on the
    device), then drain_shared and drain of the same window."""
    got = shared_async(eng, qt, qp)
    want = shared(eng, qt, qp)
    same(got, want)
    lists = expand(*got)
    assert lists == drain_lists(eng, qt, qp)
    if exp is not None:
        assert lists == exp
    return got


# ---- 1. layouts, quiet engine ---------------------------------------------------

@pytest.mark.parametrize("kind", ["unpaced", "paced0", "paced1", "compact"])
def test_tree_layouts(kind):
    eng, qt, qp, topics, hop, root, exp = run_tree_case(kind)
    with eng:
        got = check_quiet(eng, qt, qp, exp)
        check_sharing(got, qt, qp, topics, hop, root)


@pytest.mark.parametrize("paced", [False, True])
def test_mesh(paced):
    """Two parents per node.  Unpaced: a mask-layout table, classified like a
    tree's.  Paced: the arrival-order table -- a private list per query with
    a row, each numbered and laid out by the assignment passes."""
    rng = np.random.default_rng(41 + paced)
    n, root, n_msgs = 1500, 5, 300
    rp, cl = random_mesh2(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    starts = rng.integers(0, 5, size=n_msgs) if paced else None
    with PE.Engine(n, 1) as eng:
        eng.set_children(0, root, rp, cl)
        eng.set_live(live)
        eng.publish(np.zeros(n_msgs), starts)
        eng.run()
        qp = np.arange(n)
        qt = np.zeros(n, dtype=np.uint32)
        lists, off, ids = check_quiet(eng, qt, qp)
        n_reached = int(np.sum(lists != NONE))
        assert n_reached > 100
        if paced:
            assert off.size - 1 == n_reached and ids.size > n_msgs  # private lists
        else:  # a static live mask: whoever is reached holds every message
            assert off.size - 1 == 1 and ids.size == n_msgs


# ---- 2. numbering edges of the assignment kernels ------------------------------------

ORDER = (3, 1, 4, 0, 2)  # the topic of query i is ORDER[i % 5]: topic 3 is used first


@pytest.fixture(scope="module")
def small_tree():
    """Five topics over one tree of 400 peers, one of them outside it; a
    second window with a depth-1 node dead, so that the rows below it are
    stale.  Yields (engine, peer pattern): every topic's queries read, in
    order, the root, the outsider and a stale row before the first full row,
    and repeat peers afterwards."""
    rng = np.random.default_rng(7)
    n, root, outside = 400, 6, 399
    parent = random_tree(rng, n, root)
    parent[parent == outside] = root
    parent[outside] = 0xFFFFFFFF
    top = {}
    for p in range(n):
        q = p
        while p != outside and q != root and parent[q] != root:
            q = int(parent[q])
        top.setdefault(q, []).append(p)
    cut = max((k for k in top if k not in (root, outside)), key=lambda k: len(top[k]))
    stale = [p for p in top[cut] if p != cut]
    assert len(stale) >= 3
    good = [p for p in range(n) if p not in (root, outside, cut) and p not in stale]
    msg_topics = np.concatenate([np.full(c, t) for t, c in enumerate((10, 70, 64, 65, 130))]).astype(np.uint32)
    eng = PE.Engine(n, 5)
    for t in range(5):
        eng.set_tree(t, root, parent)
    eng.publish(msg_topics)
    eng.run()
    live = np.ones(n, dtype=np.uint8)
    live[cut] = 0
    eng.set_live(live)
    eng.publish(msg_topics)
    eng.run()
    pattern = [root, outside, stale[0], good[0], good[1], good[0], stale[1], cut, good[2], good[2], good[3], stale[2]]
    pattern += [int(p) for p in rng.choice(good, 40)]
    yield eng, pattern, set(good)
    eng.close()


def small_queries(pattern, n):
    i = np.arange(n)
    qt = np.array(ORDER, dtype=np.uint32)[i % 5]
    qp = np.array(pattern, dtype=np.uint32)[(i // 5) % len(pattern)]
    return qt, qp


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257, 5000])
def test_numbering_edges(small_tree, n):
    eng, pattern, good = small_tree
    qt, qp = small_queries(pattern, n)
    lists, off, ids = check_quiet(eng, qt, qp)
    if n == 0:
        assert lists.size == 0 and off.tolist() == [0] and ids.size == 0
        return
    # what the pattern promises: a list exactly where the peer was reached, one
    # per topic, numbered by the topic's first reached query
    reached = np.array([int(p) in good for p in qp])
    assert np.array_equal(lists != NONE, reached)
    first_use = []
    for t, r in zip(qt, reached):
        if r and int(t) not in first_use:
            first_use.append(int(t))
    assert off.size - 1 == len(first_use)
    assert np.array_equal(lists[reached], [first_use.index(int(t)) for t in qt[reached]])
    if n >= 63:
        assert first_use == list(ORDER)  # topic 3 first, after three empty queries of every topic


# ---- 3. widths -------------------------------------------------------------------------

def one_topic(seed):
    rng = np.random.default_rng(seed)
    n, root = 300, 3
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    return n, root, parent, live


def test_mixed_widths_in_one_call():
    """Rows of 1, 64, 65 and 130 words side by side, the queries interleaved:
    narrow bins and wide bins in one classify launch, lists of one, two and
    three segments in one numbering scan."""
    n, root, parent, live = one_topic(77)
    counts = (10, 4096, 4097, 8300)
    topics = np.concatenate([np.full(c, t) for t, c in enumerate(counts)]).astype(np.uint32)
    with PE.Engine(n, 4) as eng:
        for t in range(4):
            eng.set_tree(t, root, parent)
        eng.set_live(live)
        first = eng.publish(topics)
        eng.run()
        qt = np.tile([2, 0, 3, 1], n).astype(np.uint32)
        qp = np.repeat(np.arange(n), 4).astype(np.uint32)
        hop = tree_hops(parent, root, live)
        got = check_quiet(eng, qt, qp, oracle_lists(qt, qp, topics, None, first, hop, root))
        check_sharing(got, qt, qp, topics, hop, root)
        assert got[1].size - 1 == 4 and got[2].size == sum(counts)


@pytest.mark.parametrize("n_msgs", [4095, 4096, 4097])
def test_segment_edges(n_msgs):
    """A list of one segment, of exactly one, and of two."""
    n, root, parent, live = one_topic(n_msgs)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        first = eng.publish(np.zeros(n_msgs))
        eng.run()
        qp = np.arange(n)
        qt = np.zeros(n, dtype=np.uint32)
        hop = tree_hops(parent, root, live)
        got = check_quiet(eng, qt, qp, oracle_lists(qt, qp, np.zeros(n_msgs), None, first, hop, root))
        assert got[1].tolist() == [0, n_msgs] and got[2].tolist() == list(range(first, first + n_msgs))


# ---- 4. the private path through the seam ------------------------------------------------

@pytest.mark.parametrize("kind", ["unpaced", "paced1"])
def test_private_path_through_the_seam(kind, monkeypatch):
    """PSAMD_AB=1 PSAMD_DRAIN_SHARED=private: a full row takes a list of its
    own, so the assignment numbers one list per reached query and count /
    scan / emit read the rows; explicit caps."""
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_DRAIN_SHARED", "private")
    eng, qt, qp, topics, hop, root, exp = run_tree_case(kind)
    with eng:
        n_reached = sum(1 for x in exp if x)
        n_ids = sum(len(x) for x in exp)
        assert n_reached > 100
        got = shared_async(eng, qt, qp, list_cap=n_reached, id_cap=n_ids)
        same(got, shared(eng, qt, qp))
        lists, off, ids = got
        assert off.size - 1 == n_reached and ids.size == n_ids
        assert np.array_equal(lists[lists != NONE], np.arange(n_reached))
        assert expand(*got) == drain_lists(eng, qt, qp) == exp
        same(shared_async(eng, qt, qp, list_cap=len(qt), id_cap=n_ids + 1000), got)  # room to spare


# ---- 5. caps ---------------------------------------------------------------------------

def caps_case():
    rng = np.random.default_rng(81)
    n, root = 300, 0
    parent = random_tree(rng, n, root)
    eng = PE.Engine(n, 2)
    eng.set_tree(0, root, parent)
    eng.set_tree(1, root, parent)
    eng.publish(np.arange(100) % 2)
    eng.run()
    qp = np.tile(np.arange(n), 2)
    qt = np.repeat([1, 0], n).astype(np.uint32)
    return eng, qt, qp


def test_default_caps_hold_many_queries_per_topic():
    """600 queries over two topics: the default caps are two lists and 100
    ids, and the answer -- the synchronous call's -- fits them exactly."""
    eng, qt, qp = caps_case()
    with eng:
        want = shared(eng, qt, qp)
        assert want[1].size - 1 == 2 and want[2].size == 100
        same(shared_async(eng, qt, qp), want)
        assert raw_begin(eng, qt, qp) == 0
        rc, lists, _, n_lists, total = raw_end(eng, qt.size)
        assert rc == 0 and n_lists == 2 and total == 100 and np.array_equal(lists, want[0])
        # the same caps given explicitly, and either of them one short
        same(shared_async(eng, qt, qp, 2, 100), want)
        assert raw_begin(eng, qt, qp, 1, 100) == 0
        rc, lists, _, n_lists, total = raw_end(eng, qt.size)
        assert rc == E_RANGE and n_lists == 2 and np.array_equal(lists, want[0])
        assert raw_begin(eng, qt, qp, 2, 99) == 0
        rc, lists, op, n_lists, total = raw_end(eng, qt.size)
        assert rc == E_RANGE and n_lists == 2 and total == 100 and np.array_equal(lists, want[0])
        assert [op[i] for i in range(3)] == [0, 50, 100]
        same(shared_async(eng, qt, qp), want)


def test_caps_one_short_through_the_seam(monkeypatch):
    """Private lists, so that the counts are large: list_cap one short and
    id_cap one short each give PS_E_RANGE with the list numbers and counts
    exact, nothing written past a cap, and a following drain of the same
    window with room is correct."""
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_DRAIN_SHARED", "private")
    eng, qt, qp = caps_case()
    with eng:
        want = shared(eng, qt, qp)
        n_lists, total = want[1].size - 1, want[2].size
        assert n_lists == 2 * 299 and total == 299 * 100
        assert raw_begin(eng, qt, qp, n_lists - 1, total) == 0
        rc, lists, _, got_lists, _ = raw_end(eng, qt.size)
        assert rc == E_RANGE and got_lists == n_lists and np.array_equal(lists, want[0])
        same(shared_async(eng, qt, qp, n_lists, total), want)
        assert raw_begin(eng, qt, qp, n_lists, total - 1) == 0
        rc, lists, op, got_lists, got_total = raw_end(eng, qt.size)
        assert rc == E_RANGE and got_lists == n_lists and got_total == total and np.array_equal(lists, want[0])
        assert np.array_equal(np.ctypeslib.as_array(op, shape=(n_lists + 1,)), want[1])
        same(shared_async(eng, qt, qp, n_lists, total), want)
        same(shared_async(eng, qt, qp), want)  # (under the seam the default is one list per row)
        assert expand(*want) == drain_lists(eng, qt, qp)


def test_refused_after_staging_takes_no_slot():
    """An id_cap above 2^30 is refused after the window's table block was
    staged in the slot: the call gives the slot up.  The next begin finds the
    tables kept and writes its input where that block lay; both slots are
    still free, and both views are the synchronous call's."""
    rng = np.random.default_rng(17)
    n, root, n_msgs = 40, 2, 50
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        first = eng.publish(np.zeros(n_msgs))
        eng.run()  # (no drain yet: the window's tables are not built)
        qp = np.arange(n)
        qt = np.zeros(n, dtype=np.uint32)
        assert raw_begin(eng, qt, qp, 1, (1 << 30) + 1) == E_RANGE
        eng.drain_shared_begin(qt, qp)
        eng.drain_shared_begin(qt, qp)
        assert raw_begin(eng, qt, qp) == E_STATE  # both slots taken: the refused call took none
        got = [eng.drain_shared_end(), eng.drain_shared_end()]
        want = shared(eng, qt, qp)
        assert want[1].tolist() == [0, n_msgs] and want[2].tolist() == list(range(first, first + n_msgs))
        for g in got:
            same(g, want)


# ---- 6. pipelined ------------------------------------------------------------------------

def pipelined(e, batches, qt, qp):
    """publish, run_async, drain_shared_begin, (wait, drain_shared_end of the previous)."""
    views, res, over = [], [], 0
    for i, b in enumerate(batches):
        e.publish(b)
        e.run_async()
        e.drain_shared_begin(qt, qp)
        if i:
            st = e.wait()
            res.append(stats_key(st))
            over += st.overlapped
            views.append(e.drain_shared_end())
    st = e.wait()
    res.append(stats_key(st))
    over += st.overlapped
    views.append(e.drain_shared_end())
    return views, res, over


def blocking(e, batches, qt, qp):
    views, res = [], []
    for b in batches:
        e.publish(b)
        res.append(stats_key(e.run()))
        views.append(e.drain_shared(qt, qp))
    return views, res


def compare_runs(out, n_batches):
    assert sum(v[2].size for v in out[0][0]) > 0
    for i in range(n_batches):
        same(out[1][0][i], out[0][0][i])
    assert out[1][1] == out[0][1]
    assert out[1][2] == out[0][2]


def test_pipelined_twin_windows():
    wl = WL.cfg3(60_000, 16, 4000)
    batches = [vary(wl.msg_topics, i, 5) for i in range(12)]
    rng = np.random.default_rng(5)
    qt = np.arange(300, dtype=np.uint32) % len(wl.topics)
    qp = np.array([rng.choice(wl.topics[int(t)].join_order) for t in qt], dtype=np.uint32)
    out = []
    for mode in ("blocking", "pipelined"):
        with PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, plan={"flood": 0}) as e:  # (k_flood windows run no twins)
            WL.build_engine_topics(e, wl)
            if mode == "blocking":
                views, res = blocking(e, batches, qt, qp)
            else:
                views, res, over = pipelined(e, batches, qt, qp)
                assert over >= 6, over  # windows ran as twins
            out.append((views, res, e.seen_digest()))
    compare_runs(out, 12)


def test_pipelined_deep_overlapped_windows():
    wl = WL.cfg3(200_000, 16, 5000)
    rng = np.random.default_rng(11)
    live = (rng.random(wl.n_peers) >= 0.03).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    batches = [vary(wl.msg_topics, i, 7) for i in range(8)]
    out = []
    qt = qp = None
    for mode in ("blocking", "pipelined"):
        with PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, plan={"overlap_min_bytes": 0}) as e:
            WL.build_engine_topics(e, wl)
            e.set_live(live)
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
            if mode == "blocking":
                views, res = blocking(e, batches, qt, qp)
                assert res[-1][2] >= 12  # a deep window (rounds)
            else:
                views, res, _ = pipelined(e, batches, qt, qp)
                assert e.overlapped_windows() >= 5
            out.append((views, res, e.seen_digest()))
    compare_runs(out, 8)


# ---- 7. slots and lifetime ---------------------------------------------------------------

def test_slot_rules_and_mixed_kinds():
    rng = np.random.default_rng(81)
    n, root = 2000, 0
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1, plan={"flood": 0}) as eng:
        eng.set_tree(0, root, parent)
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_shared_begin([0], [5])
        assert ei.value.code == E_NOTREADY  # no run yet
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_shared_end()
        assert ei.value.code == E_NOTREADY  # none outstanding
        qp = rng.choice(n, 300, replace=False)
        qp[7] = root
        qt = np.zeros(300, dtype=np.uint32)
        firsts = []
        for _ in range(2):  # two runs enqueued, a drain begun behind each before any wait
            firsts.append(eng.publish(np.zeros(1000)))
            eng.run_async()
            eng.drain_shared_begin(qt, qp)
        assert raw_begin(eng, qt, qp) == E_STATE  # a third of this kind
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_begin(qt, qp)  # ... or of the other
        assert ei.value.code == E_STATE
        eng.wait()
        eng.wait()
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_end()  # the wrong kind: completes nothing
        assert ei.value.code == E_STATE
        for first in firsts:
            lists, off, ids = eng.drain_shared_end()
            assert off.tolist() == [0, 1000] and ids.tolist() == list(range(first, first + 1000))
            assert all(l == (NONE if p == root else 0) for p, l in zip(qp, lists))
        assert raw_begin(eng, [0, 0], [5, n]) == E_RANGE  # a peer out of range
        assert raw_begin(eng, [0, 1], [5, 5]) == E_RANGE  # a topic out of range
        # no slot leaked: two more fit, one of each kind, ended in order
        want = shared(eng, qt, qp)
        eng.drain_begin(qt, qp)
        eng.drain_shared_begin(qt, qp)
        assert raw_begin(eng, qt, qp) == E_STATE
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_shared_end()  # the oldest is a plain drain
        assert ei.value.code == E_STATE
        plain = split(*eng.drain_end())
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_end()  # the oldest is a shared one now
        assert ei.value.code == E_STATE
        got = eng.drain_shared_end()
        same(got, want)
        assert expand(*got) == plain == per_peer(eng, qt, qp)
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_shared_end()
        assert ei.value.code == E_NOTREADY
        # the other order, an empty drain, the root alone
        eng.drain_shared_begin([], [])
        eng.drain_begin(qt, qp)
        lists, off, ids = eng.drain_shared_end()
        assert lists.size == 0 and off.tolist() == [0] and ids.size == 0
        assert split(*eng.drain_end()) == plain
        lists, off, ids = shared_async(eng, [0, 0], [root, root])
        assert lists.tolist() == [NONE, NONE] and off.tolist() == [0] and ids.size == 0


def test_view_lifetime():
    wl = WL.cfg3(60_000, 16, 4000)
    batches = [vary(wl.msg_topics, i, 5) for i in range(4)]
    rng = np.random.default_rng(6)
    qt = np.arange(200, dtype=np.uint32) % len(wl.topics)
    qp = np.array([rng.choice(wl.topics[int(t)].join_order) for t in qt], dtype=np.uint32)
    with PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, plan={"flood": 0}) as e:
        WL.build_engine_topics(e, wl)
        for i in range(3):
            e.publish(batches[i])
            e.run_async()
            e.drain_shared_begin(qt, qp)
            e.wait()
            view = e.drain_shared_end(copy=False)
            kept = [x.copy() for x in view]
            assert kept[2].size > 0
            e.publish(batches[i + 1])
            e.run_async()
            same(view, kept)
            e.wait()
            same(view, kept)


def test_mixed_with_synchronous_calls():
    """The device-built tables serve drain, drain_shared and peer_messages of
    the same window while the drain is outstanding; and tables the host built
    serve the asynchronous call."""
    rng = np.random.default_rng(91)
    n, root = 2000, 4
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    qp = rng.choice(n, 250, replace=False)
    qt = np.zeros(250, dtype=np.uint32)
    with PE.Engine(n, 1, plan={"flood": 0}) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        first = eng.publish(np.zeros(700))
        eng.run_async()
        eng.drain_shared_begin(qt, qp)  # (builds the tables on the device)
        hop = tree_hops(parent, root, live)
        want = oracle_lists(qt, qp, np.zeros(700), None, first, hop, root)
        assert drain_lists(eng, qt, qp) == want
        sync = shared(eng, qt, qp)
        assert expand(*sync) == want
        assert per_peer(eng, qt[:40], qp[:40]) == want[:40]
        eng.wait()
        same(eng.drain_shared_end(), sync)
        # a live-mask change and a further run between begin and end: the view is batch k's
        first = eng.publish(np.zeros(650))
        eng.run_async()
        eng.drain_shared_begin(qt, qp)
        want = oracle_lists(qt, qp, np.zeros(650), None, first, hop, root)
        live2 = (rng.random(n) > 0.3).astype(np.uint8)
        live2[root] = 1
        eng.set_live(live2)
        eng.wait()
        first2 = eng.publish(np.zeros(100))
        eng.run()
        digest = eng.seen_digest()
        assert expand(*eng.drain_shared_end()) == want
        want2 = oracle_lists(qt, qp, np.zeros(100), None, first2, tree_hops(parent, root, live2), root)
        assert want2 != want
        sync = shared(eng, qt, qp)  # (builds this window's tables on the host)
        assert expand(*sync) == want2
        same(shared_async(eng, qt, qp), sync)
        assert eng.seen_digest() == digest


def test_last_window_only():
    rng = np.random.default_rng(61)
    n, root = 400, 2
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1, msg_window=128) as eng:
        eng.set_tree(0, root, parent)
        first = eng.publish(np.zeros(300))
        eng.run()
        qp = np.arange(n)
        qt = np.zeros(n, dtype=np.uint32)
        lists, off, ids = check_quiet(eng, qt, qp)
        assert off.size - 1 == 1 and 0 < ids.size <= 128
        assert ids.tolist() == list(range(int(ids[0]), first + 300))  # one window, ending with the run's last message
        assert lists[root] == NONE and np.sum(lists == 0) == n - 1


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
            assert raw_begin(e, [0, 0], [5, 6]) == E_STATE  # one rank only
            rc, _, _, n_lists, total = raw_end(e, 2)
            assert rc == E_NOTREADY and n_lists == 0xBBBB and total == 0xCCCC  # no slot was taken
            assert sum(len(x) for x in drain_lists(e, [0, 0], [5, 6])) in (0, 50, 100)  # (ps_drain still serves it)
    finally:
        for e in engines:
            e.close()
        lb.close()
