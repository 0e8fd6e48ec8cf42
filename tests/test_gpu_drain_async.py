"""GPU: the drain in two halves (ps_drain_begin / ps_drain_end, DESIGN.md
§5.5b) -- the batched drain enqueued behind a run that may still execute,
its result lent from pinned memory, while the next run floods.  Every
comparison is list for list: against drain() (ps_drain, whose tables the host
builds), against peer_messages() (the one-subscriber path) and, where a case
says so, against the oracle's hops the way test_gpu_drain_batch.py does.
The pipelined cases compare every batch's view with a second, blocking
engine's run(); drain() of the same batch."""
import threading

import numpy as np
import pytest

import oracle as O
import psengine as PE
from psengine import workloads as WL

pytestmark = pytest.mark.gpu


def random_tree(rng, n, root):
    perm = rng.permutation(n)
    perm = np.concatenate([[root], perm[perm != root]])
    parent = np.full(n, O.NONE, dtype=np.uint32)
    for i in range(1, n):
        parent[perm[i]] = perm[rng.integers(0, i)]
    return parent


def random_mesh2(rng, n, root):
    """Child lists (CSR) in which every node but the first few has two parents."""
    perm = rng.permutation(n)
    perm = np.concatenate([[root], perm[perm != root]])
    kids = [[] for _ in range(n)]
    for i in range(1, n):
        for p in set(int(x) for x in rng.integers(0, i, size=2)):
            kids[perm[p]].append(int(perm[i]))
    rp = np.zeros(n + 1, dtype=np.uint32)
    rp[1:] = np.cumsum([len(k) for k in kids])
    cl = np.array([c for k in kids for c in k], dtype=np.uint32)
    return rp, cl


def tree_hops(parent, root, live):
    rp, cl = O.parents_to_csr(parent)
    _, ohops, _ = O.disseminate(rp, cl, root, live, 1)
    return ohops[0]


def split(off, ids):
    assert off.dtype == np.uint64 and ids.dtype == np.uint32
    assert off[0] == 0 and off[-1] == ids.size and np.all(np.diff(off.astype(np.int64)) >= 0)
    return [ids[int(off[q]):int(off[q + 1])].tolist() for q in range(off.size - 1)]


def drain_lists(eng, qt, qp):
    return split(*eng.drain(qt, qp))


def async_lists(eng, qt, qp):
    eng.drain_begin(qt, qp)
    return split(*eng.drain_end())


def per_peer(eng, qt, qp):
    return [eng.peer_messages(int(t), int(p)).tolist() for t, p in zip(qt, qp)]


def oracle_lists(qt, qp, topics, starts, first, hop, root):
    """Expected drains of queries over topics that share one tree."""
    starts = np.zeros(len(topics), dtype=np.int64) if starts is None else starts
    by_topic = {}
    for t in set(int(x) for x in qt):
        ids = [m for m in range(len(topics)) if topics[m] == t]
        by_topic[t] = [first + m for m in sorted(ids, key=lambda m: (int(starts[m]), m))]
    return [[] if p == root or hop[p] == 0xFF else by_topic[int(t)] for t, p in zip(qt, qp)]


def stats_key(st):
    d = st.as_dict()
    return (st.deliveries, st.duplicates, st.rounds, st.windows, tuple(d["deliveries_per_round"]))


def check_all(eng, qt, qp, want=None):
    """The asynchronous drain first (it builds the window's tables on the
    device), then drain() and peer_messages() of the same window."""
    got = async_lists(eng, qt, qp)
    assert got == drain_lists(eng, qt, qp)
    assert got == per_peer(eng, qt, qp)
    if want is not None:
        assert got == want
    return got


# ---- 1. layouts, quiet engine ---------------------------------------------------

def test_oracle_unpaced():
    rng = np.random.default_rng(21)
    n, root, n_msgs = 2500, 7, 300
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    outside = 2499 if root != 2499 else 2498
    parent[parent == outside] = root  # a peer outside the tree: its children move to the root
    parent[outside] = O.NONE
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        topics = np.arange(n_msgs) % 2
        first = eng.publish(topics)
        eng.run()
        hop = tree_hops(parent, root, live)
        peers = [int(p) for p in rng.choice(n, 200, replace=False)] + [root, outside]
        qt = np.repeat([0, 1], len(peers))
        qp = np.tile(peers, 2)
        got = check_all(eng, qt, qp, oracle_lists(qt, qp, topics, None, first, hop, root))
        assert got[len(peers) - 1] == [] and got[len(peers) - 2] == []


@pytest.mark.parametrize("aligned", [0, 1])
def test_paced_both_layouts(aligned):
    rng = np.random.default_rng(31 + aligned)
    n, root, n_msgs = 1500, 11, 300
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    starts = rng.integers(0, 5, size=n_msgs)
    with PE.Engine(n, 2, plan=None if aligned else {"align_groups": 0}) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        topics = np.arange(n_msgs) % 2
        first = eng.publish(topics, starts)
        st = eng.run()
        assert st.level_aligned == aligned
        peers = [int(p) for p in rng.choice(n, 150, replace=False)] + [root]
        qt = np.repeat([0, 1], len(peers))
        qp = np.tile(peers, 2)
        hop = tree_hops(parent, root, live)
        check_all(eng, qt, qp, oracle_lists(qt, qp, topics, starts, first, hop, root))


def test_paced_compaction_path():
    rng = np.random.default_rng(37)
    n, root, n_msgs = 700, 2, 200
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    starts = rng.integers(0, 5, size=n_msgs)
    with PE.Engine(n, 2, flags=PE.F_COMPACT) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        topics = np.arange(n_msgs) % 2
        first = eng.publish(topics, starts)
        eng.run()
        qp = np.tile(np.arange(n), 2)
        qt = np.repeat([0, 1], n)
        hop = tree_hops(parent, root, live)
        check_all(eng, qt, qp, oracle_lists(qt, qp, topics, starts, first, hop, root))


@pytest.mark.parametrize("paced", [False, True])
def test_mesh(paced):
    """Two parents per node.  Unpaced: the device-built table; paced: the
    host's arrival-order table (the row is in window order)."""
    rng = np.random.default_rng(41 + paced)
    n, root, n_msgs = 800, 5, 300
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
        got = check_all(eng, qt, qp)
        assert sum(len(g) for g in got) > n_msgs  # (somebody was reached)
        if paced:
            full = max(got, key=len)
            assert full != sorted(full)  # arrival order differs from id order


def test_dead_subtree_stale_rows():
    """A live mask that cuts a subtree at depth 1 after a first window reached
    it: the rows below the cut keep the first window's bits under a stale
    generation, and drain empty."""
    rng = np.random.default_rng(51)
    n, root = 600, 0
    parent = random_tree(rng, n, root)
    top = np.full(n, -1, dtype=np.int64)  # the depth-1 ancestor of every peer
    for p in range(n):
        q = p
        while q != root and parent[q] != root:
            q = int(parent[q])
        top[p] = q
    sizes = {}
    for p in range(n):
        if p != root:
            sizes[int(top[p])] = sizes.get(int(top[p]), 0) + 1
    cut = max(sizes, key=sizes.get)
    below = [p for p in range(n) if p != root and top[p] == cut and p != cut]
    assert len(below) >= 10
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.publish(np.zeros(200))
        eng.run()
        qp = np.arange(n)
        qt = np.zeros(n, dtype=np.uint32)
        assert all(len(g) == 200 for q, g in enumerate(async_lists(eng, qt, qp)) if q != root)
        live = np.ones(n, dtype=np.uint8)
        live[cut] = 0
        eng.set_live(live)
        first = eng.publish(np.zeros(150))
        eng.run()
        hop = tree_hops(parent, root, live)
        got = check_all(eng, qt, qp, oracle_lists(qt, qp, np.zeros(150), None, first, hop, root))
        for p in below + [cut]:
            assert got[p] == []
        assert sum(1 for g in got if g) == n - 2 - len(below)


# ---- 2. table edges ---------------------------------------------------------------

@pytest.mark.parametrize("n_msgs", [1, 63, 64, 65, 4095, 4096, 4097, 8300])
def test_table_edges(n_msgs):
    """The last mask word, the pad word (130 words padded to even) and the
    segment boundaries of the device-built table."""
    rng = np.random.default_rng(n_msgs)
    n, root = 300, 3
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        first = eng.publish(np.zeros(n_msgs))
        eng.run()
        qp = np.arange(n)
        qt = np.zeros(n, dtype=np.uint32)
        hop = tree_hops(parent, root, live)
        want = oracle_lists(qt, qp, np.zeros(n_msgs), None, first, hop, root)
        got = async_lists(eng, qt, qp)
        assert got == want
        assert got == drain_lists(eng, qt, qp)
        sample = rng.choice(n, 20, replace=False)  # (the one-subscriber path costs a sync per query)
        assert [got[p] for p in sample] == per_peer(eng, qt[sample], qp[sample])


def test_interleaved_topics():
    """Two topics publishing 3:1 in turn: a topic's ids are not contiguous."""
    rng = np.random.default_rng(77)
    n, root, n_msgs = 300, 3, 1000
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    topics = (np.arange(n_msgs) % 4 == 3).astype(np.uint32)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        eng.publish(np.zeros(10))  # (the run's first id is not 0)
        eng.run()
        first = eng.publish(topics)
        eng.run()
        qp = np.tile(np.arange(n), 2)
        qt = np.repeat([0, 1], n)
        hop = tree_hops(parent, root, live)
        want = oracle_lists(qt, qp, topics, None, first, hop, root)
        got = async_lists(eng, qt, qp)
        assert got == want
        assert got == drain_lists(eng, qt, qp)


# ---- 3 / 4. pipelined -------------------------------------------------------------

def pipelined(e, batches, qt, qp):
    """publish, run_async, drain_begin, (wait, drain_end of the previous)."""
    views, res, over = [], [], 0
    for i, b in enumerate(batches):
        e.publish(b)
        e.run_async()
        e.drain_begin(qt, qp)
        if i:
            st = e.wait()
            res.append(stats_key(st))
            over += st.overlapped
            views.append(split(*e.drain_end()))
    st = e.wait()
    res.append(stats_key(st))
    over += st.overlapped
    views.append(split(*e.drain_end()))
    return views, res, over


def blocking(e, batches, qt, qp):
    views, res = [], []
    for b in batches:
        e.publish(b)
        res.append(stats_key(e.run()))
        views.append(drain_lists(e, qt, qp))
    return views, res


def vary(msg_topics, i, step):
    """Batch i: each topic drops up to (n_t - 1) % 64 of its last messages (its
    row width -- and so the plan -- stays; the last word differs)."""
    keep = np.ones(msg_topics.shape[0], dtype=bool)
    for t in np.unique(msg_topics):
        idx = np.nonzero(msg_topics == t)[0]
        drop = (i * step + int(t)) % ((idx.shape[0] - 1) % 64 + 1)
        if drop:
            keep[idx[-drop:]] = False
    return msg_topics[keep]


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
    assert sum(len(x) for x in out[0][0][0]) > 0
    for i in range(12):
        assert out[1][0][i] == out[0][0][i], i
    assert out[1][1] == out[0][1]
    assert out[1][2] == out[0][2]


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
    assert sum(len(x) for x in out[0][0][0]) > 0
    for i in range(8):
        assert out[1][0][i] == out[0][0][i], i
    assert out[1][1] == out[0][1]
    assert out[1][2] == out[0][2]


# ---- 5. begin before wait, and the slot rules --------------------------------------

def raw_begin(eng, qt, qp):
    qt = np.ascontiguousarray(qt, dtype=np.uint32)
    qp = np.ascontiguousarray(qp, dtype=np.uint32)
    return eng._L.ps_drain_begin(eng._h, PE._p(qt, PE.C.c_uint32), PE._p(qp, PE.C.c_uint32), qt.size)


def test_slot_rules():
    rng = np.random.default_rng(81)
    n, root = 2000, 0
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1, plan={"flood": 0}) as eng:
        eng.set_tree(0, root, parent)
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_begin([0], [5])
        assert ei.value.code == -8  # PS_E_NOTREADY: no run yet
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_end()
        assert ei.value.code == -8  # none outstanding
        qp = rng.choice(n, 300, replace=False)
        qp[7] = root
        qt = np.zeros(300, dtype=np.uint32)
        firsts = []
        for _ in range(2):  # two runs enqueued, a drain begun behind each before any wait
            firsts.append(eng.publish(np.zeros(1000)))
            eng.run_async()
            eng.drain_begin(qt, qp)
        assert raw_begin(eng, qt, qp) == -3  # PS_E_STATE: a third
        eng.wait()
        eng.wait()
        for first in firsts:
            got = split(*eng.drain_end())
            for p, g in zip(qp, got):
                assert g == ([] if p == root else list(range(first, first + 1000)))
        assert raw_begin(eng, [0, 0], [5, n]) == -7  # PS_E_RANGE: a peer out of range
        assert raw_begin(eng, [0, 1], [5, 5]) == -7  # a topic out of range
        eng.drain_begin(qt, qp)  # no slot leaked: two more fit
        eng.drain_begin([], [])
        assert raw_begin(eng, qt, qp) == -3
        base = split(*eng.drain_end())
        assert base == per_peer(eng, qt, qp)
        off, ids = eng.drain_end()
        assert off.tolist() == [0] and ids.size == 0
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_end()
        assert ei.value.code == -8
        # repeated queries in another order (the root among them), and the root alone
        tri = np.repeat(rng.permutation(300), 3)
        assert async_lists(eng, qt[tri], qp[tri]) == [base[i] for i in tri]
        assert async_lists(eng, [0, 0], [root, root]) == [[], []]


# ---- 6. view lifetime ----------------------------------------------------------------

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
            e.drain_begin(qt, qp)
            e.wait()
            off, ids = e.drain_end(copy=False)
            off0, ids0 = off.copy(), ids.copy()
            assert ids0.size > 0
            e.publish(batches[i + 1])
            e.run_async()
            assert np.array_equal(off, off0) and np.array_equal(ids, ids0)
            e.wait()
            assert np.array_equal(off, off0) and np.array_equal(ids, ids0)


# ---- 7. mixed with the synchronous calls -------------------------------------------

def test_mixed_with_synchronous_calls():
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
        eng.drain_begin(qt, qp)
        hop = tree_hops(parent, root, live)
        want = oracle_lists(qt, qp, np.zeros(700), None, first, hop, root)
        assert drain_lists(eng, qt, qp) == want  # (the same window, the drain outstanding)
        assert per_peer(eng, qt[:40], qp[:40]) == want[:40]
        eng.wait()
        assert split(*eng.drain_end()) == want
        # a live-mask change and a further run between begin and end: the view is batch k's
        first = eng.publish(np.zeros(650))
        eng.run_async()
        eng.drain_begin(qt, qp)
        want = oracle_lists(qt, qp, np.zeros(650), None, first, hop, root)
        live2 = (rng.random(n) > 0.3).astype(np.uint8)
        live2[root] = 1
        eng.set_live(live2)
        eng.wait()
        first2 = eng.publish(np.zeros(100))
        eng.run()
        digest = eng.seen_digest()
        assert split(*eng.drain_end()) == want
        hop2 = tree_hops(parent, root, live2)
        want2 = oracle_lists(qt, qp, np.zeros(100), None, first2, hop2, root)
        assert want2 != want
        assert drain_lists(eng, qt, qp) == want2
        assert async_lists(eng, qt, qp) == want2
        assert eng.seen_digest() == digest


# ---- 8. several windows ----------------------------------------------------------------

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
        got = async_lists(eng, qt, qp)
        assert got == drain_lists(eng, qt, qp)
        last = got[1 if root != 1 else 0]  # one window's ids, ending with the run's last message
        assert 0 < len(last) <= 128 and last == list(range(last[0], first + 300))
        assert got[root] == []


# ---- 9. two loopback ranks ---------------------------------------------------------------

def test_two_loopback_ranks_refuse():
    rng = np.random.default_rng(111)
    n, root, n_msgs = 1200, 4, 200
    parent = random_tree(rng, n, root)
    topics = np.arange(n_msgs) % 2
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 2) for _ in range(2)]
    try:
        for r, e in enumerate(engines):
            e.dist_init_loopback(lb, r, PE.PART_PEER)
            e.set_tree(0, root, parent)
            e.set_tree(1, root, parent)
            e.publish(topics)
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
        qp = rng.choice(n, 100, replace=False)
        qt = np.zeros(100, dtype=np.uint32)
        for e in engines:
            assert raw_begin(e, qt, qp) == -3  # PS_E_STATE: one rank only
            assert drain_lists(e, qt, qp) == per_peer(e, qt, qp)
    finally:
        for e in engines:
            e.close()
        lb.close()
