"""GPU: the batched drain (ps_drain / Engine.drain) -- client.Messages()
(client.go:26-28,124-128) of many subscribers in one call.  Every comparison
is bit-exact: against the list of peer_messages() (ps_read_peer_messages, the
one-subscriber path) over the same queries, and, where a case says so, against
the oracle's hops the way test_gpu_drain.py does (reached peers: the topic's
window messages sorted by (start round, publish order); the others: nothing).
"""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle as O
import psengine as PE

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
        got = drain_lists(eng, qt, qp)
        assert got == oracle_lists(qt, qp, topics, None, first, hop, root)
        assert got == per_peer(eng, qt, qp)
        assert got[len(peers) - 1] == [] and got[len(peers) - 2] == []


@pytest.mark.parametrize("n_msgs", [1, 63, 64, 65, 4095, 4096, 4097, 8300])
def test_segment_and_word_edges(n_msgs):
    """Word edges, exactly one segment (4096 bits), one bit into the second,
    three segments with an odd word count (130 words, padded to even)."""
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
        got = drain_lists(eng, qt, qp)
        hop = tree_hops(parent, root, live)
        assert got == oracle_lists(qt, qp, np.zeros(n_msgs), None, first, hop, root)
        assert got == per_peer(eng, qt, qp)


@pytest.mark.parametrize("aligned", [0, 1])
def test_paced_both_layouts(aligned):
    """Starts uniform in 0..4: group-major blocks (align_groups 0) and packed
    level-aligned rows (the default)."""
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
        got = drain_lists(eng, qt, qp)
        hop = tree_hops(parent, root, live)
        assert got == oracle_lists(qt, qp, topics, starts, first, hop, root)
        assert got == per_peer(eng, qt, qp)


def test_paced_compaction_path():
    """The same paced window through the compaction path (PS_F_COMPACT, no
    level mode): whatever bit order its rows have, the drain is the oracle's."""
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
        got = drain_lists(eng, qt, qp)
        hop = tree_hops(parent, root, live)
        assert got == oracle_lists(qt, qp, topics, starts, first, hop, root)
        assert got == per_peer(eng, qt, qp)


@pytest.mark.parametrize("paced", [False, True])
def test_mesh(paced):
    """Two parents per node; paced: the row is in window order, not arrival
    order (the order-table path)."""
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
        got = drain_lists(eng, qt, qp)
        assert got == per_peer(eng, qt, qp)
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
        assert all(len(g) == 200 for q, g in enumerate(drain_lists(eng, qt, qp)) if q != root)
        live = np.ones(n, dtype=np.uint8)
        live[cut] = 0
        eng.set_live(live)
        first = eng.publish(np.zeros(150))
        eng.run()
        got = drain_lists(eng, qt, qp)
        assert got == per_peer(eng, qt, qp)
        hop = tree_hops(parent, root, live)
        assert got == oracle_lists(qt, qp, np.zeros(150), None, first, hop, root)
        for p in below + [cut]:
            assert got[p] == []
        assert sum(1 for g in got if g) == n - 2 - len(below)


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
        got = drain_lists(eng, qt, qp)
        assert got == per_peer(eng, qt, qp)
        assert got[root] == []
        last = got[1 if root != 1 else 0]  # one window's ids, ending with the run's last message
        assert 0 < len(last) <= 128 and last == list(range(last[0], first + 300))
        for p in range(n):
            assert p == root or got[p] == last


def test_duplicates_order_and_empty():
    rng = np.random.default_rng(71)
    n, root = 500, 9
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        eng.publish(np.arange(500) % 2, rng.integers(0, 3, size=500))
        eng.run()
        peers = rng.choice(n, 60, replace=False)
        qt = np.concatenate([np.zeros(60), np.ones(60)]).astype(np.uint32)
        qp = np.concatenate([peers, peers]).astype(np.uint32)
        base = per_peer(eng, qt, qp)
        assert drain_lists(eng, qt, qp) == base
        perm = rng.permutation(qt.size)
        assert drain_lists(eng, qt[perm], qp[perm]) == [base[i] for i in perm]
        tri = np.repeat(np.arange(qt.size), 3)
        assert drain_lists(eng, qt[tri], qp[tri]) == [base[i] for i in tri]
        off, ids = eng.drain([], [])
        assert off.tolist() == [0] and ids.size == 0


def raw_drain(eng, qt, qp, cap, sentinel=0xDEADBEEF):
    qt = np.ascontiguousarray(qt, dtype=np.uint32)
    qp = np.ascontiguousarray(qp, dtype=np.uint32)
    off = np.full(qt.size + 1, 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    out = np.full(max(cap, 1), sentinel, dtype=np.uint32)
    total = C.c_uint64(0xBBBB)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = eng._L.ps_drain(eng._h, qt.ctypes.data_as(u32p), qp.ctypes.data_as(u32p), qt.size, off.ctypes.data_as(u64p),
                         out.ctypes.data_as(u32p) if cap else None, cap, C.byref(total))
    return rc, off, out, total.value


def test_sizing_capacity_and_errors():
    rng = np.random.default_rng(81)
    n, root = 300, 0
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        rc, off, out, total = raw_drain(eng, [0], [5], 16)
        assert rc == -8  # PS_E_NOTREADY: no run yet
        eng.publish(np.zeros(100))
        eng.run()
        qp = np.arange(40)
        qt = np.zeros(40, dtype=np.uint32)
        exp = per_peer(eng, qt, qp)
        want_off = np.concatenate([[0], np.cumsum([len(x) for x in exp])]).astype(np.uint64)
        want_total = int(want_off[-1])
        assert want_total == 39 * 100
        rc, off, out, total = raw_drain(eng, qt, qp, 0)  # the sizing call
        assert rc == -7 and total == want_total and np.array_equal(off, want_off)
        rc, off, out, total = raw_drain(eng, qt, qp, want_total - 1)
        assert rc == -7 and total == want_total and np.array_equal(off, want_off)
        assert np.all(out == 0xDEADBEEF)  # untouched
        rc, off, out, total = raw_drain(eng, qt, qp, want_total)
        assert rc == 0 and total == want_total and np.array_equal(off, want_off)
        assert split(off, out[:total]) == exp
        rc, off, out, total = raw_drain(eng, [0, 0], [5, n], 1000)  # peer out of range: nothing written
        assert rc == -7 and total == 0xBBBB and np.all(off == 0xAAAAAAAAAAAAAAAA) and np.all(out == 0xDEADBEEF)
        rc, off, out, total = raw_drain(eng, [0, 1], [5, 5], 1000)  # topic out of range
        assert rc == -7 and total == 0xBBBB


def test_slabs(monkeypatch):
    """A slab override far below the output (the engine holds a slab to at
    least one segment, 4096 ids): many slabs, single queries split across
    slabs at segment boundaries; the same ids as without the override."""
    rng = np.random.default_rng(91)
    n, root, n_msgs = 300, 3, 8300
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    qp = rng.choice(n, 50, replace=False)
    qt = np.zeros(50, dtype=np.uint32)

    def run_one():
        with PE.Engine(n, 1) as eng:
            eng.set_tree(0, root, parent)
            eng.set_live(live)
            eng.publish(np.zeros(n_msgs))
            eng.run()
            off, ids = eng.drain(qt, qp)
            return off.copy(), ids.copy(), per_peer(eng, qt, qp)

    off0, ids0, exp = run_one()
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_DRAIN_SLAB_IDS", "1000")
    off1, ids1, _ = run_one()
    assert np.array_equal(off0, off1) and np.array_equal(ids0, ids1)
    assert split(off1, ids1) == exp
    assert ids1.size > 20 * 8300


def test_after_async_runs():
    """run_async, the next batch, run_async, wait, wait, drain: the drain reads
    the last window behind both runs (twin-window size, no k_flood)."""
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
        qp = rng.choice(n, 300, replace=False)
        qt = np.zeros(300, dtype=np.uint32)
        got = drain_lists(eng, qt, qp)
        assert got == per_peer(eng, qt, qp)
        for p, g in zip(qp, got):
            assert g == ([] if p == root else list(range(first, first + 1000)))


def test_two_loopback_ranks():
    """PART_PEER over two loopback ranks: every query is answered by the rank
    that owns the peer's node, the other returns nothing."""
    rng = np.random.default_rng(111)
    n, root, n_msgs = 1200, 4, 200
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    starts = rng.integers(0, 3, size=n_msgs)
    topics = np.arange(n_msgs) % 2
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 2) for _ in range(2)]
    try:
        firsts = []
        for r, e in enumerate(engines):
            e.dist_init_loopback(lb, r, PE.PART_PEER)
            e.set_tree(0, root, parent)
            e.set_tree(1, root, parent)
            e.set_live(live)
            firsts.append(e.publish(topics, starts))
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
        assert firsts[0] == firsts[1]
        peers = [int(p) for p in rng.choice(n, 200, replace=False)] + [root]
        qt = np.repeat([0, 1], len(peers))
        qp = np.tile(peers, 2)
        hop = tree_hops(parent, root, live)
        exp = oracle_lists(qt, qp, topics, starts, firsts[0], hop, root)
        got = [drain_lists(e, qt, qp) for e in engines]
        for r, e in enumerate(engines):
            assert got[r] == per_peer(e, qt, qp)
        answered = [0, 0]
        for q in range(qt.size):
            pair = sorted([got[0][q], got[1][q]], key=len)
            assert pair == [[], exp[q]], q
            if exp[q]:
                answered[0 if got[0][q] else 1] += 1
        assert min(answered) > 0  # both ranks own some of the queried peers
    finally:
        for e in engines:
            e.close()
        lb.close()
