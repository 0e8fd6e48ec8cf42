"""GPU: the shared drain (ps_drain_shared / Engine.drain_shared) -- ps_drain's
answer with equal lists stored once.  Every comparison is bit-exact: the
expanded result against Engine.drain on the same queries and, where
test_gpu_drain_batch.py uses the oracle's hops, against those too.  Beyond
equality the tests pin down that sharing happens (one list per topic with a
reached query) and, through the PSAMD_DRAIN_SHARED=private seam, that the
private-list path gives the same ids.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle as O
import psengine as PE
from test_gpu_drain_batch import drain_lists, oracle_lists, random_mesh2, random_tree, split, tree_hops

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def shared(eng, qt, qp):
    """drain_shared, checked for well-formedness; (lists, off, ids)."""
    lists, off, ids = eng.drain_shared(qt, qp)
    assert lists.dtype == np.uint32 and off.dtype == np.uint64 and ids.dtype == np.uint32
    assert lists.size == len(qt)
    n_lists = off.size - 1
    assert off[0] == 0 and off[-1] == ids.size and np.all(np.diff(off.astype(np.int64)) >= 0)
    used = lists[lists != NONE]
    assert np.all(used < n_lists)
    # numbered by first use: the first occurrences read 0, 1, 2, ...
    _, first_at = np.unique(used, return_index=True)
    assert used[np.sort(first_at)].tolist() == list(range(n_lists))
    return lists, off, ids


def expand(lists, off, ids):
    return [[] if l == NONE else ids[int(off[l]):int(off[l + 1])].tolist() for l in lists]


def check_sharing(res, qt, qp, topics, hop, root):
    """One list per topic with a reached non-root query, holding that topic's
    window messages; every reached query of a topic names it."""
    lists, off, ids = res
    reached = np.array([p != root and hop[p] != 0xFF for p in qp], dtype=bool)
    qt = np.asarray(qt)
    live_topics = sorted(set(int(t) for t in qt[reached]))
    assert off.size - 1 == len(live_topics)
    assert ids.size == sum(int(np.sum(np.asarray(topics) == t)) for t in live_topics)
    for t in live_topics:
        assert len(set(lists[reached & (qt == t)].tolist())) == 1
    assert np.all(lists[~reached] == NONE) and np.all(lists[reached] != NONE)


def tree_case(kind):
    """The tree layouts of test_gpu_drain_batch.py: (engine kwargs, n, root,
    parent, live, topics, starts, queried peers)."""
    if kind == "unpaced":
        rng = np.random.default_rng(21)
        n, root, n_msgs = 2500, 7, 300
        parent = random_tree(rng, n, root)
        live = (rng.random(n) > 0.1).astype(np.uint8)
        live[root] = 1
        outside = 2499
        parent[parent == outside] = root  # a peer outside the tree: its children move to the root
        parent[outside] = O.NONE
        peers = [int(p) for p in rng.choice(n, 200, replace=False)] + [root, outside]
        return {}, n, root, parent, live, np.arange(n_msgs) % 2, None, peers
    if kind in ("paced0", "paced1"):
        aligned = int(kind[-1])
        rng = np.random.default_rng(31 + aligned)
        n, root, n_msgs = 1500, 11, 300
        kw = {} if aligned else {"plan": {"align_groups": 0}}
        peers = None
    else:
        assert kind == "compact"
        rng = np.random.default_rng(37)
        n, root, n_msgs = 700, 2, 200
        kw = {"flags": PE.F_COMPACT}
        peers = list(range(n))
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    starts = rng.integers(0, 5, size=n_msgs)
    if peers is None:
        peers = [int(p) for p in rng.choice(n, 150, replace=False)] + [root]
    return kw, n, root, parent, live, np.arange(n_msgs) % 2, starts, peers


def run_tree_case(kind):
    kw, n, root, parent, live, topics, starts, peers = tree_case(kind)
    eng = PE.Engine(n, 2, **kw)
    eng.set_tree(0, root, parent)
    eng.set_tree(1, root, parent)
    eng.set_live(live)
    first = eng.publish(topics, starts)
    st = eng.run()
    if kind in ("paced0", "paced1"):
        assert st.level_aligned == int(kind[-1])
    qt = np.repeat([0, 1], len(peers)).astype(np.uint32)
    qp = np.tile(peers, 2).astype(np.uint32)
    hop = tree_hops(parent, root, live)
    exp = oracle_lists(qt, qp, topics, starts, first, hop, root)
    return eng, qt, qp, topics, hop, root, exp


@pytest.mark.parametrize("kind", ["unpaced", "paced0", "paced1", "compact"])
def test_tree_layouts_equal_drain_and_share(kind):
    """Node-major rows, group-major blocks, level-aligned rows, the compaction
    path: expanded, the result is drain's and the oracle's; and it is shared
    (an implementation of private lists only would pass the first half)."""
    eng, qt, qp, topics, hop, root, exp = run_tree_case(kind)
    with eng:
        res = shared(eng, qt, qp)
        got = expand(*res)
        assert got == drain_lists(eng, qt, qp)
        assert got == exp
        check_sharing(res, qt, qp, topics, hop, root)


@pytest.mark.parametrize("paced", [False, True])
def test_mesh(paced):
    """Two parents per node.  Unpaced: a mask-layout table, classified like a
    tree's.  Paced: the arrival-order table, served through private lists."""
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
        res = shared(eng, qt, qp)
        got = expand(*res)
        assert got == drain_lists(eng, qt, qp)
        assert sum(len(g) for g in got) > n_msgs  # (somebody was reached)
        if not paced:  # a static live mask: whoever is reached holds every message
            assert res[1].size - 1 == 1 and res[2].size == n_msgs


def test_on_device_built_tables_and_back():
    """The three drains share one set of tables per window, built by whichever
    runs first.  Window A: drain_begin builds them on the device (a tree topic
    of 65 messages: two mask words, one bit in the second; a paced mesh topic:
    the arrival-order table), and drain_shared and drain read those.  Window
    B, the same batch again: drain_shared builds them on the host and
    drain_begin reads those."""
    rng = np.random.default_rng(131)
    n, roots = 300, (3, 8)
    parent = random_tree(rng, n, roots[0])
    rp, cl = random_mesh2(rng, n, roots[1])
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[list(roots)] = 1
    topics = np.concatenate([np.zeros(65), np.ones(40)]).astype(np.uint32)
    starts = np.concatenate([np.zeros(65), rng.integers(0, 5, size=40)]).astype(np.uint32)
    qt = np.repeat([0, 1], n).astype(np.uint32)
    qp = np.tile(np.arange(n), 2).astype(np.uint32)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, roots[0], parent)
        eng.set_children(1, roots[1], rp, cl)
        eng.set_live(live)

        def window(shared_first):
            first = eng.publish(topics, starts)
            eng.run()
            got = {}
            for which in ("shared", "async") if shared_first else ("async", "shared"):
                if which == "shared":
                    got[which] = expand(*shared(eng, qt, qp))
                else:
                    eng.drain_begin(qt, qp)
                    got[which] = split(*eng.drain_end())
            want = drain_lists(eng, qt, qp)
            assert got["shared"] == want
            assert got["async"] == want
            return first, want

        first_a, a = window(shared_first=False)
        hop = tree_hops(parent, roots[0], live)
        assert a[:n] == oracle_lists(qt[:n], qp[:n], topics, starts, first_a, hop, roots[0])
        # (both topics reached somebody: ten tree subscribers or more, more than one mesh subscriber)
        assert sum(1 for x in a[:n] if len(x) == 65) >= 10 and sum(len(x) for x in a[n:]) > 40
        first_b, b = window(shared_first=True)
        assert first_b == first_a + topics.size
        assert b[:n] == [[m + first_b - first_a for m in x] for x in a[:n]]
        assert [len(x) for x in b[n:]] == [len(x) for x in a[n:]]


def one_topic(n_msgs, seed):
    rng = np.random.default_rng(seed)
    n, root = 300, 3
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    return n, root, parent, live


@pytest.mark.parametrize("n_msgs", [1, 63, 64, 65, 128, 129, 1000, 4095, 4096, 4097, 8300])
def test_width_and_packing_edges(n_msgs):
    """Rows of 1, 2, 3 and 16 words (groups of 1, 2, 4 and 16 lanes), the pad
    word, exactly 64 words (one wave per row), one bit over (two waves) and
    130 words (three waves); all peers queried, so the last wave of a bin is
    partly filled."""
    n, root, parent, live = one_topic(n_msgs, n_msgs)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        first = eng.publish(np.zeros(n_msgs))
        eng.run()
        qp = np.arange(n)
        qt = np.zeros(n, dtype=np.uint32)
        res = shared(eng, qt, qp)
        got = expand(*res)
        hop = tree_hops(parent, root, live)
        assert got == oracle_lists(qt, qp, np.zeros(n_msgs), None, first, hop, root)
        assert got == drain_lists(eng, qt, qp)
        check_sharing(res, qt, qp, np.zeros(n_msgs), hop, root)


def test_mixed_widths_interleaved():
    """A 1-word and a 130-word row side by side in one batch, the queries
    interleaved: a narrow bin and a wide bin in one launch."""
    n, root, parent, live = one_topic(0, 77)
    topics = np.concatenate([np.zeros(10), np.ones(8300)]).astype(np.uint32)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        first = eng.publish(topics)
        eng.run()
        qt = np.tile([0, 1], n).astype(np.uint32)
        qp = np.repeat(np.arange(n), 2).astype(np.uint32)
        res = shared(eng, qt, qp)
        got = expand(*res)
        want = drain_lists(eng, qt, qp)
        assert got == want
        hop = tree_hops(parent, root, live)
        assert got == oracle_lists(qt, qp, topics, None, first, hop, root)
        check_sharing(res, qt, qp, topics, hop, root)
        assert res[1].size - 1 == 2 and res[2].size == 8310


def test_dead_subtree_stale_rows():
    """The cut-subtree scenario of test_gpu_drain_batch.py: the rows below the
    cut keep the first window's bits under a stale generation: PS_NONE; the
    rest share one list."""
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
        lists, off, ids = shared(eng, qt, qp)
        assert off.size - 1 == 1 and ids.size == 200 and np.sum(lists == NONE) == 1
        live = np.ones(n, dtype=np.uint8)
        live[cut] = 0
        eng.set_live(live)
        first = eng.publish(np.zeros(150))
        eng.run()
        res = shared(eng, qt, qp)
        lists, off, ids = res
        got = expand(*res)
        assert got == drain_lists(eng, qt, qp)
        hop = tree_hops(parent, root, live)
        assert got == oracle_lists(qt, qp, np.zeros(150), None, first, hop, root)
        for p in below + [cut, root]:
            assert lists[p] == NONE
        assert off.size - 1 == 1 and ids.tolist() == list(range(first, first + 150))
        assert np.sum(lists == 0) == n - 2 - len(below)


@pytest.mark.parametrize("kind", ["unpaced", "paced1"])
def test_private_path_through_the_seam(kind, monkeypatch):
    """PSAMD_AB=1 PSAMD_DRAIN_SHARED=private: a full row is treated as any
    other row, so every reached query takes a list of its own through the
    count / scan / emit passes; the same ids, n_lists = reached queries."""
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_DRAIN_SHARED", "private")
    eng, qt, qp, topics, hop, root, exp = run_tree_case(kind)
    with eng:
        res = shared(eng, qt, qp)
        lists, off, ids = res
        got = expand(*res)
        assert got == drain_lists(eng, qt, qp)
        assert got == exp
        n_reached = sum(1 for x in exp if x)
        assert n_reached > 100
        assert off.size - 1 == n_reached
        assert ids.size == sum(len(x) for x in exp)
        assert np.array_equal(lists[lists != NONE], np.arange(n_reached))


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
        base = drain_lists(eng, qt, qp)
        assert expand(*shared(eng, qt, qp)) == base
        perm = rng.permutation(qt.size)
        res = shared(eng, qt[perm], qp[perm])
        assert expand(*res) == [base[i] for i in perm]
        assert res[1].size - 1 == 2
        tri = np.repeat(np.arange(qt.size), 3)
        res = shared(eng, qt[tri], qp[tri])
        assert expand(*res) == [base[i] for i in tri]
        assert res[1].size - 1 == 2 and res[2].size == 500
        lists, off, ids = eng.drain_shared([], [])
        assert lists.size == 0 and off.tolist() == [0] and ids.size == 0


L_SENT, O_SENT, M_SENT = 0x55555555, 0xAAAAAAAAAAAAAAAA, 0xDEADBEEF


def raw_shared(eng, qt, qp, list_cap, cap):
    qt = np.ascontiguousarray(qt, dtype=np.uint32)
    qp = np.ascontiguousarray(qp, dtype=np.uint32)
    lists = np.full(qt.size, L_SENT, dtype=np.uint32)
    off = np.full(list_cap + 1, O_SENT, dtype=np.uint64)
    out = np.full(max(cap, 1), M_SENT, dtype=np.uint32)
    n_lists, total = C.c_uint32(0xBBBB), C.c_uint64(0xCCCC)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = eng._L.ps_drain_shared(eng._h, qt.ctypes.data_as(u32p), qp.ctypes.data_as(u32p), qt.size,
                                lists.ctypes.data_as(u32p), off.ctypes.data_as(u64p), list_cap,
                                out.ctypes.data_as(u32p) if cap else None, cap, C.byref(n_lists), C.byref(total))
    return rc, lists, off, out, n_lists.value, total.value


def test_sizing_capacity_and_errors():
    rng = np.random.default_rng(81)
    n, root = 300, 0
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        rc, lists, off, out, n_lists, total = raw_shared(eng, [0], [5], 4, 16)
        assert rc == -8  # PS_E_NOTREADY: no run yet
        first = eng.publish(np.arange(100) % 2)
        eng.run()
        qp = np.tile(np.arange(40), 2)
        qt = np.repeat([1, 0], 40).astype(np.uint32)
        exp = drain_lists(eng, qt, qp)
        want_lists = np.array([NONE] + [0] * 39 + [NONE] + [1] * 39, dtype=np.uint32)
        want_ids = list(range(first + 1, first + 100, 2)) + list(range(first, first + 100, 2))
        rc, lists, off, out, n_lists, total = raw_shared(eng, qt, qp, 0, 0)  # the sizing call
        assert rc == -7 and n_lists == 2 and total == 100 and np.array_equal(lists, want_lists)
        assert np.all(off == O_SENT)
        rc, lists, off, out, n_lists, total = raw_shared(eng, qt, qp, 2, 99)  # cap = total - 1
        assert rc == -7 and n_lists == 2 and total == 100 and np.array_equal(lists, want_lists)
        assert off.tolist() == [0, 50, 100]
        assert np.all(out == M_SENT)  # untouched
        rc, lists, off, out, n_lists, total = raw_shared(eng, qt, qp, 1, 100)  # list_cap = n_lists - 1
        assert rc == -7 and n_lists == 2 and total == 100 and np.array_equal(lists, want_lists)
        assert np.all(off == O_SENT) and np.all(out == M_SENT)
        rc, lists, off, out, n_lists, total = raw_shared(eng, qt, qp, 2, 100)  # exact
        assert rc == 0 and n_lists == 2 and total == 100 and np.array_equal(lists, want_lists)
        assert off.tolist() == [0, 50, 100] and out.tolist() == want_ids
        assert expand(lists, off, out) == exp
        rc, lists, off, out, n_lists, total = raw_shared(eng, qt, qp, 7, 1000)  # room to spare
        assert rc == 0 and off[:3].tolist() == [0, 50, 100] and np.all(off[3:] == O_SENT)
        assert out[:100].tolist() == want_ids and np.all(out[100:] == M_SENT)
        for bad_t, bad_p in (([0, 0], [5, n]), ([0, 2], [5, 5])):  # peer, topic out of range: nothing written
            rc, lists, off, out, n_lists, total = raw_shared(eng, bad_t, bad_p, 4, 1000)
            assert rc == -7 and n_lists == 0xBBBB and total == 0xCCCC
            assert np.all(lists == L_SENT) and np.all(off == O_SENT) and np.all(out == M_SENT)


def test_two_loopback_ranks_refused():
    """One rank only: a multi-rank engine returns PS_E_STATE, nothing written."""
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
            rc, lists, off, out, n_lists, total = raw_shared(e, [0, 0], [5, 6], 4, 200)
            assert rc == -3  # PS_E_STATE
            assert n_lists == 0xBBBB and total == 0xCCCC
            assert np.all(lists == L_SENT) and np.all(off == O_SENT) and np.all(out == M_SENT)
            assert sum(len(x) for x in drain_lists(e, [0, 0], [5, 6])) in (0, 50, 100)  # (ps_drain still serves it)
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
        qp = rng.choice(n, 300, replace=False)
        qt = np.zeros(300, dtype=np.uint32)
        lists, off, ids = shared(eng, qt, qp)
        assert expand(lists, off, ids) == drain_lists(eng, qt, qp)
        assert off.tolist() == [0, 1000] and ids.tolist() == list(range(first, first + 1000))
        assert all(l == (NONE if p == root else 0) for p, l in zip(qp, lists))


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
        lists, off, ids = shared(eng, qt, qp)
        assert expand(lists, off, ids) == drain_lists(eng, qt, qp)
        assert off.size - 1 == 1 and 0 < ids.size <= 128
        assert ids.tolist() == list(range(int(ids[0]), first + 300))  # one window, ending with the run's last message
        assert lists[root] == NONE and np.sum(lists == 0) == n - 1
