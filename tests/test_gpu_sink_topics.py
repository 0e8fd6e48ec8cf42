"""GPU: the audience sink (ps_sink_set_topics / ps_sink_take_topics, DESIGN.md
§5.5h) -- standing topics drained as ps_drain_topics does behind every window
of a run, the windows accumulated on the device into one result per run.
Two independent references:
 (a) a stepping engine: same topology and seed, fed the same messages one
     window's worth per run, Engine.drain_topics after each run, compared
     array for array after the documented shifts (list numbers by the lists
     of the windows before, exc_off by their records);
 (b) where a closed form exists, the tree hops: who is reached, and so the
     full nodes and the exceptions of every window."""
import ctypes as C
import threading

import numpy as np
import pytest

import psengine as PE
from psengine import workloads as WL
from test_gpu_drain_async import stats_key, vary
from test_gpu_drain_batch import random_mesh2, random_tree, tree_hops
from test_gpu_drain_shared import one_topic, tree_case
from test_gpu_drain_topics import kids_of, under
from test_gpu_sink import drop_engine, even_batches, splitting_window, window_chunks

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
KEYS = ("topic_list", "n_nodes", "n_full", "exc_off", "exc_peer", "exc_list", "list_off", "ids")


# ---- helpers ------------------------------------------------------------------------

def seam(monkeypatch):
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_DRAIN_SHARED", "private")


def stepped(eng, chunks, topics, starts, order, first=0):
    """Reference (a) on a second engine: one run per chunk, drain_topics after
    each, the ids mapped back to the numbering of a run that publishes
    everything at once (first + index)."""
    topics = np.asarray(topics)
    out = []
    for idx in chunks:
        f = eng.publish(topics[idx], None if starts is None else np.asarray(starts)[idx])
        st = eng.run()
        assert st.windows == 1
        r = eng.drain_topics(order)
        r["ids"] = (first + idx[r["ids"].astype(np.int64) - f]).astype(np.uint32)
        out.append(r)
    return out


def check_windows(res, ref):
    """The sink's result against reference (a), window by window, entry for entry."""
    nw = len(ref)
    assert res["n_windows"] == nw
    assert res["topic_list"].dtype == np.uint32 and res["exc_peer"].dtype == np.uint32 and res["ids"].dtype == np.uint32
    for k in ("n_nodes", "n_full", "exc_off", "list_off"):
        assert res[k].dtype == np.uint64, k
    n = res["topic_list"].shape[1]
    assert res["topic_list"].shape == res["n_nodes"].shape == res["n_full"].shape == (nw, n)
    assert res["exc_off"].size == nw * n + 1 and res["exc_off"][0] == 0
    assert res["list_off"][0] == 0 and res["list_off"][-1] == res["ids"].size
    bl = be = 0
    for w, r in enumerate(ref):
        assert r["topic_list"].size == n
        want = np.where(r["topic_list"] == NONE, NONE, r["topic_list"] + np.uint32(bl)).astype(np.uint32)
        assert np.array_equal(res["topic_list"][w], want), w
        assert np.array_equal(res["n_nodes"][w], r["n_nodes"]), w
        assert np.array_equal(res["n_full"][w], r["n_full"]), w
        assert np.array_equal(res["exc_off"][w * n:(w + 1) * n + 1], r["exc_off"] + np.uint64(be)), w
        ne = int(r["exc_off"][-1])
        assert np.array_equal(res["exc_peer"][be:be + ne], r["exc_peer"]), w
        want = np.where(r["exc_list"] == NONE, NONE, r["exc_list"] + np.uint32(bl)).astype(np.uint32)
        assert np.array_equal(res["exc_list"][be:be + ne], want), w
        nl = r["list_off"].size - 1
        seg = res["list_off"][bl:bl + nl + 1]
        assert np.array_equal(seg - seg[0], r["list_off"]), w
        assert np.array_equal(res["ids"][int(seg[0]):int(seg[-1])], r["ids"]), w
        bl += nl
        be += ne
    assert res["list_off"].size - 1 == bl and res["exc_off"][-1] == be == res["exc_peer"].size == res["exc_list"].size


def same(got, want):
    assert set(got) == set(want)
    for k in want:
        if k == "n_windows":
            assert got[k] == want[k]
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def topic_ids(res, i):
    """Entry i's deliveries of the run: its windows' shared lists in window order."""
    out = []
    for w in range(res["n_windows"]):
        l = int(res["topic_list"][w, i])
        if l != NONE:
            out += res["ids"][int(res["list_off"][l]):int(res["list_off"][l + 1])].tolist()
    return out


def raw_set(eng, topics, exc_cap=0, list_cap=0, id_cap=0):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    return eng._L.ps_sink_set_topics(eng._h, t.ctypes.data_as(U32P), t.size, exc_cap, list_cap, id_cap)


def refused(eng):
    with pytest.raises(PE.EngineError) as ei:
        eng.sink_take_topics()
    assert ei.value.code == E_RANGE
    return ei.value.partial


def counts(r):
    return int(r["exc_off"][-1]), r["list_off"].size - 1, r["ids"].size


def two(make):
    return make(), make()


# ---- 1. splits ----------------------------------------------------------------------------

def test_window_split():
    """300 messages at msg_window = 128 on one topic: three windows, every
    node full in each, three lists."""
    rng = np.random.default_rng(61)
    n, root = 400, 2
    parent = random_tree(rng, n, root)
    topics = np.zeros(300, dtype=np.uint32)
    with PE.Engine(n, 1, msg_window=128) as eng, PE.Engine(n, 1, msg_window=128) as ref:
        eng.set_tree(0, root, parent)
        ref.set_tree(0, root, parent)
        eng.sink_set_topics([0])
        first = eng.publish(topics)
        st = eng.run()
        assert st.windows == 3
        res = eng.sink_take_topics()
        check_windows(res, stepped(ref, window_chunks(topics, 128), topics, None, [0], first))
        assert res["n_full"].tolist() == [[n - 1]] * 3 == res["n_nodes"].tolist()
        assert res["topic_list"].tolist() == [[0], [1], [2]] and res["exc_off"].tolist() == [0, 0, 0, 0]
        assert res["list_off"].tolist() == [0, 128, 256, 300]
        assert topic_ids(res, 0) == list(range(first, first + 300))


@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1], [3, 1]])
def test_uneven_topics(order):
    """130 / 64 / 1 messages at msg_window = 64 over three topics, an idle
    topic and a created-but-empty one among the standing ones: a topic without
    messages in a window has n_full 0, no exception and PS_NONE in its row."""
    rng = np.random.default_rng(62)
    n, root, parent, live = one_topic(0, 62)
    topics = rng.permutation(np.concatenate([np.full(c, t) for t, c in enumerate((130, 64, 1))])).astype(np.uint32)
    chunks = window_chunks(topics, 64)
    assert len(chunks) == 3
    hop = tree_hops(parent, root, live)
    reached = sum(1 for p in range(n) if p != root and hop[p] != 0xFF)

    def make():
        e = PE.Engine(n, 5, msg_window=64)
        for t in range(4):
            e.set_tree(t, root, parent)
        e.topic_create(4, root)
        e.set_live(live)
        return e

    eng, ref = two(make)
    with eng, ref:
        eng.sink_set_topics(order)
        first = eng.publish(topics)
        st = eng.run()
        assert st.windows == 3
        res = eng.sink_take_topics()
        check_windows(res, stepped(ref, chunks, topics, None, order, first))
        eo = res["exc_off"]
        for w in range(3):
            for i, t in enumerate(order):
                active = t == 0 or (w == 0 and t in (1, 2))
                assert res["n_nodes"][w, i] == (0 if t == 4 else n - 1)
                assert res["n_full"][w, i] == (reached if active else 0)
                assert (res["topic_list"][w, i] == NONE) == (not active)
                assert eo[w * len(order) + i + 1] - eo[w * len(order) + i] == (n - 1 - reached if active else 0)
        for i, t in enumerate(order):
            want = [first + int(m) for m in np.nonzero(topics == t)[0]] if t < 3 else []
            assert topic_ids(res, i) == want, t


# ---- 2. exceptions across windows ---------------------------------------------------------

@pytest.mark.parametrize("kind", ["client", "interior", "all_but_the_roots_children"])
def test_exceptions_across_windows(kind):
    """A masked client, a masked interior subtree, and everything but the
    root's children cut: PS_NONE exceptions in every window, exc_off
    cumulative over the run."""
    rng = np.random.default_rng(70)
    n, root = 900, 0
    parent = random_tree(rng, n, root)
    kids = kids_of(parent)
    live = np.ones(n, dtype=np.uint8)
    if kind == "client":
        cut = {next(p for p in range(1, n) if p not in kids)}
        live[list(cut)] = 0
    elif kind == "interior":
        top = max((p for p in range(1, n) if parent[p] == root), key=lambda p: len(under(kids, p)))
        cut = under(kids, top) | {top}
        live[top] = 0
    else:
        first_level = [p for p in range(1, n) if parent[p] == root]
        live[:] = 0
        live[[root] + first_level] = 1
        cut = set(range(1, n)) - set(first_level)
    topics = np.zeros(150, dtype=np.uint32)
    with PE.Engine(n, 1, msg_window=64) as eng, PE.Engine(n, 1, msg_window=64) as ref:
        for e in (eng, ref):
            e.set_tree(0, root, parent)
            e.set_live(live)
        eng.sink_set_topics([0])
        first = eng.publish(topics)
        eng.run()
        res = eng.sink_take_topics()
        check_windows(res, stepped(ref, window_chunks(topics, 64), topics, None, [0], first))
        c = len(cut)
        assert res["exc_off"].tolist() == [0, c, 2 * c, 3 * c] and np.all(res["exc_list"] == NONE)
        for w in range(3):
            assert set(res["exc_peer"][w * c:(w + 1) * c].tolist()) == cut
        assert res["n_full"].tolist() == [[n - 1 - c]] * 3
        assert topic_ids(res, 0) == list(range(first, first + 150))


@pytest.mark.parametrize("c", [0, 1, 63, 64, 65, 257])
def test_exception_counts_per_window(c, monkeypatch):
    """c exceptions in each of three windows, each with a list of its own
    (through the seam every full row is one; c = 0: no seam, every row full):
    the records and their lists rebased by c and 2c, below, at and above a
    wave and a block of the commit."""
    if c:
        seam(monkeypatch)
    n = c + 1 if c else 300
    rng = np.random.default_rng(100 + c)
    parent = random_tree(rng, n, 0)
    topics = np.zeros(150, dtype=np.uint32)
    with PE.Engine(n, 1, msg_window=64) as eng, PE.Engine(n, 1, msg_window=64) as ref:
        eng.set_tree(0, 0, parent)
        ref.set_tree(0, 0, parent)
        eng.sink_set_topics([0])
        first = eng.publish(topics)
        eng.run()
        res = eng.sink_take_topics()
        check_windows(res, stepped(ref, window_chunks(topics, 64), topics, None, [0], first))
        assert res["exc_off"].tolist() == [0, c, 2 * c, 3 * c]
        assert np.array_equal(res["exc_list"], np.arange(3 * c))
        assert res["list_off"].size - 1 == (3 * c if c else 3) and res["ids"].size == 150 * (c if c else 1)


def test_more_exceptions_than_the_default_cap():
    """70,001 nodes, everything but the root's children cut, two windows: more
    than 65,536 records a window.  The engine's caps refuse with n_nodes,
    n_full and exc_off exact; the retry with exc_cap = exc_off[last] succeeds."""
    rng = np.random.default_rng(17)
    n, root = 70_001, 0
    parent = random_tree(rng, n, root)
    first_level = [p for p in range(n) if parent[p] == root]
    live = np.zeros(n, dtype=np.uint8)
    live[[root] + first_level] = 1
    topics = np.zeros(70, dtype=np.uint32)
    with PE.Engine(n, 1, msg_window=64) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.sink_set_topics([0])
        eng.publish(topics)
        assert eng.run().windows == 2
        part = refused(eng)
        n_exc = n - 1 - len(first_level)
        assert n_exc > 65_536 and part["n_windows"] == 2 and part["exc_off"].tolist() == [0, n_exc, 2 * n_exc]
        assert part["n_full"].tolist() == [[len(first_level)]] * 2 and part["n_nodes"].tolist() == [[n - 1]] * 2
        eng.sink_set_topics([0], exc_cap=int(part["exc_off"][-1]))
        first = eng.publish(topics)
        eng.run()
        res = eng.sink_take_topics()
        last = eng.drain_topics([0])  # the last window, as ever
        assert res["exc_off"].tolist() == [0, n_exc, 2 * n_exc] and np.all(res["exc_list"] == NONE)
        assert np.array_equal(res["exc_peer"][:n_exc], last["exc_peer"]) and np.array_equal(res["exc_peer"][n_exc:], last["exc_peer"])
        assert res["n_full"].tolist() == [[len(first_level)]] * 2
        assert res["list_off"].tolist() == [0, 64, 70] and res["ids"].tolist() == list(range(first, first + 70))


# ---- 3. private lists at a cursor -----------------------------------------------------------

@pytest.mark.parametrize("base,n_msgs", [(65, 70), (65, 8300), (4095, 8300), (4096, 70), (4097, 8300)])
def test_private_lists_at_an_id_base(base, n_msgs, monkeypatch):
    """Through the seam: two join topics with a dropped leaf each, so that
    each topic's first message runs in a window of its own over the old tree
    -- `base` private lists of one id -- and the second window writes private
    lists of one segment (70 ids) or three (8,300) from id `base` on."""
    seam(monkeypatch)
    small = 6
    n0 = base - (small - 2) + 2  # topic 0's peers: its reached non-root nodes are n0 - 2
    n = n0 + small
    topics = np.concatenate([[0, 1], np.ones(n_msgs - 1)]).astype(np.uint32)

    def make():
        e = PE.Engine(n, 2, msg_window=8320, seed=5)
        e.topic_create(0, 0, 2, 5)
        e.join(0, np.arange(1, n0))
        e.topic_create(1, n0, 2, 5)
        e.join(1, np.arange(n0 + 1, n))
        for t in (0, 1):
            par = e.parents(t)
            lo, hi = (0, n0) if t == 0 else (n0, n)
            leaf = max(p for p in range(lo + 1, hi) if not np.any(par == p))
            e.drop(t, [leaf])
        return e

    eng, ref = two(make)
    with eng, ref:
        eng.sink_set_topics([0, 1])
        first = eng.publish(topics)
        st = eng.run()
        assert st.windows == 2
        res = eng.sink_take_topics()
        check_windows(res, stepped(ref, [np.arange(2), np.arange(2, topics.size)], topics, None, [0, 1], first))
        nl0 = int(np.sum(res["exc_list"][:int(res["exc_off"][2])] != NONE))  # the first window's lists
        assert nl0 == base and res["list_off"][nl0] == base
        assert np.all(np.diff(res["list_off"][nl0:].astype(np.int64)) == n_msgs - 1) and res["list_off"].size - 1 > nl0


def test_none_records_between_any_ones(monkeypatch):
    """Through the seam, with a subtree cut, over three windows: the cut
    nodes' records create no list and lie between records that do."""
    seam(monkeypatch)
    rng = np.random.default_rng(51)
    n, root = 600, 0
    parent = random_tree(rng, n, root)
    kids = kids_of(parent)
    cut = max((p for p in range(n) if parent[p] == root), key=lambda p: len(under(kids, p)))
    below = under(kids, cut)
    live = np.ones(n, dtype=np.uint8)
    live[cut] = 0
    topics = np.zeros(150, dtype=np.uint32)
    with PE.Engine(n, 1, msg_window=64) as eng, PE.Engine(n, 1, msg_window=64) as ref:
        for e in (eng, ref):
            e.set_tree(0, root, parent)
            e.set_live(live)
        eng.sink_set_topics([0])
        first = eng.publish(topics)
        eng.run()
        res = eng.sink_take_topics()
        check_windows(res, stepped(ref, window_chunks(topics, 64), topics, None, [0], first))
        none = np.flatnonzero(res["exc_list"] == NONE)
        some = np.flatnonzero(res["exc_list"] != NONE)
        assert none.size == 3 * (len(below) + 1) and set(res["exc_peer"][none].tolist()) == below | {cut}
        assert np.array_equal(res["exc_list"][some], np.arange(some.size)) and res["list_off"].size - 1 == some.size
        for w in range(3):  # in every window a "none" record with "any" ones either side
            lo, hi = int(res["exc_off"][w]), int(res["exc_off"][w + 1])
            nw_, sw_ = none[(none >= lo) & (none < hi)], some[(some >= lo) & (some < hi)]
            assert sw_.min() < nw_.max() and nw_.min() < sw_.max()


# ---- 4. layouts ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["unpaced", "paced0", "paced1", "compact"])
def test_tree_layouts(kind):
    kw, n, root, parent, live, topics, starts, peers = tree_case(kind)
    kw = dict(kw, msg_window=64)
    topics = np.asarray(topics, dtype=np.uint32)
    chunks = window_chunks(topics, 64)
    assert len(chunks) >= 2
    with PE.Engine(n, 2, **kw) as eng, PE.Engine(n, 2, **kw) as ref:
        for e in (eng, ref):
            e.set_tree(0, root, parent)
            e.set_tree(1, root, parent)
            e.set_live(live)
        eng.sink_set_topics([1, 0])
        first = eng.publish(topics, starts)
        st = eng.run()
        assert st.windows == len(chunks)
        res = eng.sink_take_topics()
        check_windows(res, stepped(ref, chunks, topics, starts, [1, 0], first))
        hop = tree_hops(parent, root, live)
        reached = sum(1 for p in range(n) if p != root and parent[p] != NONE and hop[p] != 0xFF)
        assert np.all(res["n_full"][res["topic_list"] != NONE] == reached)
        s = np.zeros(topics.size, dtype=np.int64) if starts is None else np.asarray(starts)
        for i, t in enumerate((1, 0)):
            want = []
            for idx in chunks:
                mine = [int(m) for m in idx if topics[m] == t]
                want += [first + m for m in sorted(mine, key=lambda m: (int(s[m]), m))]
            assert topic_ids(res, i) == want


@pytest.mark.parametrize("paced", [False, True])
def test_mesh(paced):
    """Two parents per node; paced: the arrival-order table (kDrainGather), a
    private list per node in every window."""
    rng = np.random.default_rng(41 + paced)
    n, root, n_msgs = 800, 5, 300
    rp, cl = random_mesh2(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    starts = rng.integers(0, 5, size=n_msgs) if paced else None
    topics = np.zeros(n_msgs, dtype=np.uint32)
    chunks = window_chunks(topics, 128)
    with PE.Engine(n, 1, msg_window=128) as eng, PE.Engine(n, 1, msg_window=128) as ref:
        for e in (eng, ref):
            e.set_children(0, root, rp, cl)
            e.set_live(live)
        eng.sink_set_topics([0])
        first = eng.publish(topics, starts)
        eng.run()
        res = eng.sink_take_topics()
        assert res["n_windows"] == 3
        check_windows(res, stepped(ref, chunks, topics, starts, [0], first))
        if paced:
            assert np.all(res["topic_list"] == NONE) and np.all(res["n_full"] == 0)
            assert res["list_off"].size - 1 == int(np.sum(res["exc_list"] != NONE)) > 300
        else:
            assert res["list_off"].size - 1 == 3 and res["ids"].size == n_msgs and np.all(res["n_full"] > 100)


# ---- 5. drop ------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["one_child", "widest"])
def test_drop(which):
    """A dropped interior peer with one child, and one with several (as
    test_gpu_sink.py::test_drop): the first window runs on the old tree, the
    later ones on the repaired one, and n_nodes differs between them."""
    n, seed = 60, 3
    topics = np.array([0] * 5 + [1] * 5, dtype=np.uint32)
    with drop_engine(n, seed) as eng, drop_engine(n, seed) as ref:
        par = eng.parents(0)
        kids = kids_of(par)
        interior = [p for p in kids if p != 0]
        if which == "one_child":
            dead = max((p for p in interior if len(kids[p]) == 1), key=lambda p: len(under(kids, p)))
        else:
            dead = max(interior, key=lambda p: (len(kids[p]), len(under(kids, p))))
            assert len(kids[dead]) >= 2
        for e in (eng, ref):
            e.drop(0, [dead])
        eng.sink_set_topics([0, 1])
        first = eng.publish(topics)
        st = eng.run()
        assert st.windows >= 2
        res = eng.sink_take_topics()
        check_windows(res, stepped(ref, [np.array([0]), np.arange(1, 10)], topics, None, [0, 1], first))
        # the old tree's node space ends above the dead host; the repaired one has re-attached who it could
        below = len(under(kids, dead))
        assert res["n_nodes"][0, 0] == n - 2 - below == res["n_full"][0, 0]
        assert n - 2 - below < res["n_nodes"][1, 0] <= n - 2 and res["n_nodes"][1, 0] == res["n_full"][1, 0]
        assert res["n_nodes"][1, 1] == n - 1 == res["n_full"][1, 1]
        assert topic_ids(res, 0) == list(range(first, first + 5)) and topic_ids(res, 1) == list(range(first + 5, first + 10))
        assert res["exc_off"][-1] == 0  # who is out of the node space is not part of the answer


# ---- 6. strip reuse ----------------------------------------------------------------------

def sink_lines(capfd):
    return [l for l in capfd.readouterr().err.splitlines() if l.startswith("psamd sink_topics:")]


def test_strip_reuse(monkeypatch, capfd):
    """The entries and strips stay on the device while the node space and the
    windows' shapes stay: the second run of an unchanged shape reports them
    kept; a join and a leave (a new graph_epoch) and a row that goes from one
    to three mask words have them re-cut.  Every run against (a)."""
    monkeypatch.setenv("PSAMD_DRAIN_TIMING", "1")
    rng = np.random.default_rng(77)
    n, seed = 500, 9

    def make():
        e = PE.Engine(n, 2, msg_window=8192, seed=seed)
        for t in (0, 1):
            e.topic_create(t, t, 2, 5)
            e.join(t, np.arange(2, n - 20))
        return e

    eng, ref = two(make)
    with eng, ref:
        eng.sink_set_topics([1, 0])
        capfd.readouterr()

        def run(topics):
            topics = np.asarray(topics, dtype=np.uint32)
            f = ref.publish(topics)
            ref.run()
            want = ref.drain_topics([1, 0])
            first = eng.publish(topics)
            assert first == f
            eng.run()
            res = eng.sink_take_topics()
            check_windows(res, [want])
            lines = sink_lines(capfd)
            assert len(lines) == 1, lines
            return res, lines[0]

        a, line = run(np.arange(64) % 2)
        assert " strips uploaded " in line
        b, line = run(np.arange(64) % 2)
        assert " strips kept " in line and " upload_bytes 0 " in line
        for k in KEYS[:-1]:
            assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a["ids"] + np.uint32(64), b["ids"])
        gone = int(rng.integers(2, 100))
        for e in (eng, ref):  # a join and a leave: a new node space
            e.join(0, np.arange(n - 20, n - 10))
            e.leave(0, [gone])
        c, line = run(np.arange(64) % 2)
        assert " strips uploaded " in line and c["n_nodes"][0, 1] != a["n_nodes"][0, 1]
        run(np.arange(64) % 2)  # (the leave is pruned behind the first message through it: one more node space)
        _, line = run(np.arange(64) % 2)
        assert " strips kept " in line
        _, line = run(np.zeros(64))  # 64 messages: one mask word
        d, line = run(np.zeros(130))  # 130: three
        assert " strips uploaded " in line and d["ids"].size == 130
        _, line = run(np.zeros(130))
        assert " strips kept " in line


# ---- 7. single window ---------------------------------------------------------------------

def test_single_window_equals_drain_topics():
    """One window: all ten arrays of ps_drain_topics, entry for entry; and
    ps_drain_topics after the run still answers for the last window."""
    n, root, parent, live = one_topic(0, 64)
    with PE.Engine(n, 3) as eng:
        for t in range(3):
            eng.set_tree(t, root, parent)
        eng.set_live(live)
        eng.sink_set_topics([2, 0, 1])
        eng.publish(np.arange(200) % 2)
        eng.run()
        res = eng.sink_take_topics()
        want = eng.drain_topics([2, 0, 1])
        assert res["n_windows"] == 1
        for k in KEYS:
            got = res[k][0] if k in ("topic_list", "n_nodes", "n_full") else res[k]
            assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
        assert counts(want)[0] > 10 and want["ids"].size == 200
    with PE.Engine(n, 1, msg_window=64) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.sink_set_topics([0])
        first = eng.publish(np.zeros(100))
        eng.run()
        res = eng.sink_take_topics()
        last = eng.drain_topics([0])
        assert res["n_windows"] == 2 and last["ids"].tolist() == list(range(first + 64, first + 100))
        assert np.array_equal(res["ids"][64:], last["ids"])


# ---- 8. caps ------------------------------------------------------------------------------

def caps_engines(seed=81):
    n, root, parent, live = one_topic(0, seed)

    def make():
        e = PE.Engine(n, 2, msg_window=64)
        e.set_tree(0, root, parent)
        e.set_tree(1, root, parent)
        e.set_live(live)
        return e

    topics = np.concatenate([np.arange(256) % 2, np.zeros(40)]).astype(np.uint32)  # topic 0: 3 windows, topic 1: 2
    return make, topics


def test_caps(monkeypatch):
    """Private lists (through the seam), so that every count is large.  The
    engine's own caps hold the run, which is (a) summed; so do the exact ones;
    each cap one short gives PS_E_RANGE with n_windows, n_nodes, n_full and
    exc_off exact; the overflow comes in the last window then, and the
    windows before are exact."""
    seam(monkeypatch)
    make, topics = caps_engines()
    chunks = window_chunks(topics, 64)
    assert len(chunks) == 3
    eng, ref = two(make)
    with eng, ref:
        eng.sink_set_topics([0, 1])
        first = eng.publish(topics)
        eng.run()
        want = eng.sink_take_topics()
        steps = stepped(ref, chunks, topics, None, [0, 1], first)
        check_windows(want, steps)
        n_exc, n_lists, total = counts(want)
        assert (n_exc, n_lists, total) == tuple(sum(c) for c in zip(*(counts(r) for r in steps)))
        assert n_exc > 1000 and n_lists > 500
        exact = dict(exc_cap=n_exc, list_cap=n_lists, id_cap=total)

        def again(**caps):
            eng.sink_set_topics([0, 1], **caps)
            f = eng.publish(topics)
            eng.run()
            return f

        f = again(**exact)
        got = eng.sink_take_topics()
        got["ids"] = got["ids"] - np.uint32(f - first)
        same(got, want)
        e2, l2 = int(want["exc_off"][4]), int(np.sum(want["exc_list"][:int(want["exc_off"][4])] != NONE))
        for short in exact:
            caps = dict(exact)
            caps[short] -= 1
            f = again(**caps)
            part = refused(eng)
            assert part["n_windows"] == 3
            for k in ("n_nodes", "n_full", "exc_off"):
                assert np.array_equal(part[k], want[k]), (short, k)
            # the first two windows fit: their entries are exact
            assert np.array_equal(part["topic_list"][:2], want["topic_list"][:2])
            assert np.array_equal(part["head"]("exc_peer", e2), want["exc_peer"][:e2])
            assert np.array_equal(part["head"]("exc_list", e2), want["exc_list"][:e2])
            assert np.array_equal(part["head"]("list_off", l2 + 1), want["list_off"][:l2 + 1])
            i2 = int(want["list_off"][l2])
            assert np.array_equal(part["head"]("ids", i2) - np.uint32(f - first), want["ids"][:i2])
        f = again(exc_cap=n_exc + 7, list_cap=n_lists + 1, id_cap=total + 1000)  # room to spare
        got = eng.sink_take_topics()
        got["ids"] = got["ids"] - np.uint32(f - first)
        same(got, want)


def test_overflow_in_the_second_of_three_windows(monkeypatch):
    """An id cap that the second window passes: PS_E_RANGE, every window's
    n_nodes, n_full and exc_off exact, the first window's entries exact."""
    seam(monkeypatch)
    make, topics = caps_engines(83)
    with make() as eng:
        eng.sink_set_topics([0, 1])
        first = eng.publish(topics)
        eng.run()
        want = eng.sink_take_topics()
        n = 2
        e1 = int(want["exc_off"][n])
        l1 = int(np.sum(want["exc_list"][:e1] != NONE))
        i1 = int(want["list_off"][l1])
        for caps in (dict(id_cap=i1 + 1), dict(list_cap=l1 + 1), dict(exc_cap=e1 + 1)):
            eng.sink_set_topics([0, 1], **caps)
            f = eng.publish(topics)
            eng.run()
            part = refused(eng)
            assert part["n_windows"] == 3
            for k in ("n_nodes", "n_full", "exc_off"):
                assert np.array_equal(part[k], want[k]), (caps, k)
            assert np.array_equal(part["topic_list"][0], want["topic_list"][0])
            assert np.array_equal(part["head"]("exc_peer", e1), want["exc_peer"][:e1])
            assert np.array_equal(part["head"]("exc_list", e1), want["exc_list"][:e1])
            assert np.array_equal(part["head"]("list_off", l1 + 1), want["list_off"][:l1 + 1])
            assert np.array_equal(part["head"]("ids", i1) - np.uint32(f - first), want["ids"][:i1])


# ---- 9. pipelined -------------------------------------------------------------------------

def sink_pipelined(e, batches):
    """publish; run_async; (wait; sink_take_topics of the previous)."""
    views, res, over = [], [], 0
    for i, b in enumerate(batches):
        e.publish(b)
        e.run_async()
        if i:
            st = e.wait()
            res.append(stats_key(st))
            over += st.overlapped
            views.append(e.sink_take_topics())
    st = e.wait()
    res.append(stats_key(st))
    over += st.overlapped
    views.append(e.sink_take_topics())
    return views, res, over


def sink_blocking(e, batches):
    views, res = [], []
    for b in batches:
        e.publish(b)
        res.append(stats_key(e.run()))
        views.append(e.sink_take_topics())
    return views, res


def compare_sink_runs(out, n_batches):
    assert sum(v["ids"].size for v in out[0][0]) > 0
    for i in range(n_batches):
        assert out[0][0][i]["n_windows"] >= 2  # the batch was split
        same(out[1][0][i], out[0][0][i])
    assert out[1][1] == out[0][1]
    assert out[1][2] == out[0][2]


def step_check(make, batches, which, cap, order, views):
    """Reference (a) for the batches `which`: a stepping engine fed every batch
    before, then that batch window by window."""
    with make() as ref:
        first = 0
        for i, b in enumerate(batches):
            if i in which:
                check_windows(views[i], stepped(ref, window_chunks(b, cap), b, None, order, first))
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
    order = np.arange(len(wl.topics), dtype=np.uint32)[::-1].copy()

    def make():
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=cap, plan={"flood": 0})
        WL.build_engine_topics(e, wl)
        return e

    out = []
    for mode in ("blocking", "pipelined"):
        with make() as e:
            e.sink_set_topics(order)
            if mode == "blocking":
                views, res = sink_blocking(e, batches)
            else:
                views, res, over = sink_pipelined(e, batches)
                print("twin windows:", kind, "overlapped", over)
                if kind == "even":
                    assert over >= 6, over  # windows ran as twins
            out.append((views, res, e.seen_digest()))
    compare_sink_runs(out, 12)
    step_check(make, batches, {0, 7}, cap, order, out[1][0])


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
    order = np.arange(len(wl.topics), dtype=np.uint32)

    def make():
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=cap, plan={"overlap_min_bytes": 0})
        WL.build_engine_topics(e, wl)
        e.set_live(live)
        return e

    # (every non-root node may be a record: the engine's 65,536 a window may not hold the dead peers' subtrees)
    nodes = sum(len(ts.join_order) + 1 for ts in wl.topics)
    exc_cap = nodes * (max(int(np.bincount(b).max()) for b in batches) // cap + 1)
    out = []
    for mode in ("blocking", "pipelined"):
        with make() as e:
            e.sink_set_topics(order, exc_cap=exc_cap)
            if mode == "blocking":
                views, res = sink_blocking(e, batches)
                assert res[-1][2] >= 12  # a deep window (rounds)
                assert int(views[0]["exc_off"][-1]) > 1000  # the dead peers and what hangs below them
            else:
                views, res, _ = sink_pipelined(e, batches)
                print("deep windows:", kind, "overlapped", e.overlapped_windows())
                if kind == "even":
                    assert e.overlapped_windows() >= 5
            out.append((views, res, e.seen_digest()))
    compare_sink_runs(out, 8)
    step_check(make, batches, {1, 6}, cap, order, out[1][0])


# ---- 10. rules ----------------------------------------------------------------------------

def test_rules():
    rng = np.random.default_rng(82)
    n, root = 2000, 0
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 2, msg_window=512, plan={"flood": 0}) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        with pytest.raises(PE.EngineError) as ei:
            eng.sink_take_topics()
        assert ei.value.code == E_NOTREADY  # no sink, no run
        eng.sink_set_topics([0])
        with pytest.raises(PE.EngineError) as ei:
            eng.sink_take_topics()
        assert ei.value.code == E_NOTREADY  # no run yet
        firsts = []
        for _ in range(2):  # two runs enqueued and not taken
            firsts.append(eng.publish(np.zeros(1000)))
            eng.run_async()
        third = eng.publish(np.zeros(700))
        with pytest.raises(PE.EngineError) as ei:
            eng.run_async()  # the third: refused, its messages stay pending
        assert ei.value.code == E_STATE
        assert raw_set(eng, [0]) == E_STATE  # runs in flight
        eng.wait()
        eng.wait()
        with pytest.raises(PE.EngineError) as ei:
            eng.run()  # still both untaken
        assert ei.value.code == E_STATE
        # the take call of the other kind completes nothing
        with pytest.raises(PE.EngineError) as ei:
            eng.sink_take()
        assert ei.value.code == E_STATE
        for first in firsts:
            r = eng.sink_take_topics()
            assert r["n_windows"] == 2 and r["list_off"].tolist() == [0, 512, 1000]
            assert r["ids"].tolist() == list(range(first, first + 1000)) and r["n_full"].tolist() == [[n - 1]] * 2
        st = eng.run()  # the same messages, after a take
        assert st.windows == 2 and st.deliveries == 700 * (n - 1)
        r = eng.sink_take_topics()
        assert r["list_off"].tolist() == [0, 512, 700] and r["ids"].tolist() == list(range(third, third + 700))
        # a duplicate or a topic out of range keeps the old sink
        assert raw_set(eng, [0, 0]) == E_INVAL
        assert raw_set(eng, [0, 2]) == E_RANGE
        first = eng.publish(np.zeros(100))
        eng.run()
        r = eng.sink_take_topics()
        assert r["topic_list"].shape == (1, 1) and r["ids"].tolist() == list(range(first, first + 100))
        # each set call replaces the other kind and discards what was not taken
        eng.publish(np.zeros(100))
        eng.run()
        eng.sink_set([0, 0], [5, 6])
        for take in (eng.sink_take, eng.sink_take_topics):
            with pytest.raises(PE.EngineError) as ei:
                take()
            assert ei.value.code == E_NOTREADY
        first = eng.publish(np.zeros(100))
        eng.run()
        with pytest.raises(PE.EngineError) as ei:
            eng.sink_take_topics()
        assert ei.value.code == E_STATE
        wl, off, ids = eng.sink_take()  # ... and the query result is still there
        assert wl.shape == (1, 2) and ids.tolist() == list(range(first, first + 100))
        eng.publish(np.zeros(100))
        eng.run()
        eng.sink_set_topics([1, 0])
        with pytest.raises(PE.EngineError) as ei:
            eng.sink_take_topics()
        assert ei.value.code == E_NOTREADY
        first = eng.publish(np.ones(100))
        eng.run()
        with pytest.raises(PE.EngineError) as ei:
            eng.sink_take()
        assert ei.value.code == E_STATE
        r = eng.sink_take_topics()
        assert r["topic_list"].tolist() == [[0, NONE]] and r["ids"].tolist() == list(range(first, first + 100))
        # n == 0 clears, from either call
        for clear in (lambda: eng.sink_set_topics([]), lambda: eng.sink_set([], [])):
            eng.sink_set_topics([0])
            clear()
            eng.publish(np.zeros(10))
            eng.run()
            for take in (eng.sink_take, eng.sink_take_topics):
                with pytest.raises(PE.EngineError) as ei:
                    take()
                assert ei.value.code == E_NOTREADY
        # a run without a message: a valid, empty result, written by the host
        eng.sink_set_topics([0, 1])
        eng.run()
        r = eng.sink_take_topics()
        assert r["n_windows"] == 0 and r["topic_list"].shape == (0, 2)
        assert r["exc_off"].tolist() == [0] and r["list_off"].tolist() == [0] and r["ids"].size == 0


def test_view_lifetime():
    wl = WL.cfg3(60_000, 16, 4000)
    batches = [vary(wl.msg_topics, i, 5) for i in range(4)]
    order = np.arange(len(wl.topics), dtype=np.uint32)
    with PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=splitting_window(batches),
                   plan={"flood": 0}) as e:
        WL.build_engine_topics(e, wl)
        e.sink_set_topics(order)
        for i in range(3):
            e.publish(batches[i])
            e.run_async()
            e.wait()
            view = e.sink_take_topics(copy=False)
            kept = {k: (v.copy() if k != "n_windows" else v) for k, v in view.items()}
            assert kept["ids"].size > 0 and kept["n_windows"] >= 2
            e.publish(batches[i + 1])
            e.run_async()  # the first run after its own: the view stays
            same(view, kept)
            e.wait()
            same(view, kept)
            e.sink_take_topics()


def test_drain_slots_stay_independent():
    """The audience sink beside drain_topics_begin / _end, drain_begin and the
    synchronous drain_topics of the last window: all agree, and the drains'
    slots are their own."""
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
        eng.sink_set_topics([0])
        first = eng.publish(np.zeros(700))
        eng.run_async()
        eng.drain_topics_begin([0])
        eng.drain_begin(qt, qp)
        sync = eng.drain_topics([0])
        eng.wait()
        res = eng.sink_take_topics()
        assert res["n_windows"] == 3
        bl = (res["list_off"].size - 1) - (sync["list_off"].size - 1)
        be = int(res["exc_off"][2])
        assert res["topic_list"][2].tolist() == [bl] and sync["topic_list"].tolist() == [0]
        assert np.array_equal(res["n_full"][2], sync["n_full"]) and np.array_equal(res["n_nodes"][2], sync["n_nodes"])
        assert np.array_equal(res["exc_off"][2:] - np.uint64(be), sync["exc_off"])
        assert np.array_equal(res["exc_peer"][be:], sync["exc_peer"]) and np.all(res["exc_list"] == NONE)
        assert np.array_equal(res["ids"][int(res["list_off"][bl]):], sync["ids"])
        got = eng.drain_topics_end()
        for k in KEYS:
            assert np.array_equal(got[k], sync[k]), k
        off, ids = eng.drain_end()[:2]
        assert off.size == 251
        assert topic_ids(res, 0) == list(range(first, first + 700))


def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(3)]
    try:
        # an engine whose sink is set takes no ranks
        engines[2].sink_set_topics([0])
        with pytest.raises(PE.EngineError) as ei:
            engines[2].dist_init_loopback(lb, 0, PE.PART_PEER)
        assert ei.value.code == E_STATE
        for r, e in enumerate(engines[:2]):
            e.dist_init_loopback(lb, r, PE.PART_PEER)
            e.set_tree(0, root, parent)
            assert raw_set(e, [0]) == E_STATE  # one rank only
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
            with pytest.raises(PE.EngineError) as ei:
                e.sink_take_topics()
            assert ei.value.code == E_NOTREADY
    finally:
        for e in engines:
            e.close()
        lb.close()
