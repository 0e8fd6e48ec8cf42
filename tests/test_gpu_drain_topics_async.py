"""GPU: a topic's audience in two halves (ps_drain_topics_begin /
ps_drain_topics_end) -- ps_drain_topics' answer enqueued
behind a run that may still execute, the per-topic totals and the list
numbering computed on the device.  The comparison is always all ten outputs
(the eight arrays; n_lists and total are the sizes of list_off and ids)
against Engine.drain_topics of the same window, array for array: on a quiet
engine the same engine's, in the pipelined cases a second, blocking engine's.
The synchronous answer itself is checked against drain_shared over explicit
queries, and where a case has an oracle against that, by
test_gpu_drain_topics.check.

On a quiet engine the asynchronous call goes first: it builds the window's
tables on the device, and the synchronous call behind it reads the same ones
(the two builds may lay a paced mesh window out differently)."""
import ctypes as C
import threading

import numpy as np
import pytest

import psengine as PE
from psengine import workloads as WL
from test_gpu_drain_async import stats_key, vary
from test_gpu_drain_batch import oracle_lists, random_mesh2, random_tree, tree_hops
from test_gpu_drain_shared import one_topic, run_tree_case, shared
from test_gpu_drain_topics import (NARROW_STRIP, WIDE_STRIP, audience, check, kids_of, per_peer, under, well_formed,
                                   windows_of)

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U32P = C.POINTER(C.c_uint32)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
KEYS = ("topic_list", "n_nodes", "n_full", "exc_off", "exc_peer", "exc_list", "list_off", "ids")


def same(got, want):
    assert set(got) == set(want) == set(KEYS)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def begin_end(eng, topics, **caps):
    eng.drain_topics_begin(topics, **caps)
    return eng.drain_topics_end()


def refused(eng, topics, **caps):
    """A drain whose answer exceeds a cap: PS_E_RANGE from the end call; what it still gives."""
    eng.drain_topics_begin(topics, **caps)
    with pytest.raises(PE.EngineError) as ei:
        eng.drain_topics_end()
    assert ei.value.code == E_RANGE
    return ei.value.partial


def raw_begin(eng, topics, exc_cap=0, list_cap=0, id_cap=0):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    return eng._L.ps_drain_topics_begin(eng._h, t.ctypes.data_as(U32P), t.size, exc_cap, list_cap, id_cap)


def check_quiet(eng, topics, window=None, sharing=True, **caps):
    """begin/end first, then drain_topics of the same window (itself checked
    against drain_shared); returns (the answer, per entry Q_t)."""
    got = begin_end(eng, topics, **caps)
    well_formed(got, len(topics))
    want, Q = check(eng, topics, window, sharing)
    same(got, want)
    return got, Q


def seam(monkeypatch):
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_DRAIN_SHARED", "private")


# ---- 1. strip and reduction edges -------------------------------------------------------

@pytest.mark.parametrize("n,n_msgs", [(NARROW_STRIP, 1), (NARROW_STRIP + 1, 1), (NARROW_STRIP + 2, 1), (WIDE_STRIP, 8300),
                                      (WIDE_STRIP + 1, 8300), (WIDE_STRIP + 2, 8300)])
def test_strip_edges(n, n_msgs):
    """N - 1 non-root nodes one below, at and one above a strip, for a 1-word
    and a 130-word row: the per-topic sum over one strip, exactly one, and two
    with one node in the second."""
    rng = np.random.default_rng(n + n_msgs)
    root = n // 2
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        first = eng.publish(np.zeros(n_msgs))
        eng.run()
        r, Q = check_quiet(eng, [0], {0: list(range(first, first + n_msgs))})
        assert r["n_nodes"][0] == n - 1 == r["n_full"][0] and r["exc_peer"].size == 0
        assert r["topic_list"][0] == 0 and r["ids"].tolist() == list(range(first, first + n_msgs))


@pytest.mark.parametrize("n,n_msgs,strip", [(5000, 3, NARROW_STRIP), (100, 8300, WIDE_STRIP)])
def test_live_mask_across_a_strip_boundary(n, n_msgs, strip):
    """The last node of the first strip and the first node of the second are
    masked: an entry's records start in one strip and go on in the next."""
    rng = np.random.default_rng(n)
    root = 1
    parent = random_tree(rng, n, root)
    kids = kids_of(parent)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        nodes = audience(eng, [0])[0]
        masked = {int(nodes[strip - 1]), int(nodes[strip])}
        live = np.ones(n, dtype=np.uint8)
        live[list(masked)] = 0
        eng.set_live(live)
        first = eng.publish(np.zeros(n_msgs))
        eng.run()
        r, Q = check_quiet(eng, [0], {0: list(range(first, first + n_msgs))})
        cut = set(masked)
        for p in masked:
            cut |= under(kids, p)
        assert set(r["exc_peer"].tolist()) == cut and np.all(r["exc_list"] == NONE)
        assert r["n_full"][0] == n - 1 - len(cut) > 0


@pytest.mark.parametrize("order", [[0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1], [1], [3, 2], [2, 1, 3, 0]])
def test_entries_without_strips_between_entries_with_them(order):
    """A 1-word and a 130-word topic, an idle one and a created-but-empty
    one: entries that have no strip lie before, between and behind entries
    that have many."""
    n, root, parent, live = one_topic(0, 77)
    topics = np.concatenate([np.zeros(10), np.ones(8300)]).astype(np.uint32)
    with PE.Engine(n, 4) as eng:
        for t in range(3):
            eng.set_tree(t, root, parent)
        eng.topic_create(3, root)
        eng.set_live(live)
        first = eng.publish(topics)
        eng.run()
        window = {0: list(range(first, first + 10)), 1: list(range(first + 10, first + 8310)), 2: [], 3: []}
        r, Q = check_quiet(eng, order, window)
        hop = tree_hops(parent, root, live)
        reached = sum(1 for p in range(n) if p != root and hop[p] != 0xFF)
        for i, t in enumerate(order):
            assert r["n_nodes"][i] == (0 if t == 3 else n - 1)
            assert r["n_full"][i] == (reached if t < 2 else 0)
            assert (r["topic_list"][i] == NONE) == (t >= 2)
            assert r["exc_off"][i + 1] - r["exc_off"][i] == (n - 1 - reached if t < 2 else 0)
        assert r["ids"].size == sum(len(window[t]) for t in order)


# ---- 2. numbering -------------------------------------------------------------------------

@pytest.mark.parametrize("c", [0, 1, 63, 64, 65, 257])
def test_exception_counts(c, monkeypatch):
    """c exceptions in one topic, each with a list of its own (through the
    seam every full row is one; c = 0: no seam, every row full): record keys
    below, at and above a wave and a block of the numbering pass."""
    if c:
        seam(monkeypatch)
    n = c + 1 if c else 300
    rng = np.random.default_rng(100 + c)
    parent = random_tree(rng, n, 0)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        first = eng.publish(np.zeros(70))
        eng.run()
        r, Q = check_quiet(eng, [0], {0: list(range(first, first + 70))}, sharing=not c)
        assert r["exc_peer"].size == c and np.array_equal(r["exc_list"], np.arange(c))
        assert r["list_off"].size - 1 == (c if c else 1) and r["ids"].size == 70 * (c if c else 1)


def test_none_exceptions_between_any_ones(monkeypatch):
    """Through the seam, with a subtree cut: the cut nodes' records create no
    list and lie between records that do."""
    seam(monkeypatch)
    rng = np.random.default_rng(51)
    n, root = 600, 0
    parent = random_tree(rng, n, root)
    kids = kids_of(parent)
    cut = max((p for p in range(n) if parent[p] == root), key=lambda p: len(under(kids, p)))
    below = under(kids, cut)
    assert len(below) >= 10
    live = np.ones(n, dtype=np.uint8)
    live[cut] = 0
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        first = eng.publish(np.zeros(150))
        eng.run()
        r, Q = check_quiet(eng, [0], {0: list(range(first, first + 150))}, sharing=False)
        none = np.flatnonzero(r["exc_list"] == NONE)
        some = np.flatnonzero(r["exc_list"] != NONE)
        assert set(r["exc_peer"][none].tolist()) == below | {cut}
        assert some.min() < none.max() and none.min() < some.max()  # a "none" record with "any" ones either side
        assert np.array_equal(r["exc_list"][some], np.arange(some.size)) and r["list_off"].size - 1 == some.size


@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4], [3, 0, 4, 1, 2], [1, 3], [2, 1, 0], [4, 3, 2]])
def test_shared_and_private_lists_over_several_topics(order):
    """A row of a mask-layout topic is full or empty within a window, so one
    topic has a shared list or private ones, never both; here a request
    interleaves the two: trees (topics 0, 2: a shared list, the masked
    subtrees as "none" records), paced meshes (topics 1, 3: a private list
    per node) and an idle tree (4).  A shared list's number then counts the
    private lists of the entries before it, and the other way round."""
    rng = np.random.default_rng(71)
    n, root, n_msgs = 500, 5, 120
    parent = random_tree(rng, n, root)
    rp, cl = random_mesh2(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with PE.Engine(n, 5) as eng:
        for t in (0, 2, 4):
            eng.set_tree(t, root, parent)
        for t in (1, 3):
            eng.set_children(t, root, rp, cl)
        eng.set_live(live)
        eng.publish(np.arange(n_msgs) % 4, rng.integers(0, 5, size=n_msgs))
        eng.run()
        r, Q = check_quiet(eng, order, None)
        k = 0
        for i, t in enumerate(order):
            e0, e1 = int(r["exc_off"][i]), int(r["exc_off"][i + 1])
            lists = r["exc_list"][e0:e1]
            if t in (0, 2):
                assert r["topic_list"][i] == k and r["n_full"][i] > 100 and e1 > e0 and np.all(lists == NONE)
                k += 1
            elif t in (1, 3):
                assert r["topic_list"][i] == NONE and e1 - e0 == Q[i].size > 400
                assert np.array_equal(lists, k + np.arange(e1 - e0))
                k += e1 - e0
            else:
                assert r["topic_list"][i] == NONE and e1 == e0 and r["n_full"][i] == 0
        assert r["list_off"].size - 1 == k


def test_private_lists_of_three_segments(monkeypatch):
    """8,300 messages: every private list takes three segments, the shared
    numbering's low key half counts them (test_exception_counts: one)."""
    seam(monkeypatch)
    rng = np.random.default_rng(83)
    n, root = 40, 3
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        first = eng.publish(np.zeros(8300))
        eng.run()
        r, Q = check_quiet(eng, [0], {0: list(range(first, first + 8300))}, sharing=False)
        assert r["list_off"].tolist() == [8300 * i for i in range(n)]
        assert np.array_equal(r["ids"].reshape(n - 1, 8300), np.tile(np.arange(first, first + 8300), (n - 1, 1)))


def test_paced_tree_through_the_seam(monkeypatch):
    """Level-aligned group-major rows read by count and emit, against the oracle."""
    seam(monkeypatch)
    eng, qt, qp, topics, hop, root, exp = run_tree_case("paced1")
    with eng:
        r, Q = check_quiet(eng, [1, 0], windows_of(qt, exp), sharing=False)
        want = windows_of(qt, exp)
        for i, t in enumerate((1, 0)):
            got = per_peer(r, Q, i)
            for p, ids in got.items():
                assert ids.tolist() == ([] if hop[p] == 0xFF else want[t]), (t, p)


# ---- 3. caps ------------------------------------------------------------------------------

def caps_case():
    n, root, parent, live = one_topic(0, 81)
    eng = PE.Engine(n, 2)
    eng.set_tree(0, root, parent)
    eng.set_tree(1, root, parent)
    eng.set_live(live)
    eng.publish(np.arange(100) % 2)
    eng.run()
    return eng


def counts(r):
    return int(r["exc_off"][-1]), r["list_off"].size - 1, r["ids"].size


def test_default_and_exact_caps():
    """Full rows share: two lists, 100 ids, the masked nodes as records.  The
    engine's caps hold the synchronous answer; so do the exact ones; an
    exception cap one short does not, and says how many there are."""
    with caps_case() as eng:
        got = begin_end(eng, [1, 0])
        want = eng.drain_topics([1, 0])
        same(got, want)
        n_exc, n_lists, total = counts(want)
        assert n_exc > 10 and n_lists == 2 and total == 100
        same(begin_end(eng, [1, 0], exc_cap=n_exc, list_cap=n_lists, id_cap=total), want)
        part = refused(eng, [1, 0], exc_cap=n_exc - 1, list_cap=n_lists, id_cap=total)
        for k in ("n_nodes", "n_full", "exc_off"):
            assert np.array_equal(part[k], want[k]), k
        part = refused(eng, [1, 0], exc_cap=n_exc, list_cap=1, id_cap=total)
        assert part["n_lists"] == 2 and np.array_equal(part["exc_off"], want["exc_off"])
        part = refused(eng, [1, 0], exc_cap=n_exc, list_cap=n_lists, id_cap=total - 1)
        assert (part["n_lists"], part["total"]) == (2, 100)
        same(begin_end(eng, [1, 0]), want)


def test_caps_one_short_through_the_seam(monkeypatch):
    """Private lists, so that every count is large: each cap one short gives
    PS_E_RANGE with n_nodes, n_full and exc_off exact (and the list count
    where the exceptions fit), and a drain of the same window with room
    behind it is correct."""
    seam(monkeypatch)
    with caps_case() as eng:
        got = begin_end(eng, [0, 1])  # (under the seam the engine's caps: a list per node)
        want = eng.drain_topics([0, 1])
        same(got, want)
        n_exc, n_lists, total = counts(want)
        assert n_exc == 2 * 299 and 100 < n_lists < n_exc and total == n_lists * 50
        exact = dict(exc_cap=n_exc, list_cap=n_lists, id_cap=total)
        same(begin_end(eng, [0, 1], **exact), want)
        for short in exact:
            caps = dict(exact)
            caps[short] -= 1
            part = refused(eng, [0, 1], **caps)
            for k in ("n_nodes", "n_full", "exc_off"):
                assert np.array_equal(part[k], want[k]), (short, k)
            if short != "exc_cap":
                assert part["n_lists"] == n_lists
            if short == "id_cap":
                assert part["total"] == total
            same(begin_end(eng, [0, 1], **exact), want)
        same(begin_end(eng, [0, 1], exc_cap=n_exc + 7, list_cap=n_lists + 1, id_cap=total + 1000), want)  # room to spare


def test_more_exceptions_than_the_default_cap():
    """70,001 nodes, everything but the root's children cut: more than 65,536
    records.  The engine's caps refuse with exc_off exact; the retry with
    exc_cap = exc_off[n] is the synchronous answer."""
    rng = np.random.default_rng(17)
    n, root = 70_001, 0
    parent = random_tree(rng, n, root)
    first_level = [p for p in range(n) if parent[p] == root]
    live = np.zeros(n, dtype=np.uint8)
    live[[root] + first_level] = 1
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.publish(np.zeros(70))
        eng.run()
        part = refused(eng, [0])
        n_exc = n - 1 - len(first_level)
        assert n_exc > 65_536 and part["exc_off"].tolist() == [0, n_exc]
        assert part["n_full"].tolist() == [len(first_level)] and part["n_nodes"].tolist() == [n - 1]
        got = begin_end(eng, [0], exc_cap=int(part["exc_off"][-1]))
        same(got, eng.drain_topics([0]))
        assert got["exc_peer"].size == n_exc and np.all(got["exc_list"] == NONE) and got["ids"].size == 70


# ---- 4. pipelined -------------------------------------------------------------------------

def pipelined(e, batches, topics, **caps):
    """publish, run_async, drain_topics_begin, (wait, drain_topics_end of the previous)."""
    views, res, over = [], [], 0
    for i, b in enumerate(batches):
        e.publish(b)
        e.run_async()
        e.drain_topics_begin(topics, **caps)
        if i:
            st = e.wait()
            res.append(stats_key(st))
            over += st.overlapped
            views.append(e.drain_topics_end())
    st = e.wait()
    res.append(stats_key(st))
    over += st.overlapped
    views.append(e.drain_topics_end())
    return views, res, over


def blocking(e, batches, topics):
    views, res = [], []
    for b in batches:
        e.publish(b)
        res.append(stats_key(e.run()))
        views.append(e.drain_topics(topics))
    return views, res


def compare_runs(out, n_batches):
    assert sum(v["ids"].size for v in out[0][0]) > 0
    for i in range(n_batches):
        same(out[1][0][i], out[0][0][i])
    assert out[1][1] == out[0][1]
    assert out[1][2] == out[0][2]


def test_pipelined_twin_windows():
    wl = WL.cfg3(60_000, 16, 4000)
    batches = [vary(wl.msg_topics, i, 5) for i in range(12)]
    topics = np.arange(len(wl.topics), dtype=np.uint32)
    out = []
    for mode in ("blocking", "pipelined"):
        with PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, plan={"flood": 0}) as e:  # (k_flood windows run no twins)
            WL.build_engine_topics(e, wl)
            if mode == "blocking":
                views, res = blocking(e, batches, topics)
            else:
                views, res, over = pipelined(e, batches, topics)
                assert over >= 6, over  # windows ran as twins
            out.append((views, res, e.seen_digest()))
    compare_runs(out, 12)


def test_pipelined_deep_overlapped_windows():
    wl = WL.cfg3(200_000, 16, 5000)
    rng = np.random.default_rng(11)
    live = (rng.random(wl.n_peers) >= 0.03).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    batches = [vary(wl.msg_topics, i, 7) for i in range(8)]
    topics = np.arange(len(wl.topics), dtype=np.uint32)
    out = []
    n_nodes = 0
    for mode in ("blocking", "pipelined"):
        with PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, plan={"overlap_min_bytes": 0}) as e:
            WL.build_engine_topics(e, wl)
            e.set_live(live)
            if mode == "blocking":
                views, res = blocking(e, batches, topics)
                assert res[-1][2] >= 12  # a deep window (rounds)
                n_nodes = int(views[0]["n_nodes"].sum())
                assert int(views[0]["exc_off"][-1]) > 1000  # the dead peers and what hangs below them
            else:
                views, res, _ = pipelined(e, batches, topics, exc_cap=n_nodes)  # (every non-root node may be a record)
                assert e.overlapped_windows() >= 5
            out.append((views, res, e.seen_digest()))
    compare_runs(out, 8)


# ---- 5. rules -----------------------------------------------------------------------------

def test_slot_rules_with_three_kinds():
    rng = np.random.default_rng(81)
    n, root = 2000, 0
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 2, plan={"flood": 0}) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        assert raw_begin(eng, [0]) == E_NOTREADY  # no run yet
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_topics_end()
        assert ei.value.code == E_NOTREADY  # none outstanding
        firsts = []
        for _ in range(2):  # two runs enqueued, a drain begun behind each before any wait
            firsts.append(eng.publish(np.zeros(1000)))
            eng.run_async()
            eng.drain_topics_begin([0])
        assert raw_begin(eng, [0]) == E_STATE  # a third of this kind
        qp = rng.choice(n, 50, replace=False)
        qt = np.zeros(50, dtype=np.uint32)
        for begin in (eng.drain_begin, eng.drain_shared_begin):  # ... or of the others
            with pytest.raises(PE.EngineError) as ei:
                begin(qt, qp)
            assert ei.value.code == E_STATE
        eng.wait()
        eng.wait()
        for end in (eng.drain_end, eng.drain_shared_end):  # the wrong kinds: complete nothing
            with pytest.raises(PE.EngineError) as ei:
                end()
            assert ei.value.code == E_STATE
        for first in firsts:
            r = eng.drain_topics_end()
            assert r["n_full"].tolist() == [n - 1] and r["ids"].tolist() == list(range(first, first + 1000))
        assert raw_begin(eng, [0, 2]) == E_RANGE  # a topic out of range
        assert raw_begin(eng, [0, 1, 0]) == E_INVAL  # a topic named twice
        # no slot leaked: two more fit; every pair of kinds, ended in order by the end call of its kind
        want_t = eng.drain_topics([0, 1])
        want_s = shared(eng, qt, qp)
        kinds = {"plain": (lambda: eng.drain_begin(qt, qp), eng.drain_end),
                 "shared": (lambda: eng.drain_shared_begin(qt, qp), eng.drain_shared_end),
                 "topics": (lambda: eng.drain_topics_begin([0, 1]), eng.drain_topics_end)}
        for a, b in (("topics", "plain"), ("shared", "topics"), ("topics", "shared"), ("plain", "topics")):
            kinds[a][0]()
            kinds[b][0]()
            assert raw_begin(eng, [0]) == E_STATE
            for k in (a, b):
                for other in kinds:
                    if other != k:
                        with pytest.raises(PE.EngineError) as ei:
                            kinds[other][1]()
                        assert ei.value.code == E_STATE
                got = kinds[k][1]()
                if k == "topics":
                    same(got, want_t)
                elif k == "shared":
                    assert all(np.array_equal(x, y) for x, y in zip(got, want_s))
        with pytest.raises(PE.EngineError) as ei:
            eng.drain_topics_end()
        assert ei.value.code == E_NOTREADY
        # an empty drain beside a full one
        eng.drain_topics_begin([])
        eng.drain_topics_begin([1])
        r = eng.drain_topics_end()
        assert r["exc_off"].tolist() == [0] and r["list_off"].tolist() == [0]
        assert r["topic_list"].size == 0 and r["ids"].size == 0 and r["exc_peer"].size == 0
        r = eng.drain_topics_end()
        assert r["topic_list"].tolist() == [NONE] and r["n_nodes"].tolist() == [n - 1] and r["n_full"].tolist() == [0]
        assert r["exc_off"].tolist() == [0, 0] and r["list_off"].tolist() == [0]  # (topic 1 is idle)


def test_view_lifetime():
    """The lent view is unchanged by the next run and its wait (until the next begin)."""
    rng = np.random.default_rng(6)
    n, root = 3000, 0
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with PE.Engine(n, 1, plan={"flood": 0}) as e:
        e.set_tree(0, root, parent)
        e.set_live(live)
        for i in range(3):
            e.publish(np.zeros(500 + 64 * i))
            e.run_async()
            e.drain_topics_begin([0])
            e.wait()
            view = e.drain_topics_end(copy=False)
            kept = {k: v.copy() for k, v in view.items()}
            assert kept["ids"].size == 500 + 64 * i and kept["exc_peer"].size > 0
            e.publish(np.zeros(300))
            e.run_async()
            same(view, kept)
            e.wait()
            same(view, kept)


def test_mixed_with_synchronous_calls():
    """The device-built tables serve drain_topics and drain_shared of the same
    window while the drain is outstanding; tables the host built serve the
    asynchronous call; and a view is its own window's, whatever runs behind."""
    rng = np.random.default_rng(91)
    n, root = 2000, 4
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with PE.Engine(n, 1, plan={"flood": 0}) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        first = eng.publish(np.zeros(700))
        eng.run_async()
        eng.drain_topics_begin([0])  # (builds the tables on the device)
        sync = eng.drain_topics([0])
        qp = rng.choice(n, 100, replace=False)
        lists, off, ids = shared(eng, np.zeros(100, dtype=np.uint32), qp)
        assert off.tolist() == [0, 700] and ids.tolist() == list(range(first, first + 700))
        eng.wait()
        same(eng.drain_topics_end(), sync)
        same(check(eng, [0], {0: list(range(first, first + 700))})[0], sync)  # (the graph is read once no run is pending)
        # a live-mask change and a further run between begin and end: the view is batch k's
        first = eng.publish(np.zeros(650))
        eng.run_async()
        eng.drain_topics_begin([0])
        live2 = (rng.random(n) > 0.3).astype(np.uint8)
        live2[root] = 1
        eng.set_live(live2)
        eng.wait()
        eng.publish(np.zeros(100))
        eng.run()
        digest = eng.seen_digest()
        got = eng.drain_topics_end()
        assert np.array_equal(got["exc_peer"], sync["exc_peer"]) and got["n_full"][0] == sync["n_full"][0]
        assert got["ids"].tolist() == list(range(first, first + 650))
        sync2 = eng.drain_topics([0])  # (builds this window's tables on the host)
        assert sync2["exc_peer"].size > sync["exc_peer"].size
        same(begin_end(eng, [0]), sync2)
        assert eng.seen_digest() == digest


def test_refused_after_staging_takes_no_slot():
    """An id_cap above 2^30 is refused after the window's table block was
    staged in the slot: the call gives the slot up.  The next begin finds the
    tables kept; both slots are still free, and both views are the
    synchronous call's."""
    rng = np.random.default_rng(17)
    n, root, n_msgs = 40, 2, 50
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        first = eng.publish(np.zeros(n_msgs))
        eng.run()  # (no drain yet: the window's tables are not built)
        assert raw_begin(eng, [0], 1, 1, (1 << 30) + 1) == E_RANGE
        eng.drain_topics_begin([0])
        eng.drain_topics_begin([0])
        assert raw_begin(eng, [0]) == E_STATE  # both slots taken: the refused call took none
        got = [eng.drain_topics_end(), eng.drain_topics_end()]
        want = eng.drain_topics([0])
        assert want["list_off"].tolist() == [0, n_msgs] and want["ids"].tolist() == list(range(first, first + n_msgs))
        for g in got:
            same(g, want)


def test_last_window_only():
    rng = np.random.default_rng(61)
    n, root = 400, 2
    parent = random_tree(rng, n, root)
    with PE.Engine(n, 1, msg_window=128) as eng:
        eng.set_tree(0, root, parent)
        first = eng.publish(np.zeros(300))
        st = eng.run()
        assert st.windows == 3
        r, _ = check_quiet(eng, [0])
        ids = r["ids"]
        assert r["list_off"].size - 1 == 1 and 0 < ids.size <= 128
        assert ids.tolist() == list(range(int(ids[0]), first + 300))  # one window, ending with the run's last message
        assert r["n_full"][0] == n - 1


def test_dead_subtree_stale_rows():
    """The rows below the cut keep the first window's bits under a stale generation."""
    rng = np.random.default_rng(51)
    n, root = 600, 0
    parent = random_tree(rng, n, root)
    kids = kids_of(parent)
    cut = max((p for p in range(n) if parent[p] == root), key=lambda p: len(under(kids, p)))
    below = under(kids, cut)
    assert len(below) >= 10
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        first = eng.publish(np.zeros(200))
        eng.run()
        r, _ = check_quiet(eng, [0], {0: list(range(first, first + 200))})
        assert r["n_full"][0] == n - 1 and r["exc_peer"].size == 0
        live = np.ones(n, dtype=np.uint8)
        live[cut] = 0
        eng.set_live(live)
        first = eng.publish(np.zeros(150))
        eng.run()
        r, _ = check_quiet(eng, [0], {0: list(range(first, first + 150))})
        assert set(r["exc_peer"].tolist()) == below | {cut} and np.all(r["exc_list"] == NONE)
        assert r["n_full"][0] == n - 2 - len(below)


def test_after_churn_with_a_gpu_rebuild():
    """Join, leave and drop, then runs (test_gpu_drain_topics.test_after_churn):
    the second run's node space was rebuilt on the GPU, and the drain enqueued
    behind it, before its wait, follows the new one."""
    n, joined, seed = 400, 300, 3
    with PE.Engine(n, 1, seed=seed) as eng:
        eng.topic_create(0, 0, 2, 5)
        eng.join(0, np.arange(1, joined))
        eng.publish(np.zeros(20))
        eng.run()
        r, Q = check_quiet(eng, [0])
        assert r["n_nodes"][0] == joined - 1 == r["n_full"][0]
        kids = kids_of(eng.parents(0))
        dead = max((p for p in kids if p != 0), key=lambda p: (len(kids[p]), len(under(kids, p))))
        childless = [p for p in range(1, joined) if p not in kids and p != dead][:10]
        eng.leave(0, childless)
        eng.join(0, np.arange(joined, joined + 40))
        eng.drop(0, [dead])
        eng.publish(np.zeros(5))
        st = eng.run()  # the drop's repair, and behind the messages the prune of the peers that left
        assert st.windows >= 2
        first = eng.publish(np.zeros(5))
        eng.run_async()  # over the node space rebuilt after that prune
        eng.drain_topics_begin([0])
        eng.wait()
        got = eng.drain_topics_end()
        rep = eng.build_report()
        assert rep["last_kind"] == "gpu" and rep["fallbacks"] == 0, rep
        want, Q = check(eng, [0])
        same(got, want)
        members = set(Q[0].tolist())
        assert dead not in members and members & set(range(joined, joined + 40))
        assert got["topic_list"][0] == 0 and got["ids"].tolist() == list(range(first, first + 5))


def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(2)]
    try:
        for k, e in enumerate(engines):
            e.dist_init_loopback(lb, k, PE.PART_PEER)
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
            assert raw_begin(e, [0]) == E_STATE  # one rank only
            with pytest.raises(PE.EngineError) as ei:
                e.drain_topics_end()
            assert ei.value.code == E_NOTREADY  # no slot was taken
    finally:
        for e in engines:
            e.close()
        lb.close()
