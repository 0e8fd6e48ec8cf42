"""GPU: ps_dist_cut -- a rank's share of ps_peer_cut on
loopback ranks, and the same call on one rank.

Every sharded case is checked twice (check_cut): per rank, every array equals
the reference's per-node values masked to the nodes the rank owns
(tests/dist_cut_ref.py) -- a rank that blames a node it does not own fails even
where the sum comes out right --, and the ranks' sum equals a one-rank
engine's ps_peer_cut on the same trees, live mask, publishes and request, bit
for bit, with identities 1 (sum(missed) = the possible deliveries minus the
run's) and 2 (sum(lost) = sum(missed)).  The collective call is made from one
thread per rank.  What a shape relies on (cut points behind remote parents, a
remote root, subtrees across ranks, levels whose words decide nothing) is
asserted by name in tests/test_dist_cut_cpu.py.  No case here provokes a
mismatched collective, a transport failure or a fault."""
import ctypes as C
import threading

import numpy as np
import pytest

import cut_ref as CR
import dist_cut_ref as XC
import dist_ref as DR
import psengine as PE
from test_dist_cut_cpu import fan_live, path_dead
from test_gpu_churn import assert_builds, make_engine
from test_gpu_cut import raw_cut, same, untouched
from test_gpu_dist_report import PATHS, ROWS, Sharded, level_ends, raw as raw_report
from test_gpu_dist_report import untouched as report_untouched
from test_gpu_downstream import fan_tree, star
from test_gpu_drain_batch import random_mesh2, random_tree
from test_gpu_load import heap_tree, seam, shared_topics

pytestmark = pytest.mark.gpu

U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
FILL = 0xABABABABABABABAB


# ---- helpers ------------------------------------------------------------------------

def raw_dist_cut(eng, topics, which=(True, True, True, True)):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    a = [np.full(eng.n_peers, FILL, dtype=np.uint64) for _ in range(4)]
    rc = eng._L.ps_dist_cut(eng._h, t.ctypes.data_as(U32P) if t.size else None, t.size,
                            *(x.ctypes.data_as(U64P) if w else None for x, w in zip(a, which)))
    return rc, a


def dist_cuts(engines, req, which=None):
    """The collective call: one thread per rank, the same request on each;
    which[r]: the pointers rank r passes (None: all four, through the binding)."""
    out = [None] * len(engines)
    errs = []

    def go(r):
        try:
            if which is None:
                out[r] = engines[r].dist_cut(req)
            else:
                out[r] = raw_dist_cut(engines[r], req, which[r])
        except Exception as ex:  # noqa: BLE001
            errs.append((r, ex))

    th = [threading.Thread(target=go, args=(r,)) for r in range(len(engines))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "rank thread hung"
    assert not errs, errs
    return out


def check_cut(S, live, counts, req, deliveries=None, tag=""):
    """counts[t]: topic t's messages in the last window.  Per rank against the
    reference share; the ranks' sum against the one-rank engine's peer_cut."""
    n, world = S.trees[0].shape[0], S.world
    topics = [(S.roots[t], counts[t], S.trees[t]) for t in req]
    shares = XC.rank_cuts(n, live, topics, [S.owners[t] for t in req], world)
    got = dist_cuts(S.engines, req)
    for r in range(world):
        same(got[r], tuple(shares[r][k] for k in XC.NAMES), f"{tag} rank {r} of {world} request {list(req)}")
    total = tuple(sum(g[i] for g in got) for i in range(4))
    whole = S.one.peer_cut(req)
    same(total, whole, f"{tag} the ranks' sum, request {list(req)}")
    assert int(total[3].sum()) == int(total[0].sum()), f"{tag}: sum(lost) != sum(missed)"  # identity 2
    if deliveries is not None:  # identity 1, where the request names every topic of the window
        possible = sum(c * (int((S.owners[t] >= 0).sum()) - 1) for t, c in enumerate(counts) if t in req)
        assert int(total[0].sum()) == possible - deliveries, f"{tag}: sum(missed) != possible - deliveries"
    return got, total


# ---- 1. row widths on ranks whose node 0 is not the root ---------------------------

@pytest.fixture(scope="module")
def width_tree():
    return DR.row_width_case()


@pytest.mark.parametrize("n_msgs,plan,words", ROWS)
def test_row_widths(width_tree, n_msgs, plan, words):
    """600 peers, world 3 under the peer hash, rows of 1, 2, 64, 65 and 130
    words: 26 cut points, 17 of them behind a remote parent, on every rank."""
    parent, root, live = width_tree
    with Sharded(3, [parent], [root], plan=plan) as S:
        stats, st1 = S.run(live, np.zeros(n_msgs))
        assert sum(st.deliveries for st in stats) == st1.deliveries
        got, total = check_cut(S, live, [n_msgs], [0], st1.deliveries, f"{words} words")
        assert int(total[1].sum()) == 26 and [int(g[1].sum()) for g in got] == [6, 10, 10]


@pytest.mark.parametrize("copy", PATHS)
def test_the_cut_does_not_depend_on_the_data_path(width_tree, copy):
    parent, root, live = width_tree
    with Sharded(3, [parent], [root], copy=copy) as S:
        _, st1 = S.run(live, np.zeros(100))
        check_cut(S, live, [100], [0], st1.deliveries, f"path {copy}")


@pytest.mark.parametrize("n_msgs,words", DR.GROUP_CASES)
def test_start_groups(width_tree, n_msgs, words):
    """Starts 0..3 in turn: k counted through node-major start-group blocks."""
    parent, root, live = width_tree
    with Sharded(3, [parent], [root]) as S:
        _, st1 = S.run(live, np.zeros(n_msgs), np.arange(n_msgs) % 4)
        check_cut(S, live, [n_msgs], [0], st1.deliveries, f"groups of {words} words")


def test_the_count_seam(width_tree, monkeypatch):
    """PSAMD_LOAD_COUNT=rows: a full row's k is counted from its words; the
    decision is made from k, so the answer is the same."""
    seam(monkeypatch)
    parent, root, live = width_tree
    with Sharded(3, [parent], [root]) as S:
        _, st1 = S.run(live, np.zeros(100))
        check_cut(S, live, [100], [0], st1.deliveries, "seam")


# ---- 2. cut points among more than a wave of siblings, a remote root -------------------

@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("hub_alive", [True, False])
@pytest.mark.parametrize("deg", [65, 129])
def test_wide_fan(deg, hub_alive, world):
    """Hub alive: 3 or 4 cut points under the one remote parent among 65 or
    more siblings.  Hub dead: the hub alone, the root's child -- the root's
    fullness travels as c_t where the root is remote -- with everything behind
    it orphaned across the ranks."""
    parent, root, hub, facts, live = fan_live(deg, world, hub_alive)
    with Sharded(world, [parent], [root]) as S:
        _, st1 = S.run(live, np.zeros(50))
        got, total = check_cut(S, live, [50], [0], st1.deliveries, f"fan {deg}")
        if hub_alive:
            assert int(total[1].sum()) == (3 if deg == 65 else 4) and total[1][hub] == 0
        else:
            assert int(total[1].sum()) == 1 and total[1][hub] == 1
            assert total[2][hub] == (448 if deg == 65 else 463)
            assert got[int(S.owners[0][hub])][2][hub] == total[2][hub]


# ---- 3. ranks with empty regions, several topics, an idle one ---------------------------

@pytest.mark.parametrize("world", [5, 16])
def test_tiny_beside_large(world):
    trees, roots, facts = DR.tiny_beside_large(world=world)
    n = trees[0].shape[0]
    live = np.ones(n, dtype=np.uint8)
    live[np.random.default_rng(world).choice(n, size=20, replace=False)] = 0
    live[roots] = 1
    topics = np.array([0] * 70 + [2] * 10)  # topic 1 idle in the window
    with Sharded(world, trees, roots) as S:
        _, st1 = S.run(live, topics)
        counts = [70, 0, 10]
        check_cut(S, live, counts, [0, 1, 2], st1.deliveries, f"world {world}")
        for req in ([2, 1, 0], [2], [1]):
            check_cut(S, live, counts, req, tag=f"world {world}")
        # the large tree in a window of its own: cut points behind remote parents
        _, st1 = S.run(live, np.ones(5))
        got, total = check_cut(S, live, [0, 5, 0], [1, 0], st1.deliveries, f"world {world}, the large tree")
        assert total[1].sum() >= 1


# ---- 4. every level an exchange ---------------------------------------------------------------

@pytest.mark.parametrize("n", [40, 300])
def test_path(n):
    """path(n) at world 2 with one dead peer: one whose parent lies on the
    other rank, then n // 2, whose parent is local."""
    parent, root = DR.path(n)
    with Sharded(2, [parent], [root]) as S:
        for d in (path_dead(n), n // 2):
            live = np.ones(n, dtype=np.uint8)
            live[d] = 0
            _, st1 = S.run(live, np.zeros(3))
            got, total = check_cut(S, live, [3], [0], st1.deliveries, f"path {n}, dead {d}")
            assert total[1][d] == 1 and total[1].sum() == 1
            assert total[2][d] == n - 1 - d and total[3][d] == 3 * (n - d)


# ---- 5. the subtree partition ---------------------------------------------------------------

@pytest.mark.parametrize("world,split", [(2, 1), (2, 2), (4, 2), (4, 3)])
def test_subtree_split(world, split):
    """Downward words at the split level only; at level 1 they decide nothing."""
    trees, roots, live = DR.split_case()
    topics = np.random.default_rng(5).integers(0, 3, size=60)
    counts = [int((topics == t).sum()) for t in range(3)]
    with Sharded(world, trees, roots, partition=PE.PART_SUBTREE, split_depth=split) as S:
        _, st1 = S.run(live, topics)
        check_cut(S, live, counts, [0, 1, 2], st1.deliveries, f"split {split}")
        check_cut(S, live, counts, [2, 0], tag=f"split {split}")


# ---- 6. one wide level ----------------------------------------------------------------------

def test_star_of_3000():
    """Dead leaves at a work item's edge, every one a cut point under the root."""
    n = 3001
    parent = star(n)
    live = np.ones(n, dtype=np.uint8)
    dead = [1, 64, 65, 66, 255, 256, 257, 3000]
    live[dead] = 0
    with Sharded(4, [parent], [0]) as S:
        _, st1 = S.run(live, np.zeros(2))
        got, total = check_cut(S, live, [2], [0], st1.deliveries, "star")
        assert np.nonzero(total[1])[0].tolist() == dead and not total[2].any() and total[3].sum() == 2 * len(dead)


# ---- 7. the last window of the last run --------------------------------------------------------

def test_two_runs_and_stale_rows():
    """Two runs on the same engines, the live mask changed in between: rows of
    the earlier generation count 0."""
    world, n = 3, 600
    trees, roots, victim = DR.windows_case(n, world)
    live_a = np.ones(n, dtype=np.uint8)
    live_b = live_a.copy()
    live_b[victim] = 0
    with Sharded(world, trees, roots) as S:
        _, st1 = S.run(live_a, np.zeros(300))
        got, total = check_cut(S, live_a, [300, 0], [0, 1], st1.deliveries, "run A")
        assert not any(x.any() for x in total)  # identity 4: an all-live mask
        _, st1 = S.run(live_b, np.concatenate([np.zeros(40), np.ones(9)]))
        got, total = check_cut(S, live_b, [40, 9], [0, 1], st1.deliveries, "run B")
        assert total[1][victim] >= 1 and total[2][victim] > 0
        check_cut(S, live_b, [40, 9], [1], tag="run B")


def test_one_run_in_three_windows(width_tree):
    """msg_window 128, 300 messages with starts 0..3: the call answers for the
    last window (44 messages)."""
    parent, root, live = width_tree
    with Sharded(3, [parent], [root], msg_window=128) as S:
        stats, st1 = S.run(live, np.zeros(300), np.arange(300) % 4)
        assert st1.windows == 3 and all(st.windows == 3 for st in stats)
        check_cut(S, live, [44], [0], tag="the third window")


# ---- 8. one rank: the call equals ps_peer_cut ---------------------------------------------------

def one_rank_dead(parent, n_msgs, dead_sets, eng=None, **kw):
    """One engine over a tree rooted at 0, one run per dead set: dist_cut
    against peer_cut and the reference."""
    n = parent.size
    with (eng or PE.Engine(n, 1, **kw)) as eng:
        eng.set_tree(0, 0, parent)
        for name, dead in dead_sets.items():
            live = np.ones(n, dtype=np.uint8)
            live[list(dead)] = 0
            eng.set_live(live)
            eng.publish(np.zeros(n_msgs))
            eng.run()
            got = eng.dist_cut([0])
            same(got, eng.peer_cut([0]), f"{n} peers, dead {name}")
            same(got, CR.topic_cut(n, 0, live, n_msgs, parent)[:4], f"{n} peers, dead {name}, the reference")
            assert bool(got[1].any()) == bool(len(dead))


@pytest.mark.parametrize("n", [2047, 4100])
def test_one_rank_heaps(n):
    """A mask at a level's first and last node and across a work item's edge."""
    masks = level_ends(heap_tree(n))
    assert len(masks) >= 7
    one_rank_dead(heap_tree(n), 1, masks)


@pytest.mark.parametrize("a,b", [(64, 65), (65, 64)])
def test_one_rank_inner_fan_out(a, b):
    one_rank_dead(fan_tree(a, b), 2, {"none": [], "first_of_each": [3, 3 + a], "wide_parents": [1, 2],
                                      "every_child_of_2": list(range(3 + a, 3 + a + b))})


@pytest.mark.parametrize("kids", [256, 257])
def test_one_rank_root_fan_out(kids):
    one_rank_dead(star(kids + 1), 3, {"none": [], "ends": [1, kids], "edge": [255, 256, min(257, kids)]})


def test_one_rank_wide_rows():
    """130-word rows on a heap of 64."""
    one_rank_dead(heap_tree(64), 130 * 64 - 7, {"none": [], "inner": [2, 5], "leaf": [63]})


def test_one_rank_host_build():
    one_rank_dead(heap_tree(700), 5, {"none": [], "inner": [1, 40]}, eng=make_engine(700, False))


def test_one_rank_several_topics():
    """Four topics sharing peers, one of them idle, in several orders and subsets."""
    n, free, (r0, p0), (r1, p1), live = shared_topics()
    msgs = np.concatenate([np.full(10, 0), np.full(200, 1), np.full(3, 3)]).astype(np.uint32)
    with PE.Engine(n, 4) as eng:
        eng.set_tree(0, r0, p0)
        eng.set_tree(1, r1, p1)
        eng.set_tree(2, r0, p0)
        eng.topic_create(3, 7)
        eng.set_live(live)
        eng.publish(msgs)
        eng.run()
        assert eng.peer_cut([0, 1])[1].any()
        for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [2, 1], [3], [2], []):
            same(eng.dist_cut(order), eng.peer_cut(order), f"{order}")


def test_one_rank_gpu_built_node_space_after_churn():
    n = 3000
    rng = np.random.default_rng(17)
    eng = make_engine(n, True, seed=4)
    eng.topic_create(0, 0, 2, 5)
    eng.join(0, np.arange(1, n, 2))
    members = set(range(1, n, 2))
    built = 0
    with eng:
        for step in range(3):
            outs = [p for p in range(1, n) if p not in members]
            join = rng.choice(outs, size=20, replace=False)
            st = eng.join(0, join, check=False)
            members |= {int(p) for p, s in zip(join, st) if s == 0}
            leave = rng.choice(sorted(members), size=15, replace=False)
            try:
                eng.leave(0, leave)
            except PE.EngineError:
                pass
            members -= {int(p) for p in leave}
            live = np.ones(n, dtype=np.uint8)
            live[rng.choice(sorted(members), size=25, replace=False)] = 0
            eng.set_live(live)
            eng.publish(np.zeros(4))
            eng.run()
            got = eng.dist_cut([0])
            same(got, eng.peer_cut([0]), f"step {step}")
            assert got[1].any()
            built = assert_builds(eng, True, built)


# ---- 9. the rules ------------------------------------------------------------------------------------

def test_rules():
    rng = np.random.default_rng(82)
    n, root = 300, 1
    parent = random_tree(rng, n, root)
    rp, cl = random_mesh2(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with PE.Engine(n, 3) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_children(2, root, rp, cl)
        eng.set_live(live)
        rc, a = raw_dist_cut(eng, [0])  # before any run
        assert rc == E_NOTREADY and untouched(a)
        eng.publish(np.array([0] * 10 + [2] * 6, dtype=np.uint32))
        eng.run()
        rc, a = raw_dist_cut(eng, [0], (False, False, False, False))  # all four NULL
        assert rc == E_INVAL
        assert eng._L.ps_dist_cut(eng._h, None, 1, *(x.ctypes.data_as(U64P) for x in a)) == E_INVAL and untouched(a)
        rc, a = raw_dist_cut(eng, [0, 0])  # a topic named twice
        assert rc == E_INVAL and untouched(a)
        rc, a = raw_dist_cut(eng, [0, 3])  # a topic out of range: nothing written
        assert rc == E_RANGE and untouched(a)
        rc, a = raw_dist_cut(eng, [0, 2])  # a mesh has no subtrees
        assert rc == E_STATE and untouched(a)
        whole = eng.peer_cut([0])
        assert whole[1].any()
        # a NULL among the four is skipped
        for which in ((True, False, False, True), (False, True, False, False), (False, False, True, True)):
            rc, a = raw_dist_cut(eng, [0], which)
            assert rc == 0
            for x, w, want in zip(a, which, whole):
                assert np.array_equal(x, want) if w else (x == FILL).all()
        rc, a = raw_dist_cut(eng, [])  # n == 0: all zeros
        assert rc == 0 and not any(x.any() for x in a)
        # an idle topic adds nothing
        same(eng.dist_cut([1, 0]), whole, "an idle topic first")
        assert not any(x.any() for x in eng.dist_cut([1]))


def test_a_topic_set_anew_since_the_window():
    """A parent array set over a join topic starts the topic's record afresh:
    PS_E_STATE, nothing written, until the next run."""
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
        same(eng.dist_cut([0, 1]), eng.peer_cut([0, 1]), "both topics")
        only0 = eng.dist_cut([0])
        assert only0[1].sum() > 0
        eng.set_tree(1, 0, p1)
        rc, a = raw_dist_cut(eng, [0, 1])
        assert rc == E_STATE and untouched(a)
        same(eng.dist_cut([0]), only0, "the other topic alone")
        eng.publish(np.array([0] * 3 + [1] * 2, dtype=np.uint32))
        eng.run()
        same(eng.dist_cut([0, 1]), CR.window_cut(n, live, [(0, 3, p0), (0, 2, p1)])[:4], "after the next run")


def test_null_patterns_may_differ_between_ranks():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with Sharded(2, [parent], [root]) as S:
        _, st1 = S.run(live, np.zeros(50))
        got, total = check_cut(S, live, [50], [0], st1.deliveries)
        which = [(True, False, False, False), (False, False, True, True)]
        raw = dist_cuts(S.engines, [0], which)
        for r in range(2):
            rc, a = raw[r]
            assert rc == 0
            for x, w, want in zip(a, which[r], got[r]):
                assert np.array_equal(x, want) if w else (x == FILL).all()
        # n == 0 exchanges nothing: one rank may ask alone
        rc, a = raw_dist_cut(S.engines[1], [])
        assert rc == 0 and not any(x.any() for x in a)
        # a topic out of range, named twice: refused on every rank before anything is exchanged
        for e in S.engines:
            rc, a = raw_dist_cut(e, [0, 1])
            assert rc == E_RANGE and untouched(a)
            rc, a = raw_dist_cut(e, [0, 0])
            assert rc == E_INVAL and untouched(a)


def test_the_old_calls_still_refuse():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    live = np.ones(n, dtype=np.uint8)
    live[[7, 90]] = 0
    with Sharded(2, [parent], [root]) as S:
        S.run(live, np.zeros(50))
        for e in S.engines:
            rc, a = raw_cut(e, [0])  # ps_peer_cut on a multi-rank engine
            assert rc == E_STATE and untouched(a)
            for what in (PE.REPORT_CUT, PE.REPORT_ALL, PE.REPORT_CUT | PE.REPORT_LOAD):
                rc, a = raw_report(e, [0], what)  # ps_dist_report does not answer the cut section
                assert rc == E_INVAL and report_untouched(a)
        check_cut(S, live, [50], [0])


def test_a_run_in_flight_is_refused_on_ranks():
    rng = np.random.default_rng(5)
    n, root = 300, 2
    parent = random_tree(rng, n, root)
    live = np.ones(n, dtype=np.uint8)
    live[[9, 120]] = 0
    with Sharded(2, [parent], [root]) as S:
        S.run(live, np.zeros(10))
        seen, errs = [None] * 2, []

        def go(r):
            try:
                e = S.engines[r]
                e.publish(np.zeros(20, dtype=np.uint32))
                e.run_async()
                seen[r] = raw_dist_cut(e, [0])  # refused before anything is exchanged
                e.wait()
            except Exception as ex:  # noqa: BLE001
                errs.append((r, ex))

        th = [threading.Thread(target=go, args=(r,)) for r in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in th), "rank thread hung"
        assert not errs, errs
        for rc, a in seen:
            assert rc == E_STATE and untouched(a)
        S.one.publish(np.zeros(20, dtype=np.uint32))
        S.one.run()
        check_cut(S, live, [20], [0], tag="after the wait")
