"""GPU: ps_dist_report -- a rank's share of the load, hop and
downstream sections on loopback ranks, and the same call on one rank.

Every sharded case is checked twice (check_ranks): per rank, every array equals
the reference's per-node contributions masked to the nodes the rank owns
(tests/dist_report_ref.py) -- a rank that reports a node it does not own fails
even where the sum comes out right --, and the ranks' sum equals a one-rank
engine's ps_peer_report on the same trees, live mask, publishes and request,
bit for bit.  The collective call is made from one thread per rank.  What a
shape relies on (65 siblings behind one remote parent, a rank that owns
nothing of a topic, a lonely root, levels without a cross-rank edge) is
asserted by name in tests/test_dist_report_cpu.py.  No case here provokes a
mismatched collective, a transport failure or a fault."""
import ctypes as C
import threading

import numpy as np
import pytest

import dist_ref as DR
import dist_report_ref as XR
import psengine as PE
import report_ref as RR
from test_gpu_churn import assert_builds, make_engine
from test_gpu_dist import make_ranks, run_ranks
from test_gpu_downstream import fan_tree, star
from test_gpu_drain_batch import random_mesh2, random_tree
from test_gpu_load import heap_tree, shared_topics

pytestmark = pytest.mark.gpu

U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
FILL = 0xABABABABABABABAB
SIZE = C.sizeof(PE.Report)
DIST = PE.REPORT_DIST
PATHS = [False, True, "inplace"]
SUBSETS = list(range(1, 8))


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


def dist_reports(engines, req, what=DIST):
    """The collective call: one thread per rank, the same request on each."""
    out = [None] * len(engines)
    errs = []

    def go(r):
        try:
            out[r] = engines[r].dist_report(req, what)
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


def check_ranks(engines, one, live, trees, roots, counts, owners, req, what=DIST, tag=""):
    """counts[t]: topic t's messages in the last window.  Per rank against the
    reference share; the ranks' sum against the one-rank engine's peer_report."""
    n, world = trees[0].shape[0], len(engines)
    topics = [(roots[t], counts[t], trees[t]) for t in req]
    shares = XR.rank_reports(n, live, topics, [owners[t] for t in req], world, what)
    got = dist_reports(engines, req, what)
    for r in range(world):
        assert tuple(got[r]) == XR.names_of(what)
        same(got[r], shares[r], f"{tag} rank {r} of {world} what {what:#x} request {list(req)}")
    whole = one.peer_report(req, what)
    same(XR.total(got), whole, f"{tag} the ranks' sum, what {what:#x} request {list(req)}")
    return got, whole


class Sharded:
    """`world` loopback ranks and a one-rank engine over the same trees."""

    def __init__(self, world, trees, roots, copy=False, partition=PE.PART_PEER, split_depth=0, plan=None, **kw):
        self.trees, self.roots, self.world = trees, roots, world
        n = trees[0].shape[0]
        self.lb, self.engines = make_ranks(world, n, len(trees), partition, split_depth, copy=copy, plan=plan, **kw)
        self.one = PE.Engine(n, len(trees), plan=plan, **kw)
        self.owners = XR.owners_of(trees, roots, world, partition == PE.PART_SUBTREE, split_depth)
        for e in self.engines + [self.one]:
            for t, (par, root) in enumerate(zip(trees, roots)):
                e.set_tree(t, root, par)

    def run(self, live, topics, starts=None):
        topics = np.asarray(topics, dtype=np.uint32)
        for e in self.engines + [self.one]:
            e.set_live(live)
            e.publish(topics, starts)
        stats = run_ranks(self.engines)
        return stats, self.one.run()

    def check(self, live, counts, req, what=DIST, tag=""):
        return check_ranks(self.engines, self.one, live, self.trees, self.roots, counts, self.owners, req, what, tag)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for e in self.engines + [self.one]:
            e.close()
        self.lb.close()


def filled(eng, n_topics, skip=()):
    arrays = {k: np.full((n_topics, PE.MAX_ROUNDS) if k in ("nodes", "reached", "deliv") else eng.n_peers, FILL, dtype=np.uint64)
              for k in RR.NAMES}
    rep = PE.Report()
    for k, a in arrays.items():
        if k not in skip:
            setattr(rep, k, a.ctypes.data_as(U64P))
    return arrays, rep


def raw(eng, topics, what, skip=(), size=SIZE, call="ps_dist_report"):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    arrays, rep = filled(eng, t.size, skip)
    rc = getattr(eng._L, call)(eng._h, t.ctypes.data_as(U32P) if t.size else None, t.size, what, C.byref(rep), size)
    return rc, arrays


def untouched(arrays):
    return all((a == FILL).all() for a in arrays.values())


# ---- 1. row widths on ranks whose node 0 is not the root ---------------------------

@pytest.fixture(scope="module")
def width_tree():
    return DR.row_width_case()


ROWS = [c for c in DR.ROW_CASES if c[2] in (1, 2, 64, 65)] + [(130 * 64 - 7, None, 130)]


@pytest.mark.parametrize("n_msgs,plan,words", ROWS)
def test_row_widths(width_tree, n_msgs, plan, words):
    """600 peers, fan-out <= 4, 8 % dead, world 3 under the peer hash, rows of
    1, 2, 64, 65 and 130 words: classify's narrow and wide branches on ranks
    whose node 0 is no root."""
    parent, root, live = width_tree
    with Sharded(3, [parent], [root], plan=plan) as S:
        stats, st1 = S.run(live, np.zeros(n_msgs))
        assert sum(st.deliveries for st in stats) == st1.deliveries
        got, whole = S.check(live, [n_msgs], [0], tag=f"{words} words")
        # carried at the root's peer on the root's owner: every delivery of the one topic
        own_root = int(S.owners[0][root])
        assert got[own_root]["carried"][root] == st1.deliveries == int(whole["recv"].sum())
        assert int(whole["below"].sum()) == int((whole["nodes"][0] * np.arange(PE.MAX_ROUNDS, dtype=np.uint64)).sum())


@pytest.mark.parametrize("copy", PATHS)
def test_the_report_does_not_depend_on_the_data_path(width_tree, copy):
    parent, root, live = width_tree
    with Sharded(3, [parent], [root], copy=copy) as S:
        S.run(live, np.zeros(100))
        S.check(live, [100], [0], tag=f"path {copy}")


@pytest.mark.parametrize("n_msgs,words", DR.GROUP_CASES)
def test_start_groups(width_tree, n_msgs, words):
    """Starts 0..3 in turn: k counted through node-major start-group blocks."""
    parent, root, live = width_tree
    with Sharded(3, [parent], [root]) as S:
        S.run(live, np.zeros(n_msgs), np.arange(n_msgs) % 4)
        S.check(live, [n_msgs], [0], tag=f"groups of {words} words")


# ---- 2. more than a wave of siblings in one slot --------------------------------------

@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("hub_alive", [True, False])
@pytest.mark.parametrize("deg", [65, 129])
def test_wide_fan(deg, hub_alive, world):
    """65 or more children of one remote parent on one rank push into one slot;
    a dead parent's subtree adds to below and nothing to carried."""
    parent, root, hub, facts = DR.wide_fan(deg, world)
    live = np.ones(parent.shape[0], dtype=np.uint8)
    kids = facts["kids"]
    live[[kids[0], kids[63], kids[64], kids[-1]]] = 0
    live[hub] = hub_alive
    with Sharded(world, [parent], [root]) as S:
        S.run(live, np.zeros(50))
        got, whole = S.check(live, [50], [0], tag=f"fan {deg}")
        assert whole["below"][hub] >= deg
        if not hub_alive:
            assert whole["carried"][hub] == 0


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
        S.run(live, topics)
        counts = [70, 0, 10]
        for req in ([0, 1, 2], [2, 1, 0], [2], [1]):
            got, whole = S.check(live, counts, req, tag=f"world {world}")
        S.check(live, counts, [0, 2], PE.REPORT_DOWNSTREAM)
        # the lonely root's owner reports the root's share of sent and the whole topic below it
        r2 = facts["lonely_root"]
        lone = S.engines[int(S.owners[2][r2])].dist_report([2], PE.REPORT_LOAD)
        assert lone["sent"][r2] == 10 * 12 and lone["sent"].sum() == 120 and not lone["recv"].any()


# ---- 4. every level an exchange or a skipped one ------------------------------------------

@pytest.mark.parametrize("n", [40, 300])
def test_path(n):
    """path(n) at world 2 with one dead peer in the middle; the path of 300
    fills the clamped hop column 255 while below / carried stay exact."""
    parent, root = DR.path(n)
    live = np.ones(n, dtype=np.uint8)
    live[n // 2] = 0
    with Sharded(2, [parent], [root]) as S:
        S.run(live, np.zeros(3))
        got, whole = S.check(live, [3], [0], tag=f"path {n}")
        assert np.array_equal(whole["below"], np.arange(n - 1, -1, -1).astype(np.uint64))
        assert whole["carried"][0] == 3 * (n // 2 - 1)
        if n > 256:
            assert whole["nodes"][0, 255] == n - 255


# ---- 5. the subtree partition ---------------------------------------------------------------

@pytest.mark.parametrize("world,split", [(2, 1), (2, 2), (4, 2), (4, 3)])
def test_subtree_split(world, split):
    """Exchanges at the split level only; a peer's nodes of two topics lie on
    different ranks."""
    trees, roots, live = DR.split_case()
    topics = np.random.default_rng(5).integers(0, 3, size=60)
    counts = [int((topics == t).sum()) for t in range(3)]
    with Sharded(world, trees, roots, partition=PE.PART_SUBTREE, split_depth=split) as S:
        S.run(live, topics)
        S.check(live, counts, [0, 1, 2], tag=f"split {split}")
        S.check(live, counts, [2, 0], tag=f"split {split}")


# ---- 6. one wide level, and the root's owner closes the root ----------------------------------

def test_star_of_3000():
    n = 3001
    parent = star(n)
    live = np.ones(n, dtype=np.uint8)
    live[[1, 64, 65, 66, 3000]] = 0
    with Sharded(4, [parent], [0]) as S:
        S.run(live, np.zeros(2))
        got, whole = S.check(live, [2], [0], tag="star")
        assert whole["below"][0] == 3000 and whole["carried"][0] == 2 * 2995 and whole["below"][1:].sum() == 0


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
        S.run(live_a, np.zeros(300))
        S.check(live_a, [300, 0], [0, 1], tag="run A")
        S.run(live_b, np.concatenate([np.zeros(40), np.ones(9)]))
        got, whole = S.check(live_b, [40, 9], [0, 1], tag="run B")
        assert whole["below"][victim] > 0 and whole["carried"][victim] == 0
        S.check(live_b, [40, 9], [1], tag="run B")


def test_one_run_in_three_windows(width_tree):
    """msg_window 128, 300 messages with starts 0..3: the call answers for the
    last window (44 messages)."""
    parent, root, live = width_tree
    with Sharded(3, [parent], [root], msg_window=128) as S:
        stats, st1 = S.run(live, np.zeros(300), np.arange(300) % 4)
        assert st1.windows == 3 and all(st.windows == 3 for st in stats)
        S.check(live, [44], [0], tag="the third window")


# ---- 8. sections that exchange nothing, from one rank alone ---------------------------------------

def test_load_and_hops_from_a_single_rank(width_tree):
    parent, root, live = width_tree
    with Sharded(3, [parent], [root]) as S:
        S.run(live, np.zeros(70))
        shares = XR.rank_reports(600, live, [(root, 70, parent)], S.owners, 3)
        for r in (2, 0):
            for what in (PE.REPORT_LOAD, PE.REPORT_HOPS, PE.REPORT_LOAD | PE.REPORT_HOPS):
                got = S.engines[r].dist_report([0], what)  # the other ranks do not call
                same(got, {k: shares[r][k] for k in XR.names_of(what)}, f"rank {r} alone, what {what:#x}")


# ---- 9. one rank: the call equals ps_peer_report ----------------------------------------------------

def one_rank_dead(parent, n_msgs, dead_sets, eng=None, **kw):
    """One engine over a tree rooted at 0, one run per dead set: dist_report
    against peer_report for every non-empty subset of 0x7."""
    n = parent.size
    with (eng or PE.Engine(n, 1, **kw)) as eng:
        eng.set_tree(0, 0, parent)
        for name, dead in dead_sets.items():
            live = np.ones(n, dtype=np.uint8)
            live[list(dead)] = 0
            eng.set_live(live)
            eng.publish(np.zeros(n_msgs))
            eng.run()
            for what in SUBSETS:
                same(eng.dist_report([0], what), eng.peer_report([0], what), f"{n} peers, dead {name}, what {what:#x}")


def level_ends(parent):
    """Dead sets at the first and the last node of every level wider than a wave."""
    lv = DR.bfs_levels(np.where(np.arange(parent.size) == 0, DR.NONE, parent), 0)
    out = {"none": []}
    for l in range(1, int(lv.max()) + 1):
        at = np.nonzero(lv == l)[0]
        if at.size > 64:
            out[f"l{l}_first"], out[f"l{l}_last"] = [int(at[0])], [int(at[-1])]
            out[f"l{l}_item_edge"] = [int(at[min(255, at.size - 1)]), int(at[min(256, at.size - 1)])]
    return out


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
        for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [2, 1], [3], [2], []):
            for what in SUBSETS:
                same(eng.dist_report(order, what), eng.peer_report(order, what), f"{order} what {what:#x}")


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
            eng.publish(np.zeros(4))
            eng.run()
            for what in SUBSETS:
                same(eng.dist_report([0], what), eng.peer_report([0], what), f"step {step} what {what:#x}")
            built = assert_builds(eng, True, built)


# ---- 10. the rules ------------------------------------------------------------------------------------

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
        for what in (DIST, PE.REPORT_LOAD):  # before any run
            rc, a = raw(eng, [0], what)
            assert rc == E_NOTREADY and untouched(a)
        eng.publish(np.array([0] * 10 + [2] * 6, dtype=np.uint32))
        eng.run()
        for what in (PE.REPORT_CUT, PE.REPORT_ALL, PE.REPORT_CUT | PE.REPORT_LOAD, 0x10):  # the cut section is not answered
            rc, a = raw(eng, [0], what)
            assert rc == E_INVAL and untouched(a), what
        assert raw(eng, [0], 0)[0] == E_INVAL
        rc, a = raw(eng, [0, 0], DIST)  # a topic named twice
        assert rc == E_INVAL and untouched(a)
        for what in (DIST, PE.REPORT_LOAD):  # a topic out of range: nothing written
            rc, a = raw(eng, [0, 3], what)
            assert rc == E_RANGE and untouched(a)
        rc, a = raw(eng, [0], DIST, size=SIZE - 8)  # a wrong out_size
        assert rc == E_INVAL and untouched(a)
        rc, a = raw(eng, [0], DIST, skip=("below", "carried"))  # a selected section without a pointer
        assert rc == E_INVAL and untouched(a)
        # pointers of sections that are not selected are not touched; a NULL inside a selected one is skipped
        rc, a = raw(eng, [0], PE.REPORT_LOAD | PE.REPORT_DOWNSTREAM, skip=("carried",))
        assert rc == 0 and untouched({k: a[k] for k in RR.NAMES if k not in ("recv", "sent", "below")})
        whole = eng.peer_report([0], 0x5)
        same({k: a[k] for k in ("recv", "sent", "below")}, {k: whole[k] for k in ("recv", "sent", "below")},
             "a NULL pointer inside a section")
        # n == 0: the peer-space arrays read zero, the hop arrays are not written
        rc, a = raw(eng, [], DIST)
        assert rc == 0 and not any(a[k].any() for k in ("recv", "sent", "below", "carried"))
        assert untouched({k: a[k] for k in ("missed", "cuts", "orphaned", "lost")})
        # an idle topic
        same(eng.dist_report([1, 0]), eng.peer_report([1, 0], DIST), "an idle topic first")
        assert not any(v.any() for v in eng.dist_report([1]).values())
        # a mesh answers the load section alone
        same(eng.dist_report([2, 0], PE.REPORT_LOAD), eng.peer_report([2, 0], PE.REPORT_LOAD), "a mesh's load")
        for what in SUBSETS[1:]:
            rc, a = raw(eng, [0, 2], what)
            assert rc == E_STATE and untouched(a), what


def test_the_old_calls_still_refuse_ranks():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    live = np.ones(n, dtype=np.uint8)
    with Sharded(2, [parent], [root]) as S:
        S.run(live, np.zeros(50))
        for e in S.engines:
            for what in (PE.REPORT_ALL, PE.REPORT_LOAD):
                rc, a = raw(e, [0], what, call="ps_peer_report")
                assert rc == E_STATE and untouched(a)
            rc, a = raw(e, [0], PE.REPORT_CUT)
            assert rc == E_INVAL and untouched(a)
        S.check(live, [50], [0])
