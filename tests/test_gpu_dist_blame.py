"""GPU: ps_dist_blame -- a rank's share of ps_topic_blame on
loopback ranks, and the same call on one rank.

Every sharded case is checked three times (check_blame).  Ownership: per rank
and request position, the records are the reference's table masked to the
nodes the rank owns (tests/dist_blame_ref.py), as a set keyed by peer with hop
never decreasing -- a rank that reports a node it does not own fails even
where the union comes out right.  Union: keyed by (request position, peer) the
ranks' records are, field for field, a one-rank engine's ps_topic_blame on the
same trees, live mask, publishes and request.  And against ps_dist_cut on the
same window: per rank bincount(rec_peer, rec_missed) is its missed and
#(rec_peer == rec_cut_peer) its cuts; over the ranks' sum bincount(rec_cut_peer,
rec_missed) is the summed lost.  The collective call is made from one thread
per rank.  What a shape relies on (cut points on other ranks, paths that
change rank twice or more) is asserted by name in
tests/test_dist_blame_cpu.py.  No case here provokes a mismatched collective,
a transport failure or a fault."""
import ctypes as C
import threading

import numpy as np
import pytest

import blame_ref as BR
import dist_blame_ref as XB
import dist_ref as DR
import psengine as PE
from test_blame_cpu import SENTINEL, lent, lent_untouched
from test_dist_blame_cpu import two_dead
from test_dist_cut_cpu import fan_live, path_dead
from test_gpu_blame import raw_topic_blame
from test_gpu_churn import assert_builds, make_engine
from test_gpu_dist_cut import dist_cuts
from test_gpu_dist_report import PATHS, ROWS, Sharded, level_ends
from test_gpu_downstream import fan_tree, star
from test_gpu_drain_batch import random_mesh2, random_tree
from test_gpu_load import heap_tree, seam, shared_topics

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
KEYS = XB.KEYS


# ---- helpers ------------------------------------------------------------------------

def raw_dist_blame(eng, topics, which=(True,) * 5, want_off=True, want_total=True):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    off, ptrs, total = lent()
    rc = eng._L.ps_dist_blame(eng._h, t.ctypes.data_as(U32P) if t.size else None, t.size, C.byref(off) if want_off else None,
                              *(C.byref(p) if w else None for p, w in zip(ptrs, which)),
                              C.byref(total) if want_total else None)
    return rc, off, ptrs, total


def read(ptr, count, dtype):
    """A copy of `count` words behind a lent pointer."""
    if count == 0:
        return np.empty(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True)


def dist_blames(engines, req, which=None):
    """The collective call: one thread per rank, the same request on each;
    which[r]: the record pointers rank r passes (None: all five, through the
    binding)."""
    out = [None] * len(engines)
    errs = []

    def go(r):
        try:
            if which is None:
                out[r] = engines[r].dist_blame(req)
            else:
                out[r] = raw_dist_blame(engines[r], req, which[r])
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


def well_formed(r, n_topics, what=""):
    assert set(r) == {"rec_off", *KEYS} and r["rec_off"].dtype == np.uint64 and r["rec_off"].size == n_topics + 1, what
    off = r["rec_off"].astype(np.int64)
    assert off[0] == 0 and np.all(np.diff(off) >= 0), what
    assert all(r[k].size == off[-1] and r[k].dtype == np.uint32 for k in KEYS), what
    return off


def slices(r, off, i):
    return tuple(r[k][off[i]:off[i + 1]] for k in KEYS)


def check_blame(S, live, counts, req, tag=""):
    """counts[t]: topic t's messages in the last window.  Ownership, union and
    the identities against ps_dist_cut (the module's docstring)."""
    n, world = S.trees[0].shape[0], S.world
    req = [int(t) for t in req]
    tables = {t: BR.topic_blame(n, S.roots[t], live, counts[t], S.trees[t]) for t in req}
    got = dist_blames(S.engines, req)
    whole = S.one.topic_blame(req)
    woff = well_formed(whole, len(req))
    offs = [well_formed(g, len(req), f"{tag} rank {r}") for r, g in enumerate(got)]
    for i, t in enumerate(req):
        shares = [slices(got[r], offs[r], i) for r in range(world)]
        for r in range(world):  # ownership
            XB.compare(shares[r], tables[t], S.owners[t], r, f"{tag} rank {r} of {world} topic {t}")
        want = XB.keyed(slices(whole, woff, i))  # union
        for k, g, w in zip(KEYS, XB.union(shares), want):
            assert np.array_equal(g, w), f"{tag} the ranks' union, topic {t}: {k}"
    # against ps_dist_cut on the same window
    cuts = dist_cuts(S.engines, req)
    lost = np.zeros(n, dtype=np.uint64)
    u64 = lambda x: x.astype(np.uint64)
    for r, g in enumerate(got):
        w = g["missed"].astype(np.int64)
        own = g["peer"] == g["cut_peer"]
        assert np.array_equal(u64(np.bincount(g["peer"], weights=w, minlength=n)), cuts[r][0]), f"{tag} rank {r}: missed"
        assert np.array_equal(u64(np.bincount(g["peer"][own], minlength=n)), cuts[r][1]), f"{tag} rank {r}: cuts"
        lost += u64(np.bincount(g["cut_peer"], weights=w, minlength=n))
    assert np.array_equal(lost, sum(c[3] for c in cuts)), f"{tag}: lost"
    return got, whole


# ---- 1. row widths on ranks whose node 0 is not the root ---------------------------

@pytest.fixture(scope="module")
def width_tree():
    return DR.row_width_case()


@pytest.mark.parametrize("n_msgs,plan,words", ROWS)
def test_row_widths(width_tree, n_msgs, plan, words):
    """600 peers, world 3 under the peer hash, rows of 1, 2, 64, 65 and 130
    words: 282 records, 93 / 94 / 95 per rank, 26 cut points up to 21 hops up."""
    parent, root, live = width_tree
    with Sharded(3, [parent], [root], plan=plan) as S:
        S.run(live, np.zeros(n_msgs))
        got, whole = check_blame(S, live, [n_msgs], [0], f"{words} words")
        assert [g["peer"].size for g in got] == [93, 94, 95]
        assert int((whole["peer"] == whole["cut_peer"]).sum()) == 26
        assert int((whole["hop"] - whole["cut_hop"]).max()) == 21
        assert (whole["missed"] == n_msgs).all()  # a dead peer forwards nothing


@pytest.mark.parametrize("copy", PATHS)
def test_the_blame_does_not_depend_on_the_data_path(width_tree, copy):
    parent, root, live = width_tree
    with Sharded(3, [parent], [root], copy=copy) as S:
        S.run(live, np.zeros(100))
        check_blame(S, live, [100], [0], f"path {copy}")


@pytest.mark.parametrize("n_msgs,words", DR.GROUP_CASES)
def test_start_groups(width_tree, n_msgs, words):
    """Starts 0..3 in turn: k counted through node-major start-group blocks."""
    parent, root, live = width_tree
    with Sharded(3, [parent], [root]) as S:
        S.run(live, np.zeros(n_msgs), np.arange(n_msgs) % 4)
        check_blame(S, live, [n_msgs], [0], f"groups of {words} words")


def test_the_count_seam(width_tree, monkeypatch):
    """PSAMD_LOAD_COUNT=rows: a full row's k is counted from its words; the
    decision is made from k, so the answer is the same."""
    seam(monkeypatch)
    parent, root, live = width_tree
    with Sharded(3, [parent], [root]) as S:
        S.run(live, np.zeros(100))
        check_blame(S, live, [100], [0], "seam")


# ---- 2. more than a wave of siblings under one remote parent, a remote root ---------

@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("hub_alive", [True, False])
@pytest.mark.parametrize("deg", [65, 129])
def test_wide_fan(deg, hub_alive, world):
    """Hub dead: every record behind the hub, on every rank, names the hub and
    level 1 -- one pair inherited by 65 or more siblings of one remote parent
    -- and the hub hangs under a root that is remote (but at (65, 2))."""
    parent, root, hub, facts, live = fan_live(deg, world, hub_alive)
    with Sharded(world, [parent], [root]) as S:
        S.run(live, np.zeros(50))
        got, whole = check_blame(S, live, [50], [0], f"fan {deg}")
        if hub_alive:
            assert int((whole["peer"] == whole["cut_peer"]).sum()) == (3 if deg == 65 else 4)
        else:
            assert whole["peer"].size == (449 if deg == 65 else 464)
            for g in got:
                assert g["peer"].size and (g["cut_peer"] == hub).all() and (g["cut_hop"] == 1).all()


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
            got, whole = check_blame(S, live, counts, req, f"world {world}")
        assert whole["peer"].size == 0  # the idle topic alone: no record anywhere
        # the large tree in a window of its own: cut points on other ranks
        S.run(live, np.ones(5))
        got, whole = check_blame(S, live, [0, 5, 0], [1, 0], f"world {world}, the large tree")
        assert whole["peer"].size > int((whole["peer"] == whole["cut_peer"]).sum()) >= 1


# ---- 4. every level an exchange ---------------------------------------------------------------

@pytest.mark.parametrize("n", [40, 300])
def test_path(n):
    """path(n) at world 2: the dead peer at the first, a middle and the last
    node, one whose parent lies on the other rank, and two dead peers on the
    one path -- the nearer cut point wins.  Hops past 255 stay exact."""
    parent, root = DR.path(n)
    with Sharded(2, [parent], [root]) as S:
        for dead in ([1], [n // 2], [n - 1], [path_dead(n)], two_dead(n)):
            live = np.ones(n, dtype=np.uint8)
            live[dead] = 0
            S.run(live, np.zeros(3))
            got, whole = check_blame(S, live, [3], [0], f"path {n}, dead {dead}")
            d = dead[0]
            assert np.array_equal(np.sort(whole["peer"]), np.arange(d, n))
            assert (whole["cut_peer"] == d).all() and (whole["cut_hop"] == d).all()
            assert np.array_equal(whole["hop"], whole["peer"])  # a path: the peer id is the level, unclamped


def test_path_40_at_world_3():
    """The shapes whose per-rank counts tests/test_dist_blame_cpu.py states."""
    parent, root = DR.path(40)
    with Sharded(3, [parent], [root]) as S:
        for d, per_rank in ((1, [13, 13, 13]), (20, [7, 6, 7])):
            live = np.ones(40, dtype=np.uint8)
            live[d] = 0
            S.run(live, np.zeros(3))
            got, whole = check_blame(S, live, [3], [0], f"dead {d}")
            assert [g["peer"].size for g in got] == per_rank


# ---- 5. the subtree partition ---------------------------------------------------------------

@pytest.mark.parametrize("world,split", [(2, 1), (2, 2), (4, 2), (4, 3), (4, 40)])
def test_subtree_split(world, split):
    """Pairs travel at the split level only; split level 40 lies past every
    depth: one rank owns everything and nothing is exchanged."""
    trees, roots, live = DR.split_case()
    topics = np.random.default_rng(5).integers(0, 3, size=60)
    counts = [int((topics == t).sum()) for t in range(3)]
    with Sharded(world, trees, roots, partition=PE.PART_SUBTREE, split_depth=split) as S:
        S.run(live, topics)
        check_blame(S, live, counts, [0, 1, 2], f"split {split}")
        check_blame(S, live, counts, [2, 0], f"split {split}")


def test_split_case_under_the_peer_hash():
    """Topic 0 at world 4: 865 records, 205 / 231 / 216 / 213 per rank."""
    trees, roots, live = DR.split_case()
    with Sharded(4, trees, roots) as S:
        S.run(live, np.zeros(7))
        got, whole = check_blame(S, live, [7, 0, 0], [0], "split_case, peer hash")
        assert [g["peer"].size for g in got] == [205, 231, 216, 213]
        assert int((whole["peer"] == whole["cut_peer"]).sum()) == 84


# ---- 6. one wide level ----------------------------------------------------------------------

def test_star_of_3000():
    """Dead leaves at a work item's edge, every one its own cut point under a
    root that three of the four ranks do not own."""
    n = 3001
    parent = star(n)
    live = np.ones(n, dtype=np.uint8)
    dead = [1, 64, 65, 66, 255, 256, 257, 3000]
    live[dead] = 0
    with Sharded(4, [parent], [0]) as S:
        S.run(live, np.zeros(2))
        got, whole = check_blame(S, live, [2], [0], "star")
        assert sorted(whole["peer"].tolist()) == dead and np.array_equal(whole["peer"], whole["cut_peer"])
        assert (whole["hop"] == 1).all() and (whole["cut_hop"] == 1).all() and (whole["missed"] == 2).all()


# ---- 7. the last window of the last run --------------------------------------------------------

def test_two_runs_and_stale_rows():
    """Two runs on the same engines, the live mask changed in between: rows of
    the earlier generation count 0.  Run A is all-live: total 0 on every rank."""
    world, n = 3, 600
    trees, roots, victim = DR.windows_case(n, world)
    live_a = np.ones(n, dtype=np.uint8)
    live_b = live_a.copy()
    live_b[victim] = 0
    with Sharded(world, trees, roots) as S:
        S.run(live_a, np.zeros(300))
        got, whole = check_blame(S, live_a, [300, 0], [0, 1], "run A")
        assert whole["peer"].size == 0 and all(g["peer"].size == 0 and not g["rec_off"].any() for g in got)
        S.run(live_b, np.concatenate([np.zeros(40), np.ones(9)]))
        got, whole = check_blame(S, live_b, [40, 9], [0, 1], "run B")
        assert (whole["cut_peer"] == victim).any()
        check_blame(S, live_b, [40, 9], [1], "run B")


def test_one_run_in_three_windows(width_tree):
    """msg_window 128, 300 messages with starts 0..3: the call answers for the
    last window (44 messages)."""
    parent, root, live = width_tree
    with Sharded(3, [parent], [root], msg_window=128) as S:
        stats, st1 = S.run(live, np.zeros(300), np.arange(300) % 4)
        assert st1.windows == 3 and all(st.windows == 3 for st in stats)
        got, whole = check_blame(S, live, [44], [0], "the third window")
        assert whole["missed"].size and (whole["missed"] == 44).all()


# ---- 8. one rank: the call equals ps_topic_blame -------------------------------------------------

def same_answer(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{what}: {k}"


def one_rank_dead(parent, n_msgs, dead_sets, eng=None, **kw):
    """One engine over a tree rooted at 0, one run per dead set: dist_blame
    against topic_blame entry for entry, order included, and the reference."""
    n = parent.size
    with (eng or PE.Engine(n, 1, **kw)) as eng:
        eng.set_tree(0, 0, parent)
        order = eng.graph(PE.G_NODE_PEER)[:n].astype(np.int64)
        for name, dead in dead_sets.items():
            live = np.ones(n, dtype=np.uint8)
            live[list(dead)] = 0
            eng.set_live(live)
            eng.publish(np.zeros(n_msgs))
            eng.run()
            got = eng.dist_blame([0])
            same_answer(got, eng.topic_blame([0]), f"{n} peers, dead {name}")
            want = BR.records(BR.topic_blame(n, 0, live, n_msgs, parent), order)
            for k, w in zip(KEYS, want):
                assert np.array_equal(got[k], w), f"{n} peers, dead {name}, the reference: {k}"
            assert bool(got["peer"].size) == bool(len(dead))


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
        assert eng.topic_blame([0, 1])["peer"].size
        for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [2, 1], [3], [2], []):
            same_answer(eng.dist_blame(order), eng.topic_blame(order), f"{order}")


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
            got = eng.dist_blame([0])
            same_answer(got, eng.topic_blame([0]), f"step {step}")
            assert got["peer"].size
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
        assert raw_dist_blame(eng, [0])[0] == E_NOTREADY  # before any run
        assert lent_untouched(*raw_dist_blame(eng, [0])[1:])
        eng.publish(np.array([0] * 10 + [2] * 6, dtype=np.uint32))
        eng.run()
        for rc, *o in (raw_dist_blame(eng, [0], want_off=False), raw_dist_blame(eng, [0], want_total=False)):
            assert rc == E_INVAL and lent_untouched(*o)
        off, ptrs, total = lent()
        assert eng._L.ps_dist_blame(eng._h, None, 1, C.byref(off), *(C.byref(p) for p in ptrs), C.byref(total)) == E_INVAL
        assert lent_untouched(off, ptrs, total)
        rc, *o = raw_dist_blame(eng, [0, 0])  # a topic named twice
        assert rc == E_INVAL and lent_untouched(*o)
        rc, *o = raw_dist_blame(eng, [0, 3])  # a topic out of range: nothing written
        assert rc == E_RANGE and lent_untouched(*o)
        rc, *o = raw_dist_blame(eng, [0, 2])  # a mesh has no cut points
        assert rc == E_STATE and lent_untouched(*o)
        whole = eng.topic_blame([0])
        assert whole["peer"].size
        same_answer(eng.dist_blame([0]), whole, "one topic")
        # a NULL record pointer: neither written nor lent
        for which in ((True, False, False, False, True), (False, True, False, False, False), (False,) * 5):
            rc, off, ptrs, total = raw_dist_blame(eng, [0], which)
            assert rc == 0 and total.value == whole["peer"].size
            assert np.array_equal(read(off, 2, np.uint64), whole["rec_off"])
            for k, p, w in zip(KEYS, ptrs, which):
                if w:
                    assert np.array_equal(read(p, total.value, np.uint32), whole[k]), k
                else:
                    assert C.cast(p, C.c_void_p).value == SENTINEL, k
        rc, off, ptrs, total = raw_dist_blame(eng, [])  # n == 0: rec_off = {0}, total 0
        assert rc == 0 and total.value == 0 and read(off, 1, np.uint64)[0] == 0
        # an idle topic has no records
        r = eng.dist_blame([1, 0])
        assert r["rec_off"].tolist() == [0, 0, whole["peer"].size] and np.array_equal(r["cut_peer"], whole["cut_peer"])
        assert eng.dist_blame([1])["peer"].size == 0


def test_the_view_stays_until_the_next_call():
    """The lent arrays are read back after other calls -- ps_topic_blame's view
    is separate -- and after another run."""
    rng = np.random.default_rng(7)
    n = 500
    parent = random_tree(rng, n, 0)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[0] = 1
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        eng.set_live(live)
        eng.publish(np.zeros(9))
        eng.run()
        rc, off, ptrs, total = raw_dist_blame(eng, [0])
        assert rc == 0 and total.value
        first = [read(p, total.value, np.uint32) for p in ptrs]
        first_off = read(off, 2, np.uint64)
        whole = eng.topic_blame([0])
        eng.dist_cut([0])
        eng.peer_cut([0])
        eng.blame(np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32))
        eng.set_live(np.ones(n, dtype=np.uint8))
        eng.publish(np.zeros(4))
        eng.run()
        assert eng.topic_blame([0])["peer"].size == 0
        for k, p, w in zip(KEYS, ptrs, first):
            assert np.array_equal(read(p, total.value, np.uint32), w) and np.array_equal(w, whole[k]), k
        assert np.array_equal(read(off, 2, np.uint64), first_off)
        assert eng.dist_blame([0])["peer"].size == 0  # the next call: the all-live window


def test_a_topic_set_anew_since_the_window():
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
        same_answer(eng.dist_blame([0, 1]), eng.topic_blame([0, 1]), "both topics")
        only0 = eng.dist_blame([0])
        assert only0["peer"].size
        eng.set_tree(1, 0, p1)
        rc, *o = raw_dist_blame(eng, [0, 1])
        assert rc == E_STATE and lent_untouched(*o)
        same_answer(eng.dist_blame([0]), only0, "the other topic alone")
        eng.publish(np.array([0] * 3 + [1] * 2, dtype=np.uint32))
        eng.run()
        same_answer(eng.dist_blame([0, 1]), eng.topic_blame([0, 1]), "after the next run")


def test_null_patterns_may_differ_between_ranks():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with Sharded(2, [parent], [root]) as S:
        S.run(live, np.zeros(50))
        got, whole = check_blame(S, live, [50], [0])
        which = [(True, False, False, False, True), (False, True, True, False, False)]
        raw = dist_blames(S.engines, [0], which)
        for r in range(2):
            rc, off, ptrs, total = raw[r]
            assert rc == 0 and total.value == got[r]["peer"].size
            assert np.array_equal(read(off, 2, np.uint64), got[r]["rec_off"])
            for k, p, w in zip(KEYS, ptrs, which[r]):
                if w:
                    assert np.array_equal(read(p, total.value, np.uint32), got[r][k]), (r, k)
                else:
                    assert C.cast(p, C.c_void_p).value == SENTINEL, (r, k)
        # n == 0 exchanges nothing: one rank may ask alone
        rc, off, ptrs, total = raw_dist_blame(S.engines[1], [])
        assert rc == 0 and total.value == 0 and read(off, 1, np.uint64)[0] == 0
        # a topic out of range, named twice: refused on every rank before anything is exchanged
        for e in S.engines:
            rc, *o = raw_dist_blame(e, [0, 1])
            assert rc == E_RANGE and lent_untouched(*o)
            rc, *o = raw_dist_blame(e, [0, 0])
            assert rc == E_INVAL and lent_untouched(*o)


def test_the_one_rank_calls_still_refuse():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    live = np.ones(n, dtype=np.uint8)
    live[[7, 90]] = 0
    with Sharded(2, [parent], [root]) as S:
        S.run(live, np.zeros(50))
        for e in S.engines:
            rc, *o = raw_topic_blame(e, [0])  # ps_topic_blame on a multi-rank engine
            assert rc == E_STATE and lent_untouched(*o)
            a = [np.full(1, 0xABABABAB, dtype=np.uint32) for _ in range(4)]
            t = np.zeros(1, dtype=np.uint32)
            rc = e._L.ps_blame(e._h, t.ctypes.data_as(U32P), t.ctypes.data_as(U32P), 1, *(x.ctypes.data_as(U32P) for x in a))
            assert rc == E_STATE and all((x == 0xABABABAB).all() for x in a)
        check_blame(S, live, [50], [0])


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
                seen[r] = raw_dist_blame(e, [0])  # refused before anything is exchanged
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
        for rc, *o in seen:
            assert rc == E_STATE and lent_untouched(*o)
        S.one.publish(np.zeros(20, dtype=np.uint32))
        S.one.run()
        check_blame(S, live, [20], [0], "after the wait")
