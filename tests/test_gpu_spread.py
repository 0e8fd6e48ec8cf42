"""GPU: hops and duplicate copies for meshes and trees alike (ps_topic_spread;
DESIGN.md §5.5p) -- per topic and hop the forwarders reached and the messages
they hold, the nodes left out, and per peer the copies sent to it and those
beyond what it received, from a frontier BFS over the child lists.

Every comparison is bit-exact, all six arrays, against tests/spread_ref.py fed
from mesh_ref.Flood (meshes) or the oracle (trees): tests/test_spread_cpu.py
holds that reference against the flood itself.  Where every active topic is
named, deliv.sum() equals ps_stats.deliveries and dup.sum() ps_stats.duplicates.
The seam (PSAMD_AB=1 PSAMD_LOAD_COUNT=rows) makes the kernel count full rows
from their words."""
import ctypes as C
import threading

import numpy as np
import pytest

import hops_ref as HR
import load_ref as LR
import mesh_ref as MR
import psengine as PE
import spread_ref as SR
from test_gpu_drain_batch import random_tree
from test_gpu_drain_topics import kids_of, under
from test_gpu_load import seam

pytestmark = pytest.mark.gpu

COLS = PE.MAX_ROUNDS
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
FILL = 0xABABABABABABABAB
NAMES = ("reached", "deliv", "unreached", "stranded", "copies", "dup")


# ---- helpers ------------------------------------------------------------------------

def same(got, want, what=""):
    """The six arrays against spread_ref.window_spread's, bit for bit."""
    for name in NAMES:
        g, w = got[name], want[name]
        assert g.dtype == np.uint64 and g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what} {name}: {len(bad)} words differ, first {bad[:6].tolist()} got "
                                 f"{[int(g[tuple(b)]) for b in bad[:6]]} want {[int(w[tuple(b)]) for b in bad[:6]]}")


def mesh_topic(g, c, n=None, live=None):
    """A builder's graph as a reference topic of c messages: its reached set
    from mesh_ref.Flood, over n peers (the extra ones in no list) and under
    `live` where given."""
    rp, cl, root, lv = g[:4]
    n = len(lv) if n is None else n
    rp = np.concatenate([rp, np.full(n - len(lv), rp[-1], dtype=rp.dtype)])
    if live is None:
        live = np.concatenate([lv, np.ones(n - len(lv), dtype=np.uint8)])
    F = MR.flood(rp, cl, root, live)
    return (rp, cl, root, F.level >= 0, c), F


def tree_topic(n, parent, root, live, c):
    rp, cl = SR.tree_csr(parent, root)
    return rp, cl, root, LR.topic_load(n, root, live, c, parent=parent)[0] > 0, c


def against_stats(got, st, flood_dups):
    """Every active topic named, one window, one start round."""
    assert got["deliv"].sum() == st.deliveries
    assert got["dup"].astype(np.int64).sum() == st.duplicates == flood_dups
    per_round = np.array(list(st.deliveries_per_round), dtype=np.uint64)
    assert np.array_equal(got["deliv"].sum(axis=0)[:COLS - 1], per_round[:COLS - 1])
    assert not got["reached"][:, 0].any() and not got["deliv"][:, 0].any()


def raw_spread(eng, topics, which=(True,) * 6):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    rows = max(t.size, 1)
    a = [np.full((rows, COLS), FILL, dtype=np.uint64), np.full((rows, COLS), FILL, dtype=np.uint64),
         np.full(rows, FILL, dtype=np.uint64), np.full(rows, FILL, dtype=np.uint64),
         np.full(eng.n_peers, FILL, dtype=np.uint64), np.full(eng.n_peers, FILL, dtype=np.uint64)]
    rc = eng._L.ps_topic_spread(eng._h, t.ctypes.data_as(U32P), t.size,
                                *(x.ctypes.data_as(U64P) if w else None for x, w in zip(a, which)))
    return rc, a


def run_mesh(g, starts, what=""):
    """One run of len(starts) messages of topic 0 over a builder's graph; the
    six arrays against the reference, the engine's own totals against both."""
    c = len(starts)
    topic, F = mesh_topic(g, c)
    rp, cl, root, live = g[:4]
    want = SR.window_spread(len(live), [topic])
    starts = np.asarray(starts, dtype=np.uint32)
    with PE.Engine(len(live), 1) as eng:
        eng.set_children(0, root, rp, cl)
        eng.set_live(live)
        eng.publish(np.zeros(c), starts if starts.any() else None)
        st = eng.run()
        assert st.expand_mode == PE.MODE_COMPACT and st.windows == 1
        got = eng.topic_spread([0])
        same(got, want, what)
        assert got["deliv"].sum() == st.deliveries == c * F.deliveries
        assert got["dup"].astype(np.int64).sum() == st.duplicates == c * F.duplicates
        if not starts.any():
            against_stats(got, st, c * F.duplicates)
        assert got["stranded"][0] == 0
    return got, F


@pytest.fixture(scope="module")
def specials():
    g = MR.mesh_with_specials(300)
    MR.check_specials(*g, MR.flood(*g[:4]))
    return g


@pytest.fixture(scope="module")
def hubs():
    out = {}
    for deg in (63, 64, 65, 129, 600):
        g = MR.hub_mesh(deg)
        MR.check_hub(*g, MR.flood(*g[:4]))
        out[deg] = g
    return out


# ---- 1. the specials at four row widths ---------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("c", [1, 64, 65, 64 * 64 + 40])
def test_specials(specials, c, rows, monkeypatch):
    """A self-loop, a repeated edge, an edge into the root, two parents in one
    round, a later hit, a dead parent with a cut-off live child -- at rows of
    1, 1, 2 and 66 words; under the seam every row is counted word by word."""
    seam(monkeypatch, rows)
    got, F = run_mesh(specials, np.zeros(c), f"c {c}")
    facts = specials[4]
    root = specials[2]
    assert got["copies"][root] == c and got["dup"][root] == c  # everything sent to the root is a duplicate
    for p in (facts["self_loop"], facts["repeated"][1], facts["same_round"][0], facts["later"][0]):
        assert got["dup"][p] >= c, p
    for p in (facts["dead_parent"], facts["cut_off"]):
        assert got["copies"][p] == 0 and F.level[p] < 0
    assert got["unreached"][0] >= 2


# ---- 2. a hub: a frontier and a fan-out past one wave and one block -------------------

@pytest.mark.parametrize("wide", [None, 0, 1 << 20])
@pytest.mark.parametrize("deg", [63, 64, 65, 129, 600])
def test_hub(hubs, deg, wide, monkeypatch):
    """Exactly the live hub children carry dup == c.  By default the hub is
    walked by its wave and everybody else lane by lane; PSAMD_SPREAD_WIDE = 0
    walks every node by the wave and 2^20 none: the answer does not move."""
    if wide is not None:
        monkeypatch.setenv("PSAMD_AB", "1")
        monkeypatch.setenv("PSAMD_SPREAD_WIDE", str(wide))
    g = hubs[deg]
    c = 70
    got, F = run_mesh(g, np.zeros(c), f"hub {deg}")
    live, facts = g[3], g[4]
    want = np.zeros(len(live), dtype=np.uint64)
    want[[ch for ch in facts["listed"] if live[ch]]] = c
    assert np.array_equal(got["dup"], want)
    assert got["unreached"][0] == len(facts["dead_pos"])


# ---- 3. hops far past the node space's BFS depth ---------------------------------------

@pytest.mark.parametrize("n_chain", [8, 40, 300])
def test_detour(n_chain):
    """The node space is two levels deep; the forwarders' path is the chain:
    n_chain - 1 level launches, and from 255 hops on the clamped column."""
    got, F = run_mesh(MR.detour(n_chain), np.zeros(70), f"detour {n_chain}")
    assert got["unreached"][0] == 1 and not got["dup"].any()
    if n_chain == 300:
        assert (got["reached"][0, 1:255] == 1).all() and got["reached"][0, 255] == 45
        assert got["deliv"][0, 255] == 45 * 70
    else:
        assert (got["reached"][0, 1:n_chain] == 1).all() and not got["reached"][0, n_chain:].any()


# ---- 4. several start rounds: k through the gather path --------------------------------

@pytest.mark.parametrize("which", ["specials", "hub129"])
def test_start_rounds(specials, hubs, which):
    g = specials if which == "specials" else hubs[129]
    n_msgs = 200
    starts = np.random.default_rng(n_msgs).integers(0, 6, size=n_msgs)
    starts[:2] = (5, 0)
    multi, _ = run_mesh(g, starts, which)
    single, _ = run_mesh(g, np.zeros(n_msgs), which)
    for name in NAMES:
        assert np.array_equal(multi[name], single[name]), name


# ---- 5. two meshes that share peers, an idle topic and a tree in one request ------------

@pytest.mark.parametrize("order", [[0, 1, 2, 3], [3, 2, 1, 0], [1], [2], [3, 0]])
def test_several_topics(specials, hubs, order):
    n = 400
    rng = np.random.default_rng(52)
    live = np.ones(n, dtype=np.uint8)
    live[:300] &= specials[3]
    live[:len(hubs[65][3])] &= hubs[65][3]
    live[0] = 1
    par = random_tree(rng, n, 7)
    live[7] = 1
    counts = {0: 70, 1: 130, 2: 0, 3: 5}
    t0, F0 = mesh_topic(specials, counts[0], n, live)
    t1, F1 = mesh_topic(hubs[65], counts[1], n, live)
    t3 = tree_topic(n, par, 7, live, counts[3])
    topics = {0: t0, 1: t1, 2: (t3[0], t3[1], 7, t3[3], 0), 3: t3}
    with PE.Engine(n, 4) as eng:
        eng.set_children(0, specials[2], t0[0], t0[1])
        eng.set_children(1, hubs[65][2], t1[0], t1[1])
        eng.set_tree(2, 7, par)
        eng.set_tree(3, 7, par)
        eng.set_live(live)
        eng.publish(np.concatenate([np.full(k, t) for t, k in counts.items()]).astype(np.uint32))
        st = eng.run()
        assert st.windows == 1
        got = eng.topic_spread(order)
        same(got, SR.window_spread(n, [topics[t] for t in order]), str(order))
        assert not got["stranded"].any()
        if len(order) == 4:
            against_stats(got, st, counts[0] * F0.duplicates + counts[1] * F1.duplicates)
            # the call made twice gives equal arrays
            again = eng.topic_spread(order)
            for name in NAMES:
                assert np.array_equal(got[name], again[name]), name
        # the tree-only reads still refuse a mesh, and answer the tree beside it
        for call in (eng.topic_hops, eng.peer_downstream, eng.peer_cut):
            with pytest.raises(PE.EngineError) as ei:
                call([0])
            assert ei.value.code == E_STATE
            call([3])


# ---- 6. a tree alone --------------------------------------------------------------------

@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("c", [3, 8300])
def test_a_tree_alone(c, cut):
    """reached / deliv are ps_topic_hops' rows, copies is ps_peer_load's recv,
    dup is 0, and unreached is what the hop rows leave of the nodes."""
    rng = np.random.default_rng(66)
    n, root = 500, 2
    parent = random_tree(rng, n, root)
    live = np.ones(n, dtype=np.uint8)
    if cut:
        kids = kids_of(parent)
        live[max((p for p in kids if p != root), key=lambda p: len(under(kids, p)))] = 0
        live[rng.choice(np.setdiff1d(np.arange(n), [root]), 30, replace=False)] = 0
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.publish(np.zeros(c))
        st = eng.run()
        got = eng.topic_spread([0])
        same(got, SR.window_spread(n, [tree_topic(n, parent, root, live, c)]), "tree")
        nodes, reached, deliv = eng.topic_hops([0])
        recv, _ = eng.peer_load([0])
        assert np.array_equal(got["reached"], reached) and np.array_equal(got["deliv"], deliv)
        assert np.array_equal(got["copies"], recv) and not got["dup"].any() and not got["stranded"].any()
        assert got["unreached"][0] == nodes.sum() - reached.sum()
        assert (got["unreached"][0] > 0) == cut
        assert np.array_equal(nodes, HR.window_hops(n, live, [(root, c, parent)])[0])
        against_stats(got, st, 0)


# ---- 7. the last of three windows after a wider one ---------------------------------------

def test_last_window_after_a_wider_one(specials):
    """msg_window = 320: a run of one five-word window, then a run of three
    windows whose last holds 7 messages in one word.  The answer is the last
    window's; what the wider windows left in the rows is not counted."""
    rp, cl, root, live, _ = specials
    n = len(live)
    with PE.Engine(n, 1, msg_window=320) as eng:
        eng.set_children(0, root, rp, cl)
        eng.set_live(live)
        eng.publish(np.zeros(320))
        assert eng.run().windows == 1
        same(eng.topic_spread([0]), SR.window_spread(n, [mesh_topic(specials, 320)[0]]), "the wide window")
        eng.publish(np.zeros(2 * 320 + 7))
        assert eng.run().windows == 3
        got = eng.topic_spread([0])
        same(got, SR.window_spread(n, [mesh_topic(specials, 7)[0]]), "the last of three")
        again = eng.topic_spread([0])
        for name in NAMES:
            assert np.array_equal(got[name], again[name]), name


# ---- 8. the rules -------------------------------------------------------------------------

def test_rules(specials):
    rp, cl, root, live, _ = specials
    n = len(live)
    rng = np.random.default_rng(82)
    parent = random_tree(rng, n, 1)
    with PE.Engine(n, 3) as eng:
        eng.set_children(0, root, rp, cl)
        eng.set_tree(1, 1, parent)
        eng.set_live(live)
        rc, a = raw_spread(eng, [0])
        assert rc == E_NOTREADY and all((x == FILL).all() for x in a)  # before any run
        eng.publish(np.zeros(10))
        eng.run()
        assert raw_spread(eng, [0, 0])[0] == E_INVAL  # a topic named twice
        rc, a = raw_spread(eng, [0, 3])
        assert rc == E_RANGE and all((x == FILL).all() for x in a)  # nothing written
        assert raw_spread(eng, [0], which=(False,) * 6)[0] == E_INVAL
        assert eng._L.ps_topic_spread(eng._h, None, 1, a[0].ctypes.data_as(U64P), None, None, None, None, None) == E_INVAL
        # each output alone: written in full, the others untouched
        full = eng.topic_spread([0, 1])
        same(full, SR.window_spread(n, [mesh_topic(specials, 10)[0], tree_topic(n, parent, 1, live, 0)]), "full")
        for k, name in enumerate(NAMES):
            rc, a = raw_spread(eng, [0, 1], which=tuple(j == k for j in range(6)))
            assert rc == 0 and np.array_equal(a[k], full[name]), name
            assert all((a[j] == FILL).all() for j in range(6) if j != k), name
        # no topic: the peer arrays read zero, the others are not written
        rc, a = raw_spread(eng, [])
        assert rc == 0 and not a[4].any() and not a[5].any() and all((x == FILL).all() for x in a[:4])
        # an idle topic alone: zeros everywhere
        rc, a = raw_spread(eng, [1])
        assert rc == 0 and not any(x.any() for x in a)


def test_a_tree_set_anew_since_the_window():
    """Set over a join topic, a tree's record starts afresh: PS_E_STATE until
    the next run.  A mesh keeps no such record and the window's child lists
    stay on the device until the next build."""
    rng = np.random.default_rng(83)
    n = 200
    live = np.ones(n, dtype=np.uint8)
    p1 = random_tree(rng, n, 0)
    with PE.Engine(n, 1) as eng:
        eng.topic_create(0, 0, 2, 5)
        eng.join(0, np.arange(1, n))
        eng.publish(np.zeros(6))
        eng.run()
        before = eng.topic_spread([0])
        assert before["deliv"].sum() == 6 * (n - 1) and not before["dup"].any()
        eng.set_tree(0, 0, p1)
        rc, a = raw_spread(eng, [0])
        assert rc == E_STATE and all((x == FILL).all() for x in a)
        eng.publish(np.zeros(2))
        eng.run()
        same(eng.topic_spread([0]), SR.window_spread(n, [tree_topic(n, p1, 0, live, 2)]), "after the next run")


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
            rc, a = raw_spread(e, [0])
            assert rc == E_STATE and all((x == FILL).all() for x in a)
    finally:
        for e in engines:
            e.close()
