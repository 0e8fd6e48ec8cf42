"""GPU: blame records behind every window (ps_blame_track / ps_blame_take;
DESIGN.md §5.5s) -- ps_topic_blame's records of every window of every run,
appended on the device at a cursor that lives there, lent by one take.

Every record is compared bit for bit against tests/blame_track_ref.py (blame_ref
per window, composed), ordered by the engine's G_NODE_PEER; a run of one window
also against ps_topic_blame called right after it.  Where the node space
changes inside a run (a drop, churn) a past window's node order cannot be read
back: there each (window, topic) slice is compared as a set keyed by peer, and
hop must not decrease inside a slice."""
import ctypes as C

import numpy as np
import pytest

import blame_ref as BR
import blame_track_ref as TR
import oracle as O
import psengine as PE
from psengine import workloads as WL
from test_blame_cpu import SENTINEL
from test_blame_track_cpu import take_outs, take_untouched
from test_gpu_blame import node_order
from test_gpu_churn import assert_builds, make_engine
from test_gpu_downstream import fan_tree, path
from test_gpu_drain_batch import random_mesh2, random_tree
from test_gpu_drain_shared import one_topic
from test_gpu_drain_topics import kids_of, under
from test_gpu_load import heap_tree, seam
from test_gpu_sink import drop_engine, even_batches

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U32P = C.POINTER(C.c_uint32)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
KEYS = TR.KEYS
COUNT_KEYS = ("n_windows", "n_skipped", "total", "stored")


# ---- helpers ------------------------------------------------------------------------

def take(eng):
    """blame_take's dict and whether it overflowed (PS_E_RANGE: the dict rides on the error)."""
    try:
        return eng.blame_take(), False
    except PE.EngineError as ex:
        assert ex.code == E_RANGE
        return ex.partial, True


def same(got, want, what=""):
    assert set(got) == {"rec_off", *KEYS, *COUNT_KEYS}, what
    assert got["rec_off"].dtype == np.uint64 and all(got[k].dtype == np.uint32 for k in KEYS), what
    for k in COUNT_KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["rec_off"], want["rec_off"]), (what, got["rec_off"][:12], want["rec_off"][:12])
    for k in KEYS:
        g, w = got[k], want[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{what} {k}: {bad.size} records differ, first {bad[:6]} got {g[bad[:6]]} want {w[bad[:6]]}")


def check_take(eng, n, windows, what="", cap=None, n_skipped=0):
    """One take against the windows composed (and cut down to `cap`)."""
    want = TR.compose(windows, n, n_skipped)
    over = False
    if cap is not None:
        want, over = TR.capped(want, cap)
    got, got_over = take(eng)
    assert got_over == over, (what, got["total"], cap)
    same(got, want, what)
    return got


def row(eng, topics, tables):
    """A window's row on the node space that stands: tables[i] None where position i holds no record."""
    return TR.window(tables, [node_order(eng, t) if tab is not None else None for t, tab in zip(topics, tables)])


def against_topic_blame(eng, topics, got, w, what=""):
    """Window w of a take against ps_topic_blame on the window that stands."""
    r = eng.topic_blame(topics)
    n = len(topics)
    off = got["rec_off"].astype(np.int64)
    lo = int(off[w * n])
    assert np.array_equal(off[w * n:w * n + n + 1] - lo, r["rec_off"].astype(np.int64)), what
    for k in KEYS:
        assert np.array_equal(got[k][lo:lo + r[k].size], r[k]), (what, k)


def dead_mask(n, dead):
    live = np.ones(n, dtype=np.uint8)
    live[list(dead)] = 0
    return live


def raw_track(eng, topics, rec_cap=0):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    return eng._L.ps_blame_track(eng._h, t.ctypes.data_as(U32P) if t.size else None, t.size, rec_cap)


def raw_take(eng, which=(True,) * 5):
    off, ptrs, counts = take_outs()
    rc = eng._L.ps_blame_take(eng._h, C.byref(off), *(C.byref(p) if w else None for p, w in zip(ptrs, which)),
                              *(C.byref(c) for c in counts))
    return rc, off, ptrs, counts


# ---- 1. windows, runs and takes -----------------------------------------------------

def test_tracking_windows_runs_and_takes():
    """msg_window = 64, 150 + 70 messages: windows of (64, 64), (64, 6), (22, 0),
    tracked in request order [1, 0]; then single-window runs under two other
    masks and an all-live one -- a window without a record between two with;
    one take of six windows, a take of none, take-run-take, track again, a subset."""
    n, root, parent, live = one_topic(0, 71)
    rng = np.random.default_rng(71)
    p1 = random_tree(rng, n, 9)
    live[9] = 1
    live2 = (rng.random(n) > 0.2).astype(np.uint8)
    live2[[root, 9]] = 1
    all_live = np.ones(n, dtype=np.uint8)
    req = [1, 0]

    def tabs(lv, c0, c1):
        return [BR.topic_blame(n, 9, lv, c1, p1), BR.topic_blame(n, root, lv, c0, parent)]

    with PE.Engine(n, 2, msg_window=64) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, 9, p1)
        eng.set_live(live)
        eng.blame_track(req)
        same(eng.blame_take(), TR.compose([], 2), "nothing has run")
        eng.publish(rng.permutation(np.concatenate([np.zeros(150), np.ones(70)])).astype(np.uint32))
        st = eng.run()
        assert st.windows == 3
        wins = [row(eng, req, tabs(live, c0, c1)) for c0, c1 in ((64, 64), (64, 6), (22, 0))]
        last = eng.topic_blame(req)  # the blocking call while the records stand: the last window alone
        assert last["rec_off"][1] == 0 and last["peer"].size > 0
        for lv, c0, c1 in ((live2, 10, 3), (all_live, 0, 64), (live2, 5, 0)):
            eng.set_live(lv)
            eng.publish(np.concatenate([np.zeros(c0), np.ones(c1)]).astype(np.uint32))
            assert eng.run().windows == 1
            wins.append(row(eng, req, tabs(lv, c0, c1)))
        got = check_take(eng, 2, wins, "six windows")
        assert got["n_windows"] == 6 and got["total"] > 0
        off = got["rec_off"].astype(np.int64)
        assert off[8] == off[10] and off[6] < off[8] and off[10] < off[12]  # the all-live window lies between two with records
        against_topic_blame(eng, req, got, 5, "the last run")
        lo = int(off[4])
        assert np.array_equal(got["peer"][lo:int(off[6])], last["peer"])  # window 2 is what the blocking call saw
        same(eng.blame_take(), TR.compose([], 2), "a second take")
        # take, run, take: the new run alone, equal to the blocking call's answer
        eng.set_live(live)
        eng.publish(np.zeros(40))
        eng.run()
        got = check_take(eng, 2, [row(eng, req, tabs(live, 40, 0))], "the new run")
        against_topic_blame(eng, req, got, 0, "the new run")
        # tracking again discards what was not taken; a subset tracked
        eng.publish(np.zeros(5))
        eng.run()
        eng.blame_track([0])
        same(eng.blame_take(), TR.compose([], 1), "tracked again")
        eng.publish(np.concatenate([np.zeros(7), np.ones(9)]).astype(np.uint32))
        eng.run()
        got = check_take(eng, 1, [row(eng, [0], [BR.topic_blame(n, root, live, 7, parent)])], "topic 0 alone")
        against_topic_blame(eng, [0], got, 0, "topic 0 alone")


# ---- 2. cursor bases ----------------------------------------------------------------

@pytest.mark.parametrize("n", [2048, 2049, 2050])
@pytest.mark.parametrize("first", [1, 63, 64, 65])
def test_cursor_bases(first, n):
    """One message: one-word rows, 2,048 to a strip, so strips of 2,047 / 2,048
    / 2,049 nodes.  The first window leaves exactly `first` records (dead
    leaves); the second emits from that base, with records at a strip's first
    and last node."""
    parent = heap_tree(n)
    leaves = list(range(n - first, n))
    assert n - first > (n - 1) // 2  # leaves all
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        eng.blame_track([0])
        wins = []
        for dead in (leaves, [1, n - 1]):
            live = dead_mask(n, dead)
            eng.set_live(live)
            eng.publish(np.zeros(1))
            eng.run()
            wins.append(row(eng, [0], [BR.topic_blame(n, 0, live, 1, parent)]))
        got = check_take(eng, 1, wins, f"base {first}, {n} peers")
        off = got["rec_off"].tolist()
        assert off[1] == first and off[2] - off[1] > 1000
        second = got["peer"][first:]
        assert second[0] == 1 and second[-1] == n - 1 and (2048 in second) == (n > 2048)
        against_topic_blame(eng, [0], got, 1, "second window")


# ---- 3. caps ------------------------------------------------------------------------

def test_caps():
    """Four one-window runs on a path of 40 leave 10, 5, 20 and 2 records: a
    cap of 1, the total, the total less one, at a window boundary, between two
    records of one strip (the last window would fit behind: it stores nothing)."""
    n = 40
    parent = path(n)
    deads = (30, 35, 20, 38)
    total = sum(n - d for d in deads)
    assert total == 37
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        for cap in (1, total, total - 1, 10, 15, 12, 36, total + 1, 0):
            eng.blame_track([0], cap)
            wins = []
            for d in deads:
                live = dead_mask(n, [d])
                eng.set_live(live)
                eng.publish(np.zeros(2))
                eng.run()
                wins.append(row(eng, [0], [BR.topic_blame(n, 0, live, 2, parent)]))
            got = check_take(eng, 1, wins, f"cap {cap}", cap=cap or None)
            assert got["rec_off"].tolist() == [0, 10, 15, 35, 37] and got["total"] == total
            assert got["stored"] == (min(cap, total) if cap else total)
            same(eng.blame_take(), TR.compose([], 1), f"cap {cap}: the flag is cleared")
        assert raw_track(eng, [0], (1 << 30) + 1) == E_RANGE
        assert raw_track(eng, [0], 1 << 62) == E_RANGE


def test_own_cap_grows_with_the_windows():
    """The engine's own cap: 40 one-window runs on a path of 16 between two
    takes -- rec_off and the record arrays grow with their contents kept; the
    next interval of the same shape finds the room."""
    n = 16
    parent = path(n)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        eng.blame_track([0])
        for rep in range(2):
            wins = []
            for i in range(40):
                live = dead_mask(n, [1 + i % 15] if i % 7 else [])
                eng.set_live(live)
                eng.publish(np.zeros(1 + i % 3))
                eng.run()
                wins.append(row(eng, [0], [BR.topic_blame(n, 0, live, 1 + i % 3, parent)]))
            got = check_take(eng, 1, wins, f"interval {rep}")
            assert got["n_windows"] == 40 and got["total"] == got["stored"] > 200


# ---- 4. a request wider than a block ------------------------------------------------

def test_more_topics_than_a_block():
    """600 tracked topics, paths of 4 peers each, most idle in each window: the
    commit kernel's rows span three blocks."""
    rng = np.random.default_rng(8)
    n, nt = 60, 600
    trees = []
    for t in range(nt):
        peers = rng.choice(n, size=4, replace=False)
        p = np.full(n, NONE, dtype=np.uint32)
        p[peers[1:]] = peers[:-1]
        trees.append((int(peers[0]), p))
    req = rng.permutation(nt).astype(np.uint32)
    with PE.Engine(n, nt) as eng:
        for t, (root, p) in enumerate(trees):
            eng.set_tree(t, root, p)
        eng.blame_track(req)
        wins = []
        for w in range(3):
            live = (rng.random(n) > 0.3).astype(np.uint8)
            eng.set_live(live)
            active = rng.choice(nt, size=(5, 300, 40)[w], replace=False)
            msgs = np.repeat(active, rng.integers(1, 4, size=active.size)).astype(np.uint32)
            eng.publish(rng.permutation(msgs))
            assert eng.run().windows == 1
            c = np.bincount(msgs, minlength=nt)
            tables = [BR.topic_blame(n, trees[t][0], live, int(c[t]), trees[t][1]) if c[t] else None for t in req]
            wins.append(row(eng, req, tables))
        got = check_take(eng, nt, wins, "600 topics")
        assert got["total"] > 50 and got["rec_off"].size == 3 * nt + 1
        against_topic_blame(eng, req, got, 2, "600 topics, last window")


# ---- 5. the shapes the front and the sweep are pinned at ----------------------------

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("n_msgs", [1, 4096, 4097, 8300])
def test_row_widths(n_msgs, rows, monkeypatch):
    """Rows of 1, 64, 65 and 130 words, plain and with every full row counted from its words."""
    seam(monkeypatch, rows)
    n, root, parent, live = one_topic(n_msgs, n_msgs)
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, root, parent)
        eng.set_live(live)
        eng.blame_track([0])
        eng.publish(np.zeros(n_msgs))
        eng.run()
        got = check_take(eng, 1, [row(eng, [0], [BR.topic_blame(n, root, live, n_msgs, parent)])], f"n_msgs {n_msgs}")
        assert got["total"] > 1 and (got["missed"] == n_msgs).all()
        against_topic_blame(eng, [0], got, 0, f"n_msgs {n_msgs}")


@pytest.mark.parametrize("a,b", [(64, 65), (65, 64)])
def test_fan_out_64_and_65_under_a_node_that_lacks_messages(a, b):
    parent = fan_tree(a, b)
    n = parent.size
    with PE.Engine(n, 1) as eng:
        eng.set_tree(0, 0, parent)
        eng.blame_track([0])
        wins = []
        for dead in ([1], [2], [1, 2], [3, 2 + a, 3 + a, 2 + a + b]):
            live = dead_mask(n, dead)
            eng.set_live(live)
            eng.publish(np.zeros(2))
            eng.run()
            wins.append(row(eng, [0], [BR.topic_blame(n, 0, live, 2, parent)]))
        got = check_take(eng, 1, wins, f"fan {a} {b}")
        assert np.diff(got["rec_off"].astype(np.int64)).tolist() == [1 + 2 * a, 1 + 2 * b, 2 + 2 * (a + b), 8]
        against_topic_blame(eng, [0], got, 3, "fan, last window")


# ---- 6. the node space changing inside a run ----------------------------------------

def tree_windows(ot, n, k, dropped=False):
    """k messages over oracle.Tree ot as the engine runs them (the windows of
    test_gpu_cut.tree_window): every window's table and peers, and the deliveries."""
    left, out, deliveries = k, [], 0
    while left:
        par = ot.parents()
        hop = ot.message()
        c = 1 if dropped or not np.array_equal(ot.parents(), par) else left
        dropped = False
        for _ in range(c - 1):
            assert np.array_equal(ot.message(), hop)
        got = hop != 0xFF
        got[ot.root] = False
        out.append(BR.from_parents(n, ot.root, par, c * got, c))
        deliveries += c * int(got.sum())
        left -= c
    return out, deliveries


def as_set(table):
    """A table's records in ascending peer order."""
    return BR.records(table, np.concatenate([[0], np.nonzero(table.member)[0]]))


def same_slices_as_sets(got, n_req, windows, what=""):
    """windows[w][i]: the table of window w, position i, or None.  Each slice
    as a set keyed by peer; hop never decreases inside one."""
    assert got["n_windows"] == len(windows) and got["stored"] == got["total"], what
    for w, tables in enumerate(windows):
        for i, tab in enumerate(tables):
            s = TR.slice_of(got, n_req, w, i)
            assert (np.diff(s[2].astype(np.int64)) >= 0).all(), (what, w, i)
            want = as_set(tab) if tab is not None else tuple(np.empty(0, dtype=np.uint32) for _ in KEYS)
            by_peer = np.argsort(s[0], kind="stable")
            for k, g, x in zip(KEYS, s, want):
                assert np.array_equal(g[by_peer], x), (what, w, i, k)


def test_a_run_split_by_a_drop():
    """An interior peer dropped: topic 0's first message runs alone over the
    old tree, the rest over the repaired one -- a rebuilt node space between
    two windows of one run; then a masked run over the repaired trees."""
    n, seed = 60, 3
    topics = np.array([0] * 5 + [1] * 5, dtype=np.uint32)
    ots = [O.Tree(n, 0, 2, 5, PE.Engine.topic_seed(seed, t)) for t in (0, 1)]
    for ot in ots:
        ot.join_all(range(1, n))
    with drop_engine(n, seed) as eng:
        kids = kids_of(eng.parents(0))
        dead = max((p for p in kids if p != 0), key=lambda p: (len(kids[p]), len(under(kids, p))))
        eng.drop(0, [dead])
        assert ots[0].drop(dead) == 0
        eng.blame_track([0, 1])
        eng.publish(topics)
        st = eng.run()
        (t0, d0), (t1, d1) = tree_windows(ots[0], n, 5, dropped=True), tree_windows(ots[1], n, 5)
        assert (len(t0), len(t1), st.windows) == (2, 1, 2) and d0 + d1 == st.deliveries
        wins = [[t0[0], t1[0]], [t0[1], None]]
        # something to blame on the repaired trees
        live = (np.random.default_rng(3).random(n) > 0.15).astype(np.uint8)
        live[0] = 1
        eng.set_live(live)
        eng.publish(topics)
        assert eng.run().windows == 1
        masked = []
        for ot in ots:
            par = ot.parents()
            rp, cl = O.parents_to_csr(np.where(np.arange(n) == 0, NONE, par).astype(np.uint32))
            _, hops, _ = O.disseminate(rp, cl, 0, live, 5)
            got = hops != 0xFF
            got[:, 0] = False
            masked.append(BR.from_parents(n, 0, par, got.sum(axis=0), 5))
        wins.append(masked)
        got, over = take(eng)
        assert not over and got["n_skipped"] == 0 and got["total"] > 0
        same_slices_as_sets(got, 2, wins, "drop")
        against_topic_blame(eng, [0, 1], got, 2, "drop, the masked run")


@pytest.mark.parametrize("gpu_build", [True, False])
def test_churn(gpu_build):
    """Joins, leaves and drops between runs, the node space rebuilt on the GPU
    or on the host every batch, a live mask on top: every window's records
    follow the oracle's trees."""
    rng = np.random.default_rng(17)
    n, seed = 3000, 4
    eng = make_engine(n, gpu_build, seed=seed)
    ot = O.Tree(n, 0, 2, 5, PE.Engine.topic_seed(seed, 0))
    eng.topic_create(0, 0, 2, 5)
    eng.join(0, np.arange(1, n, 2))
    ot.join_all(range(1, n, 2))
    members = set(range(1, n, 2))
    eng.blame_track([0])
    wins, built = [], 0
    with eng:
        for step in range(6):
            outs = [p for p in range(1, n) if p not in members]
            join = rng.choice(outs, size=20, replace=False)
            st = eng.join(0, join, check=False)
            for p, s in zip(join, st):
                assert ot.join(int(p)) == s
            members |= {int(p) for p, s in zip(join, st) if s == 0}
            leave = rng.choice(sorted(members), size=15, replace=False)
            for p in leave:
                assert ot.leave(int(p)) in (0, -3)
            try:
                eng.leave(0, leave)
            except PE.EngineError:
                pass
            members -= {int(p) for p in leave}
            if step % 3 == 1:
                p = int(rng.choice(sorted(members)))
                eng.drop(0, [p])
                assert ot.drop(p) == 0
                members.discard(p)
            k = int(rng.integers(2, 6))
            eng.publish(np.zeros(k))
            run = eng.run()
            tables, d = tree_windows(ot, n, k, dropped=step % 3 == 1)
            assert run.deliveries == d and run.windows == len(tables), step
            wins += [[t] for t in tables]
            assert np.array_equal(eng.parents(0), ot.parents()), step
            built = assert_builds(eng, gpu_build, built)
        live = (rng.random(n) > 0.05).astype(np.uint8)
        live[0] = 1
        eng.set_live(live)
        eng.publish(np.zeros(3))
        eng.run()
        par = ot.parents()
        rp, cl = O.parents_to_csr(np.where(np.arange(n) == 0, NONE, par).astype(np.uint32))
        _, hops, _ = O.disseminate(rp, cl, 0, live, 3)
        reached = hops != 0xFF
        reached[:, 0] = False
        wins.append([BR.from_parents(n, 0, par, reached.sum(axis=0), 3)])
        got, over = take(eng)
        assert not over and got["total"] > 0
        same_slices_as_sets(got, 1, wins, f"churn gpu_build {gpu_build}")
        against_topic_blame(eng, [0], got, len(wins) - 1, "churn, the masked run")


# ---- 7. pipelined -------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["deep", "twin"])
def test_pipelined(shape):
    """Six run_async over a shape whose windows overlap their predecessors
    (test_gpu_cut.test_pipelined's), 3 % dead: the records of the same six
    batches run one after the other, entry for entry."""
    if shape == "deep":
        wl = WL.cfg3(200_000, 16, 5000)
        batches, plan = even_batches(len(wl.topics), 6, 52), {"overlap_min_bytes": 0}
    else:
        wl = WL.cfg3(60_000, 16, 4000)
        batches, plan = even_batches(len(wl.topics), 6, 51), {"flood": 0}
    live = (np.random.default_rng(11).random(wl.n_peers) >= 0.03).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    order = np.arange(len(wl.topics), dtype=np.uint32)[::-1].copy()

    def make():
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=64, plan=plan)
        WL.build_engine_topics(e, wl)
        e.set_live(live)
        e.blame_track(order, 1 << 22)
        return e

    with make() as e:
        for b in batches:
            e.publish(b)
            e.run()
        t0 = e.blame_take()
        last = e.topic_blame(order)
    with make() as e:
        for i, b in enumerate(batches):
            e.publish(b)
            e.run_async()
            if i:
                e.wait()
        rc, off, ptrs, counts = raw_take(e)  # a run in flight: refused, nothing changes
        assert rc == E_STATE and take_untouched(off, ptrs, counts)
        e.wait()
        t1 = e.blame_take()
        over = e.overlapped_windows()
        against_topic_blame(e, order, t1, 11, shape + " last window")
    print("pipelined", shape, "overlapped", over, "records", t1["total"])
    assert over > 0 and t0["n_windows"] == t1["n_windows"] == 12 and t1["total"] == t1["stored"] > 0
    same(t1, t0, shape)
    # the same node space and mask in each of the 12 windows
    assert t1["total"] == 12 * last["peer"].size
    for k in KEYS:
        assert np.array_equal(t1[k], np.tile(last[k], 12)), k


# ---- 8. beside the sink and the other trackers --------------------------------------

def test_with_a_sink_and_the_other_trackers():
    """A topics sink and load, hop, downstream, cut and report tracking at
    once: the blame records against their reference, against ps_cut_take over
    the same windows (three bincount identities) and against the sink's
    exceptions, slice for slice."""
    n, root, parent, live = one_topic(0, 91)
    rng = np.random.default_rng(91)
    msgs = [rng.integers(0, 2, size=150).astype(np.uint32), np.zeros(70, dtype=np.uint32)]
    c = [int((msgs[0] == t).sum()) for t in (0, 1)]
    assert 64 < min(c) and max(c) <= 128
    counts = [(64, 64), (c[0] - 64, c[1] - 64), (64, 0), (6, 0)]

    def go(others):
        with PE.Engine(n, 2, msg_window=64) as e:
            e.set_tree(0, root, parent)
            e.set_tree(1, root, parent)
            e.set_live(live)
            if others:
                e.sink_set_topics([0, 1])
                e.load_track([0, 1])
                e.hops_track([0, 1])
                e.downstream_track([0, 1])
                e.cut_track([0, 1])
                e.report_track([0, 1])
            e.blame_track([0, 1])
            views = []
            for m in msgs:
                e.publish(m)
                e.run()
                if others:
                    views.append(e.sink_take_topics())
            wins = [row(e, [0, 1], [BR.topic_blame(n, root, live, ct, parent) for ct in cs]) for cs in counts]
            return e.blame_take(), wins, views, e.cut_take() if others else None

    got, wins, views, cut = go(True)
    alone = go(False)[0]
    same(got, TR.compose(wins, 2), "beside the others")
    same(got, alone, "as alone")
    assert got["n_windows"] == 4 and got["total"] > 0
    # ps_cut_take over the same windows
    assert cut[4:] == (4, 0)
    w = got["missed"].astype(np.int64)
    own = got["peer"] == got["cut_peer"]
    u64 = lambda x: x.astype(np.uint64)
    assert np.array_equal(u64(np.bincount(got["peer"], weights=w, minlength=n)), cut[0])
    assert np.array_equal(u64(np.bincount(got["cut_peer"], weights=w, minlength=n)), cut[3])
    assert int(own.sum()) == int(cut[1].sum()) and np.array_equal(u64(np.bincount(got["peer"][own], minlength=n)), cut[1])
    # the sink's exceptions, (window, topic) slice for slice: the same peers in the same order
    w0 = 0
    for v in views:
        eo = v["exc_off"].astype(np.int64)
        for j in range(v["n_windows"] * 2):
            s = TR.slice_of(got, 2, w0 + j // 2, j % 2)
            assert np.array_equal(s[0], v["exc_peer"][eo[j]:eo[j + 1]]), (w0, j)
        w0 += v["n_windows"]
    assert w0 == 4


# ---- 9. meshes and refusals ---------------------------------------------------------

def test_meshes():
    rng = np.random.default_rng(41)
    n, root = 400, 5
    rp, cl = random_mesh2(rng, n, root)
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_children(1, root, rp, cl)
        eng.set_live(live)
        assert raw_track(eng, [0, 1]) == E_STATE and raw_track(eng, [1]) == E_STATE  # a mesh is not tracked
        assert raw_take(eng)[0] == E_NOTREADY
        eng.blame_track([0])
        eng.publish(np.concatenate([np.zeros(70), np.ones(70)]).astype(np.uint32))
        assert eng.run().windows == 1
        wins = [row(eng, [0], [BR.topic_blame(n, root, live, 70, parent)])]
        # the tracked tree becomes a mesh: that window's slice is empty, and it is counted
        eng.set_children(0, root, rp, cl)
        eng.publish(np.zeros(5))
        eng.run()
        wins.append([None])
        # ... and a tree again
        eng.set_tree(0, root, parent)
        eng.publish(np.zeros(3))
        eng.run()
        wins.append(row(eng, [0], [BR.topic_blame(n, root, live, 3, parent)]))
        got = check_take(eng, 1, wins, "tree, mesh, tree", n_skipped=1)
        assert got["rec_off"][1] == got["rec_off"][2] < got["rec_off"][3]
        against_topic_blame(eng, [0], got, 2, "a tree again")


def test_a_topic_set_anew_over_another_kind():
    """A parent array set over a join topic between two runs: the tracker
    follows the new tree from its first window on."""
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
        eng.blame_track([0, 1])
        eng.publish(np.array([0] * 4, dtype=np.uint32))
        eng.run()
        wins = [row(eng, [0, 1], [BR.topic_blame(n, 0, live, 4, p0), None])]
        eng.set_tree(1, 0, p1)
        eng.publish(np.array([0] * 3 + [1] * 2, dtype=np.uint32))
        eng.run()
        wins.append(row(eng, [0, 1], [BR.topic_blame(n, 0, live, 3, p0), BR.topic_blame(n, 0, live, 2, p1)]))
        got = check_take(eng, 2, wins, "set anew")
        assert got["rec_off"][3] < got["rec_off"][4]
        against_topic_blame(eng, [0, 1], got, 1, "set anew")


def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(3)]
    try:
        # an engine that is tracking takes no ranks
        engines[2].blame_track([0])
        with pytest.raises(PE.EngineError) as ei:
            engines[2].dist_init_loopback(lb, 0, PE.PART_PEER)
        assert ei.value.code == E_STATE
        for r, e in enumerate(engines[:2]):
            e.dist_init_loopback(lb, r, PE.PART_PEER)
            e.set_tree(0, root, parent)
            assert raw_track(e, [0]) == E_STATE  # one rank only
            assert raw_take(e)[0] == E_NOTREADY
    finally:
        for e in engines:
            e.close()


# ---- 10. return codes and views -----------------------------------------------------

def test_rules():
    rng = np.random.default_rng(82)
    n, root = 300, 1
    parent = random_tree(rng, n, root)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    with PE.Engine(n, 2) as eng:
        eng.set_tree(0, root, parent)
        eng.set_tree(1, root, parent)
        eng.set_live(live)
        rc, off, ptrs, counts = raw_take(eng)
        assert rc == E_NOTREADY and take_untouched(off, ptrs, counts)
        # tracking: a refused call leaves the previous tracking
        eng.blame_track([0])
        assert raw_track(eng, [1, 1]) == E_INVAL and raw_track(eng, [0, 5]) == E_RANGE
        assert eng._L.ps_blame_track(eng._h, None, 2, 0) == E_INVAL
        assert raw_track(eng, [1], (1 << 30) + 1) == E_RANGE
        eng.publish(np.zeros(3))
        eng.run()
        w3 = row(eng, [0], [BR.topic_blame(n, root, live, 3, parent)])
        want = TR.compose([w3], 1)
        total = want["total"]
        assert total > 0
        # the take's arguments: nothing is written, nothing is taken
        o, ps, cs = take_outs()
        recs, cnt = [C.byref(p) for p in ps], [C.byref(c) for c in cs]
        assert eng._L.ps_blame_take(eng._h, None, *recs, *cnt) == E_INVAL
        for i in range(4):
            assert eng._L.ps_blame_take(eng._h, C.byref(o), *recs, *(None if j == i else c for j, c in enumerate(cnt))) == E_INVAL
        assert take_untouched(o, ps, cs)
        same(eng.blame_take(), want, "three messages")
        # all 32 NULL patterns of the five record pointers: those asked for are lent, the others left alone
        for mask in range(32):
            which = tuple(bool(mask >> i & 1) for i in range(5))
            eng.publish(np.zeros(3))
            eng.run()
            rc, off, ptrs, counts = raw_take(eng, which)
            assert rc == 0 and [c.value for c in counts] == [1, 0, total, total], which
            assert PE._view(off, 2, np.uint64).tolist() == [0, total]
            for k, p, w in zip(KEYS, ptrs, which):
                if w:
                    assert np.array_equal(PE._view(p, total, np.uint32), want[k]), (which, k)
                else:
                    assert C.cast(p, C.c_void_p).value == SENTINEL, (which, k)
        # the view read back after other calls and another run: valid until the next take or track call
        eng.publish(np.zeros(3))
        eng.run()
        rc, off, ptrs, counts = raw_take(eng)
        assert rc == 0
        blocking = eng.topic_blame([0])  # a view of its own
        eng.peer_cut([0])
        eng.set_live(np.ones(n, dtype=np.uint8))
        eng.publish(np.zeros(9))
        eng.run()
        assert PE._view(off, 2, np.uint64).tolist() == [0, total]
        for k, p in zip(KEYS, ptrs):
            assert np.array_equal(PE._view(p, total, np.uint32), want[k]) and np.array_equal(blocking[k], want[k]), k
        same(eng.blame_take(), TR.compose([row(eng, [0], [BR.topic_blame(n, root, np.ones(n, dtype=np.uint8), 9, parent)])], 1),
             "all live")
        eng.set_live(live)
        # a run in flight
        eng.publish(np.zeros(3))
        eng.run_async()
        assert raw_track(eng, [1]) == E_STATE
        rc, off, ptrs, counts = raw_take(eng)
        assert rc == E_STATE and take_untouched(off, ptrs, counts)
        eng.wait()
        same(eng.blame_take(), want, "three messages, asynchronous")
        # an overflowing take sets every output
        eng.blame_track([0], total - 1)
        eng.publish(np.zeros(3))
        eng.run()
        rc, off, ptrs, counts = raw_take(eng)
        assert rc == E_RANGE and [c.value for c in counts] == [1, 0, total, total - 1]
        assert PE._view(off, 2, np.uint64).tolist() == [0, total]
        for k, p in zip(KEYS, ptrs):
            assert np.array_equal(PE._view(p, total - 1, np.uint32), want[k][:total - 1]), k
        # clearing: nothing is tracked, the run is as ever
        eng.blame_track([])
        rc, off, ptrs, counts = raw_take(eng)
        assert rc == E_NOTREADY and take_untouched(off, ptrs, counts)
        eng.publish(np.zeros(3))
        eng.run()
        assert np.array_equal(eng.topic_blame([0])["peer"], want["peer"])
