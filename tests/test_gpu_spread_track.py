"""GPU: hops and duplicate copies behind every window (ps_spread_track /
ps_spread_take) -- ps_topic_spread's answer of every window
of every run, meshes and trees alike, summed on the device and copied by one
take.

Every comparison is bit-exact, all six arrays, against tests/spread_track_ref.py
(spread_ref.window_spread summed over the windows) or against the sum of the
blocking call's answers on the same engine.  Every healthy case asserts
n_truncated == 0 and stranded == 0: the pass enqueues the window's last round
+ 1 level launches with no look at the frontier, and a loss would show there."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as MR
import psengine as PE
import spread_ref as SR
import spread_track_ref as TR
from psengine import workloads as WL
from test_gpu_churn import assert_builds, make_engine
from test_gpu_drain_batch import random_tree
from test_gpu_load import seam
from test_gpu_sink import even_batches
from test_gpu_spread import mesh_topic, same, tree_topic

pytestmark = pytest.mark.gpu

COLS = PE.MAX_ROUNDS
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL, E_STATE, E_RANGE, E_NOTREADY = -1, -3, -7, -8
FILL = 0xABABABABABABABAB
NAMES = TR.NAMES


# ---- helpers ------------------------------------------------------------------------

def healthy(got, n_windows, what=""):
    assert got["n_windows"] == n_windows and got["n_truncated"] == 0, (what, got["n_windows"], got["n_truncated"])
    assert not got["stranded"].any(), what


def times(part, k):
    """A window's arrays k times over (modulo 2^64, as the device adds)."""
    total = TR.zeros(part["copies"].shape[0], part["unreached"].shape[0])
    for _ in range(k):
        TR.add(total, part)
    return total


def raw_track(eng, topics):
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    return eng._L.ps_spread_track(eng._h, t.ctypes.data_as(U32P) if t.size else None, t.size)


def raw_take(eng, n, which=(True,) * 6, counts=(True, True)):
    rows = max(n, 1)
    a = [np.full((rows, COLS), FILL, dtype=np.uint64), np.full((rows, COLS), FILL, dtype=np.uint64),
         np.full(rows, FILL, dtype=np.uint64), np.full(rows, FILL, dtype=np.uint64),
         np.full(eng.n_peers, FILL, dtype=np.uint64), np.full(eng.n_peers, FILL, dtype=np.uint64)]
    c = [C.c_uint64(0xC0C0), C.c_uint64(0xC1C1)]
    rc = eng._L.ps_spread_take(eng._h, *(x.ctypes.data_as(U64P) if w else None for x, w in zip(a, which)),
                               *(C.byref(x) if w else None for x, w in zip(c, counts)))
    return rc, a, [x.value for x in c]


def mesh_engine(g, **kw):
    rp, cl, root, live = g[:4]
    eng = PE.Engine(len(live), 1, **kw)
    eng.set_children(0, root, rp, cl)
    eng.set_live(live)
    return eng


def tracked_runs(g, starts, runs=1, what=""):
    """`runs` runs of len(starts) messages of topic 0 over a builder's graph,
    tracked; one take against the reference summed, a second reads zeros."""
    c = len(starts)
    topic, F = mesh_topic(g, c)
    n = len(g[3])
    starts = np.asarray(starts, dtype=np.uint32)
    with mesh_engine(g) as eng:
        eng.spread_track([0])
        for _ in range(runs):
            eng.publish(np.zeros(c), starts if starts.any() else None)
            st = eng.run()
            assert st.expand_mode == PE.MODE_COMPACT and st.windows == 1
        got = eng.spread_take()
        same(got, TR.windows_spread(n, [[topic]] * runs), what)
        healthy(got, runs, what)
        assert got["deliv"].sum() == runs * c * F.deliveries
        assert got["dup"].astype(np.int64).sum() == runs * c * F.duplicates
        again = eng.spread_take()
        same(again, TR.zeros(n, 1), what + ": a second take")
        assert again["n_windows"] == 0 and again["n_truncated"] == 0
    return got


@pytest.fixture(scope="module")
def specials():
    g = MR.mesh_with_specials(300)
    MR.check_specials(*g, MR.flood(*g[:4]))
    return g


@pytest.fixture(scope="module")
def hubs():
    return {deg: MR.hub_mesh(deg) for deg in (64, 65, 129, 600)}


# ---- 1. the specials at four row widths ---------------------------------------------

@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("c", [1, 64, 65, 64 * 64 + 40])
def test_specials(specials, c, rows, monkeypatch):
    """Rows of 1, 1, 2 and 66 words, plain and counted word by word: three
    runs, one take -- three times the blocking answer's reference."""
    seam(monkeypatch, rows)
    tracked_runs(specials, np.zeros(c), 3, f"c {c}")


# ---- 2. the take against the sum of the blocking calls --------------------------------

def test_take_against_the_blocking_calls(specials, hubs):
    """ps_topic_spread after every run, over other topics and in another
    order than the tracker's: its buffers are not the tracker's, and one take
    at the end equals the sum of its answers."""
    n = 400
    live = np.ones(n, dtype=np.uint8)
    live[:300] &= specials[3]
    live[0] = 1
    t0 = mesh_topic(specials, 1, n, live)[0]
    t1 = mesh_topic(hubs[65], 1, n, live)[0]
    with PE.Engine(n, 2) as eng:
        eng.set_children(0, specials[2], t0[0], t0[1])
        eng.set_children(1, hubs[65][2], t1[0], t1[1])
        eng.set_live(live)
        eng.spread_track([1, 0])
        total = TR.zeros(n, 2)
        for k0, k1 in ((70, 3), (5, 130), (64, 0), (0, 9)):
            eng.publish(np.concatenate([np.zeros(k0), np.ones(k1)]).astype(np.uint32))
            assert eng.run().windows == 1
            eng.topic_spread([0])  # (other entries, other strips, other sums)
            TR.add(total, eng.topic_spread([1, 0]))
        got = eng.spread_take()
        same(got, total, "sum of the blocking answers")
        healthy(got, 4)
        assert got["deliv"][0].any() and got["deliv"][1].any() and got["dup"].any()


# ---- 3. a run of several windows -----------------------------------------------------

def test_a_run_of_three_windows(specials):
    """msg_window = 320: 647 messages run as windows of 320, 320 and 7 -- five
    words wide, five, one."""
    n = len(specials[3])
    with mesh_engine(specials, msg_window=320) as eng:
        eng.spread_track([0])
        eng.publish(np.zeros(2 * 320 + 7))
        st = eng.run()
        assert st.windows == 3
        got = eng.spread_take()
        same(got, TR.windows_spread(n, [[mesh_topic(specials, c)[0]] for c in (320, 320, 7)]), "three windows")
        healthy(got, st.windows)
        assert got["deliv"].sum() == st.deliveries and got["dup"].astype(np.int64).sum() == st.duplicates
        # the blocking call answers for the last of them alone
        same(eng.topic_spread([0]), SR.window_spread(n, [mesh_topic(specials, 7)[0]]), "the last window")


# ---- 4. hubs --------------------------------------------------------------------------

@pytest.mark.parametrize("wide", [None, 0, 1 << 20])
@pytest.mark.parametrize("deg", [64, 65, 600])
def test_hub(hubs, deg, wide, monkeypatch):
    if wide is not None:
        monkeypatch.setenv("PSAMD_AB", "1")
        monkeypatch.setenv("PSAMD_SPREAD_WIDE", str(wide))
    g = hubs[deg]
    got = tracked_runs(g, np.zeros(70), 2, f"hub {deg}")
    live, facts = g[3], g[4]
    want = np.zeros(len(live), dtype=np.uint64)
    want[[ch for ch in facts["listed"] if live[ch]]] = 2 * 70
    assert np.array_equal(got["dup"], want)


# ---- 5. hops far past the node space's BFS depth -----------------------------------------

@pytest.mark.parametrize("n_chain", [8, 40, 300])
def test_detour(n_chain):
    """The node space is two levels deep, the forwarders' path n_chain - 1
    hops: the window ran that many rounds, and its last round + 1 launches
    reach the chain's end; from 255 hops on the clamped column."""
    got = tracked_runs(MR.detour(n_chain), np.zeros(70), 1, f"detour {n_chain}")
    assert got["unreached"][0] == 1 and not got["dup"].any()
    if n_chain == 300:
        assert (got["reached"][0, 1:255] == 1).all() and got["reached"][0, 255] == 45
    else:
        assert (got["reached"][0, 1:n_chain] == 1).all() and not got["reached"][0, n_chain:].any()


# ---- 6. start rounds ----------------------------------------------------------------------

@pytest.mark.parametrize("which", ["specials", "hub129"])
def test_start_rounds(specials, hubs, which):
    g = specials if which == "specials" else hubs[129]
    n_msgs = 200
    starts = np.random.default_rng(n_msgs).integers(0, 8, size=n_msgs)
    starts[:2] = (7, 0)
    multi = tracked_runs(g, starts, 1, which)
    single = tracked_runs(g, np.zeros(n_msgs), 1, which)
    for name in NAMES:
        assert np.array_equal(multi[name], single[name]), name


# ---- 7. two meshes that share peers, an idle topic and a tree in one request ----------------

@pytest.mark.parametrize("order", [[0, 1, 2, 3], [3, 2, 1, 0]])
def test_a_mixed_request(specials, hubs, order):
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
        eng.spread_track(order)
        eng.publish(np.concatenate([np.full(k, t) for t, k in counts.items()]).astype(np.uint32))
        st = eng.run()
        assert st.windows == 1
        got = eng.spread_take()
        same(got, TR.windows_spread(n, [[topics[t] for t in order]]), str(order))
        healthy(got, 1)
        assert got["deliv"].sum() == st.deliveries
        assert got["dup"].astype(np.int64).sum() == st.duplicates == counts[0] * F0.duplicates + counts[1] * F1.duplicates
        assert not got["reached"][order.index(2)].any() and got["unreached"][order.index(2)] == 0  # the idle topic


# ---- 8. the live mask changed between runs --------------------------------------------------

def test_live_mask_changed_between_runs(specials):
    """The second run's mask takes a third of the first run's forwarders out:
    what the first window left in the rows and in the pass's words must not
    count."""
    rp, cl, root, live, _ = specials
    n = len(live)
    F = MR.flood(rp, cl, root, live)
    rng = np.random.default_rng(8)
    live2 = live.copy()
    reached = np.flatnonzero(F.level > 0)
    live2[rng.choice(reached, size=reached.size // 3, replace=False)] = 0
    wins = [[mesh_topic(specials, 70, n, live)[0]], [mesh_topic(specials, 66, n, live2)[0]], [mesh_topic(specials, 3, n, live)[0]]]
    assert wins[1][0][3].sum() < wins[0][0][3].sum()
    with mesh_engine(specials) as eng:
        eng.spread_track([0])
        for w, (mask, c) in enumerate(((live, 70), (live2, 66), (live, 3))):
            eng.set_live(mask)
            eng.publish(np.zeros(c))
            eng.run()
            same(eng.topic_spread([0]), SR.window_spread(n, wins[w]), f"window {w}")
        got = eng.spread_take()
        same(got, TR.windows_spread(n, wins), "three masks")
        healthy(got, 3)


# ---- 9. a tree rebuilt between runs ------------------------------------------------------------

@pytest.mark.parametrize("gpu_build", [True, False])
def test_a_tree_rebuilt_between_runs(gpu_build):
    """Joins and leaves between the runs of a tracked join tree, the node
    space rebuilt on the GPU (its host mirror is not read back for the pass) or
    on the host; a second tracked topic in front keeps its own row.  The take
    equals the sum of the blocking answers; on a tree every delivery is a hop
    and nothing is a duplicate."""
    rng = np.random.default_rng(17)
    n, seed = 3000, 4
    eng = make_engine(n, gpu_build, n_topics=2, seed=seed)
    par1 = random_tree(rng, n, 5)
    with eng:
        eng.topic_create(0, 0, 2, 5)
        eng.join(0, np.arange(1, n, 2))
        eng.set_tree(1, 5, par1)
        members = set(range(1, n, 2))
        eng.spread_track([1, 0])
        total = TR.zeros(n, 2)
        deliveries, built, windows = 0, 0, 0
        for step in range(4):
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
            k = int(rng.integers(2, 6))
            eng.publish(np.concatenate([np.zeros(k), np.ones(step)]).astype(np.uint32))
            run = eng.run()
            assert run.windows == 1
            windows += run.windows
            deliveries += run.deliveries
            TR.add(total, eng.topic_spread([1, 0]))  # (in front of the build report: reading it may build anew)
            built = assert_builds(eng, gpu_build, built)
        got = eng.spread_take()
        same(got, total, f"churn gpu_build {gpu_build}")
        healthy(got, windows)
        assert got["deliv"].sum() == deliveries > 0 and not got["dup"].any()
        assert got["deliv"][0].any() and got["deliv"][1].any()


# ---- 10. pipelined -----------------------------------------------------------------------------

def test_pipelined_trees():
    """Six run_async over tree topics whose last windows are deferred: the
    window's last round is the slot's by then.  The same batches run one after
    the other give the same totals, and every window saw one node space and
    one mask: 12 times the blocking answer."""
    wl = WL.cfg3(60_000, 16, 4000)
    batches, plan = even_batches(len(wl.topics), 6, 51), {"flood": 0}
    live = (np.random.default_rng(11).random(wl.n_peers) >= 0.03).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    order = np.arange(len(wl.topics), dtype=np.uint32)[::-1].copy()

    def make():
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=64, plan=plan)
        WL.build_engine_topics(e, wl)
        e.set_live(live)
        e.spread_track(order)
        return e

    with make() as e:
        for b in batches:
            e.publish(b)
            e.run()
        t0 = e.spread_take()
        last = e.topic_spread(order)
    with make() as e:
        for i, b in enumerate(batches):
            e.publish(b)
            e.run_async()
            if i:
                e.wait()
        rc, a, counts = raw_take(e, len(order))  # a run in flight: refused, nothing changes
        assert rc == E_STATE and all((x == FILL).all() for x in a) and counts == [0xC0C0, 0xC1C1]
        e.wait()
        t1 = e.spread_take()
    same(t1, t0, "pipelined against one after the other")
    healthy(t1, 12)
    same(t1, times(last, 12), "12 windows of one shape")
    assert t1["deliv"].sum() > 0 and not t1["dup"].any() and t1["unreached"].any()


def test_pipelined_mesh(specials):
    n = len(specials[3])
    topic = mesh_topic(specials, 70)[0]
    with mesh_engine(specials) as eng:
        eng.spread_track([0])
        for i in range(4):
            eng.publish(np.zeros(70))
            eng.run_async()
            if i:
                eng.wait()
        eng.wait()
        got = eng.spread_take()
        same(got, TR.windows_spread(n, [[topic]] * 4), "four pipelined mesh runs")
        healthy(got, 4)


# ---- 11. all seven trackers at once ---------------------------------------------------------------

def flat(x):
    if isinstance(x, dict):
        return [v for k in sorted(x) for v in flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [v for y in x for v in flat(y)]
    return [np.asarray(x)]


def test_all_seven_trackers_at_once(specials):
    """Load, hops, downstream, cut, report, blame and spread set together, two
    trees and a mesh, two runs of two windows: every other tracker's take is
    what it is with spread untracked, and spread's is what it is alone."""
    n = 400
    rng = np.random.default_rng(91)
    par = random_tree(rng, n, 3)
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[:300] &= specials[3]
    live[[0, 3]] = 1
    t2 = mesh_topic(specials, 1, n, live)[0]
    msgs = [rng.integers(0, 3, size=300).astype(np.uint32), np.full(70, 2, dtype=np.uint32)]

    def go(others, spread):
        with PE.Engine(n, 3, msg_window=64) as e:
            e.set_tree(0, 3, par)
            e.set_tree(1, 3, par)
            e.set_children(2, specials[2], t2[0], t2[1])
            e.set_live(live)
            if others:
                e.load_track([0, 1, 2])
                e.hops_track([0, 1])
                e.downstream_track([0, 1])
                e.cut_track([0, 1])
                e.report_track([0, 1])
                e.blame_track([0, 1])
            if spread:
                e.spread_track([2, 0, 1])
            windows = 0
            for m in msgs:
                e.publish(m)
                windows += e.run().windows
            takes = [e.load_take(), e.hops_take(), e.downstream_take(), e.cut_take(), e.report_take(), e.blame_take()] if others else None
            return takes, e.spread_take() if spread else None, windows

    both, sp_both, windows = go(True, True)
    without, _, _ = go(True, False)
    _, sp_alone, _ = go(False, True)
    assert windows >= 4
    for k, (a, b) in enumerate(zip(both, without)):
        fa, fb = flat(a), flat(b)
        assert len(fa) == len(fb) and all(np.array_equal(x, y) for x, y in zip(fa, fb)), k
    same(sp_both, sp_alone, "beside the others")
    healthy(sp_both, windows)
    assert (sp_both["deliv"].sum(axis=1) > 0).all() and sp_both["dup"].any()


# ---- 12. the truncation seam ------------------------------------------------------------------------

def test_truncation_is_detected_and_counted(monkeypatch):
    """detour(40) under PSAMD_SPREAD_TRACK_LEVELS=10: launches 0 .. 9 run, and
    launch L gives hop L + 1, so the last exact column of reached and deliv is
    10 -- the forwarders at hop 10 are visited and counted, but have not sent.
    Every window is counted as truncated, the forwarders beyond hop 10 are
    stranded, and the blocking call on the same engine -- the seam is the
    tracker's alone -- answers whole; so does an engine without the seam."""
    g = MR.detour(40)
    n = len(g[3])
    topic = mesh_topic(g, 70)[0]
    part = TR.truncated(topic, 10)
    assert part["truncated"] and part["stranded"][0] == 29 and part["reached"][0, 10] == 1 and not part["reached"][0, 11:].any()
    whole = SR.window_spread(n, [topic])
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_SPREAD_TRACK_LEVELS", "10")
    with mesh_engine(g) as eng:
        eng.spread_track([0])
        for _ in range(3):
            eng.publish(np.zeros(70))
            eng.run()
            same(eng.topic_spread([0]), whole, "the blocking call")
        got = eng.spread_take()
        same(got, times(part, 3), "cut short after 10 launches")
        assert got["n_windows"] == 3 and got["n_truncated"] == 3
        assert got["stranded"][0] == 3 * 29
        again = eng.spread_take()
        assert again["n_truncated"] == 0 and again["n_windows"] == 0
    monkeypatch.delenv("PSAMD_SPREAD_TRACK_LEVELS")
    with mesh_engine(g) as eng:
        eng.spread_track([0])
        eng.publish(np.zeros(70))
        eng.run()
        got = eng.spread_take()
        same(got, whole, "the seam off")
        healthy(got, 1)


# ---- 13. return codes ----------------------------------------------------------------------------------

def test_two_loopback_ranks_refused():
    rng = np.random.default_rng(111)
    n, root = 400, 4
    parent = random_tree(rng, n, root)
    lb = PE.Loopback(2)
    engines = [PE.Engine(n, 1) for _ in range(3)]
    try:
        # an engine that is tracking takes no ranks
        engines[2].spread_track([0])
        with pytest.raises(PE.EngineError) as ei:
            engines[2].dist_init_loopback(lb, 0, PE.PART_PEER)
        assert ei.value.code == E_STATE
        for r, e in enumerate(engines[:2]):
            e.dist_init_loopback(lb, r, PE.PART_PEER)
            e.set_tree(0, root, parent)
            assert raw_track(e, [0]) == E_STATE  # one rank only
            assert raw_take(e, 1)[0] == E_NOTREADY
    finally:
        for e in engines:
            e.close()


def test_rules(specials):
    rp, cl, root, live, _ = specials
    n = len(live)
    rng = np.random.default_rng(82)
    parent = random_tree(rng, n, 1)
    t10 = mesh_topic(specials, 10)[0]
    idle = tree_topic(n, parent, 1, live, 0)
    with PE.Engine(n, 3) as eng:
        eng.set_children(0, root, rp, cl)
        eng.set_tree(1, 1, parent)
        eng.set_live(live)
        rc, a, counts = raw_take(eng, 1)
        assert rc == E_NOTREADY and all((x == FILL).all() for x in a) and counts == [0xC0C0, 0xC1C1]
        # tracking: a refused call leaves the previous tracking
        eng.spread_track([0, 1])
        assert raw_track(eng, [1, 1]) == E_INVAL and raw_track(eng, [0, 3]) == E_RANGE
        assert eng._L.ps_spread_track(eng._h, None, 2) == E_INVAL
        eng.publish(np.zeros(10))
        eng.run()
        want = TR.windows_spread(n, [[t10, idle]])
        # the take's count pointers: nothing is written, nothing is taken
        assert raw_take(eng, 2, counts=(False, True))[0] == E_INVAL and raw_take(eng, 2, counts=(True, False))[0] == E_INVAL
        rc, a, counts = raw_take(eng, 2)
        assert rc == 0 and counts == [1, 0]
        for x, name in zip(a, NAMES):
            assert np.array_equal(x, want[name]), name
        # each output alone: written in full, the others untouched; and all six NULL
        for k, name in enumerate(NAMES):
            eng.publish(np.zeros(10))
            eng.run()
            rc, a, counts = raw_take(eng, 2, which=tuple(j == k for j in range(6)))
            assert rc == 0 and counts == [1, 0] and np.array_equal(a[k], want[name]), name
            assert all((a[j] == FILL).all() for j in range(6) if j != k), name
        eng.publish(np.zeros(10))
        eng.run()
        rc, a, counts = raw_take(eng, 2, which=(False,) * 6)
        assert rc == 0 and counts == [1, 0] and all((x == FILL).all() for x in a)
        same(eng.spread_take(), TR.zeros(n, 2), "taken with no array")
        # a run in flight
        eng.publish(np.zeros(10))
        eng.run_async()
        assert raw_track(eng, [1]) == E_STATE
        rc, a, counts = raw_take(eng, 2)
        assert rc == E_STATE and all((x == FILL).all() for x in a) and counts == [0xC0C0, 0xC1C1]
        eng.wait()
        got = eng.spread_take()
        same(got, want, "asynchronous")
        healthy(got, 1)
        # tracked again: the totals start at zero, the rows follow the new request
        eng.publish(np.zeros(10))
        eng.run()
        eng.spread_track([1, 0])
        got = eng.spread_take()
        same(got, TR.zeros(n, 2), "tracked again")
        assert got["n_windows"] == 0
        eng.publish(np.zeros(10))
        eng.run()
        same(eng.spread_take(), TR.windows_spread(n, [[idle, t10]]), "the new request")
        # clearing: nothing is tracked, the run is as ever
        eng.spread_track([])
        assert raw_take(eng, 0)[0] == E_NOTREADY
        eng.publish(np.zeros(10))
        eng.run()
        same(eng.topic_spread([0, 1]), SR.window_spread(n, [t10, idle]), "untracked")
