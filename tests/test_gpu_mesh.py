"""GPU: mesh dissemination and the direct expand path (k_expand<*, true>,
expand_direct in csrc/kernels.hip) at their edges, bit for bit against
tests/mesh_ref.py -- a plain Python flood that tests/test_mesh_ref_cpu.py
holds against oracle/psoracle.c.

A window that holds a mesh topic never runs level mode: every topic in it
goes through the compaction path, mesh entries through the direct instance
(returning 64-bit atomicOr on `seen`, OR-accumulated arrival rows consumed
and cleared, no generation bytes).  Unless a case says otherwise each one runs
the recording instance (hops per message) and the production instance
(delivered bits, per-peer lists, digest), and in both compares
ps_stats.deliveries, .duplicates and .deliveries_per_round[1:] with the
reference and expects MODE_COMPACT.
"""
import time

import numpy as np
import pytest

import mesh_ref as MR
import oracle as O
import psengine as PE
from test_gpu_parity import random_tree

pytestmark = pytest.mark.gpu

NO_PAD = {"pad_words": 1 << 20}  # rows keep their odd word counts (plan.cpp pads rows of >= pad_words words to even)

# message count -> row words of a mesh topic, as plan_window_layout lays it
# out: ceil(count / 64), padded to even from 16 words on unless NO_PAD
# (tests/test_mesh_ref_cpu.py::test_row_counts_give_these_widths asks the planner)
ROW_CASES = [(1, None, 1), (64, None, 1), (65, None, 2), (129, None, 3), (320, None, 5),
             (63 * 64, NO_PAD, 63), (63 * 64, None, 64), (63 * 64 + 1, None, 64), (64 * 64, None, 64),
             (64 * 64 + 1, NO_PAD, 65), (64 * 64 + 1, None, 66), (130 * 64 - 20, None, 130)]


def sample(n_msgs):
    """Every message up to 300, else every 97th plus the first and the last."""
    return list(range(n_msgs)) if n_msgs <= 300 else sorted(set(range(0, n_msgs, 97)) | {0, n_msgs - 1})


def pick_peers(ref, live):
    """A reached peer (the farthest), a live peer out of reach and a dead
    peer, where the graph has them; the root."""
    lv = ref.level
    out = [int(np.argmax(lv)), ref.root]
    cut = [p for p in range(ref.n) if lv[p] < 0 and live[p] and p != ref.root]
    dead = [p for p in range(ref.n) if not live[p] and p != ref.root]
    return out + cut[:1] + dead[:1] + dead[-1:]


def check_stats(st, ref, starts, n_windows=1):
    starts = np.asarray(starts)
    k = len(starts)
    assert st.expand_mode == PE.MODE_COMPACT
    assert st.windows == n_windows
    assert st.deliveries == k * ref.deliveries
    assert st.duplicates == k * ref.duplicates
    assert list(st.deliveries_per_round)[1:] == list(ref.per_round(starts))[1:]


def check_rows(eng, first, ref, starts, live, record, topic=0, msgs=None):
    """The last window's readbacks of messages first .. first + len(starts)."""
    k = len(starts)
    for m in (sample(k) if msgs is None else msgs):
        if record:
            got = eng.hops(first + m)
            if not np.array_equal(got, ref.hops):
                bad = np.nonzero(got != ref.hops)[0][:10]
                raise AssertionError(f"msg {m}: peers {bad} engine {got[bad]} reference {ref.hops[bad]}")
        got = eng.delivered(first + m)
        if not np.array_equal(got, ref.delivered):
            bad = np.nonzero(got != ref.delivered)[0][:10]
            raise AssertionError(f"msg {m}: peers {bad} delivered {got[bad]} reference {ref.delivered[bad]}")
    if msgs is None:
        order = [first + m for m in MR.arrival_order(starts)]
        for p in pick_peers(ref, live):
            assert eng.peer_messages(topic, p).tolist() == (order if ref.level[p] >= 0 else []), p


def run_both(graph, starts, plan=None):
    """One run of len(starts) messages on a fresh engine per instance."""
    rp, cl, root, live = graph[:4]
    ref = MR.flood(rp, cl, root, live)
    starts = np.asarray(starts, dtype=np.uint32)
    digests = []
    for record in (True, False):
        with PE.Engine(ref.n, 1, record_hops=record, plan=plan) as eng:
            eng.set_children(0, root, rp, cl)
            eng.set_live(live)
            first = eng.publish(np.zeros(len(starts)), starts if starts.any() else None)
            st = eng.run()
            check_stats(st, ref, starts)
            check_rows(eng, first, ref, starts, live, record)
            digests.append(eng.seen_digest())
    assert digests[0] == digests[1]
    return ref


@pytest.fixture(scope="module")
def specials():
    g = MR.mesh_with_specials(300)
    MR.check_specials(*g, MR.flood(*g[:4]))
    return g


@pytest.fixture(scope="module")
def hubs():
    out = {}
    for deg in (63, 64, 65, 128, 129, 200):
        g = MR.hub_mesh(deg)
        MR.check_hub(*g, MR.flood(*g[:4]))
        out[deg] = g
    return out


# --- 1. row widths ------------------------------------------------------------

@pytest.mark.parametrize("n_msgs,plan,words", ROW_CASES)
def test_row_widths(specials, n_msgs, plan, words):
    """mesh_with_specials (self-loop, repeated edge, edge into the root, two
    parents in one round and a round apart, a dead peer with live children) at
    rows of 1, 1, 2, 3, 5, 63, 64, 64, 64, 65, 66 and 130 words: the packed
    branch of expand_direct at wp = 1, 2, 4, 8 and 64 (wp > W at 3, 5 and 63
    words: idle lanes in every child group), the word-block branch at exactly
    one block, one and two words past it and three blocks with a ragged tail.
    63 and 65 words need pad_words out of the way: by default rows of 16 words
    and more are padded to even, so 63 * 64 messages give 64 words and
    64 * 64 + 1 give 66 -- both run."""
    assert (n_msgs + 63) // 64 in (words, words - 1)
    run_both(specials, np.zeros(n_msgs), plan)


# --- 2. fan-out ---------------------------------------------------------------

@pytest.mark.parametrize("words", [1, 5, 65])
@pytest.mark.parametrize("deg", [63, 64, 65, 128, 129, 200])
def test_fan_out(hubs, deg, words):
    """A hub of `deg` children (one block of 64 short of full, full, one over,
    two full, two and one, three and a ragged last), every child hit twice --
    before, with or after the hub by its other parent -- dead children at list
    positions 0, 63, 64 and deg - 1.  The atomicOr decides which parent wins;
    the duplicate count (one per live hub child and message) does not move."""
    n_msgs = words * 64 - 7
    ref = run_both(hubs[deg], np.zeros(n_msgs), NO_PAD)
    assert ref.duplicates == deg - len(hubs[deg][4]["dead_pos"])


# --- 3. start rounds ----------------------------------------------------------

@pytest.mark.parametrize("n_msgs", [200, 64 * 64 + 40])
@pytest.mark.parametrize("which", ["specials", "hub129"])
def test_start_rounds(specials, hubs, which, n_msgs):
    """Start rounds uniform over 0..5: a message entering at round 5 reaches a
    level-1 peer in round 6, four rounds after that peer forwarded the round-0
    messages -- its row is consumed, cleared and filled again.  Per-round
    deliveries are the hop histogram shifted by every start; a peer's list is
    in (start, id) order (test_gpu_drain_batch.oracle_lists)."""
    g = specials if which == "specials" else hubs[129]
    starts = np.random.default_rng(n_msgs).integers(0, 6, size=n_msgs)
    starts[:2] = (5, 0)  # the first message published is the last to enter
    ref = run_both(g, starts)
    assert ref.rounds >= 3 and set(starts.tolist()) == set(range(6))


# --- 4. a tree beside a mesh --------------------------------------------------

def tree_hops(parent, root, live):
    rp, cl = O.parents_to_csr(parent)
    total, hops, _ = O.disseminate(rp, cl, root, live, 1)
    return total, hops[0]


def per_round_of(hops, starts):
    out = np.zeros(MR.MAX_ROUNDS, dtype=np.int64)
    h = np.bincount(hops[hops != 0xFF], minlength=MR.MAX_ROUNDS).astype(np.int64)
    for s, k in zip(*np.unique(starts, return_counts=True)):
        out[s:] += int(k) * h[:MR.MAX_ROUNDS - s]
    return out


def hub_tree(rng, n, root, hub, deg, live):
    """A random tree in which `hub` (a child of the root) has exactly `deg`
    children and nobody else more than a handful."""
    assert live[root] and live[hub]
    others = [int(p) for p in rng.permutation(n) if p not in (root, hub)]
    parent = np.full(n, O.NONE, dtype=np.uint32)
    parent[hub] = root
    kids, rest = others[:deg], others[deg:]
    parent[kids] = hub
    placed = [root] + kids
    for p in rest:
        parent[p] = placed[int(rng.integers(0, len(placed)))]
        placed.append(p)
    assert int((parent == hub).sum()) == deg
    return parent


@pytest.mark.parametrize("record", [False, True])
def test_tree_beside_mesh(specials, record):
    """Three topics in one window: the mesh; a tree of short rows (12 words in
    three start groups: the flat path of the production instance, which no
    recording test reaches) over the same 12 % dead peers; a tree whose hub has
    90 children and 96-word rows in three start groups (direct path, arrival
    extents).  The trees ride through compaction because the mesh shares their
    window: their deliveries and rows equal oracle.disseminate, the mesh's
    equal mesh_ref, the duplicates are the mesh's alone.  Then a second,
    smaller window on the same engine."""
    rp, cl, root, live, _ = specials
    n = len(live)
    ref = MR.flood(rp, cl, root, live)
    rng = np.random.default_rng(44)
    alive = [int(p) for p in np.nonzero(live)[0]]
    par1 = random_tree(rng, n, alive[5])
    par2 = hub_tree(rng, n, alive[9], alive[20], 90, live)
    trees = {1: (par1, alive[5]), 2: (par2, alive[9])}
    exp = {t: tree_hops(par, r, live) for t, (par, r) in trees.items()}
    with PE.Engine(n, 3, record_hops=record) as eng:
        eng.set_children(0, root, rp, cl)
        for t, (par, r) in trees.items():
            eng.set_tree(t, r, par)
        eng.set_live(live)
        assert eng.graph_topic(2)["max_deg"] == 90
        for counts in ({0: 200, 1: 500, 2: 3 * 2048}, {0: 70, 1: 3, 2: 3 * 128 + 5}):
            topics = np.concatenate([np.full(k, t) for t, k in counts.items()])
            topics = topics[rng.permutation(len(topics))]
            starts = rng.integers(0, 3, size=len(topics))
            starts[topics == 0] = rng.integers(0, 2, size=counts[0])
            starts[topics == 2] = np.arange(counts[2]) % 3  # start groups of equal size: 3 x 32 words in the first window
            first = eng.publish(topics, starts)
            st = eng.run()
            assert st.expand_mode == PE.MODE_COMPACT and st.windows == 1
            total = counts[0] * ref.deliveries + sum(counts[t] * exp[t][0] for t in trees)
            per = ref.per_round(starts[topics == 0])
            for t in trees:
                per = per + per_round_of(exp[t][1], starts[topics == t])
            assert st.deliveries == total
            assert st.duplicates == counts[0] * ref.duplicates
            assert list(st.deliveries_per_round)[1:] == list(per)[1:]
            for t in range(3):
                idx = np.nonzero(topics == t)[0]
                hops = ref.hops if t == 0 else exp[t][1]
                for m in idx[sample(len(idx))]:
                    if record:
                        assert np.array_equal(eng.hops(first + int(m)), hops), (t, m)
                    assert np.array_equal(eng.delivered(first + int(m)), (hops != 0xFF).astype(np.uint8)), (t, m)
                order = [first + int(m) for m in sorted(idx, key=lambda m: (int(starts[m]), m))]
                tr = alive[5] if t == 1 else alive[9] if t == 2 else root
                reached = int(np.argmax(np.where(hops == 0xFF, 0, hops)))
                dead = int(np.nonzero(live == 0)[0][3])
                assert eng.peer_messages(t, reached).tolist() == order
                assert eng.peer_messages(t, dead).tolist() == []
                assert eng.peer_messages(t, tr).tolist() == []


# --- 5. paths longer than the BFS depth ---------------------------------------

def run_detour(n_chain, record, n_msgs=70):
    g = MR.detour(n_chain)
    rp, cl, root, live, facts = g
    ref = MR.flood(rp, cl, root, live)
    MR.check_detour(*g, ref)
    eng = PE.Engine(ref.n, 1, record_hops=record)
    eng.set_children(0, root, rp, cl)
    eng.set_live(live)
    assert eng.depth(0)[0] == facts["bfs_depth"]
    return eng, g, ref


def check_detour_run(eng, first, st, ref, live, record, n_msgs, planned):
    n_chain = ref.n - 1
    check_stats(st, ref, np.zeros(n_msgs))
    assert st.duplicates == 0 and st.deliveries == n_msgs * (n_chain - 1)
    # the live path outlives the planned rounds; extensions come 8 rounds at a time
    assert n_chain - 1 > planned and n_chain - 1 <= st.rounds < n_chain - 1 + 8
    check_rows(eng, first, ref, np.zeros(n_msgs), live, record, msgs=[0, n_msgs - 1])
    if record:
        assert eng.hops(first)[n_chain - 1] == min(n_chain - 1, 254)
    assert eng.peer_messages(0, n_chain - 1).tolist() == list(range(first, first + n_msgs))
    assert eng.peer_messages(0, n_chain).tolist() == []  # S, dead


@pytest.mark.parametrize("record", [True, False])
@pytest.mark.parametrize("n_chain", [8, 40, 300])
def test_path_outlives_planned_rounds(n_chain, record):
    """detour(n_chain): the node space is 2 deep (planned rounds: depth + 1 =
    3), the live path n_chain - 1 hops because the shortcut peer S is dead.
    compaction_rounds then adds 8 rounds at a time, on the full expand grid:
    8 ends inside the first extension, 40 takes five, 300 takes 37 and passes
    PS_MAX_ROUNDS -- hops saturate at 254, deliveries_per_round counts 70 in
    every round 1..255, the total counts all 299 hops."""
    eng, g, ref = run_detour(n_chain, record)
    with eng:
        first = eng.publish(np.zeros(70))
        st = eng.run()
        check_detour_run(eng, first, st, ref, g[3], record, 70, planned=3)
        if n_chain == 300:
            assert all(st.deliveries_per_round[q] == 70 for q in range(1, PE.MAX_ROUNDS))
            assert st.deliveries == 70 * 299
            if record:
                assert eng.hops(first + 69)[250:300].tolist() == list(range(250, 255)) + [254] * 45


@pytest.mark.parametrize("n_chain", [300, 600])
def test_long_path_leaves_the_deferred_path(n_chain):
    """run_async() / wait() of a window whose last round is past PS_MAX_ROUNDS:
    the pinned slot of a deferred window holds PS_MAX_ROUNDS + 1 counter rows,
    so defers() must send it down the blocking path; stats and rows equal the
    blocking run's.  (At 600 the counter rows would pass the end of the slot's
    allocation, apply rows included.)"""
    eng, g, ref = run_detour(n_chain, False)
    with eng:
        first = eng.publish(np.zeros(70))
        blocking = eng.run()
        digest = eng.seen_digest()
        check_detour_run(eng, first, blocking, ref, g[3], False, 70, planned=3)
        for _ in range(2):
            first = eng.publish(np.zeros(70))
            eng.run_async()
            st = eng.wait()
            check_detour_run(eng, first, st, ref, g[3], False, 70, planned=3)
            assert st.rounds == blocking.rounds
            assert list(st.deliveries_per_round) == list(blocking.deliveries_per_round)
            assert eng.seen_digest() == digest


@pytest.mark.parametrize("record", [True, False])
def test_path_past_the_round_buffers(record):
    """detour(4300): 4,299 rounds, past the kMaxRoundsCap (4,096) counter rows,
    so grow_stats_rows copies the counted rows into a larger buffer mid-window.
    Then S comes alive and the same engine gives the two-round answer: every
    chain peer from 2 on two hops away and hit once more by its chain parent."""
    n_chain = 4300
    t0 = time.perf_counter()
    eng, g, ref = run_detour(n_chain, record)
    rp, cl, root, live, facts = g
    with eng:
        first = eng.publish(np.zeros(70))
        st = eng.run()
        t1 = time.perf_counter()
        check_detour_run(eng, first, st, ref, live, record, 70, planned=3)
        assert st.deliveries == 70 * 4299 and st.duplicates == 0
        assert list(st.deliveries_per_round)[1:] == [70] * 255
        up = live.copy()
        up[facts["S"]] = 1
        ref2 = MR.flood(rp, cl, root, up)
        eng.set_live(up)
        first = eng.publish(np.zeros(70))
        st = eng.run()
        check_stats(st, ref2, np.zeros(70))
        assert st.rounds == 3 and st.duplicates == 70 * (n_chain - 2) and st.deliveries == 70 * n_chain
        check_rows(eng, first, ref2, np.zeros(70), up, record, msgs=[0, 69])
    print(f"detour(4300) record={record}: long run {t1 - t0:.2f} s, whole test {time.perf_counter() - t0:.2f} s")


# --- 6. windows and stale bits ------------------------------------------------

@pytest.mark.parametrize("record", [True, False])
def test_narrower_window_after_wider(specials, record):
    """Mesh rows are zeroed per window by window_init_block, 64 blocks
    striding the topic's rows: a window of 300-word rows, then one of 3
    messages, then one of 130-word rows on the same engine.  Every window's
    rows, lists and digest equal a fresh engine's for that window alone."""
    rp, cl, root, live, _ = specials
    ref = MR.flood(rp, cl, root, live)
    counts = (300 * 64, 3, 130 * 64 - 1)

    def one(eng, k):
        first = eng.publish(np.zeros(k))
        st = eng.run()
        check_stats(st, ref, np.zeros(k))
        check_rows(eng, first, ref, np.zeros(k), live, record)
        return eng.seen_digest()

    def engine():
        eng = PE.Engine(ref.n, 1, record_hops=record)
        eng.set_children(0, root, rp, cl)
        eng.set_live(live)
        return eng

    with engine() as eng:
        got = [one(eng, k) for k in counts]
    fresh = []
    for k in counts:
        with engine() as eng:
            fresh.append(one(eng, k))
    assert got == fresh and len(set(got)) == 3


@pytest.mark.parametrize("record", [True, False])
def test_300_windows_beside_a_tree(specials, record):
    """msg_window = 64 and 64 * 300 messages per topic: 300 one-word windows of
    the mesh beside a tree topic in one run, the 8-bit generation wraps.
    Totals are 300 times one window's; the last window's readbacks are exact."""
    rp, cl, root, live, _ = specials
    n = len(live)
    ref = MR.flood(rp, cl, root, live)
    rng = np.random.default_rng(61)
    troot = int(np.nonzero(live)[0][7])
    par = random_tree(rng, n, troot)
    ttotal, thops = tree_hops(par, troot, live)
    k = 64 * 300
    with PE.Engine(n, 2, record_hops=record, msg_window=64) as eng:
        eng.set_children(0, root, rp, cl)
        eng.set_tree(1, troot, par)
        eng.set_live(live)
        topics = np.tile([0, 1], k)
        first = eng.publish(topics)
        st = eng.run()
        assert st.windows == 300 and st.expand_mode == PE.MODE_COMPACT
        assert st.deliveries == k * (ref.deliveries + ttotal)
        assert st.duplicates == k * ref.duplicates
        per = ref.per_round(np.zeros(k)) + per_round_of(thops, np.zeros(k, dtype=np.int64))
        assert list(st.deliveries_per_round)[1:] == list(per)[1:]
        last = range(2 * k - 128, 2 * k)
        for m in last:
            hops = ref.hops if m % 2 == 0 else thops
            assert np.array_equal(eng.delivered(first + m), (hops != 0xFF).astype(np.uint8)), m
        if record:
            for m in sample(2 * k):
                assert np.array_equal(eng.hops(first + m), ref.hops if m % 2 == 0 else thops), m
        with pytest.raises(PE.EngineError, match="not in the last window"):
            eng.delivered(first)
        far = int(np.argmax(ref.level))
        assert eng.peer_messages(0, far).tolist() == [first + m for m in last if m % 2 == 0]
        assert eng.peer_messages(0, int(np.nonzero(live == 0)[0][0])).tolist() == []
        tfar = int(np.argmax(np.where(thops == 0xFF, 0, thops)))
        assert eng.peer_messages(1, tfar).tolist() == [first + m for m in last if m % 2 == 1]
        one = PE.Engine(n, 2, msg_window=64)
        with one:
            one.set_children(0, root, rp, cl)
            one.set_tree(1, troot, par)
            one.set_live(live)
            one.publish(np.tile([0, 1], 64))
            one.run()
            assert one.seen_digest() == eng.seen_digest()


# --- 7. live changes and pipelining -------------------------------------------

@pytest.mark.parametrize("record", [True, False])
def test_live_changes_between_runs(specials, hubs, record):
    """Between runs on one engine: a live hub child dies and a dead one (list
    position 63) comes alive, an "earlier" parent dies; on the scaffold, peer 5
    (two parents) dies and the dead peer 8 comes alive, which brings in the
    peer it alone feeds.  Every run equals the reference under its own mask."""
    for g, flips in ((hubs[129], None), (specials, [(5, 8), (5,), (9, 6)])):
        rp, cl, root, live, facts = g
        if flips is None:
            listed = facts["listed"]
            later = [c for c in facts["classes"]["later"] if live[c]]
            earlier_parent = MR.parents_of(rp, cl, facts["classes"]["earlier"][0])
            earlier_parent.remove(facts["hub"])
            flips = [(later[0], listed[63]), (earlier_parent[0],), (later[0], listed[0], listed[64])]
        live = live.copy()
        with PE.Engine(len(live), 1, record_hops=record) as eng:
            eng.set_children(0, root, rp, cl)
            seen = set()
            for flip in [()] + flips:
                for p in flip:
                    live[p] ^= 1
                eng.set_live(live)
                ref = MR.flood(rp, cl, root, live)
                seen.add(ref.delivered.tobytes())
                first = eng.publish(np.zeros(129))
                st = eng.run()
                check_stats(st, ref, np.zeros(129))
                check_rows(eng, first, ref, np.zeros(129), live, record)
            assert len(seen) == len(flips) + 1  # every flip changed the answer


def test_pipelined_batches_equal_blocking(specials):
    """Six batches through run_async with wait lagging by one, against the
    same six run blocking: stats batch by batch, the last window's rows, the
    digest.  (Meshes never overlap the previous window: nothing is asserted on
    overlapped_windows.)"""
    rp, cl, root, live, _ = specials
    ref = MR.flood(rp, cl, root, live)
    rng = np.random.default_rng(77)
    sizes = (70, 200, 1, 64 * 64 + 3, 65, 129)
    batches = [rng.integers(0, 4, size=k) if i % 2 else np.zeros(k, dtype=np.int64) for i, k in enumerate(sizes)]
    key = lambda st: (st.deliveries, st.duplicates, st.rounds, st.windows, list(st.deliveries_per_round))
    res = {}
    for mode in ("blocking", "pipelined"):
        with PE.Engine(ref.n, 1) as eng:
            eng.set_children(0, root, rp, cl)
            eng.set_live(live)
            out = []
            for i, b in enumerate(batches):
                first = eng.publish(np.zeros(len(b)), b if b.any() else None)
                if mode == "blocking":
                    st = eng.run()
                    check_stats(st, ref, b)
                    out.append(key(st))
                else:
                    eng.run_async()
                    if i:
                        out.append(key(eng.wait()))
            if mode == "pipelined":
                out.append(key(eng.wait()))
            check_rows(eng, first, ref, batches[-1], live, False)
            res[mode] = (out, eng.seen_digest())
    assert res["blocking"] == res["pipelined"]


def test_two_ranks_refuse_a_mesh(specials):
    """Meshes are single-GPU only: the node-space build of a rank refuses one."""
    rp, cl, root, live, _ = specials
    lb = PE.Loopback(2)
    engines = [PE.Engine(len(live), 1) for _ in range(2)]
    try:
        for r, e in enumerate(engines):
            e.dist_init_loopback(lb, r, PE.PART_PEER)
            e.set_children(0, root, rp, cl)
            with pytest.raises(PE.EngineError, match="multi-GPU engines support tree topics only") as ei:
                e.depth(0)
            assert ei.value.code == -3  # PS_E_STATE
    finally:
        for e in engines:
            e.close()
        lb.close()
