"""GPU: the sharded level path (pull_resolve's ghost branch, pull_ship, k_pack
in csrc/pull.hip; plan_ghost / annotate_chunks in csrc/plan.cpp;
partition_topic in csrc/graph.cpp) at its edges, rank by rank, on the
in-process loopback transport -- against tests/dist_ref.py, a plain reference
that tests/test_dist_ref_cpu.py holds against oracle/psoracle.c and
ps_partition_owner.

Every case is checked per rank, never as the union over ranks (check_ranks):
every message's hops equal the reference masked to the rank's owned peers, so
a rank that reports a peer it does not own, or an owned peer a hop late, fails
even where another rank reports it right; deliveries, deliveries_per_round and
frontier_per_round equal the rank's own share; the shares and the digests add
up to a one-rank engine's.  The conditions a case relies on (row words, 65
children behind one record, blocks of 15 / 16 / 17 words, ranks that own
nothing) are asserted on the CPU by the tests named in each docstring.

Not here, because another test holds it: a mesh topic on a two-rank engine is
PS_E_STATE (tests/test_gpu_mesh.py::test_two_ranks_refuse_a_mesh)."""
import ctypes as C

import numpy as np
import pytest

import dist_ref as DR
import psengine as PE
from test_gpu_dist import make_ranks, run_ranks

pytestmark = pytest.mark.gpu

PATHS = [False, True, "inplace"]
PATH_OF = {False: PE.XCHG_ZERO_COPY, True: PE.XCHG_COPY, "inplace": PE.XCHG_IN_PLACE}


def owners_of(trees, roots, world, partition=PE.PART_PEER, split_depth=0):
    n = trees[0].shape[0]
    out = []
    for par, root in zip(trees, roots):
        if partition == PE.PART_PEER:
            out.append(np.where(DR.bfs_levels(par, root) >= 0, DR.owner_peer(np.arange(n), world), -1))
        else:
            out.append(DR.owner_subtree(par, root, world, split_depth))
    return out


def one_rank(n, trees, roots, live, topics, starts, plan=None, **kw):
    """(stats, digest) of the same run on a one-rank engine."""
    with PE.Engine(n, len(trees), plan=plan, **kw) as one:
        for t, (par, root) in enumerate(zip(trees, roots)):
            one.set_tree(t, root, par)
        one.set_live(live)
        one.publish(topics, starts)
        st = one.run()
        return st, one.seen_digest()


def check_ranks(engines, stats, firsts, trees, roots, live, topics, starts, owners, copy, one, *,
                windows=None, exchanges=True):
    """The per-rank check.  one: (stats, digest) of a one-rank engine on the
    same run.  windows: the run's windows as lists of message indices (default
    one window of everything): ps_read_delivered answers for the last window
    only, and the frontier counts a (topic, start round) pair once a window."""
    world = len(engines)
    k = len(topics)
    hops, mine, share = DR.expect(trees, roots, live, topics, starts, owners, world)
    windows = [list(range(k))] if windows is None else windows
    front = np.zeros((world, DR.MAX_ROUNDS), dtype=np.int64)
    tp = np.asarray(topics)
    sr = np.zeros(k, dtype=np.int64) if starts is None else np.asarray(starts)
    for w in windows:
        front += DR.expect_frontier(trees, roots, live, tp[w], sr[w], owners, world)
    assert len(set(firsts)) == 1
    first = firsts[0]
    for r, (eng, st) in enumerate(zip(engines, stats)):
        assert st.expand_mode == PE.MODE_LEVEL_PULL and st.windows == len(windows), (r, st.expand_mode, st.windows)
        got = np.stack([eng.hops(first + m) for m in range(k)])
        if not np.array_equal(got, mine[r]):
            m, p = (int(x[0]) for x in np.nonzero(got != mine[r]))
            raise AssertionError(f"rank {r} msg {m} peer {p} (owner {owners[int(tp[m])][p]}): hop {got[m, p]}, "
                                 f"reference {mine[r][m, p]}; {(got != mine[r]).sum()} differ")
        # the last window's first and last message and the first of every topic in it (a rank that owns
        # nothing of a topic answers with zeros)
        last = windows[-1]
        for m in sorted({last[0], last[-1]} | {next(i for i in last if tp[i] == t) for t in set(tp[last].tolist())}):
            d = eng.delivered(first + m)
            assert np.array_equal(d, (mine[r][m] != DR.HOP_NONE).astype(np.uint8)), (r, m)
            assert not d[owners[int(tp[m])] != r].any()
        assert st.deliveries == share["total"][r], (r, st.deliveries, share["total"][r])
        assert list(st.deliveries_per_round) == share["per_round"][r].tolist(), r
        assert st.duplicates == 0
        # include/psengine.h: a rank counts every reached parent it reads for a child it owns
        assert list(st.frontier_per_round) == front[r].tolist(), (r, list(st.frontier_per_round)[:12],
                                                                  front[r].tolist()[:12])
        assert st.xchg_path == (PATH_OF[copy] if st.xchg_rounds else PE.XCHG_NONE), (r, st.xchg_path, st.xchg_rounds)
    if exchanges:
        assert all(st.xchg_rounds > 0 for st in stats), [st.xchg_rounds for st in stats]
    st1, d1 = one
    assert sum(st.deliveries for st in stats) == st1.deliveries == int(share["total"].sum())
    assert np.array_equal(np.sum([list(st.deliveries_per_round) for st in stats], axis=0),
                          np.array(list(st1.deliveries_per_round)))
    assert sum(e.seen_digest() for e in engines) % (1 << 64) == d1
    # the frontier counters cannot add up: a rank counts every reached parent it reads, so a parent with
    # children on k ranks counts k times (include/psengine.h).  One rank counts each once -- the same
    # reference at world 1 -- and the ranks' sum is that plus k - 1 per parent.
    whole = [np.where(o >= 0, 0, -1) for o in owners]
    front1 = sum(DR.expect_frontier(trees, roots, live, tp[w], sr[w], whole, 1) for w in windows)[0]
    assert list(st1.frontier_per_round) == front1.tolist()
    assert (front.sum(axis=0) >= front1).all()
    assert sum(st.frontier_entries for st in stats) >= st1.frontier_entries


def run_case(world, trees, roots, live, topics, starts, copy, *, overlap=None, partition=PE.PART_PEER,
             split_depth=0, plan=None, exchanges=True, msg_window=None, windows=None):
    """One sharded run on fresh engines, checked per rank; returns the stats."""
    n = trees[0].shape[0]
    plan = dict(plan or {})
    if overlap is not None:
        plan["xchg_overlap"] = overlap
    kw = {} if msg_window is None else {"msg_window": msg_window}
    topics = np.asarray(topics, dtype=np.uint32)
    lb, engines = make_ranks(world, n, len(trees), partition, split_depth, copy=copy, plan=plan or None, **kw)
    try:
        for e in engines:
            for t, (par, root) in enumerate(zip(trees, roots)):
                e.set_tree(t, root, par)
            e.set_live(live)
        firsts = [e.publish(topics, starts) for e in engines]
        stats = run_ranks(engines)
        owners = owners_of(trees, roots, world, partition, split_depth)
        one_plan = {k: v for k, v in plan.items() if k != "xchg_overlap"} or None
        one = one_rank(n, trees, roots, live, topics, starts, one_plan, **kw)
        check_ranks(engines, stats, firsts, trees, roots, live, topics, starts, owners, copy, one,
                    windows=windows, exchanges=exchanges)
        return stats
    finally:
        for e in engines:
            e.close()
        lb.close()


# --- 1. row widths --------------------------------------------------------------

@pytest.fixture(scope="module")
def width_tree():
    return DR.row_width_case()


@pytest.mark.parametrize("copy", PATHS)
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("n_msgs,plan,words", DR.ROW_CASES)
def test_row_widths(width_tree, n_msgs, plan, words, overlap, copy):
    """One topic of 600 peers, fan-out <= 4, 8 % dead, world 3 under the peer
    hash, rows of 1, 2, 3, 4, 5, 16, 17, 63, 64, 65 and 66 words: pull_ship's
    word branch (odd) and pair branch (even: w = 2 * r, only the head word of
    an unreached parent's record zeroed), k_pack's two branches, every message
    compared.  17, 63 and 65 words need pad_words out of the way; by default
    the same counts travel as 18, 64 and 66.  (Widths:
    test_dist_ref_cpu.py::test_row_counts_give_these_widths; dead parents with
    remote children: ::test_row_width_tree_has_the_dead_parents.)"""
    parent, root, live = width_tree
    run_case(3, [parent], [root], live, np.zeros(n_msgs), None, copy, overlap=overlap, plan=plan)


@pytest.mark.parametrize("copy", PATHS)
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("n_msgs,words", DR.GROUP_CASES)
def test_row_widths_staggered(width_tree, n_msgs, words, overlap, copy):
    """Starts 0..3 in turn: four start groups, each block 2 or 6 words (a
    block is padded to even: 5 words of messages travel as 6), each group's
    records exchanged in its own rounds."""
    parent, root, live = width_tree
    run_case(3, [parent], [root], live, np.zeros(n_msgs), np.arange(n_msgs) % 4, copy, overlap=overlap)


# --- 2. block padding -------------------------------------------------------------

@pytest.mark.parametrize("copy", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_block_padding(world, copy):
    """padding_case: (round, a -> b, topic) blocks of fewer than 16 record
    words, exactly 16 and more than 16 in one window, two topics sharing every
    region (test_dist_ref_cpu.py::test_padding_seed_hits_15_16_17).  The copy
    and zero-copy paths: the in-place path ships no records below level 1."""
    trees, roots, live, topics = DR.padding_case(0)
    run_case(world, trees, roots, live, topics, None, copy)


# --- 3. fan-out past 64 across ranks ----------------------------------------------

@pytest.mark.parametrize("copy", PATHS)
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("hub_alive", [True, False])
@pytest.mark.parametrize("n_msgs", [50, 200])
@pytest.mark.parametrize("deg", [65, 128, 129])
def test_wide_fan_across_ranks(deg, n_msgs, hub_alive, world, copy):
    """wide_fan: 65 or more consecutive ghost-fed nodes on one rank read one
    remote parent's record (pull_resolve's j0 loop; lane 0 of the second batch
    learns its predecessor's parent from ghost_ref, which the frontier count
    shows), at rows of 1 and 4 words, a few of the children dead, the wide
    parent alive or dead (then its record is the zero head word and nothing
    below it is reached).
    (test_dist_ref_cpu.py::test_wide_fan_puts_65_children_behind_one_record.)"""
    parent, root, hub, facts = DR.wide_fan(deg, world)
    live = np.ones(parent.shape[0], dtype=np.uint8)
    kids = facts["kids"]
    live[[kids[0], kids[63], kids[64], kids[-1]]] = 0
    live[hub] = hub_alive
    run_case(world, [parent], [root], live, np.zeros(n_msgs), None, copy)


# --- 4. world sizes -----------------------------------------------------------------

@pytest.mark.parametrize("world,copy", [(2, False), (3, True), (8, "inplace"), (5, False), (5, True), (5, "inplace"),
                                        (16, False), (16, True), (16, "inplace")])
def test_world_sizes(world, copy):
    """tiny_beside_large at worlds 2 to 16 (the ABI's limit: kMaxRanks, the
    rank select chain of rank_base, the rank bits of a ghost reference): a
    5-node topic most ranks own nothing of beside a 400-node one, and a topic
    whose root's owner owns only the root, so k_pack ships every level-1
    record and reads none back
    (test_dist_ref_cpu.py::test_tiny_beside_large_leaves_ranks_empty_and_plans_agree)."""
    trees, roots, facts = DR.tiny_beside_large(world=world)
    n = trees[0].shape[0]
    live = np.ones(n, dtype=np.uint8)
    live[np.random.default_rng(world).choice(n, size=20, replace=False)] = 0
    live[roots] = 1
    topics = np.array([0] * 70 + [1] * 130 + [2] * 10)
    np.random.default_rng(1).shuffle(topics)
    run_case(world, trees, roots, live, topics, None, copy)


def test_world_17_is_refused():
    """ps_loopback_create and ps_dist_init_loopback refuse a world of 17
    (PS_E_INVAL); the engine stays a one-rank engine and still runs."""
    with pytest.raises(PE.EngineError):
        PE.Loopback(17)
    lb = PE.Loopback(16)
    with PE.Engine(64, 1, record_hops=True) as eng:
        dc = PE.DistConfig(0, 17, PE.PART_PEER, 0, 0, 0)
        assert PE.load().ps_dist_init_loopback(eng._h, C.byref(dc), lb._h) == -1
        parent, root = DR.path(64)
        eng.set_tree(0, root, parent)
        first = eng.publish(np.zeros(3))
        assert eng.run().deliveries == 3 * 63 and eng.hops(first)[63] == 63
    lb.close()


# --- 5. subtree split -----------------------------------------------------------------

@pytest.fixture(scope="module")
def split_trees():
    trees, roots, live = DR.split_case()
    depth = min(int(DR.bfs_levels(t, r).max()) for t, r in zip(trees, roots))
    deepest = max(int(DR.bfs_levels(t, r).max()) for t, r in zip(trees, roots))
    return trees, roots, live, depth, deepest


@pytest.mark.parametrize("chain_max", [1, 2, 4])
@pytest.mark.parametrize("split", ["auto", 1, 2, "depth", "past"])
@pytest.mark.parametrize("world", [2, 4])
def test_subtree_split(split_trees, world, split, chain_max):
    """PS_PART_SUBTREE with an explicit split level: 0 (the first level of 64 *
    world nodes), 1, 2, the shallowest topic's depth, and three past the
    deepest -- where one rank owns everything, nothing is exchanged and the
    others deliver nothing.  Three topics of 3,000 peers, single launches,
    pairs and chains (flood off).  Ownership is dist_ref.owner_subtree's
    (test_dist_ref_cpu.py::test_owner_subtree_matches_partition_owner)."""
    trees, roots, live, depth, deepest = split_trees
    sd = {"auto": 0, "depth": depth, "past": deepest + 3}.get(split, split)
    topics = np.random.default_rng(5).integers(0, 3, size=240)
    stats = run_case(world, trees, roots, live, topics, None, False, partition=PE.PART_SUBTREE, split_depth=sd,
                     plan={"chain_max": chain_max, "flood": 0}, exchanges=split != "past")
    # one exchange round per (topic, start group): only the edges into the split level cross ranks
    assert all(st.xchg_rounds <= 3 for st in stats), [st.xchg_rounds for st in stats]
    kinds = {int(k) for st in stats for k in st.round_kernel}
    if chain_max == 4:
        assert kinds & {PE.K_CHAIN, PE.K_PAIR}, kinds
    if chain_max == 1:
        assert not kinds & {PE.K_CHAIN, PE.K_PAIR, PE.K_PAIR2, PE.K_CHAIN2}, kinds
    if split == "past":
        assert sorted(st.deliveries for st in stats)[:-1] == [0] * (world - 1)
        assert all(st.xchg_rounds == 0 and st.xchg_path == PE.XCHG_NONE for st in stats)


# --- 6. consecutive exchange rounds -------------------------------------------------------

@pytest.mark.parametrize("copy", PATHS)
@pytest.mark.parametrize("staggered", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_path_exchanges_every_round(world, staggered, copy):
    """path(300) under the peer hash: about half (world 2) or two thirds (world
    3) of 299 rounds ship one record, runs of consecutive exchange rounds
    longer than the three send parts, so the parts alternate and are reused
    some hundred times (test_dist_ref_cpu.py::test_path_exchanges_nearly_every_round);
    a few dead-end side branches keep other records in the regions.  Hops past
    254 saturate as the restatement has them; rounds past 255 leave
    deliveries_per_round."""
    parent, root = DR.path(300)
    n = 330
    parent = np.concatenate([parent, np.arange(0, 300, 10, dtype=np.uint32)])  # peer 300 + i under peer 10 * i
    live = np.ones(n, dtype=np.uint8)
    n_msgs = 90
    starts = np.arange(n_msgs) % 3 if staggered else None
    run_case(world, [parent], [root], live, np.zeros(n_msgs), starts, copy)


# --- 7. windows over the same buffers --------------------------------------------------------

@pytest.mark.parametrize("copy", PATHS)
def test_runs_share_the_buffers(copy):
    """World 3 on one set of engines kept open.  Run A: 5-word rows on topic 0,
    all peers live.  Run B: 1-word rows on topic 0 with `victim` dead -- an
    internal peer whose children all sit on other ranks
    (test_dist_ref_cpu.py::test_windows_victim_and_split_roots): its record
    slot still holds run A's five words and must read as unreached.  Run C:
    topic 1 only, over the same send and receive buffers.  Every message of
    every run is checked on every rank."""
    world, n = 3, 600
    trees, roots, victim = DR.windows_case(n, world)
    owners = owners_of(trees, roots, world)
    dead = np.ones(n, dtype=np.uint8)
    dead[victim] = 0
    some = (np.random.default_rng(3).random(n) > 0.05).astype(np.uint8)
    some[roots] = 1
    runs = [(np.zeros(300), np.ones(n, dtype=np.uint8)), (np.zeros(40), dead), (np.ones(90), some),
            (np.zeros(300), dead)]
    lb, engines = make_ranks(world, n, 2, PE.PART_PEER, copy=copy)
    one = PE.Engine(n, 2)
    try:
        for e in engines + [one]:
            for t in range(2):
                e.set_tree(t, roots[t], trees[t])
        for topics, live in runs:
            topics = topics.astype(np.uint32)
            for e in engines + [one]:
                e.set_live(live)
            firsts = [e.publish(topics) for e in engines]
            stats = run_ranks(engines)
            one.publish(topics)
            st1 = one.run()
            check_ranks(engines, stats, firsts, trees, roots, live, topics, None, owners, copy,
                        (st1, one.seen_digest()))
    finally:
        for e in engines + [one]:
            e.close()
        lb.close()


@pytest.mark.parametrize("copy", PATHS)
def test_one_run_in_three_windows(width_tree, copy):
    """msg_window = 128 and 300 messages with starts 0..3: three windows (128,
    128 and 44 messages, the last one narrower) in one run over the same
    buffers, each with its own start groups."""
    parent, root, live = width_tree
    k = 300
    windows = [list(range(0, 128)), list(range(128, 256)), list(range(256, 300))]
    run_case(3, [parent], [root], live, np.zeros(k), np.arange(k) % 4, copy, msg_window=128, windows=windows)


# --- 8. refusals ----------------------------------------------------------------------------------

def test_copy_with_inplace_is_refused():
    """PS_DIST_F_COPY | PS_DIST_F_INPLACE: PS_E_INVAL, and the engine is left
    on one rank."""
    lb = PE.Loopback(2)
    with PE.Engine(64, 1, record_hops=True) as eng:
        with pytest.raises(PE.EngineError) as ei:
            eng.dist_init_loopback(lb, 0, copy=True, inplace=True)
        assert ei.value.code == -1
        parent, root = DR.path(64)
        eng.set_tree(0, root, parent)
        eng.publish(np.zeros(3))
        assert eng.run().deliveries == 3 * 63
    lb.close()
