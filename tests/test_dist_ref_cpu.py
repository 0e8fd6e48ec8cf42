"""CPU: tests/dist_ref.py (the plain reference of the sharded level path)
against the engine's host code -- or_disseminate for the hops and shares,
ps_partition_owner for the two partitions -- and the promises of its shape
builders, read off the host-only planner probe (psengine.plan.Plan).  The GPU
cases of tests/test_gpu_dist_edges.py rely on these conditions and name the
test that guarantees each."""
import numpy as np
import pytest

import dist_ref as DR
import oracle as O
import psengine as PE
from psengine import plan as PL
from psengine import workloads as WL

MASK = (1 << 27) - 1  # kRemoteIdMask: a ghost reference is rank << 27 | record
NONE = DR.NONE
PAD_SEED = 0  # found by search from 0 up: the first seed that holds all three block sizes at world 2 and at world 3


def pad16(w):
    return (w + 15) & ~15


def test_owner_peer_is_the_workloads_hash():
    p = np.arange(5000)
    for world in (2, 3, 5, 8, 16):
        assert np.array_equal(DR.owner_peer(p, world), WL.owner(p, world))


# --- expect against or_disseminate ---------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_expect_matches_or_disseminate(seed):
    """Random trees over part of the peers, 10 % dead, starts 0..4: the hops
    are the oracle's for every message (relative to the start), the ranks'
    shares partition them, and the per-round deliveries are the oracle's hop
    histogram shifted by every start."""
    rng = np.random.default_rng(seed)
    n, world = 700, 3
    roots = [int(x) for x in rng.choice(n, size=3, replace=False)]
    trees = [DR.random_tree(rng, n, r, 4, members=m) for r, m in zip(roots, (n, 300, 40))]
    live = (rng.random(n) > 0.1).astype(np.uint8)
    topics = rng.integers(0, 3, size=60)
    starts = rng.integers(0, 5, size=60)
    owners = [np.where(DR.bfs_levels(t, r) >= 0, DR.owner_peer(np.arange(n), world), -1) for t, r in zip(trees, roots)]
    hops, mine, share = DR.expect(trees, roots, live, topics, starts, owners, world)
    per_round = np.zeros(DR.MAX_ROUNDS, dtype=np.int64)
    total = 0
    for t in range(3):
        rp, cl = O.parents_to_csr(trees[t])
        tot, oh, hist = O.disseminate(rp, cl, roots[t], live, 1)
        for m in np.nonzero(topics == t)[0]:
            assert np.array_equal(hops[m], oh[0]), (t, m)
            s = int(starts[m])
            per_round[s:] += hist[:DR.MAX_ROUNDS - s].astype(np.int64)
            total += tot
    assert np.array_equal(share["per_round"].sum(axis=0), per_round)
    assert share["total"].sum() == total
    # every reached (message, peer) is in exactly one rank's share, with its hop
    assert np.array_equal(mine.min(axis=0), hops)
    assert ((mine != DR.HOP_NONE).sum(axis=0) == (hops != DR.HOP_NONE)).all()
    for r in range(world):
        assert (mine[r] != DR.HOP_NONE).sum() == share["total"][r]


def test_expect_saturates_like_the_oracle():
    """path(300): hops 1..254 then 254 for ever; rounds from 256 on leave the
    per-round table and stay in the total."""
    parent, root = DR.path(300)
    live = np.ones(300, dtype=np.uint8)
    rp, cl = O.parents_to_csr(parent)
    tot, oh, _ = O.disseminate(rp, cl, root, live, 1)
    own = [DR.owner_peer(np.arange(300), 2)]
    hops, mine, share = DR.expect([parent], [root], live, [0, 0], [0, 2], own, 2)
    assert np.array_equal(hops[0], oh[0]) and np.array_equal(hops[1], oh[0])
    assert hops[0][250:].tolist() == list(range(250, 255)) + [254] * 45
    assert share["total"].sum() == 2 * tot == 2 * 299
    assert share["per_round"].sum() == 255 + 253


# --- owner_subtree against ps_partition_owner -------------------------------------

def tie_tree():
    """Level 1: peers 1..6; subtrees of 9, 9, 9, 5, 5 and 1 nodes, so the
    dealing order among the equal ones and the rank of equal loads matter."""
    parent = [NONE] + [0] * 6
    for top, extra in zip(range(1, 7), (8, 8, 8, 4, 4, 0)):
        last = top
        for _ in range(extra):
            parent.append(last)
            last = len(parent) - 1
    parent += [NONE] * 3  # peers outside the tree
    return np.array(parent, dtype=np.uint32), 0


@pytest.mark.parametrize("world", [2, 3, 5, 8, 16])
def test_owner_subtree_matches_partition_owner(world):
    rng = np.random.default_rng(world)
    cases = [tie_tree()]
    for n, fan in ((900, 4), (2500, 3)):
        root = int(rng.integers(0, n))
        cases.append((DR.random_tree(rng, n, root, fan, members=n - 50), root))
    # ids shuffled: peer order and BFS order differ
    par, root = tie_tree()
    perm = rng.permutation(par.shape[0])
    shuf = np.full(par.shape[0], NONE, dtype=np.uint32)
    for c in range(par.shape[0]):
        if par[c] != NONE:
            shuf[perm[c]] = perm[par[c]]
    cases.append((shuf, int(perm[root])))
    for parent, root in cases:
        depth = int(DR.bfs_levels(parent, root).max())
        for sd in (0, 1, 2, depth, depth + 3):
            got = PE.partition_owner(parent, root, 0, world, PE.PART_SUBTREE, sd)
            assert np.array_equal(DR.owner_subtree(parent, root, world, sd), got), (world, sd, parent.shape[0])
        got = PE.partition_owner(parent, root, 0, world, PE.PART_PEER)
        inside = DR.bfs_levels(parent, root) >= 0
        assert np.array_equal(np.where(inside, DR.owner_peer(np.arange(parent.shape[0]), world), -1), got)


def test_tie_rules_decide_the_tie_tree():
    """The tie tree really has equal level-1 subtrees, and reversing either
    tie rule changes the outcome (so the comparison above holds them)."""
    parent, root = tie_tree()
    own = DR.owner_subtree(parent, root, 3, 1)
    top = DR.mix64(0) % 3
    # largest first, smaller id first: 1, 2, 3 go to the three least-loaded ranks in rank order
    order = sorted(range(3), key=lambda q: ((1 if q == top else 0), q))
    assert [int(own[k]) for k in (1, 2, 3)] == order
    assert np.array_equal(own, PE.partition_owner(parent, root, 0, 3, PE.PART_SUBTREE, 1))


def test_world_17_is_refused():
    parent, root = tie_tree()
    with pytest.raises(PE.EngineError) as ei:
        PE.partition_owner(parent, root, 0, 17, PE.PART_SUBTREE)
    assert ei.value.code == -1  # PS_E_INVAL
    with pytest.raises(PE.EngineError) as ei:
        PE.partition_owner(parent, root, 0, 17, PE.PART_PEER)
    assert ei.value.code == -1


# --- the builders' promises, through the planner probe --------------------------

def plans_for(trees, roots, world, topics, starts=None, partition=PE.PART_PEER, split_depth=0, opts=None):
    plans = [PL.Plan(np.stack(trees), roots, world, r, partition, split_depth, plan=opts) for r in range(world)]
    for p in plans:
        p.window(topics, starts)
    return plans


def ghost_runs(plan, t, d):
    """{ghost reference: how many consecutive nodes of topic t's level d on
    this rank read it} from GHOST_REF and the level tables."""
    T = plan.topic(t)
    if d > T["depth"] or not T["n_nodes"]:
        return {}
    gref = plan.get(PL.GHOST_REF).astype(np.int64)
    lo = T["level_off"]
    a, b = T["nbase"] + lo[d] + T["level_local"][d], T["nbase"] + lo[d + 1]
    out = {}
    for u in range(a, b):
        assert gref[u] != NONE
        if u > a and gref[u] != gref[u - 1]:
            assert int(gref[u]) not in out, "a parent's ghost-fed children are not consecutive"
        out[int(gref[u])] = out.get(int(gref[u]), 0) + 1
    return out


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("deg", [65, 128, 129])
def test_wide_fan_puts_65_children_behind_one_record(deg, world):
    """wide_fan's promise: on facts["rank"], level 2 holds a run of at least
    65 consecutive ghost-fed nodes that read one record (the hub's), and the
    hub's children number exactly deg."""
    parent, root, hub, facts = DR.wide_fan(deg, world)
    assert int((parent == hub).sum()) == deg and parent[hub] == root
    assert facts["on_rank"] >= 65 and facts["rank"] != facts["hub_owner"]
    assert DR.bfs_levels(parent, root).min() == 0  # every peer is in the tree
    plans = plans_for([parent], [root], world, np.zeros(10, dtype=np.uint32))
    runs = ghost_runs(plans[facts["rank"]], 0, 2)
    big = {g: k for g, k in runs.items() if k >= 65}
    assert len(big) == 1 and list(big.values())[0] == facts["on_rank"], runs
    assert list(big)[0] >> 27 == facts["hub_owner"]
    # ... and one k_pull chunk holds the whole run (kPullMaxKids = 512 nodes a chunk)
    p = plans[facts["rank"]]
    lo, split, hi, ch = p.chunks(PL.PULL, 2)
    gref = p.get(PL.GHOST_REF).astype(np.int64)
    assert any((gref[c["node_begin"]:c["node_end"]] == list(big)[0]).sum() >= 65 for c in ch[split - lo:])


def test_tiny_beside_large_leaves_ranks_empty_and_plans_agree():
    """At world 16 at least one rank owns no node of the tiny topic, the
    lonely root's owner owns nothing else of topic 2, and every rank still
    plans the same rounds, exchange rounds and region sizes."""
    world = 16
    trees, roots, facts = DR.tiny_beside_large(world=world)
    n = trees[0].shape[0]
    own = DR.owner_peer(np.arange(n), world)
    plans = plans_for(trees, roots, world, np.array([0] * 70 + [1] * 130 + [2] * 10, dtype=np.uint32))
    empty = [r for r in range(world) if plans[r].topic(0)["n_nodes"] == 0]
    assert len(empty) >= 11 and len(empty) == world - len(set(own[facts["tiny"]].tolist()))
    r2 = facts["lonely_root"]
    assert plans[own[r2]].topic(2)["n_nodes"] == 1 and plans[own[r2]].topic(2)["root_local"]
    assert all(own[c] != own[r2] for c in np.nonzero(DR.bfs_levels(trees[2], r2) > 0)[0])
    info = [p.info() for p in plans]
    assert len({i["rounds"] for i in info}) == 1
    for q in range(1, info[0]["rounds"] + 1):
        xs = [p.xchg(q) for p in plans]
        assert len({x["any"] for x in xs}) == 1
        if xs[0]["any"]:
            for a in range(world):
                for b in range(world):
                    if a != b:
                        assert xs[a]["s_len"][b] == xs[b]["r_len"][a], (q, a, b)


def block_words(plans, trees, q):
    """{(a, b, topic): records * rw} of round q of a single-start window, read
    off the receivers' ghost references; checked against the regions: every
    region a -> b is the sum of its blocks, each padded to 16 words (xchg),
    and the segments' bases step by those padded sizes (segs)."""
    world = len(plans)
    out = {}
    for b in range(world):
        x = plans[b].xchg(q)
        if not x["any"]:
            continue
        regions = {a: 0 for a in range(world) if a != b}
        for t in range(len(trees)):
            rw = plans[b].layout(t)["W"]
            runs = ghost_runs(plans[b], t, q)
            for a in regions:
                k = sum(1 for g in runs if g >> 27 == a)
                if k:
                    out[(a, b, t)] = k * rw
                regions[a] += pad16(k * rw)
        for a, w in regions.items():
            assert x["r_len"][a] == 8 * w, (q, a, b, x["r_len"][a], w)
            assert plans[a].xchg(q)["s_len"][b] == 8 * w
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_padding_seed_hits_15_16_17(world):
    """padding_case(PAD_SEED): some (round, a -> b, block) has records * rw of
    exactly 16 words, one has 1..15 and one has 17 or more -- pad16 at, below
    and above its boundary -- and the regions add up from the padded blocks."""
    trees, roots, live, topics = DR.padding_case(PAD_SEED)
    plans = plans_for(trees, roots, world, topics)
    assert [plans[0].layout(t)["W"] for t in (0, 1)] == [2, 4]
    sizes = set()
    for q in range(1, plans[0].info()["rounds"] + 1):
        sizes |= set(block_words(plans, trees, q).values())
    assert 16 in sizes and any(0 < s <= 15 for s in sizes) and any(s >= 17 for s in sizes), sorted(sizes)
    segs = plans[0].segs()
    assert segs and all(int(b) % 16 == 0 for s in segs for b in s["sbase"]) and {s["rw"] for s in segs} == {2, 4}


@pytest.mark.parametrize("world", [2, 3])
def test_path_exchanges_nearly_every_round(world):
    """path(300) under the peer hash: at least 150 consecutive-pair hand-overs
    cross ranks, so the send parts alternate round after round."""
    parent, root = DR.path(300)
    plans = plans_for([parent], [root], world, np.zeros(5, dtype=np.uint32))
    rounds = plans[0].info()["rounds"]
    assert rounds in (299, 300)  # (depth, or depth + 1: the planner keeps one round past the deepest level)
    ex = [plans[0].xchg(q)["any"] for q in range(1, rounds + 1)]
    own = DR.owner_peer(np.arange(300), world)
    assert sum(ex) == int((own[1:] != own[:-1]).sum()) >= 140
    run = best = 0
    for x in ex:
        run = run + 1 if x else 0
        best = max(best, run)
    assert best >= 4  # more consecutive exchange rounds than there are send parts (3)


def test_row_counts_give_these_widths():
    """ROW_CASES and GROUP_CASES name the row words the planner really lays
    out for their message counts, on every rank."""
    parent, root, live = DR.row_width_case()
    for n_msgs, opts, words in DR.ROW_CASES:
        for p in plans_for([parent], [root], 3, np.zeros(n_msgs, dtype=np.uint32), opts=opts):
            assert p.layout(0)["W"] == words, (n_msgs, opts, p.layout(0))
            assert {s["rw"] for s in p.segs()} == {words}
    for n_msgs, words in DR.GROUP_CASES:
        starts = np.arange(n_msgs, dtype=np.uint32) % 4
        for p in plans_for([parent], [root], 3, np.zeros(n_msgs, dtype=np.uint32), starts):
            assert [g[2] for g in p.layout(0)["groups"]] == [words] * 4, p.layout(0)
            assert {s["rw"] for s in p.segs()} == {words}


def test_row_width_tree_has_the_dead_parents():
    """row_width_case at world 3: dead internal peers, reached parents, whose
    children sit on other ranks (their records must carry a zero head word),
    and reached parents whose children sit on two ranks or more (so the ranks'
    frontier counts cannot add up to one rank's)."""
    parent, root, live = DR.row_width_case()
    n = parent.shape[0]
    own = DR.owner_peer(np.arange(n), 3)
    kids = DR.children_of(parent)
    hop = DR.reach_levels(parent, root, live)
    dead_up = [p for p in range(n) if not live[p] and p != root and hop[int(parent[p])] >= 0
               and any(own[c] != own[p] for c in kids[p])]
    assert len(dead_up) >= 5
    spread = [p for p in range(n) if hop[p] >= 0 and len({int(own[c]) for c in kids[p]}) >= 2]
    assert len(spread) >= 20
    assert 40 <= int((live == 0).sum()) <= 60


def test_windows_victim_and_split_roots():
    trees, roots, victim = DR.windows_case()
    own = DR.owner_peer(np.arange(600), 3)
    kids = DR.children_of(trees[0])
    assert kids[victim] and all(own[c] != own[victim] for c in kids[victim])
    assert DR.bfs_levels(trees[0], roots[0])[victim] >= 2
    trees, roots, live = DR.split_case()
    for world in (2, 4):
        assert len({int(x) for x in DR.owner_peer(roots, world)}) == 1
    depths = [int(DR.bfs_levels(t, r).max()) for t, r in zip(trees, roots)]
    assert all(8 <= d <= 40 for d in depths), depths
    # the automatic split level exists at world 4: some level holds 256 nodes
    assert all(np.bincount(DR.bfs_levels(t, r)).max() >= 256 for t, r in zip(trees, roots))
