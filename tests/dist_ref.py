"""A plain reference of the sharded (multi-rank) level path: who owns what,
what every rank must report of its own share, and three tree shapes built to
sit on the path's edges.  Plain Python and numpy; it carries the oracle's
conventions (oracle/psoracle.c: the root forwards and is no recipient, one hop
per tree edge, hops relative to the start round, 0xFF where nothing arrives,
saturated at 254) and restates the two partitions from their comments
(csrc/graph.cpp partition_topic, include/psengine.h).  It owns no engine code:
tests/test_dist_ref_cpu.py holds it against or_disseminate and
ps_partition_owner, and holds the shapes to what they promise."""
import numpy as np

NONE = 0xFFFFFFFF
HOP_NONE = 0xFF
HOP_MAX = 254
MAX_ROUNDS = 256  # PS_MAX_ROUNDS: the rounds ps_stats counts one by one
MASK64 = (1 << 64) - 1


def mix64(x: int) -> int:
    """splitmix64 of x (one step of the generator seeded with x)."""
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def owner_peer(peers, world: int) -> np.ndarray:
    """PS_PART_PEER: owner(p) = splitmix64(p) mod world."""
    return np.array([mix64(int(p)) % world for p in np.asarray(peers).ravel()], dtype=np.int64)


def children_of(parent) -> list:
    """Child lists of a parent array (NONE: absent or the root), ascending."""
    parent = np.asarray(parent)
    kids = [[] for _ in range(parent.shape[0])]
    for c in range(parent.shape[0]):
        if parent[c] != NONE:
            kids[int(parent[c])].append(c)
    return kids


def bfs_levels(parent, root: int) -> np.ndarray:
    """BFS level of every peer of the tree under `root`; -1 outside it."""
    kids = children_of(parent)
    level = np.full(len(kids), -1, dtype=np.int64)
    level[root] = 0
    cur = [root]
    while cur:
        nxt = []
        for p in cur:
            for c in kids[p]:
                if level[c] < 0 and c != root:
                    level[c] = level[p] + 1
                    nxt.append(c)
        cur = nxt
    return level


def owner_subtree(parent, root: int, world: int, split_depth: int = 0) -> np.ndarray:
    """PS_PART_SUBTREE.  L = split_depth, or (0) the first BFS level holding at
    least 64 * world nodes, else the deepest level.  The levels above L belong
    to the root's owner (peer hash of the root).  The level-L subtrees are
    dealt largest first (ties: the smaller peer id first), each to the
    least-loaded rank (ties: the lower rank); the top levels' node count is
    charged to the root's owner before the dealing starts.  An L of 0 (a tree
    of one level) falls back to the peer hash; an L past the depth leaves
    everything with the root's owner.  -1 outside the tree."""
    parent = np.asarray(parent)
    n = parent.shape[0]
    level = bfs_levels(parent, root)
    out = np.full(n, -1, dtype=np.int64)
    inside = np.nonzero(level >= 0)[0]
    if world <= 1:
        out[inside] = 0
        return out
    L = split_depth
    if L == 0:
        cnt = np.bincount(level[inside])
        L = len(cnt) - 1
        for d, c in enumerate(cnt):
            if c >= 64 * world:
                L = d
                break
    if L == 0:
        out[inside] = owner_peer(inside, world)
        return out
    top = mix64(root) % world
    # the level-L ancestor of every node at or below L
    anc = np.full(n, -1, dtype=np.int64)
    for p in sorted(inside, key=lambda p: level[p]):
        if level[p] == L:
            anc[p] = p
        elif level[p] > L:
            anc[p] = anc[int(parent[p])]
    size = np.bincount(anc[anc >= 0], minlength=n)
    load = [0] * world
    load[top] = int((level[inside] < L).sum())
    sub_owner = {}
    for u in sorted(np.nonzero(level == L)[0], key=lambda u: (-size[u], u)):
        best = min(range(world), key=lambda q: (load[q], q))
        sub_owner[int(u)] = best
        load[best] += int(size[u])
    for p in inside:
        out[p] = top if level[p] < L else sub_owner[int(anc[p])]
    return out


def reach_levels(parent, root: int, live) -> np.ndarray:
    """One message's flood down the tree: the hop at which every peer receives
    it (a peer receives iff it is live and its parent received; the root
    forwards whatever its own state and is no recipient), -1 where nothing
    arrives.  Unsaturated."""
    kids = children_of(parent)
    hop = np.full(len(kids), -1, dtype=np.int64)
    cur, h = [root], 0
    while cur:
        h += 1
        nxt = []
        for p in cur:
            for c in kids[p]:
                if live[c] and hop[c] < 0 and c != root:
                    hop[c] = h
                    nxt.append(c)
        cur = nxt
    return hop


def expect(trees, roots, live, msg_topics, starts, owners, world=None):
    """What a sharded run must report.  trees[t]: parent array, roots[t], live:
    one mask, msg_topics[m] / starts[m] (None: all 0) per message, owners[t]:
    owner rank per peer (-1 outside topic t's tree).  Returns
      hops   uint8 [n_msgs, n]: the hop of every peer, relative to the
             message's start round, 0xFF where nothing arrives, saturated at 254;
      mine   uint8 [world, n_msgs, n]: the same with 0xFF wherever owner != rank;
      share  {"per_round": int64 [world, MAX_ROUNDS], "total": int64 [world]}:
             each rank's deliveries by absolute round (start + hop; rounds from
             MAX_ROUNDS on are dropped there) and all of them."""
    msg_topics = np.asarray(msg_topics, dtype=np.int64)
    starts = np.zeros_like(msg_topics) if starts is None else np.asarray(starts, dtype=np.int64)
    if world is None:
        world = int(max(int(o.max()) for o in owners)) + 1
    n = np.asarray(trees[0]).shape[0]
    lv = [reach_levels(trees[t], roots[t], live) for t in range(len(trees))]
    sat = [np.where(l < 0, HOP_NONE, np.minimum(l, HOP_MAX)).astype(np.uint8) for l in lv]
    hops = np.empty((len(msg_topics), n), dtype=np.uint8)
    mine = np.full((world, len(msg_topics), n), HOP_NONE, dtype=np.uint8)
    per_round = np.zeros((world, MAX_ROUNDS), dtype=np.int64)
    total = np.zeros(world, dtype=np.int64)
    masked, hist = {}, {}  # (topic, rank) -> the rank's share of the hops / its deliveries by hop
    for t in range(len(trees)):
        own = np.asarray(owners[t])
        for r in range(world):
            sel = own == r
            masked[(t, r)] = np.where(sel, sat[t], HOP_NONE).astype(np.uint8)
            got = lv[t][sel]
            hist[(t, r)] = np.bincount(got[got >= 0], minlength=1)
    for m, (t, s) in enumerate(zip(msg_topics.tolist(), starts.tolist())):
        hops[m] = sat[t]
        for r in range(world):
            mine[r, m] = masked[(t, r)]
            h = hist[(t, r)]
            total[r] += int(h.sum())
            k = min(len(h), max(0, MAX_ROUNDS - s))
            per_round[r, s:s + k] += h[:k]
    return hops, mine, {"per_round": per_round, "total": total}


def expect_frontier(trees, roots, live, msg_topics, starts, owners, world):
    """int64 [world, MAX_ROUNDS]: rank r's ps_stats.frontier_per_round as
    include/psengine.h states it for a sharded level run -- per round q, over
    the (topic, start round s) pairs the window's messages form, the reached
    parents at level q - s - 1 (the root always) with at least one child, live
    or not, owned by r.  A parent with children on k ranks counts on each."""
    msg_topics = np.asarray(msg_topics, dtype=np.int64)
    starts = np.zeros_like(msg_topics) if starts is None else np.asarray(starts, dtype=np.int64)
    out = np.zeros((world, MAX_ROUNDS), dtype=np.int64)
    for t in sorted(set(msg_topics.tolist())):
        lv = reach_levels(trees[t], roots[t], live)
        lv[roots[t]] = 0
        own = np.asarray(owners[t])
        kids = children_of(trees[t])
        by_level = np.zeros((world, MAX_ROUNDS + 1), dtype=np.int64)  # parents at level d, per reading rank
        for p in np.nonzero(lv >= 0)[0]:
            ranks = {int(own[c]) for c in kids[p] if c != roots[t]}
            for r in ranks:
                if lv[p] < MAX_ROUNDS:
                    by_level[r, lv[p]] += 1
        for s in sorted(set(starts[msg_topics == t].tolist())):
            for d in range(MAX_ROUNDS):
                q = s + d + 1  # the parents of level d feed round s + d + 1
                if q < MAX_ROUNDS:
                    out[:, q] += by_level[:, d]
    return out


# --- shapes --------------------------------------------------------------------

def wide_fan(deg: int, world: int, n: int = 480, seed: int = 0):
    """(parent, root, hub, facts): a tree of n peers in which `hub`, a child of
    the root, has exactly `deg` children, at least 65 of them on one rank
    (facts["rank"]) other than the hub's own under the peer hash -- peer ids
    are searched until that holds, so that rank reads more than 64 consecutive
    ghost-fed nodes off one remote parent's record.  Every hub child has up to
    two children of its own (the subtrees a dead hub cuts off); the root has a
    few other children so the hub's level is shared.  facts["kids"]: the
    hub's children, ascending."""
    assert world >= 2 and n >= 3 * deg + 8
    rng = np.random.default_rng(1000 * deg + world + seed)
    ids = [int(p) for p in rng.permutation(n)]
    own = owner_peer(np.arange(n), world)
    root = ids[0]
    hub = ids[1]
    rest = [p for p in ids if p not in (root, hub)]
    # the rank other than the hub's with the most candidates
    rank = max((q for q in range(world) if q != own[hub]), key=lambda q: sum(own[p] == q for p in rest))
    there = [p for p in rest if own[p] == rank]
    assert len(there) >= 65, "widen n"
    k_there = max(65, min(len(there), deg - deg // 4)) if deg > 65 else 65
    kids = there[:k_there]
    others = [p for p in rest if p not in set(kids)]
    kids = sorted(kids + others[:deg - len(kids)])
    assert len(kids) == deg
    left = [p for p in rest if p not in set(kids)]
    parent = np.full(n, NONE, dtype=np.uint32)
    parent[hub] = root
    parent[kids] = hub
    side = left[:5]
    parent[side] = root
    grand = left[5:]
    hosts = kids + side
    for i, p in enumerate(grand):
        parent[p] = hosts[i % len(hosts)] if i < 2 * len(hosts) else grand[i - 2 * len(hosts)]
    facts = {"rank": int(rank), "kids": kids, "on_rank": int(sum(own[c] == rank for c in kids)),
             "hub_owner": int(own[hub])}
    return parent, root, hub, facts


def tiny_beside_large(n: int = 400, world: int = 16, seed: int = 0):
    """(trees, roots, facts): two topics over n peers -- topic 0 a 5-node tree
    (root, two children, two grandchildren under one child), topic 1 a random
    tree over every peer with fan-out up to 4.  With 5 nodes and 16 ranks at
    least 11 ranks own nothing of topic 0.  Topic 2: a root whose owner under
    the peer hash owns nothing else of it -- 12 children and their 24
    children, all on other ranks (ids searched), so k_pack ships every level-1
    record and the root's rank reads none back.  facts: {"tiny": the 5 peers,
    "lonely_root": topic 2's root}."""
    rng = np.random.default_rng(77 + seed)
    own = owner_peer(np.arange(n), world)
    ids = [int(p) for p in rng.permutation(n)]
    t0 = np.full(n, NONE, dtype=np.uint32)
    r0, a, b, c, d = ids[:5]
    t0[[a, b]] = r0
    t0[[c, d]] = a
    r1 = ids[5]
    order = [r1] + [p for p in ids if p != r1]
    t1 = np.full(n, NONE, dtype=np.uint32)
    fan = np.zeros(n, dtype=np.int64)
    for i in range(1, n):
        while True:
            p = order[int(rng.integers(max(0, i - 30), i))]
            if fan[p] < 4:
                break
        t1[order[i]] = p
        fan[p] += 1
    r2 = ids[6]
    away = [p for p in ids if own[p] != own[r2] and p != r2]
    assert len(away) >= 36
    t2 = np.full(n, NONE, dtype=np.uint32)
    t2[away[:12]] = r2
    for i, p in enumerate(away[12:36]):
        t2[p] = away[i % 12]
    return [t0, t1, t2], [r0, r1, r2], {"tiny": [r0, a, b, c, d], "lonely_root": r2}


def path(n: int):
    """(parent, root): a chain n peers deep, peer i under peer i - 1.  Under
    the peer hash consecutive peers mostly sit on different ranks, so
    essentially every round ships a record."""
    parent = np.full(n, NONE, dtype=np.uint32)
    parent[1:] = np.arange(n - 1, dtype=np.uint32)
    return parent, 0


def random_tree(rng, n: int, root: int, fan: int = 4, members: int = None, near: int = 40):
    """A random tree over `members` (default all n) peers, fan-out <= fan; a
    peer's parent is one of the `near` peers placed before it (deep and thin),
    or any earlier one (near = 0: shallow and wide)."""
    perm = rng.permutation(n)
    perm = np.concatenate([[root], perm[perm != root]])[:members or n]
    parent = np.full(n, NONE, dtype=np.uint32)
    kids = np.zeros(n, dtype=np.int64)
    for i in range(1, len(perm)):
        while True:
            p = perm[rng.integers(max(0, i - near) if near else 0, i)]
            if kids[p] < fan:
                break
        parent[perm[i]] = p
        kids[p] += 1
    return parent


def padding_case(seed: int, n: int = 300):
    """(trees, roots, live, msg_topics): the block-padding case -- two small
    random trees (fan-out <= 3), 70 and 200 messages: rows of 2 and 4 words,
    so a block of k records is 2k or 4k words and blocks of 15 or fewer, exactly
    16 and 17 or more words all occur for the committed seed
    (tests/test_dist_ref_cpu.py::test_padding_seed_hits_15_16_17)."""
    rng = np.random.default_rng(seed)
    roots = [int(x) for x in rng.choice(n, size=2, replace=False)]
    trees = [random_tree(rng, n, roots[0], 3, members=90), random_tree(rng, n, roots[1], 3)]
    live = (rng.random(n) > 0.06).astype(np.uint8)
    live[roots] = 1
    msg_topics = np.concatenate([np.zeros(70, dtype=np.int64), np.ones(200, dtype=np.int64)])
    return trees, roots, live, msg_topics


NO_PAD = {"pad_words": 1 << 20}  # rows keep odd word counts (plan.cpp pads rows of >= pad_words words to even)

# (messages of the one topic, plan options, row words): ceil(count / 64) words,
# padded to even from 16 words on unless NO_PAD -- so 17, 63 and 65 words need
# the padding out of the way, and by default 63 * 64 messages give 64 words and
# 64 * 64 + 1 give 66 (tests/test_dist_ref_cpu.py::test_row_counts_give_these_widths)
ROW_CASES = [(40, None, 1), (100, None, 2), (150, None, 3), (200, None, 4), (300, None, 5), (1000, None, 16),
             (1060, NO_PAD, 17), (63 * 64 - 5, NO_PAD, 63), (63 * 64 - 5, None, 64), (64 * 64 + 1, NO_PAD, 65),
             (64 * 64 + 1, None, 66)]
# staggered (starts 0..3 in turn): (messages, words of every start group's
# block) -- a block is ceil(count / 64) words padded to even, whatever
# pad_words says, so 300 messages a group (5 words) travel as 6
GROUP_CASES = [(4 * 100, 2), (4 * 300, 6)]


def row_width_case(n: int = 600):
    """(parent, root, live): the row-width tree -- n peers, fan-out <= 4, about
    8 % dead (the root alive), dead internal peers with children on other
    ranks among them at world 3
    (tests/test_dist_ref_cpu.py::test_row_width_tree_has_the_dead_parents)."""
    rng = np.random.default_rng(600)
    root = int(rng.integers(0, n))
    parent = random_tree(rng, n, root, 4)
    live = (rng.random(n) > 0.08).astype(np.uint8)
    live[root] = 1
    return parent, root, live


def split_case(n: int = 3000):
    """(trees, roots, live): the subtree-split case -- three shallow wide trees
    over all n peers (fan-out <= 4, parents drawn from every earlier peer), 4 %
    dead, the three roots on one rank at world 2 and at world 4 (so a split
    level past every depth leaves one rank with everything)."""
    rng = np.random.default_rng(3000)
    roots = []
    for p in rng.permutation(n):
        if mix64(int(p)) % 4 == 1:
            roots.append(int(p))
        if len(roots) == 3:
            break
    trees = [random_tree(rng, n, r, 4, near=0) for r in roots]
    live = (rng.random(n) > 0.04).astype(np.uint8)
    live[roots] = 1
    return trees, roots, live


def windows_case(n: int = 600, world: int = 3):
    """(trees, roots, victim): two trees over n peers for the runs that share
    one set of buffers; `victim` is an internal peer of topic 0, two levels or
    more below the root, with children of its own and all of them on ranks
    other than its own under the peer hash: killed, its record must read as
    unreached on those ranks."""
    rng = np.random.default_rng(7)
    roots = [int(x) for x in rng.choice(n, size=2, replace=False)]
    trees = [random_tree(rng, n, r, 4) for r in roots]
    own = owner_peer(np.arange(n), world)
    kids = children_of(trees[0])
    lv = bfs_levels(trees[0], roots[0])
    victim = next(p for p in range(n) if lv[p] >= 2 and len(kids[p]) >= 2 and all(own[c] != own[p] for c in kids[p])
                  and any(kids[c] for c in kids[p]))
    return trees, roots, victim
