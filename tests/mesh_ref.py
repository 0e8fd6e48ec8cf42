"""Mesh dissemination restated in plain Python/numpy, and the graphs the mesh
tests run (tests/test_mesh_ref_cpu.py, tests/test_gpu_mesh.py).

No engine call, no GPU, no C: a level-synchronous flood over child lists
(row_ptr, col) from a root under a live mask, with the conventions of
oracle/psoracle.c or_disseminate -- the root forwards and is not a recipient
(whatever its live byte), a dead child neither receives nor forwards, a hop is
one edge, hops saturate at 254 and 0xFF means "not reached".

On top of the hops it states what the oracle does not: ps_stats.duplicates
(include/psengine.h: bits suppressed by the seen test) and the per-round
delivery histogram of messages published at different start rounds.

The builders are deterministic from their arguments and return
(row_ptr, col, root, live, facts): `facts` names the nodes that make the case
what it promises; check_* asserts the promise from the reference itself.
"""
from __future__ import annotations

import numpy as np

HOP_NONE = 0xFF
HOP_MAX = 254
MAX_ROUNDS = 256  # PS_MAX_ROUNDS: the rounds ps_stats counts one by one


class Flood:
    """One message's flood: level[p] (-1: not reached; the root too), hops[p]
    (uint8, saturated), deliveries, duplicates."""

    def __init__(self, row_ptr, col, root: int, live):
        rp = np.asarray(row_ptr, dtype=np.int64)
        cl = np.asarray(col, dtype=np.int64)
        lv = np.asarray(live, dtype=np.uint8)
        n = rp.shape[0] - 1
        assert lv.shape[0] == n and 0 <= root < n
        level = np.full(n, -1, dtype=np.int64)
        have = np.zeros(n, dtype=bool)  # the root has its own message
        have[root] = True
        cur, h = [root], 0
        forwarded = 0  # child entries a forwarder sent the message along, the child live (the root always is)
        while cur:
            h += 1
            nxt = []
            for p in cur:
                for c in cl[rp[p]:rp[p + 1]]:
                    if not (lv[c] or c == root):
                        continue
                    forwarded += 1
                    if have[c]:
                        continue
                    have[c] = True
                    level[c] = h
                    nxt.append(int(c))
            cur = nxt
        self.n = n
        self.root = root
        self.level = level
        self.hops = np.where(level < 0, HOP_NONE, np.minimum(level, HOP_MAX)).astype(np.uint8)
        self.delivered = (level >= 0).astype(np.uint8)
        self.deliveries = int((level >= 0).sum())
        # every forwarder (the root and every reached peer) forwards once, to
        # every live child entry; what is not a delivery met a set seen bit
        self.duplicates = forwarded - self.deliveries
        self.rounds = int(level.max()) if self.deliveries else 0

    def hist(self, length: int = MAX_ROUNDS) -> np.ndarray:
        """Deliveries by hop (unsaturated), hops >= length dropped."""
        lv = self.level[self.level >= 0]
        return np.bincount(lv[lv < length], minlength=length).astype(np.int64)

    def per_round(self, starts, length: int = MAX_ROUNDS) -> np.ndarray:
        """Deliveries by round of messages published at the rounds `starts`: a
        message started at round s is delivered at hop h in round s + h.
        Rounds >= length are dropped (ps_stats.deliveries_per_round)."""
        out = np.zeros(length, dtype=np.int64)
        h = self.hist(length)
        for s, k in zip(*np.unique(np.asarray(starts, dtype=np.int64), return_counts=True)):
            if s < length:
                out[s:] += int(k) * h[:length - s]
        return out


def flood(row_ptr, col, root, live) -> Flood:
    return Flood(row_ptr, col, root, live)


def arrival_order(starts) -> list:
    """Run-relative message ids in the order a reached peer receives them:
    by (start round, id) -- every message takes the same number of hops."""
    s = np.asarray(starts, dtype=np.int64)
    return sorted(range(s.shape[0]), key=lambda m: (int(s[m]), m))


def csr(children, n: int):
    """(row_ptr, col) of a dict / list of child lists."""
    row_ptr = np.zeros(n + 1, dtype=np.uint32)
    col = []
    for p in range(n):
        kids = children[p] if not isinstance(children, dict) else children.get(p, [])
        col.extend(int(c) for c in kids)
        row_ptr[p + 1] = len(col)
    return row_ptr, np.asarray(col, dtype=np.uint32)


def parents_of(row_ptr, col, c: int) -> list:
    """The peers whose child list names c, once per entry."""
    return [p for p in range(len(row_ptr) - 1) for k in range(row_ptr[p], row_ptr[p + 1]) if col[k] == c]


# ------------------------------------------------------------------ builders

def mesh_with_specials(n: int = 300, seed: int = 0):
    """A random mesh of n peers (out-degree <= 6, 10-15 % dead) below a small
    scaffold of peers 0..10 that only the scaffold's own edges reach:

      0 (root) -> 1, 2, 3 and body peers
      1 -> 1 (self-loop), 4, 4 (repeated edge), 0 (edge into the root), 5
      2 -> 5, 6, 8           5: both parents (1, 2) reach it in round 2
      3 -> 7;  7 -> 6, ...   6: reached by 2 in round 2, hit again by 7 in round 3
      8: dead, children 9 (only parent 8: never reached), 10 (also below 4), body peers
    """
    assert n >= 40
    rng = np.random.default_rng(1000 + seed)
    body = np.arange(11, n)
    kids = {p: [int(c) for c in rng.choice(body, size=int(rng.integers(0, 7)))] for p in body}
    # every body peer is named at least once somewhere above it (few stay out of reach)
    pick = lambda k: [int(c) for c in rng.choice(body, size=k)]
    kids[0] = [1, 2, 3] + pick(3)
    kids[1] = [1, 4, 4, 0, 5]
    kids[2] = [5, 6, 8]
    kids[3] = [7]
    kids[4] = [10] + pick(4)
    kids[5] = pick(5)
    kids[6] = pick(6)
    kids[7] = [6] + pick(3)
    kids[8] = [9, 10] + pick(2)
    kids[9] = pick(2)
    kids[10] = pick(3)
    live = np.ones(n, dtype=np.uint8)
    live[rng.choice(body, size=n // 8 - 1, replace=False)] = 0  # 12.5 % dead with peer 8
    live[8] = 0
    row_ptr, col = csr(kids, n)
    facts = {"self_loop": 1, "repeated": (1, 4), "into_root": 1, "same_round": (5, 1, 2),
             "later": (6, 2, 7), "dead_parent": 8, "cut_off": 9}
    return row_ptr, col, 0, live, facts


def check_specials(row_ptr, col, root, live, facts, ref: Flood):
    n = len(row_ptr) - 1
    kids = lambda p: [int(c) for c in col[row_ptr[p]:row_ptr[p + 1]]]
    deg = np.diff(row_ptr.astype(np.int64))
    assert deg.max() <= 6 and live[root]
    assert 0.10 <= 1 - live.mean() <= 0.15, live.mean()
    p = facts["self_loop"]
    assert p in kids(p) and ref.level[p] > 0
    p, c = facts["repeated"]
    assert kids(p).count(c) == 2 and ref.level[p] > 0 and live[c]
    p = facts["into_root"]
    assert root in kids(p) and ref.level[p] > 0
    c, a, b = facts["same_round"]
    assert c in kids(a) and c in kids(b) and ref.level[a] == ref.level[b] == ref.level[c] - 1
    c, a, b = facts["later"]
    assert c in kids(a) and c in kids(b) and ref.level[a] == ref.level[c] - 1 and ref.level[b] >= ref.level[c]
    d = facts["dead_parent"]
    assert not live[d] and any(live[c] for c in kids(d)) and ref.level[d] < 0
    assert any(d in kids(q) and ref.level[q] > 0 for q in range(n))  # a reached peer sends to it
    c = facts["cut_off"]
    assert live[c] and ref.level[c] < 0
    assert ref.duplicates > 0 and ref.deliveries > n // 2


def hub_mesh(deg: int, seed: int = 0):
    """One hub with exactly `deg` children, every one of them with a second
    parent elsewhere:

      0 (root) -> 1, E*        E*: the "earlier" parents, level 1
      1 -> H (hub), W*         W*: the "with" parents, level 2 like the hub
      W* -> L*                 L*: the "later" parents, level 3

    Hub child i (level 3 through the hub) is also a child of E[i // 48] when
    i % 3 == 0 (reached in round 2, before the hub), of W[i // 48] when i % 3
    == 1 (round 3, with the hub) and of L[i // 48] when i % 3 == 2 (hit again
    in round 4).  Every second live hub child has a leaf below it.  The hub's
    children at list positions 0, 63, 64 and deg - 1 are dead (where they
    exist); everything else is live.  The second parents have at most 17
    children each."""
    assert deg >= 3
    n_par = (deg + 47) // 48
    H = 2
    E = list(range(3, 3 + n_par))
    Wt = list(range(3 + n_par, 3 + 2 * n_par))
    Lt = list(range(3 + 2 * n_par, 3 + 3 * n_par))
    c0 = 3 + 3 * n_par
    hub_kids = list(range(c0, c0 + deg))
    # the hub's list in a shuffled order: list position and peer id are unrelated
    rng = np.random.default_rng(2000 + deg + seed)
    order = [int(x) for x in rng.permutation(deg)]
    listed = [hub_kids[i] for i in order]
    dead_pos = sorted({q for q in (0, 63, 64, deg - 1) if q < deg})
    n = c0 + deg
    kids = {0: [1] + E, 1: [H] + Wt, H: listed}
    for j in range(n_par):
        kids[Wt[j]] = [Lt[j]]
        kids[E[j]], kids[Lt[j]] = [], []
    classes = {"earlier": [], "with": [], "later": []}
    for i, c in enumerate(hub_kids):
        par, name = ((E, "earlier"), (Wt, "with"), (Lt, "later"))[i % 3]
        kids[par[i // 48]].append(c)
        classes[name].append(c)
    live_kids = [c for q, c in enumerate(listed) if q not in dead_pos]
    for c in live_kids[::2]:
        kids[c] = [n]
        n += 1
    live = np.ones(n, dtype=np.uint8)
    for q in dead_pos:
        live[listed[q]] = 0
    row_ptr, col = csr(kids, n)
    facts = {"hub": H, "deg": deg, "dead_pos": dead_pos, "classes": classes, "listed": listed}
    return row_ptr, col, 0, live, facts


def check_hub(row_ptr, col, root, live, facts, ref: Flood):
    H, deg = facts["hub"], facts["deg"]
    n = len(row_ptr) - 1
    out = np.diff(row_ptr.astype(np.int64))
    assert out[H] == deg and np.delete(out, H).max() <= 17
    listed = [int(c) for c in col[row_ptr[H]:row_ptr[H + 1]]]
    assert listed == facts["listed"] and len(set(listed)) == deg
    assert [q for q, c in enumerate(listed) if not live[c]] == facts["dead_pos"]
    assert int((1 - live).sum()) == len(facts["dead_pos"])
    hl = ref.level[H]
    assert hl == 2
    seen_classes = set()
    for name, want in (("earlier", hl), ("with", hl + 1), ("later", hl + 1)):
        for c in facts["classes"][name]:
            ps = parents_of(row_ptr, col, c)
            assert len(ps) == 2 and H in ps
            other = ps[0] if ps[1] == H else ps[1]
            if not live[c]:
                assert ref.level[c] < 0
                continue
            assert ref.level[c] == want, (name, c)
            # the other parent forwards one round before / with / after the hub
            assert ref.level[other] - hl == {"earlier": -1, "with": 0, "later": 1}[name]
            seen_classes.add(name)
    assert seen_classes == {"earlier", "with", "later"}
    n_live = deg - len(facts["dead_pos"])
    # every live hub child is hit twice; nothing else is
    assert ref.duplicates == n_live
    assert ref.deliveries == n - 1 - len(facts["dead_pos"])


def detour(n_chain: int):
    """A chain 0 -> 1 -> ... -> n_chain - 1 from the root 0, plus one peer S =
    n_chain: a child of the root and a parent of every chain peer the root
    does not feed itself (2 .. n_chain - 1), dead.  Over the node space
    everything is within two hops of the root; with S dead the live path is
    the chain, n_chain - 1 hops.  With S made live every chain peer from 2 on
    is two hops away and is hit once more by its chain parent."""
    assert n_chain >= 4
    S = n_chain
    kids = {p: [p + 1] for p in range(n_chain - 1)}
    kids[n_chain - 1] = []
    kids[0] = [1, S]
    kids[S] = list(range(2, n_chain))
    live = np.ones(n_chain + 1, dtype=np.uint8)
    live[S] = 0
    row_ptr, col = csr(kids, n_chain + 1)
    return row_ptr, col, 0, live, {"S": S, "n_chain": n_chain, "bfs_depth": 2}


def check_detour(row_ptr, col, root, live, facts, ref: Flood):
    S, k = facts["S"], facts["n_chain"]
    assert not live[S] and row_ptr[S + 1] - row_ptr[S] == k - 2
    # depth of the node space (every peer live): 2
    assert flood(row_ptr, col, root, np.ones_like(live)).rounds == facts["bfs_depth"] == 2
    assert np.array_equal(ref.level[1:k], np.arange(1, k)) and ref.level[S] < 0
    assert ref.deliveries == k - 1 and ref.duplicates == 0 and ref.rounds == k - 1
    up = live.copy()
    up[S] = 1
    r2 = flood(row_ptr, col, root, up)
    assert r2.deliveries == k and r2.duplicates == k - 2 and r2.rounds == 2
