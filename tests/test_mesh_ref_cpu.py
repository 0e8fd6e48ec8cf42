"""CPU: tests/mesh_ref.py -- the mesh tests' expected answer -- against
oracle/psoracle.c (hops, total, hop histogram), its duplicate count against a
direct count along the oracle's frontier order, and every builder's promise."""
import numpy as np
import pytest

import mesh_ref as MR
import oracle as O
from test_gpu_drain_batch import random_mesh2
from test_gpu_parity import random_mesh

HUB_DEGS = (63, 64, 65, 128, 129, 200)


def against_oracle(rp, cl, root, live):
    ref = MR.flood(rp, cl, root, live)
    total, hops, hist = O.disseminate(rp, cl, root, live, 1, hist_len=MR.MAX_ROUNDS)
    assert np.array_equal(ref.hops, hops[0])
    assert ref.deliveries == total
    assert np.array_equal(ref.hist(), hist.astype(np.int64))
    assert np.array_equal(ref.delivered, (hops[0] != 0xFF).astype(np.uint8))
    assert ref.hops[root] == 0xFF
    return ref


def brute_duplicates(rp, cl, root, live):
    """Copies that meet a peer which already has the message, counted one by
    one in or_disseminate's frontier order (the root has it from the start and
    forwards whatever its live byte)."""
    n = len(rp) - 1
    has = [False] * n
    has[root] = True
    cur, dup, deliv = [root], 0, 0
    while cur:
        nxt = []
        for p in cur:
            for e in range(int(rp[p]), int(rp[p + 1])):
                c = int(cl[e])
                if not live[c] and c != root:
                    continue  # a dead host takes nothing: neither delivered nor suppressed
                if has[c]:
                    dup += 1
                    continue
                has[c] = True
                deliv += 1
                nxt.append(c)
        cur = nxt
    return dup, deliv


def test_specials_against_oracle_and_facts():
    for seed in range(3):
        rp, cl, root, live, facts = MR.mesh_with_specials(300, seed)
        ref = against_oracle(rp, cl, root, live)
        MR.check_specials(rp, cl, root, live, facts, ref)
    a, b = MR.mesh_with_specials(300, 1), MR.mesh_with_specials(300, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a[:2] + a[3:4], b[:2] + b[3:4]))  # deterministic


@pytest.mark.parametrize("deg", HUB_DEGS + (12, 48, 49))
def test_hub_against_oracle_and_facts(deg):
    rp, cl, root, live, facts = MR.hub_mesh(deg)
    ref = against_oracle(rp, cl, root, live)
    MR.check_hub(rp, cl, root, live, facts, ref)
    assert facts["dead_pos"] == sorted({q for q in (0, 63, 64, deg - 1) if q < deg})


@pytest.mark.parametrize("n_chain", [4, 8, 40, 300, 4300])
def test_detour_against_oracle_and_facts(n_chain):
    rp, cl, root, live, facts = MR.detour(n_chain)
    ref = against_oracle(rp, cl, root, live)
    MR.check_detour(rp, cl, root, live, facts, ref)
    # saturation: the hop byte stops at 254, the histogram and the rounds do not
    assert ref.hops[n_chain - 1] == min(n_chain - 1, 254)
    assert ref.rounds == n_chain - 1
    per = ref.per_round([0] * 70)
    assert all(per[q] == (70 if q < n_chain else 0) for q in range(1, MR.MAX_ROUNDS))
    up = live.copy()
    up[facts["S"]] = 1
    against_oracle(rp, cl, root, up)


@pytest.mark.parametrize("seed", range(6))
def test_random_meshes_against_oracle(seed):
    rng = np.random.default_rng(300 + seed)
    n = int(rng.integers(2, 1500))
    root = int(rng.integers(0, n))
    live = (rng.random(n) > 0.15).astype(np.uint8)  # (the root may be dead: it forwards all the same)
    rp, cl = random_mesh(rng, n, 1 + seed % 4)
    ref = against_oracle(rp, cl, root, live)
    assert (ref.duplicates, ref.deliveries) == brute_duplicates(rp, cl, root, live)
    rp, cl = random_mesh2(rng, n, root)
    ref = against_oracle(rp, cl, root, live)
    assert (ref.duplicates, ref.deliveries) == brute_duplicates(rp, cl, root, live)


def test_duplicates_by_hand_and_brute_force():
    """Three small graphs whose duplicate count can be read off the picture."""
    # a diamond: 0 -> 1, 2; 1 -> 3; 2 -> 3: one duplicate at 3
    rp, cl = MR.csr({0: [1, 2], 1: [3], 2: [3]}, 4)
    live = np.ones(4, np.uint8)
    ref = MR.flood(rp, cl, 0, live)
    assert (ref.duplicates, ref.deliveries) == brute_duplicates(rp, cl, 0, live) == (1, 3)
    # ... with 3 dead: nothing delivered to it, nothing suppressed
    live[3] = 0
    ref = MR.flood(rp, cl, 0, live)
    assert (ref.duplicates, ref.deliveries) == brute_duplicates(rp, cl, 0, live) == (0, 2)
    # a self-loop, a repeated edge, an edge into the root, a cycle back:
    # 0 -> 1, 1; 1 -> 1, 0, 2; 2 -> 1.  Suppressed: the second 0->1, 1->1, 1->0, 2->1
    rp, cl = MR.csr({0: [1, 1], 1: [1, 0, 2], 2: [1]}, 3)
    live = np.ones(3, np.uint8)
    ref = MR.flood(rp, cl, 0, live)
    assert (ref.duplicates, ref.deliveries) == brute_duplicates(rp, cl, 0, live) == (4, 2)
    # ... and the same with a dead root: it still forwards, and still suppresses the edge into it
    live[0] = 0
    ref = MR.flood(rp, cl, 0, live)
    assert (ref.duplicates, ref.deliveries) == brute_duplicates(rp, cl, 0, live) == (4, 2)
    total, hops, _ = O.disseminate(rp, cl, 0, live, 1)
    assert total == 2 and np.array_equal(hops[0], ref.hops)
    # a dead peer in the middle cuts what is only below it: 0 -> 1 -> 2, 0 -> 3 -> 2 with 1 dead
    rp, cl = MR.csr({0: [1, 3], 1: [2], 3: [2]}, 4)
    live = np.array([1, 0, 1, 1], np.uint8)
    ref = MR.flood(rp, cl, 0, live)
    assert (ref.duplicates, ref.deliveries) == brute_duplicates(rp, cl, 0, live) == (0, 2)
    assert list(ref.hops) == [0xFF, 0xFF, 2, 1]


def test_per_round_and_arrival_order():
    rp, cl, root, live, _ = MR.mesh_with_specials(300, 0)
    ref = MR.flood(rp, cl, root, live)
    starts = np.array([0, 3, 3, 5, 0, 1])
    per = ref.per_round(starts)
    exp = np.zeros(MR.MAX_ROUNDS, dtype=np.int64)
    for s in starts:  # message by message, peer by peer
        for p in np.nonzero(ref.level >= 0)[0]:
            exp[s + ref.level[p]] += 1
    assert np.array_equal(per, exp) and per[0] == 0 and per.sum() == len(starts) * ref.deliveries
    assert MR.arrival_order(starts) == [0, 4, 5, 1, 2, 3]
    # a round past the table is dropped, not wrapped
    rp, cl, root, live, _ = MR.detour(300)
    ref = MR.flood(rp, cl, root, live)
    per = ref.per_round([0, 250])
    assert per[255] == 2 and per[5] == 1 and per[251] == 2 and per.sum() == 255 + 5


def test_row_counts_give_these_widths():
    """The message counts tests/test_gpu_mesh.py runs give the row widths it
    names: plan_window_layout's own answer (a mesh topic's row is laid out as a
    single-start topic's: ceil(count / 64) words, even from pad_words on)."""
    from psengine import plan as PL
    from test_gpu_mesh import NO_PAD, ROW_CASES

    parent = np.array([O.NONE, 0, 0, 1], dtype=np.uint32)
    for n_msgs, opts, words in ROW_CASES:
        p = PL.Plan(parent[None, :], [0], plan=opts)
        p.window(np.zeros(n_msgs))
        assert p.layout(0)["W"] == words, (n_msgs, opts)
        p.close()
    assert sorted({w for _, _, w in ROW_CASES}) == [1, 2, 3, 5, 63, 64, 65, 66, 130]
    assert NO_PAD["pad_words"] > 130
