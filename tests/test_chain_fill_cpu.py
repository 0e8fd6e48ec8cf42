"""The fill segment table of chain launches, through the
host-only planner probe (PS_PLAN_FILL): for random level profiles the
segments of a launch cover exactly the node ranges of its whole-row chain
chunks and their levels, once; the pieces tile each segment's words in order,
cut on 128-B lines; and the planner's other outputs are byte for byte what
they are with the fill switched off."""
import numpy as np
import pytest

import oracle as O
from psengine import plan as PL

LINE = 16       # kFillLine: words of a 128-B line
PIECE = 2048    # kFillPieceWords
NODES = 2048    # kFillPieceNodes
BLOCK = 256     # kFillReachBlock


def random_tree(rng, n, root, fan, members):
    perm = rng.permutation(n)[:members]
    perm = np.concatenate([[root], perm[perm != root]])
    parent = np.full(n, O.NONE, dtype=np.uint32)
    kids = np.zeros(n, dtype=np.int64)
    for i in range(1, len(perm)):
        while True:
            p = perm[rng.integers(max(0, i - 4 * fan), i)]
            if kids[p] < fan:
                break
        parent[perm[i]] = p
        kids[p] += 1
    return parent


def make_plan(monkeypatch, fill, parents, roots, msgs, starts=None, **opts):
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_CHAIN_FILL_BYTES", "0")
    monkeypatch.setenv("PSAMD_CHAIN_FILL_ROW_WORDS", "0")
    monkeypatch.setenv("PSAMD_CHAIN_FILL", "1" if fill else "0")
    p = PL.Plan(parents, roots, plan={"flood": 0, **opts})
    p.window(msgs, starts)
    return p


def existing_outputs(p):
    """Everything the probe reported before PS_PLAN_FILL, as bytes."""
    out = [p.get(PL.INFO).tobytes(), p.get(PL.ROUND_KIND).tobytes(), p.get(PL.SCHEDULE).tobytes()]
    for t in range(p.n_topics):
        out += [p.get(PL.TOPIC, t).tobytes(), p.get(PL.LAYOUT, t).tobytes()]
    kinds = p.get(PL.ROUND_KIND)
    for q in range(1, p.info()["rounds"] + 1):
        out += [p.get(PL.PULL, q).tobytes(), p.get(PL.CHAIN, q).tobytes()]
        if kinds[q] == 3:  # PS_K_PAIR: the round's pair chunks (a chain round's lo .. hi index chain chunks)
            out.append(p.get(PL.PAIR, q).tobytes())
    return out


def case(rng):
    n = int(rng.integers(300, 5000))
    nt = int(rng.integers(1, 6))
    roots = rng.choice(n, size=nt, replace=False)
    parents = [random_tree(rng, n, int(r), int(rng.integers(2, 7)), int(rng.integers(1, n))) for r in roots]
    widths = rng.choice([1, 2, 3, 15, 16, 17, 64, 65, 330, 769], size=nt)
    msgs = np.concatenate([np.full(64 * int(w) - int(rng.integers(0, 60)), t, dtype=np.uint32)
                           for t, w in enumerate(widths)])
    rng.shuffle(msgs)
    return n, parents, roots, msgs


@pytest.mark.parametrize("seed", range(12))
def test_segments_cover_chain_launches(monkeypatch, seed):
    rng = np.random.default_rng(5100 + seed)
    n, parents, roots, msgs = case(rng)
    chain_max = int(rng.choice([3, 4, 6]))
    on = make_plan(monkeypatch, True, parents, roots, msgs, chain_max=chain_max)
    off = make_plan(monkeypatch, False, parents, roots, msgs, chain_max=chain_max)
    assert existing_outputs(on) == existing_outputs(off)
    kinds = on.get(PL.ROUND_KIND)
    launches = 0
    for q in range(len(kinds)):
        assert off.fill(q) == (0, [], [])
        rounds, chunks = on.chain(q)
        blocks, segs, pieces = on.fill(q)
        whole = [c for c in chunks if c["S"] == c["W"]]
        if not whole:
            assert not segs
            continue
        launches += 1
        # the chunks' nodes: every level of every whole-row (topic, run) -- the runs tile level d, and
        # the levels below are whole levels of the topic
        want = {}
        for c in whole:
            assert c["r0"] == 0 and c["w0"] == 0
            want.setdefault(c["topic"], (c["W"], c["row0"], c["levels"], c["first"]))
        assert [s["topic"] for s in segs] == sorted(want)  # once each, in address order
        piece_at = blk_at = 0
        it = iter(pieces)
        for s in segs:
            W, row0, levels, first = want[s["topic"]]
            assert (s["W"], s["row0"], s["levels"]) == (W, row0, levels)
            assert s["pw"] == min(PIECE, max(LINE, NODES * W // LINE * LINE)) and s["pw"] % LINE == 0
            assert s["first"][:levels + 1] == first[:levels + 1]
            runs = sorted((c["node_begin"], c["node_end"]) for c in whole if c["topic"] == s["topic"])
            assert runs[0][0] == first[0] and runs[-1][1] == first[1]
            assert all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
            assert s["piece0"] == piece_at and s["blk0"] == blk_at
            lo = row0 + (first[0] - s["nbase"]) * W
            hi = row0 + (first[levels] - s["nbase"]) * W
            assert hi > lo
            at = lo
            while at < hi:
                p = next(it)
                piece_at += 1
                assert p["w0"] == at and 0 < p["nw"] <= s["pw"]
                assert at == lo or at % LINE == 0
                at += p["nw"]
                assert at == hi or at % LINE == 0
                assert p["node0"] == s["nbase"] + (p["w0"] - row0) // W and p["off0"] == (p["w0"] - row0) % W
            assert at == hi
            blk_at += -(-(first[levels] - first[0]) // BLOCK)
        assert next(it, None) is None and blocks == blk_at
    assert launches > 0


def test_staggered_and_sharded_windows_have_no_segments(monkeypatch):
    rng = np.random.default_rng(5201)
    n, parents, roots, msgs = case(rng)
    starts = rng.integers(0, 4, size=msgs.shape[0]).astype(np.uint32)
    p = make_plan(monkeypatch, True, parents, roots, msgs, starts)
    assert all(p.fill(q) == (0, [], []) for q in range(len(p.get(PL.ROUND_KIND))))
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_CHAIN_FILL_BYTES", "0")
    monkeypatch.setenv("PSAMD_CHAIN_FILL_ROW_WORDS", "0")
    for rank in range(2):
        d = PL.Plan(parents, roots, world=2, rank=rank, plan={"flood": 0})
        d.window(msgs)
        assert all(d.fill(q) == (0, [], []) for q in range(len(d.get(PL.ROUND_KIND))))
