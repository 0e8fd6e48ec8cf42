"""Chain launches as reach + fill (k_fill_reach, k_fill_rows).

In a single-start window every reached node's row is its topic root's seeded
row and an unreached node's row is zeros, so a chain launch's whole rows can
be written as one metadata pass (reach, generation stamps, counters) and one
front-to-back fill of each topic's contiguous node range.  Every case runs on
an engine with the fill forced for every eligible chain launch
(PSAMD_CHAIN_FILL_BYTES=0, PSAMD_CHAIN_FILL_ROW_WORDS=0: any size, any row
width) and on one with it off (PSAMD_CHAIN_FILL=0, the chain kernel), and is checked against the restatement (or_disseminate): every
ps_stats counter and per-round array but the byte model's (edge_words is the
parent words read, which the fill changes on purpose; expand_bytes follow it)
and the timings, the seen digest, and sampled delivered sets bit for bit.
ps_chain_fill_launches says which path ran.
"""
import threading

import numpy as np
import pytest

import oracle as O
import psengine as PE
from psengine import workloads as WL
from test_gpu_pair import make_case, oracle_hops, random_tree

pytestmark = pytest.mark.gpu

SKIP = {"edge_words", "expand_bytes", "expand_bytes_per_round", "run_ms", "expand_ms", "host_ms",
        "expand_ms_per_round", "reserved2"}


def stats_key(st):
    return tuple((k, tuple(v) if isinstance(v, list) else v) for k, v in sorted(st.as_dict().items())
                 if k not in SKIP)


def engine(monkeypatch, fill, n, nt, **kw):
    monkeypatch.setenv("PSAMD_AB", "1")
    monkeypatch.setenv("PSAMD_CHAIN_FILL_BYTES", "0")
    monkeypatch.setenv("PSAMD_CHAIN_FILL_ROW_WORDS", "0")
    monkeypatch.setenv("PSAMD_CHAIN_FILL", "1" if fill else "0")
    kw.setdefault("plan", {"flood": 0})
    return PE.Engine(n, nt, **kw)


def run_windows(monkeypatch, fill, n, topics, lives, batches, starts=None, **kw):
    """One window per (live mask, batch); per window the stats key, the digest
    and the delivered sets of its first, middle and last message."""
    out = []
    with engine(monkeypatch, fill, n, len(topics), **kw) as eng:
        for t, (root, parent) in enumerate(topics):
            eng.set_tree(t, root, parent)
        for live, msg_topics in zip(lives, batches):
            eng.set_live(live)
            first = eng.publish(msg_topics, starts)
            st = eng.run()
            m = len(msg_topics)
            deliv = [eng.delivered(first + i).tolist() for i in sorted({0, m // 2, m - 1})]
            out.append((stats_key(st), eng.seen_digest(), deliv, list(st.round_kernel)[: st.rounds + 1]))
        fills = eng.chain_fill_launches()
    return out, fills


def both(monkeypatch, n, topics, lives, batches, expect_fill=True, **kw):
    """Fill on against fill off, window by window; the oracle's deliveries and
    delivered sets; the dispatch counter."""
    on, fills = run_windows(monkeypatch, True, n, topics, lives, batches, **kw)
    off, fills_off = run_windows(monkeypatch, False, n, topics, lives, batches, **kw)
    assert fills_off == 0
    assert (fills > 0) == expect_fill, fills
    for w, (a, b) in enumerate(zip(on, off)):
        assert a[0] == b[0], (w, [x for x in zip(a[0], b[0]) if x[0] != x[1]])
        assert a[1] == b[1], w
        assert a[2] == b[2], w
        assert a[3] == b[3], w  # the same round kinds: the plan is untouched
        if kw.get("starts") is None:
            assert PE.K_CHAIN in a[3], a[3]
            exp = oracle_hops(topics, lives[w])
            mt = batches[w]
            assert dict(a[0])["deliveries"] == sum(int((exp[t] != 0xFF).sum()) * int((mt == t).sum()) for t in exp)
            for i, got in zip(sorted({0, len(mt) // 2, len(mt) - 1}), a[2]):
                assert got == (exp[int(mt[i])] != 0xFF).astype(np.uint8).tolist(), (w, i)
    return on, fills


def msgs_for_widths(widths, rng):
    """A batch giving topic t a row of widths[t] words (64 * W - 5 messages)."""
    mt = np.concatenate([np.full(64 * w - 5, t, dtype=np.uint32) for t, w in enumerate(widths)])
    rng.shuffle(mt)
    return mt


def test_row_widths(monkeypatch):
    """Rows of 1, 3 and 15 words (odd: rows 8-B aligned only), 16, 17, 64, 65
    (padded to 66), 330 (cfg3's hot topic: rows straddle the 16-KB pieces) and
    769 words: the last is wider than the chain's stage, so it stays on the
    chain kernel's column slices while the others are filled beside it in the
    same launch slot."""
    rng = np.random.default_rng(4101)
    n = 2500
    widths = [1, 3, 15, 16, 17, 64, 65, 330, 769]
    topics = []
    for t in range(len(widths)):
        root = 10 + t
        topics.append((root, random_tree(rng, n, root, 3)))
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[[r for r, _ in topics]] = 1
    _, fills = both(monkeypatch, n, topics, [live], [msgs_for_widths(widths, rng)], msg_window=1 << 16)
    assert fills >= 2


@pytest.mark.parametrize("seed", range(4))
def test_random_trees_dead_peers(monkeypatch, seed):
    """Random trees, ~15 % dead peers at every depth: internal nodes of a
    launch's first level, mid levels and leaves, and a dead child of every
    root (its subtree is cut in an earlier launch: the later launches' parents
    were never reached)."""
    rng = np.random.default_rng(4200 + seed)
    n, topics, live = make_case(rng, 2000, 6000)
    mt = rng.integers(0, len(topics), size=int(rng.integers(1, 900))).astype(np.uint32)
    both(monkeypatch, n, topics, [live], [mt])


def test_level_ranges(monkeypatch):
    """Topics of different depth in one launch: a path-like deep tree, a
    shallow one (fewer levels than the launch), a root-only topic, a topic
    with no message in the window, and level ranges far shorter than a piece;
    a second window publishes to the idle topic and not to another."""
    rng = np.random.default_rng(4301)
    n = 2000
    none = np.full(n, O.NONE, dtype=np.uint32)
    shallow = none.copy()
    shallow[100:140] = 5  # depth 1 under root 5
    shallow[140:150] = 100  # depth 2
    topics = [(1, random_tree(rng, n, 1, 2)), (5, shallow), (7, none.copy()), (9, random_tree(rng, n, 9, 4)),
              (11, random_tree(rng, n, 11, 3))]
    live = np.ones(n, dtype=np.uint8)
    b0 = np.array([0] * 70 + [1] * 130 + [2] * 3 + [3] * 700, dtype=np.uint32)  # topic 4 idle
    b1 = np.array([0] * 70 + [4] * 200 + [2] * 3 + [1] * 10, dtype=np.uint32)  # topic 3 idle
    both(monkeypatch, n, topics, [live, live], [b0, b1])


def test_cut_subtree_spans_pieces_and_live_changes(monkeypatch):
    """330-word rows (2.6 KB): a dead node high in a launch's first level cuts
    a subtree whose zero rows span several 16-KB pieces; then the live mask
    changes between windows (the cut moves, the old one heals), and changes
    back."""
    rng = np.random.default_rng(4401)
    n = 3000
    parent = random_tree(rng, n, 0, 3)
    topics = [(0, parent)]
    depth = np.zeros(n, dtype=np.int64)
    order = [0]
    kids = {}
    for c, p in enumerate(parent):
        if p != O.NONE:
            kids.setdefault(int(p), []).append(c)
    for u in order:
        for c in kids.get(u, []):
            depth[c] = depth[u] + 1
            order.append(c)
    lives = []
    for d in (5, 2, 5):  # a node of a later launch's first level; of the first launch; back
        live = np.ones(n, dtype=np.uint8)
        cand = [u for u in order if depth[u] == d and len(kids.get(u, [])) >= 2]
        live[cand[0]] = 0
        live[[u for u in order if depth[u] == depth.max()][0]] = 0  # and a leaf
        lives.append(live)
    mt = np.zeros(64 * 330 - 9, dtype=np.uint32)
    both(monkeypatch, n, topics, lives, [mt, mt[:-40], mt], msg_window=1 << 16)


def test_generation_wrap(monkeypatch):
    """270 windows on a tiny engine: the generation byte wraps; every window's
    counters and digest equal the chain kernel's."""
    rng = np.random.default_rng(4501)
    n = 300
    topics = [(0, random_tree(rng, n, 0, 2))]
    live = (rng.random(n) > 0.05).astype(np.uint8)
    live[0] = 1
    out = []
    for fill in (True, False):
        res = []
        with engine(monkeypatch, fill, n, 1) as eng:
            eng.set_tree(0, 0, topics[0][1])
            eng.set_live(live)
            for w in range(270):
                eng.publish(np.zeros(1 + w % 70, dtype=np.uint32))
                st = eng.run()
                res.append((stats_key(st), eng.seen_digest()))
            fills = eng.chain_fill_launches()
        assert (fills >= 270) == fill, fills
        out.append(res)
    assert out[0] == out[1]


def vary_counts(msg_topics, i):
    keep = np.ones(msg_topics.shape[0], dtype=bool)
    for t in np.unique(msg_topics):
        idx = np.nonzero(msg_topics == t)[0]
        drop = (i * 7 + int(t)) % ((idx.shape[0] - 1) % 64 + 1)
        if drop:
            keep[idx[-drop:]] = False
    return msg_topics[keep]


def test_pipelined_deep_windows(monkeypatch):
    """8 pipelined deep windows (alternating row sets, overlapped prefixes),
    each with other message counts per topic: the fill engine's windows equal
    the blocking runs of the chain kernel, and as many windows overlapped as
    with the fill off."""
    wl = WL.cfg3(200_000, 16, 5000)
    rng = np.random.default_rng(4601)
    live = (rng.random(wl.n_peers) >= 0.03).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    batches = [vary_counts(wl.msg_topics, i) for i in range(8)]
    res = {}
    for mode in ("off-blocking", "off-pipelined", "on-pipelined"):
        e = engine(monkeypatch, mode.startswith("on"), wl.n_peers, len(wl.topics), seed=wl.seed,
                   plan={"overlap_min_bytes": 0})
        WL.build_engine_topics(e, wl)
        e.set_live(live)
        keys = []
        if mode.endswith("pipelined"):
            for i in range(8):
                e.publish(batches[i])
                e.run_async()
                if i:
                    keys.append(stats_key(e.wait()))
            keys.append(stats_key(e.wait()))
        else:
            for i in range(8):
                e.publish(batches[i])
                keys.append(stats_key(e.run()))
        res[mode] = (keys, e.seen_digest(), e.overlapped_windows(), e.chain_fill_launches())
        e.close()
    drop = ("overlapped", "prefix_rounds")  # (scheduling diagnostics: blocking runs have none)
    strip = lambda keys: [tuple(kv for kv in k if kv[0] not in drop) for k in keys]  # noqa: E731
    assert res["on-pipelined"][0] == res["off-pipelined"][0]
    assert strip(res["on-pipelined"][0]) == strip(res["off-blocking"][0])
    assert res["on-pipelined"][1] == res["off-pipelined"][1] == res["off-blocking"][1]
    assert res["off-pipelined"][2] >= 5
    assert res["on-pipelined"][2] == res["off-pipelined"][2]
    assert res["on-pipelined"][3] >= 8 and res["off-pipelined"][3] == 0 and res["off-blocking"][3] == 0


@pytest.mark.parametrize("case", ["eager-seen", "hop-record", "staggered"])
def test_fallbacks(monkeypatch, case):
    """Eager seen rows (PS_F_NO_LAZY_SEEN), hop recording and staggered starts
    keep the chain kernel: the fill does not run, and nothing changes."""
    rng = np.random.default_rng(4701)
    n, topics, live = make_case(rng, 1500, 3000)
    mt = rng.integers(0, len(topics), size=600).astype(np.uint32)
    kw = {}
    if case == "eager-seen":
        kw["flags"] = PE.F_NO_LAZY_SEEN
    elif case == "hop-record":
        kw["record_hops"] = True
    else:
        kw["starts"] = rng.integers(0, 5, size=mt.shape[0]).astype(np.uint32)
    both(monkeypatch, n, topics, [live], [mt], expect_fill=False, **kw)


def test_fallback_two_loopback_ranks(monkeypatch):
    """A sharded (2-rank loopback) engine keeps its chain launches: the fill
    does not run, and the ranks' deliveries add up to the oracle's."""
    rng = np.random.default_rng(4801)
    n, root = 3000, 4
    parent = random_tree(rng, n, root, 3)
    live = np.ones(n, dtype=np.uint8)
    lb = PE.Loopback(2)
    engines = [engine(monkeypatch, True, n, 1) for _ in range(2)]
    try:
        for k, e in enumerate(engines):
            e.dist_init_loopback(lb, k, PE.PART_PEER)
            e.set_tree(0, root, parent)
            e.publish(np.zeros(50))
        stats, errs = [None, None], []

        def go(k):
            try:
                stats[k] = engines[k].run()
            except Exception as ex:  # noqa: BLE001
                errs.append(ex)

        th = [threading.Thread(target=go, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in th) and not errs, errs
        assert [e.chain_fill_launches() for e in engines] == [0, 0]
        exp = oracle_hops([(root, parent)], live)[0]
        assert sum(s.deliveries for s in stats) == 50 * int((exp != 0xFF).sum())
    finally:
        for e in engines:
            e.close()
        lb.close()
