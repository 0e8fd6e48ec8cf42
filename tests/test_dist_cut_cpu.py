"""ps_dist_cut without a GPU: the header and the binding, the argument checks
that need no engine, the reference of a rank's share (tests/dist_cut_ref.py)
against the one-rank cut reference and its identities, and -- by name -- what
the shapes of tests/test_gpu_dist_cut.py rely on: where the cut points lie,
whose parent is remote, whose subtree spans ranks.  (An engine needs a device:
everything that needs one is in tests/test_gpu_dist_cut.py.)"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import cut_ref as CR
import dist_cut_ref as XC
import dist_ref as DR
import dist_report_ref as XR
import psengine as PE
from test_dist_report_cpu import N_MSGS, SHAPES, WORLDS, shape

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
FILL = 0xABABABABABABABAB


# ---- the header and the binding ---------------------------------------------------

def test_header_declares_the_call():
    with open(HEADER) as f:
        text = f.read()
    line = ("int ps_dist_cut(ps_engine* e, const uint32_t* topic, size_t n,\n"
            "                uint64_t* missed_out, uint64_t* cuts_out,\n"
            "                uint64_t* orphaned_out, uint64_t* lost_out);")
    assert line in text
    assert "#define PS_ABI_VERSION 5" in " ".join(text.split())
    flat = " ".join(text.replace("\n *", " ").split())
    for phrase in ("This rank's share of ps_peer_cut", "COLLECTIVE whenever n > 0", "may differ between the ranks",
                   "PS_REPORT_CUT is not answered across ranks"):  # (ps_dist_report's sentence stays)
        assert phrase in flat, phrase


def test_binding_matches_the_header():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert protos["ps_dist_cut"][1] is C.c_int and protos["ps_dist_cut"][2] == protos["ps_peer_cut"][2]
    assert PE.load().ps_dist_cut.restype is C.c_int
    assert hasattr(PE.Engine, "dist_cut")
    assert PE.load().ps_abi_version() == 5 and PE.ABI_VERSION == 5
    assert PE.REPORT_DIST == 0x7  # the report's sections stay: the cut is a call of its own


def test_arguments_are_checked_before_the_engine_is_touched():
    """PS_E_INVAL with every array untouched; any non-NULL engine pointer will
    do for the checks behind the first (4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    a = [np.full(8, FILL, dtype=np.uint64) for _ in range(4)]
    p = [x.ctypes.data_as(U64P) for x in a]
    assert lib.ps_dist_cut(None, tp, 1, *p) == -1  # no engine
    assert lib.ps_dist_cut(h, None, 1, *p) == -1  # n > 0 without topic
    assert lib.ps_dist_cut(h, tp, 1, None, None, None, None) == -1  # all four NULL
    assert lib.ps_dist_cut(h, None, 0, None, None, None, None) == -1  # ... at n == 0 too
    assert all((x == FILL).all() for x in a)


# ---- the reference of a rank's share ----------------------------------------------

@functools.lru_cache(maxsize=None)
def shape_values(name):
    trees, roots, live = shape(name)
    n = trees[0].shape[0]
    return tuple(XC.topic_values(n, live, r, N_MSGS, t) for t, r in zip(trees, roots))


@functools.lru_cache(maxsize=None)
def shape_whole(name):
    trees, roots, live = shape(name)
    return CR.window_cut(trees[0].shape[0], live, [(r, N_MSGS, t) for t, r in zip(trees, roots)])


@pytest.mark.parametrize("subtree", [False, True])
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", SHAPES)
def test_shares_sum_to_the_one_rank_cut(name, world, subtree):
    trees, roots, live = shape(name)
    n = trees[0].shape[0]
    topics = [(r, N_MSGS, t) for t, r in zip(trees, roots)]
    owners = XR.owners_of(trees, roots, world, subtree, split_depth=2 if subtree else 0)
    shares = XC.rank_cuts(n, live, topics, owners, world, values=shape_values(name))
    want = shape_whole(name)
    got = XC.total(shares)
    for k, w in zip(XC.NAMES, want[:4]):
        assert got[k].dtype == np.uint64 and np.array_equal(got[k], w), (k, world)
    if world == 1:  # world 1's share is the whole answer
        for k, w in zip(XC.NAMES, want[:4]):
            assert np.array_equal(shares[0][k], w), k
    # identities 1 and 2 of ps_peer_cut on the ranks' sum
    assert int(got["missed"].sum()) == want[5] - want[4]
    assert int(got["lost"].sum()) == int(got["missed"].sum())
    # nobody reports a node it does not own: per topic alone, a rank's arrays
    # are zero outside its peers
    for i, t in enumerate(topics):
        alone = XC.rank_cuts(n, live, [t], [owners[i]], world, values=[shape_values(name)[i]])
        for r in range(world):
            for k in XC.NAMES:
                assert not alone[r][k][owners[i] != r].any(), (k, r)


@pytest.mark.parametrize("name", SHAPES)
def test_an_all_live_mask_cuts_nothing(name):
    """Identity 4: every peer alive, every array zero on every rank."""
    trees, roots, _ = shape(name)
    n = trees[0].shape[0]
    live = np.ones(n, dtype=np.uint8)
    topics = [(r, N_MSGS, t) for t, r in zip(trees, roots)]
    for world in (1, 3):
        for s in XC.rank_cuts(n, live, topics, XR.owners_of(trees, roots, world), world):
            assert not any(a.any() for a in s.values())


def test_an_idle_topic_adds_nothing():
    trees, roots, live = shape("tiny_beside_large")
    n = trees[0].shape[0]
    topics = [(roots[0], 2, trees[0]), (roots[1], 0, trees[1]), (roots[2], 5, trees[2])]
    owners = XR.owners_of(trees, roots, 5)
    got = XC.total(XC.rank_cuts(n, live, topics, owners, 5))
    want = CR.window_cut(n, live, topics)
    for k, w in zip(XC.NAMES, want[:4]):
        assert np.array_equal(got[k], w), k
    alone = XC.total(XC.rank_cuts(n, live, [topics[1]], [owners[1]], 5))
    assert not any(a.any() for a in alone.values())


# ---- what the GPU cases rely on -----------------------------------------------------

def cut_facts(parent, root, live, own, c=N_MSGS):
    """Where one topic's cut points lie: the cut points, those whose parent is
    on another rank, those whose T(u) has a node on another rank, the cut
    points per rank, and the nodes with a miss that are no cut point."""
    n = parent.shape[0]
    missed, cuts, orphaned, _ = CR.topic_cut(n, root, live, c, parent)[:4]
    par = np.asarray(parent, dtype=np.uint32).copy()
    par[root] = DR.NONE
    kids = DR.children_of(par)
    at = [int(u) for u in np.nonzero(cuts)[0]]

    def spans(u):
        todo, ranks = [u], set()
        while todo:
            x = todo.pop()
            ranks.add(int(own[x]))
            todo.extend(kids[x])
        return len(ranks) > 1

    return {"at": at, "remote": [u for u in at if own[par[u]] != own[u]], "spans": [u for u in at if spans(u)],
            "per_rank": np.bincount(own[at], minlength=int(own.max()) + 1).tolist() if at else [],
            "missing_not_cut": int(((missed > 0) & (cuts == 0)).sum()), "orphaned": orphaned, "parent": par}


def test_row_width_case_has_cut_points_of_every_kind():
    parent, root, live = DR.row_width_case()
    own = XR.owners_of([parent], [root], 3)[0]
    f = cut_facts(parent, root, live, own)
    assert len(f["at"]) == 26 and len(f["remote"]) == 17  # 17 behind a remote parent, 9 behind a local one
    assert len(f["spans"]) == 14  # T(u) lies on several ranks
    assert f["per_rank"] == [6, 10, 10]  # cut points on every rank
    assert f["missing_not_cut"] == 256  # a miss under a parent that misses too: no cut point


def fan_live(deg, world, hub_alive):
    parent, root, hub, facts = DR.wide_fan(deg, world)
    live = np.ones(parent.shape[0], dtype=np.uint8)
    kids = facts["kids"]
    live[[kids[0], kids[63], kids[64], kids[-1]]] = 0
    live[hub] = hub_alive
    return parent, root, hub, facts, live


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("deg", [65, 129])
def test_wide_fan_cuts_under_one_remote_parent(deg, world):
    """Hub alive: the dead children are the cut points, all under the hub, all
    on the rank that holds 65 or more of its children and not the hub's."""
    parent, root, hub, facts, live = fan_live(deg, world, True)
    own = XR.owners_of([parent], [root], world)[0]
    f = cut_facts(parent, root, live, own)
    assert len(f["at"]) == (3 if deg == 65 else 4)
    assert all(f["parent"][u] == hub for u in f["at"]) and f["remote"] == f["at"]
    assert all(own[u] == facts["rank"] for u in f["at"]) and facts["on_rank"] >= 65


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("deg", [65, 129])
def test_wide_fan_dead_hub_is_the_one_cut_point_under_the_root(deg, world):
    """Hub dead: the hub alone, the root's child, everything behind it spread
    over the ranks; the root is on another rank but at (65, 2) -- there a
    root's fullness travels as c_t although its k word is 0."""
    parent, root, hub, facts, live = fan_live(deg, world, False)
    own = XR.owners_of([parent], [root], world)[0]
    f = cut_facts(parent, root, live, own)
    assert f["at"] == [hub] and f["parent"][hub] == root and f["spans"] == [hub]
    assert f["orphaned"][hub] == (448 if deg == 65 else 463)
    assert (own[hub] != own[root]) == ((deg, world) != (65, 2))
    assert (f["remote"] == [hub]) == ((deg, world) != (65, 2))


def path_dead(n, world=2):
    """The first peer from n // 2 on whose parent lies on another rank."""
    own = DR.owner_peer(np.arange(n), world)
    return next(d for d in range(n // 2, n - 1) if own[d] != own[d - 1])


@pytest.mark.parametrize("n", [40, 300])
def test_path_dead_peer_has_a_remote_parent(n):
    parent, root = DR.path(n)
    own = XR.owners_of([parent], [root], 2)[0]
    for d, remote in ((path_dead(n), True), (n // 2, False)):  # (n // 2: the parent is local)
        live = np.ones(n, dtype=np.uint8)
        live[d] = 0
        f = cut_facts(parent, root, live, own)
        assert f["at"] == [d] and (f["remote"] == [d]) == remote and (own[d] != own[d - 1]) == remote
        assert f["orphaned"][d] == n - 1 - d and f["spans"] == [d]


@pytest.mark.parametrize("world,split,remote", [(2, 1, [0, 0, 0]), (2, 2, [2, 0, 0]), (4, 2, [2, 0, 0]), (4, 3, [2, 1, 0])])
def test_split_case_remote_parent_cut_points(world, split, remote):
    """Split level 1: no cut point has a remote parent -- the downward words
    travel and decide nothing; levels 2 and 3: one or two on some topics."""
    trees, roots, live = DR.split_case()
    owners = XR.owners_of(trees, roots, world, True, split)
    got = []
    for t, r, own in zip(trees, roots, owners):
        f = cut_facts(t, r, live, own)
        assert len(f["at"]) >= 60
        got.append(len(f["remote"]))
        par = f["parent"]
        kids = np.nonzero(own >= 0)[0]
        kids = kids[kids != r]
        assert (own[kids] != own[par[kids]]).any()  # words do travel
    assert got == remote


@pytest.mark.parametrize("world", [5, 16])
def test_tiny_beside_large_has_empty_ranks_an_idle_topic_and_a_lonely_root(world):
    trees, roots, facts = DR.tiny_beside_large(400, world)
    owners = XR.owners_of(trees, roots, world)
    assert any(not (owners[0] == r).any() for r in range(world))  # a rank that owns nothing of a topic
    r2 = facts["lonely_root"]
    assert np.nonzero(owners[2] == owners[2][r2])[0].tolist() == [r2]  # every child of that root reads c_t off a remote root
    n = trees[0].shape[0]
    live = np.ones(n, dtype=np.uint8)
    live[np.random.default_rng(world).choice(n, size=20, replace=False)] = 0
    live[roots] = 1
    f = cut_facts(trees[1], roots[1], live, owners[1])
    assert f["remote"] and f["spans"]  # the large tree's cut points: remote parents, subtrees across ranks
