"""ps_dist_report without a GPU: the header and the binding, the argument checks
that need no engine, the reference of a rank's share (tests/dist_report_ref.py)
against the one-rank report reference and its closed forms, and -- by name --
what the shapes of tests/test_gpu_dist_report.py rely on.  (An engine needs a
device: everything that needs one is in tests/test_gpu_dist_report.py.)"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import dist_ref as DR
import dist_report_ref as XR
import load_ref as LR
import psengine as PE
import report_ref as RR

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
FILL = 0xABABABABABABABAB
SIZE = C.sizeof(PE.Report)
WORLDS = (1, 2, 3, 4, 16)


def report(n=8, only=None):
    arrays = {k: np.full(n, FILL, dtype=np.uint64) for k in RR.NAMES}
    rep = PE.Report()
    for k, a in arrays.items():
        if only is None or k in only:
            setattr(rep, k, a.ctypes.data_as(U64P))
    return arrays, rep


def untouched(arrays):
    return all((a == FILL).all() for a in arrays.values())


# ---- the header and the binding ---------------------------------------------------

def test_header_declares_the_call():
    with open(HEADER) as f:
        text = f.read()
    for line in ("#define PS_REPORT_DIST 0x7u",
                 "int ps_dist_report(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what,\n"
                 "                   const ps_report* out, size_t out_size);"):
        assert line in text, line
    assert "#define PS_ABI_VERSION 5" in " ".join(text.split())
    flat = " ".join(text.replace("\n *", " ").split())
    for phrase in ("COLLECTIVE, as ps_run is", "PS_REPORT_HOPS alone exchange nothing", "PS_REPORT_CUT is not answered across ranks"):
        assert phrase in flat, phrase


def test_binding_matches_the_header():
    assert PE.REPORT_DIST == 0x7 == PE.REPORT_LOAD | PE.REPORT_HOPS | PE.REPORT_DOWNSTREAM == XR.DIST
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert protos["ps_dist_report"][1] is C.c_int and protos["ps_dist_report"][2] == protos["ps_peer_report"][2]
    assert PE.load().ps_dist_report.restype is C.c_int
    assert hasattr(PE.Engine, "dist_report")
    assert PE.load().ps_abi_version() == 5 and PE.ABI_VERSION == 5


def test_arguments_are_checked_before_the_engine_is_touched():
    """PS_E_INVAL with every array untouched; any non-NULL engine pointer will
    do for the checks behind the first (4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    a, rep = report()
    assert lib.ps_dist_report(None, tp, 1, PE.REPORT_DIST, C.byref(rep), SIZE) == -1
    assert lib.ps_dist_report(h, tp, 1, 0, C.byref(rep), SIZE) == -1  # what == 0
    for what in (PE.REPORT_CUT, PE.REPORT_ALL, PE.REPORT_CUT | PE.REPORT_LOAD, 0x10, 0x17):  # a bit outside PS_REPORT_DIST
        assert lib.ps_dist_report(h, tp, 1, what, C.byref(rep), SIZE) == -1, what
    assert lib.ps_dist_report(h, tp, 1, PE.REPORT_DIST, C.byref(rep), SIZE - 8) == -1  # wrong out_size
    assert lib.ps_dist_report(h, tp, 1, PE.REPORT_DIST, None, SIZE) == -1  # no out
    assert lib.ps_dist_report(h, None, 1, PE.REPORT_DIST, C.byref(rep), SIZE) == -1  # n > 0 without topic
    assert untouched(a)
    # a selected section whose pointers are all NULL
    a, rep = report(only=("recv", "sent", "below"))
    assert lib.ps_dist_report(h, tp, 1, PE.REPORT_LOAD | PE.REPORT_HOPS, C.byref(rep), SIZE) == -1
    assert untouched(a)


# ---- the reference of a rank's share ----------------------------------------------

N_MSGS = 3


@functools.lru_cache(maxsize=None)
def shape(name):
    """(trees, roots, live) of a named shape; the same trees for every world."""
    rng = np.random.default_rng(11)
    if name == "random_tree":
        root = 17
        trees, roots = [DR.random_tree(rng, 300, root)], [root]
    elif name == "wide_fan":
        parent, root, _, _ = DR.wide_fan(65, 2)
        trees, roots = [parent], [root]
    elif name == "tiny_beside_large":
        trees, roots, _ = DR.tiny_beside_large(400, 16)
    elif name == "path":
        parent, root = DR.path(40)
        trees, roots = [parent], [root]
    else:
        trees, roots, live = DR.split_case()
        return trees, roots, live
    n = trees[0].shape[0]
    live = (rng.random(n) > 0.08).astype(np.uint8)
    live[roots] = 1
    return trees, roots, live


@functools.lru_cache(maxsize=None)
def shape_values(name):
    trees, roots, live = shape(name)
    n = trees[0].shape[0]
    return tuple(XR.topic_values(n, live, r, N_MSGS, t) for t, r in zip(trees, roots))


SHAPES = ("random_tree", "wide_fan", "tiny_beside_large", "path", "split_case")


@pytest.mark.parametrize("subtree", [False, True])
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", SHAPES)
def test_shares_sum_to_the_one_rank_report(name, world, subtree):
    trees, roots, live = shape(name)
    n = trees[0].shape[0]
    topics = [(r, N_MSGS, t) for t, r in zip(trees, roots)]
    owners = XR.owners_of(trees, roots, world, subtree, split_depth=2 if subtree else 0)
    shares = XR.rank_reports(n, live, topics, owners, world, values=shape_values(name))
    want = RR.window_report(n, live, [(r, c, t, None) for r, c, t in topics], XR.DIST)
    got = XR.total(shares)
    assert set(got) == set(want) == set(XR.names_of(XR.DIST))
    for k in want:
        assert got[k].dtype == np.uint64 and np.array_equal(got[k], want[k]), (k, world)
    if world == 1:  # world 1's share is the whole report
        for k in want:
            assert np.array_equal(shares[0][k], want[k]), k
    # nobody reports a node it does not own: per topic alone, a rank's arrays
    # are zero outside its peers
    for i, t in enumerate(topics):
        alone = XR.rank_reports(n, live, [t], [owners[i]], world, values=[shape_values(name)[i]])
        for r in range(world):
            for k in ("recv", "sent", "below", "carried"):
                assert not alone[r][k][owners[i] != r].any(), (k, r)


def test_an_idle_topic_adds_nothing_and_keeps_its_row():
    trees, roots, live = shape("tiny_beside_large")
    n = trees[0].shape[0]
    topics = [(roots[0], 2, trees[0]), (roots[1], 0, trees[1]), (roots[2], 5, trees[2])]
    owners = XR.owners_of(trees, roots, 5)
    shares = XR.rank_reports(n, live, topics, owners, 5)
    want = RR.window_report(n, live, [(r, c, t, None) for r, c, t in topics], XR.DIST)
    got = XR.total(shares)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert not got["nodes"][1].any() and got["nodes"][0].any() and got["nodes"][2].any()


@pytest.mark.parametrize("n", [40, 300])
def test_path_closed_forms(n):
    """below of the node at depth d is n - 1 - d, on its owner only; the hop
    columns clamp at PS_MAX_ROUNDS - 1 while below stays exact."""
    parent, root = DR.path(n)
    live = np.ones(n, dtype=np.uint8)
    owners = XR.owners_of([parent], [root], 2)
    shares = XR.rank_reports(n, live, [(root, 2, parent)], owners, 2)
    for r in range(2):
        want = np.where(owners[0] == r, n - 1 - np.arange(n), 0)
        assert np.array_equal(shares[r]["below"], want.astype(np.uint64))
    tot = XR.total(shares)
    assert tot["nodes"][0, :min(n, 255)].tolist() == [0] + [1] * (min(n, 255) - 1)
    assert tot["nodes"][0, 255] == max(0, n - 255)
    assert tot["carried"][root] == 2 * (n - 1) and tot["below"].sum() == n * (n - 1) // 2


@pytest.mark.parametrize("name", SHAPES)
def test_carried_at_a_root_is_the_topic_s_deliveries(name):
    trees, roots, live = shape(name)
    n = trees[0].shape[0]
    for t, r in zip(trees, roots):
        _, _, deliveries = LR.topic_load(n, r, live, N_MSGS, parent=t)
        owners = XR.owners_of([t], [r], 3)
        shares = XR.rank_reports(n, live, [(r, N_MSGS, t)], owners, 3)
        own_root = int(owners[0][r])
        assert shares[own_root]["carried"][r] == deliveries
        assert all(shares[q]["carried"][r] == 0 for q in range(3) if q != own_root)


# ---- what the GPU cases rely on -----------------------------------------------------

@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("deg", [65, 129])
def test_wide_fan_has_65_children_behind_one_remote_parent(deg, world):
    parent, root, hub, facts = DR.wide_fan(deg, world)
    own = DR.owner_peer(np.arange(parent.shape[0]), world)
    kids = np.nonzero(parent == hub)[0]
    assert len(kids) == deg and facts["rank"] != own[hub]
    assert int((own[kids] == facts["rank"]).sum()) >= 65  # more than a wave of siblings push into one slot


@pytest.mark.parametrize("world", [5, 16])
def test_tiny_beside_large_has_a_rank_without_topic_0_and_a_lonely_root(world):
    trees, roots, facts = DR.tiny_beside_large(400, world)
    owners = XR.owners_of(trees, roots, world)
    assert any(not (owners[0] == r).any() for r in range(world))  # a rank that owns nothing of a topic
    r2 = facts["lonely_root"]
    mine = np.nonzero(owners[2] == owners[2][r2])[0]
    assert mine.tolist() == [r2]  # a root's owner that owns only the root
    assert (trees[2] == r2).sum() == 12


@pytest.mark.parametrize("world,split", [(2, 1), (2, 2), (4, 2), (4, 3)])
def test_split_case_crosses_ranks_at_the_split_level_only(world, split):
    trees, roots, _ = DR.split_case()
    owners = XR.owners_of(trees, roots, world, True, split)
    some = False
    for t, r, own in zip(trees, roots, owners):
        par = t.copy()
        par[r] = DR.NONE
        lv = DR.bfs_levels(par, r)
        kids = np.nonzero((lv >= 1))[0]
        crossing = kids[own[kids] != own[par[kids]]]
        assert (lv[crossing] == split).all()  # every other level has no cross-rank edge
        assert int(lv.max()) > split
        some |= crossing.size > 0
    assert some
    # a peer's nodes of two topics lie on different ranks: a rank's share is not
    # "the reference masked by one owner array"
    assert ((owners[0] != owners[1]) & (owners[0] >= 0) & (owners[1] >= 0)).any()
