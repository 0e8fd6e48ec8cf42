"""ps_dist_blame without a GPU: the header and the binding, the argument checks
that need no engine, the reference of a rank's share (tests/dist_blame_ref.py)
against the one-rank blame reference and against dist_cut_ref on the same
window, and -- by name -- what the shapes of tests/test_gpu_dist_blame.py rely
on: records whose cut point lies on another rank, and records whose path up to
it changes rank twice or more.  (An engine needs a device: everything that
needs one is in tests/test_gpu_dist_blame.py.)"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import blame_ref as BR
import dist_blame_ref as XB
import dist_cut_ref as XC
import dist_ref as DR
import dist_report_ref as XR
import psengine as PE
from test_blame_cpu import lent, lent_untouched
from test_dist_cut_cpu import fan_live, path_dead
from test_dist_report_cpu import N_MSGS, SHAPES, WORLDS, shape
from test_gpu_downstream import star

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


# ---- the header and the binding ---------------------------------------------------

def test_header_declares_the_call():
    with open(HEADER) as f:
        text = f.read()
    assert "int ps_dist_blame(ps_engine* e, const uint32_t* topic, size_t n,\n" in text
    decl = text[text.index("int ps_dist_blame("):]
    decl = decl[:decl.index(";") + 1]
    for name in ("rec_off_out", "rec_peer_out", "rec_cut_peer_out", "rec_hop_out", "rec_cut_hop_out", "rec_missed_out"):
        assert re.search(r"const uint(32|64)_t\*\* " + name + r"[,;) ]", decl), name
    assert "uint64_t* total_out);" in decl
    assert "#define PS_ABI_VERSION 5" in " ".join(text.split())
    flat = " ".join(text.replace("\n *", " ").split())
    for phrase in ("This rank's share of ps_topic_blame", "COLLECTIVE whenever n > 0", "may differ between the ranks",
                   "valid until the next ps_dist_blame or ps_destroy", "no clamp at PS_MAX_ROUNDS",
                   "ps_topic_blame and ps_blame keep refusing multi-rank engines",
                   "no sharded form of ps_blame, no tracker and no _begin / _end form",
                   "valid until the next ps_topic_blame or ps_destroy"):  # (ps_topic_blame's sentence stays)
        assert phrase in flat, phrase


def test_binding_matches_the_header():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert protos["ps_dist_blame"][1] is C.c_int and protos["ps_dist_blame"][2] == protos["ps_topic_blame"][2]
    PP32, PP64 = C.POINTER(U32P), C.POINTER(U64P)
    assert protos["ps_dist_blame"][2][1:] == [U32P, C.c_size_t, PP64, PP32, PP32, PP32, PP32, PP32, U64P]
    assert PE.load().ps_dist_blame.restype is C.c_int
    assert hasattr(PE.Engine, "dist_blame")
    assert PE.load().ps_abi_version() == 5 and PE.ABI_VERSION == 5


def test_arguments_are_checked_before_the_engine_is_touched():
    """PS_E_INVAL with every output untouched; any non-NULL engine pointer will
    do for the checks behind the first (4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    off, ptrs, total = lent()
    byref = [C.byref(p) for p in ptrs]
    assert lib.ps_dist_blame(None, tp, 1, C.byref(off), *byref, C.byref(total)) == -1  # no engine
    assert lib.ps_dist_blame(None, None, 0, C.byref(off), *byref, C.byref(total)) == -1
    assert lib.ps_dist_blame(h, None, 1, C.byref(off), *byref, C.byref(total)) == -1  # n > 0 without topic
    assert lib.ps_dist_blame(h, tp, 1, None, *byref, C.byref(total)) == -1  # no rec_off
    assert lib.ps_dist_blame(h, tp, 1, C.byref(off), *byref, None) == -1  # no total
    assert lib.ps_dist_blame(h, None, 0, None, *byref, C.byref(total)) == -1  # ... at n == 0 too
    assert lib.ps_dist_blame(h, None, 0, C.byref(off), None, None, None, None, None, None) == -1
    assert lent_untouched(off, ptrs, total)


# ---- the reference of a rank's share ----------------------------------------------

@functools.lru_cache(maxsize=None)
def shape_tables(name):
    trees, roots, live = shape(name)
    n = trees[0].shape[0]
    return tuple(BR.topic_blame(n, r, live, N_MSGS, t) for t, r in zip(trees, roots))


@functools.lru_cache(maxsize=None)
def shape_cut_values(name):
    trees, roots, live = shape(name)
    n = trees[0].shape[0]
    return tuple(XC.topic_values(n, live, r, N_MSGS, t) for t, r in zip(trees, roots))


@pytest.mark.parametrize("subtree", [False, True])
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", SHAPES)
def test_shares_union_is_the_one_rank_blame(name, world, subtree):
    """Properties 1 and 2 of the reference, and property 4 against
    dist_cut_ref's shares of the same window."""
    trees, roots, live = shape(name)
    n = trees[0].shape[0]
    owners = XR.owners_of(trees, roots, world, subtree, split_depth=2 if subtree else 0)
    tables = shape_tables(name)
    topics = [(r, N_MSGS, t) for t, r in zip(trees, roots)]
    cuts = XC.rank_cuts(n, live, topics, owners, world, values=shape_cut_values(name))
    per_rank = [[XB.share(T, own, r) for T, own in zip(tables, owners)] for r in range(world)]
    any_record = False
    for i, (T, own) in enumerate(zip(tables, owners)):
        shares = [per_rank[r][i] for r in range(world)]
        # the union: blame_ref's records of the topic, keyed by peer
        whole = np.nonzero(T.miss > 0)[0]
        want = tuple(x.astype(np.uint32) for x in (whole, T.cut_peer[whole], T.hop[whole], T.cut_hop[whole], T.miss[whole]))
        for k, g, w in zip(XB.KEYS, XB.union(shares), want):
            assert np.array_equal(g, w), (k, world)
        # ownership: a rank's records are its own peers', and every one of them
        for r, s in enumerate(shares):
            assert (own[s[0]] == r).all() and s[0].size == int(((own == r) & (T.miss > 0)).sum())
        any_record |= whole.size > 0
    assert any_record
    # against dist_cut_ref: missed and cuts per rank, lost on the ranks' sum
    lost = np.zeros(n, dtype=np.uint64)
    for r in range(world):
        peer, cut_peer, _, _, missed = (np.concatenate([s[j] for s in per_rank[r]]) for j in range(5))
        w = missed.astype(np.int64)
        assert np.array_equal(np.bincount(peer, weights=w, minlength=n).astype(np.uint64), cuts[r]["missed"]), r
        assert np.array_equal(np.bincount(peer[peer == cut_peer], minlength=n).astype(np.uint64), cuts[r]["cuts"]), r
        lost += np.bincount(cut_peer, weights=w, minlength=n).astype(np.uint64)
    assert np.array_equal(lost, XC.total(cuts)["lost"])


@pytest.mark.parametrize("name", SHAPES)
def test_an_all_live_mask_has_no_record(name):
    trees, roots, _ = shape(name)
    n = trees[0].shape[0]
    live = np.ones(n, dtype=np.uint8)
    for t, r, own in zip(trees, roots, XR.owners_of(trees, roots, 3)):
        T = BR.topic_blame(n, r, live, N_MSGS, t)
        assert all(XB.share(T, own, q)[0].size == 0 for q in range(3))


def test_compare_refuses_a_foreign_record_a_wrong_field_and_a_falling_hop():
    parent, root, live = DR.row_width_case()
    own = XR.owners_of([parent], [root], 3)[0]
    T = BR.topic_blame(parent.shape[0], root, live, N_MSGS, parent)
    mine, other = XB.share(T, own, 0), XB.share(T, own, 1)
    by_hop = np.argsort(mine[2], kind="stable")
    good = tuple(x[by_hop] for x in mine)
    XB.compare(good, T, own, 0)
    with pytest.raises(AssertionError):  # a record of a node the rank does not own
        XB.compare(tuple(np.concatenate([g, o[:1]]) for g, o in zip(good, other)), T, own, 0)
    with pytest.raises(AssertionError):  # one too few
        XB.compare(tuple(g[:-1] for g in good), T, own, 0)
    bad = tuple(g.copy() for g in good)
    bad[1][0] ^= 1
    with pytest.raises(AssertionError):  # a wrong cut point
        XB.compare(bad, T, own, 0)
    with pytest.raises(AssertionError):  # hop falls
        XB.compare(tuple(g[::-1] for g in good), T, own, 0)


# ---- what the GPU cases rely on -----------------------------------------------------

def blame_facts(parent, root, live, own, world, c=N_MSGS):
    """Where one topic's records lie: per rank the records, those whose cut
    point another rank owns, and those whose path up to the cut point changes
    rank twice or more; the cut points; the longest way up to one."""
    n = parent.shape[0]
    T = BR.topic_blame(n, root, live, c, parent)
    par = np.asarray(parent, dtype=np.int64)
    rec = np.nonzero(T.miss > 0)[0]
    per, remote, twice, far = [0] * world, [0] * world, [0] * world, 0
    for u in rec:
        r, cp = int(own[u]), int(T.cut_peer[u])
        per[r] += 1
        remote[r] += int(own[cp] != r)
        x, handovers, steps = int(u), 0, 0
        while x != cp:
            handovers += int(own[par[x]] != own[x])
            x, steps = int(par[x]), steps + 1
        assert steps == T.hop[u] - T.cut_hop[u]
        twice[r] += int(handovers >= 2)
        far = max(far, steps)
    return {"records": int(rec.size), "per_rank": per, "remote": remote, "twice": twice,
            "cuts": int((T.cut_peer[rec] == rec).sum()), "far": far, "table": T}


def test_row_width_case_facts():
    parent, root, live = DR.row_width_case()
    f = blame_facts(parent, root, live, XR.owners_of([parent], [root], 3)[0], 3)
    assert f["records"] == 282 and f["per_rank"] == [93, 94, 95]
    assert f["remote"] == [80, 57, 35] and f["twice"] == [70, 76, 70]
    assert f["cuts"] == 26 and f["far"] == 21


@pytest.mark.parametrize("dead,records,per_rank,remote", [(1, 39, [13, 13, 13], [13, 13, 0]), (20, 20, [7, 6, 7], [0, 6, 7])])
def test_path_40_at_world_3_facts(dead, records, per_rank, remote):
    parent, root = DR.path(40)
    live = np.ones(40, dtype=np.uint8)
    live[dead] = 0
    f = blame_facts(parent, root, live, XR.owners_of([parent], [root], 3)[0], 3)
    assert (f["records"], f["per_rank"], f["remote"], f["cuts"]) == (records, per_rank, remote, 1)
    assert all(f["twice"])


def test_split_case_topic_0_at_world_4_facts():
    trees, roots, live = DR.split_case()
    f = blame_facts(trees[0], roots[0], live, XR.owners_of(trees, roots, 4)[0], 4)
    assert f["records"] == 865 and f["per_rank"] == [205, 231, 216, 213]
    assert f["remote"] == [85, 203, 183, 123] and f["cuts"] == 84


def two_dead(n):
    """Two dead peers on path(n): the nearer one wins for everything behind it."""
    return [n // 4, n // 2]


def gpu_shapes():
    """Every sharded shape of tests/test_gpu_dist_blame.py that is no stated
    exception: name -> (parent, root, live, own, world)."""
    out = {}
    parent, root, live = DR.row_width_case()
    out["row_width"] = (parent, root, live, XR.owners_of([parent], [root], 3)[0], 3)
    for deg in (65, 129):
        for world in (2, 4):
            for alive in (True, False):
                parent, root, hub, facts, live = fan_live(deg, world, alive)
                out[f"fan_{deg}_{world}_{int(alive)}"] = (parent, root, live, XR.owners_of([parent], [root], world)[0], world)
    for n in (40, 300):
        parent, root = DR.path(n)
        own = XR.owners_of([parent], [root], 2)[0]
        for name, dead in (("first", [1]), ("middle", [n // 2]), ("remote_parent", [path_dead(n)]), ("two", two_dead(n))):
            live = np.ones(n, dtype=np.uint8)
            live[dead] = 0
            out[f"path_{n}_{name}"] = (parent, root, live, own, 2)
    trees, roots, live = DR.split_case()
    for world, split in ((2, 2), (4, 2), (4, 3)):
        owners = XR.owners_of(trees, roots, world, True, split)
        out[f"split_{world}_{split}"] = (trees[0], roots[0], live, owners[0], world)
    trees, roots, victim = DR.windows_case(600, 3)
    live = np.ones(600, dtype=np.uint8)
    live[victim] = 0
    out["windows_run_b"] = (trees[0], roots[0], live, XR.owners_of(trees, roots, 3)[0], 3)
    return out


@pytest.mark.parametrize("name", sorted(gpu_shapes()))
def test_no_gpu_shape_passes_vacuously(name):
    """Every rank of a shape holds records, one of them behind a cut point on
    another rank and one whose path up to its cut point changed rank twice or
    more.  The exceptions, stated: the owner of a shape's one cut point names
    no remote one; under the subtree partition a path changes rank once at
    most, at the split level, and at split level 2 no cut point lies above it;
    with the fan's hub alive the few records hang right below their cut
    points, so the shape as a whole shows both kinds and not every rank."""
    parent, root, live, own, world = gpu_shapes()[name]
    f = blame_facts(parent, root, live, own, world)
    assert f["records"] > 0 and all(f["per_rank"])
    if name.startswith("split_"):
        assert not any(f["twice"])
        assert (sum(f["remote"]) > 0) == (name == "split_4_3")
    elif name.startswith("fan_") and name.endswith("_1"):
        assert f["far"] <= 3 and sum(f["remote"]) > 0 and sum(f["twice"]) > 0
    else:
        T = f["table"]
        cut_points = np.unique(T.cut_peer[T.miss > 0])
        for r in range(world):
            assert f["twice"][r] > 0, r
            assert f["remote"][r] > 0 or (cut_points.size == 1 and own[cut_points[0]] == r), r


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("deg", [65, 129])
def test_wide_fan_dead_hub_every_record_behind_it_names_the_hub(deg, world):
    parent, root, hub, facts, live = fan_live(deg, world, False)
    own = XR.owners_of([parent], [root], world)[0]
    f = blame_facts(parent, root, live, own, world)
    T = f["table"]
    rec = np.nonzero(T.miss > 0)[0]
    assert f["cuts"] == 1 and (T.cut_peer[rec] == hub).all() and (T.cut_hop[rec] == 1).all()
    assert rec.size == (449 if deg == 65 else 464) and all(f["per_rank"])  # the hub and everything behind it, on every rank
    assert (own[hub] != own[root]) == ((deg, world) != (65, 2))  # the hub hangs under a remote root


@pytest.mark.parametrize("n", [40, 300])
def test_two_dead_peers_on_a_path_the_nearer_wins(n):
    parent, root = DR.path(n)
    a, b = two_dead(n)
    live = np.ones(n, dtype=np.uint8)
    live[[a, b]] = 0
    T = BR.topic_blame(n, root, live, N_MSGS, parent)
    # a dead peer forwards nothing: everything behind the first lacks every
    # message, its parent too, so the walk up ends at the first dead peer
    assert (T.cut_peer[a:] == a).all() and (T.cut_hop[a:] == a).all() and (T.miss[a:] == N_MSGS).all()
    assert (T.miss[:a] == 0).all()


@pytest.mark.parametrize("world", [5, 16])
def test_tiny_beside_large_has_empty_ranks_and_remote_cut_points(world):
    trees, roots, facts = DR.tiny_beside_large(400, world)
    owners = XR.owners_of(trees, roots, world)
    n = trees[0].shape[0]
    live = np.ones(n, dtype=np.uint8)
    live[np.random.default_rng(world).choice(n, size=20, replace=False)] = 0
    live[roots] = 1
    assert any(not (owners[0] == r).any() for r in range(world))  # a rank that owns nothing of a topic
    f = blame_facts(trees[1], roots[1], live, owners[1], world)
    assert sum(f["remote"]) > 0 and sum(f["twice"]) > 0


def test_star_records_are_their_own_cut_points():
    n = 3001
    parent = star(n)
    live = np.ones(n, dtype=np.uint8)
    live[[1, 64, 65, 66, 255, 256, 257, 3000]] = 0
    f = blame_facts(parent, 0, live, XR.owners_of([parent], [0], 4)[0], 4)
    assert f["records"] == f["cuts"] == 8 and f["far"] == 0  # stated exception: nothing inherited, one wide level
