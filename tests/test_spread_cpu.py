"""ps_topic_spread without a GPU: the reference (tests/spread_ref.py) against
mesh_ref.Flood on every builder of that file and against hops_ref / load_ref on
a tree, the header and the binding, and the argument checks that need no
engine.  (With an engine the call needs a device: tests/test_gpu_spread.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

import hops_ref as HR
import load_ref as LR
import mesh_ref as MR
import oracle as O
import psengine as PE
import spread_ref as SR
from test_gpu_drain_batch import random_tree

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
FILL = 0xABABABABABABABAB

GRAPHS = ([("specials", s) for s in (0, 1, 2)] + [("hub", d) for d in (63, 64, 65, 129, 200)] +
          [("detour", k) for k in (8, 40, 300)])


def build(kind, arg):
    if kind == "specials":
        return MR.mesh_with_specials(300, seed=arg)
    return MR.hub_mesh(arg) if kind == "hub" else MR.detour(arg)


# ---- the reference against the flood -------------------------------------------------

@pytest.mark.parametrize("kind,arg", GRAPHS)
@pytest.mark.parametrize("c", [1, 70])
def test_reference_restates_the_flood(kind, arg, c):
    """From the reached set alone: the BFS within the forwarders gives every
    peer the hop the flood delivered it at, the copies beyond the receipts sum
    to the flood's duplicates, and nobody that holds messages is left out."""
    rp, cl, root, live, _ = build(kind, arg)
    F = MR.flood(rp, cl, root, live)
    S = SR.topic_spread(rp, cl, root, F.level >= 0, c)
    want = F.level.copy()
    want[root] = 0
    assert np.array_equal(S.level, want)
    assert S.dup.min() >= 0 and S.dup.sum() == c * F.duplicates
    assert S.deliv.sum() == c * F.deliveries and S.reached.sum() == F.deliveries
    assert S.stranded == 0
    assert S.reached[0] == S.deliv[0] == 0 and np.array_equal(S.deliv, c * S.reached)
    assert np.array_equal(S.reached[:SR.COLS - 1], F.hist(SR.COLS)[:SR.COLS - 1])
    member = LR.csr_members(rp, cl, root)
    assert S.unreached == int(member.sum()) - 1 - F.deliveries
    # what a peer was sent: once per entry of a forwarder that names it
    assert S.copies.sum() == c * (F.deliveries + F.duplicates)


def test_reference_specials_by_name():
    rp, cl, root, live, facts = MR.mesh_with_specials(300)
    F = MR.flood(rp, cl, root, live)
    c = 5
    S = SR.topic_spread(rp, cl, root, F.level >= 0, c)
    assert S.copies[root] == S.dup[root] == c  # the edge into the root: all of it a duplicate
    p = facts["self_loop"]
    assert S.dup[p] >= c  # its own entry sends it what it has
    p, ch = facts["repeated"]
    assert S.dup[ch] >= c  # the second entry of the same parent
    assert S.dup[facts["same_round"][0]] >= c and S.dup[facts["later"][0]] >= c
    d, cut = facts["dead_parent"], facts["cut_off"]
    assert S.level[d] < 0 and S.level[cut] < 0 and S.copies[d] == S.copies[cut] == 0
    assert S.unreached >= 2


@pytest.mark.parametrize("deg", [63, 129])
def test_reference_hub_children_carry_the_duplicates(deg):
    rp, cl, root, live, facts = MR.hub_mesh(deg)
    F = MR.flood(rp, cl, root, live)
    S = SR.topic_spread(rp, cl, root, F.level >= 0, 3)
    want = np.zeros(len(live), dtype=np.int64)
    want[[ch for ch in facts["listed"] if live[ch]]] = 3
    assert np.array_equal(S.dup, want)


def test_reference_detour_clamps_into_the_last_column():
    rp, cl, root, live, _ = MR.detour(300)
    F = MR.flood(rp, cl, root, live)
    S = SR.topic_spread(rp, cl, root, F.level >= 0, 2)
    assert S.level.max() == 299
    assert (S.reached[1:255] == 1).all() and S.reached[255] == 45 and S.deliv[255] == 90
    assert S.unreached == 1 and not S.dup.any()  # S, dead: sent nothing, named by the root alone


def test_reference_on_a_tree_is_hops_and_load():
    rng = np.random.default_rng(11)
    n, root = 300, 3
    parent = random_tree(rng, n, root)
    outside = 299
    parent[parent == outside] = root
    parent[outside] = O.NONE
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    for c in (1, 65):
        nodes, reached, deliv, tot = HR.topic_hops(n, root, live, c, parent)
        recv = LR.topic_load(n, root, live, c, parent=parent)[0]
        rp, cl = SR.tree_csr(parent, root)
        S = SR.topic_spread(rp, cl, root, recv > 0, c)
        assert np.array_equal(S.reached, reached) and np.array_equal(S.deliv, deliv) and tot == S.deliv.sum()
        assert np.array_equal(S.copies, recv) and not S.dup.any() and S.stranded == 0
        assert S.unreached == nodes.sum() - reached.sum() > 0


def test_reference_reports_the_stranded():
    """Rows that hold messages behind a node that holds none -- what a healthy
    engine never leaves -- are counted, not visited."""
    rp, cl = MR.csr({0: [1], 1: [2], 2: [3], 3: []}, 4)
    S = SR.topic_spread(rp, cl, 0, np.array([0, 4, 0, 4]), 4)
    assert S.stranded == 1 and S.unreached == 1 and S.reached.sum() == 1 and S.level[3] < 0
    assert S.copies.tolist() == [0, 4, 0, 0] and S.dup.tolist() == [0, 0, 0, -4]


def test_reference_window_sum():
    a, b = MR.mesh_with_specials(300), MR.hub_mesh(65)
    n = 400
    topics = []
    for g, c in ((a, 3), (b, 0), (b, 5)):
        rp, cl, root, live, _ = g
        pad = n - len(live)
        rp = np.concatenate([rp, np.full(pad, rp[-1], dtype=rp.dtype)])
        lv = np.concatenate([live, np.zeros(pad, dtype=np.uint8)])
        topics.append((rp, cl, root, MR.flood(rp, cl, root, lv).level >= 0, c))
    W = SR.window_spread(n, topics)
    S0, S2 = SR.topic_spread(*topics[0]), SR.topic_spread(*topics[2])
    assert W["reached"].dtype == W["dup"].dtype == np.uint64 and W["reached"].shape == (3, SR.COLS)
    assert np.array_equal(W["deliv"][0], S0.deliv.astype(np.uint64)) and not W["deliv"][1].any()
    assert W["unreached"].tolist() == [S0.unreached, 0, S2.unreached]
    assert np.array_equal(W["copies"], (S0.copies + S2.copies).astype(np.uint64))
    assert np.array_equal(W["dup"], (S0.dup + S2.dup).astype(np.uint64))


# ---- the header, the binding, the argument checks --------------------------------------

def test_prototype_is_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert len(protos["ps_topic_spread"][2]) == 9
    with open(HEADER) as f:
        text = f.read()
    assert "int ps_topic_spread(ps_engine* e, const uint32_t* topic, size_t n,\n" in text
    assert "uint64_t* reached_out, uint64_t* deliv_out," in text
    assert "uint64_t* unreached_out, uint64_t* stranded_out," in text
    assert "uint64_t* copies_out, uint64_t* dup_out);" in text
    assert hasattr(PE.Engine, "topic_spread")
    assert PE.load().ps_topic_spread.restype is C.c_int


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5
    assert SR.COLS == PE.MAX_ROUNDS == 256


def outs():
    a = [np.full(2 * PE.MAX_ROUNDS, FILL, dtype=np.uint64) for _ in range(6)]
    return a, [x.ctypes.data_as(U64P) for x in a]


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    a, p = outs()
    assert lib.ps_topic_spread(None, t.ctypes.data_as(U32P), 1, *p) == -1  # PS_E_INVAL
    assert lib.ps_topic_spread(None, None, 0, *p) == -1
    assert all((x == FILL).all() for x in a)


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    a, p = outs()
    assert lib.ps_topic_spread(h, None, 1, *p) == -1  # topics announced, none given
    assert lib.ps_topic_spread(h, None, 3, None, None, None, None, None, p[5]) == -1
    assert lib.ps_topic_spread(h, tp, 1, None, None, None, None, None, None) == -1  # all six outputs NULL
    assert lib.ps_topic_spread(h, None, 0, None, None, None, None, None, None) == -1
    assert all((x == FILL).all() for x in a)
