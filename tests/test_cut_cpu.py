"""ps_peer_cut / ps_cut_track / ps_cut_take without a GPU: the argument checks
that need no engine, the binding and the header, and the reference helper
(tests/cut_ref.py) against closed forms and the oracle's own totals.  (With an
engine the calls need a device: tests/test_gpu_cut.py.)"""
import ctypes as C
import os
import re

import numpy as np

import cut_ref as CR
import downstream_ref as DR
import oracle as O
import psengine as PE
from test_downstream_cpu import heap_subtree, heap_tree
from test_gpu_drain_batch import random_tree

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
FILL = 0xABABABABABABABAB


def outs(n=8):
    a = [np.full(n, FILL, dtype=np.uint64) for _ in range(4)]
    return a, [x.ctypes.data_as(U64P) for x in a]


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    a, p = outs()
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    assert lib.ps_peer_cut(None, tp, 1, *p) == -1  # PS_E_INVAL
    assert lib.ps_peer_cut(None, None, 0, *p) == -1
    assert lib.ps_cut_track(None, tp, 1) == -1
    assert lib.ps_cut_track(None, None, 0) == -1
    assert lib.ps_cut_take(None, *p, C.byref(nw), C.byref(nsk)) == -1
    assert lib.ps_cut_take(None, None, None, None, None, None, None) == -1
    assert all((x == FILL).all() for x in a) and nw.value == 0xCCCC and nsk.value == 0xDDDD


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    a, p = outs()
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    assert lib.ps_peer_cut(h, None, 1, *p) == -1  # topics announced, none given
    assert lib.ps_peer_cut(h, None, 3, None, p[1], None, None) == -1
    assert lib.ps_peer_cut(h, tp, 1, None, None, None, None) == -1  # all four outputs NULL
    assert lib.ps_peer_cut(h, None, 0, None, None, None, None) == -1
    assert lib.ps_cut_track(h, None, 1) == -1
    assert lib.ps_cut_track(h, None, 7) == -1
    assert lib.ps_cut_take(h, *p, None, C.byref(nsk)) == -1  # no window count
    assert lib.ps_cut_take(h, *p, C.byref(nw), None) == -1  # no skipped count
    assert lib.ps_cut_take(h, None, None, None, None, None, None) == -1
    assert all((x == FILL).all() for x in a) and nw.value == 0xCCCC and nsk.value == 0xDDDD


def test_prototypes_are_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert len(protos["ps_peer_cut"][2]) == 7
    assert len(protos["ps_cut_track"][2]) == 3
    assert len(protos["ps_cut_take"][2]) == 7
    with open(HEADER) as f:
        text = f.read()
    assert "int ps_peer_cut(ps_engine* e, const uint32_t* topic, size_t n,\n" in text
    assert "                uint64_t* missed_out, uint64_t* cuts_out,\n" in text
    assert "                uint64_t* orphaned_out, uint64_t* lost_out);" in text
    assert "int ps_cut_track(ps_engine* e, const uint32_t* topic, size_t n);" in text
    assert "int ps_cut_take(ps_engine* e, uint64_t* missed_out, uint64_t* cuts_out,\n" in text
    assert "                uint64_t* n_windows_out, uint64_t* n_skipped_out);" in text
    # the semantics and the four identities are stated
    flat = " ".join(re.sub(r"\n \*", " ", text).split())  # (the comment's line breaks and stars folded away)
    for phrase in ("the root counts as full", "c_t * (n_nodes_t - 1) - deliveries_t",
                   "sum of lost equals the sum of missed", "lost[p] = c_t * (1 + orphaned[p])", "orphaned[p] = below[p]",
                   "carried[p] = 0", "all-live mask all four arrays are zero"):
        assert phrase in flat, phrase
    for name in ("peer_cut", "cut_track", "cut_take"):
        assert hasattr(PE.Engine, name), name
    lib = PE.load()
    for name in ("ps_peer_cut", "ps_cut_track", "ps_cut_take"):
        assert getattr(lib, name).restype is C.c_int


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5


# ---- the reference helper ----------------------------------------------------------

def path(n):
    parent = np.arange(-1, n - 1).astype(np.uint32)
    parent[0] = O.NONE
    return parent


def test_helper_path_is_closed_form():
    n, c = 300, 3
    parent = path(n)
    for j in (1, 150, 298, 299):
        live = np.ones(n, dtype=np.uint8)
        live[j] = 0
        missed, cuts, orphaned, lost, tot, members = CR.topic_cut(n, 0, live, c, parent)
        assert members == n and tot == c * (j - 1)
        assert cuts.sum() == 1 and cuts[j] == 1
        assert orphaned[j] == n - 1 - j and orphaned.sum() == n - 1 - j
        assert lost[j] == c * (n - j) and lost.sum() == lost[j]
        assert not missed[:j].any() and (missed[j:] == c).all()


def test_helper_all_live_is_zero():
    for n, w in ((2, 2), (64, 2), (100, 3)):
        r = CR.topic_cut(n, 0, np.ones(n, dtype=np.uint8), 5, heap_tree(n, w))
        assert not any(x.any() for x in r[:4]) and r[4] == 5 * (n - 1) and r[5] == n
    live = np.ones(64, dtype=np.uint8)
    live[7] = 0
    r = CR.topic_cut(64, 0, live, 0, heap_tree(64))
    assert not any(x.any() for x in r[:4]) and r[4:] == (0, 0)  # idle: nothing at all


def test_helper_heap_with_one_dead_inner_node():
    n, c = 127, 4
    parent = heap_tree(n)
    live = np.ones(n, dtype=np.uint8)
    live[5] = 0  # the subtree of 5: 5, 11, 12, 23 .. 26, 47 .. 54, 95 .. 110: 31 nodes
    sub = [5, 11, 12] + list(range(23, 27)) + list(range(47, 55)) + list(range(95, 111))
    assert len(sub) == heap_subtree(5, n, 2) == 31
    missed, cuts, orphaned, lost, tot, _ = CR.topic_cut(n, 0, live, c, parent)
    want = np.zeros(n, dtype=np.int64)
    want[sub] = c
    assert np.array_equal(missed, want)
    assert cuts.sum() == 1 and cuts[5] == 1 and orphaned.sum() == orphaned[5] == 30 and lost.sum() == lost[5] == c * 31
    assert tot == c * (n - 1 - 31)
    # identity 3 against the downstream helper
    below, carried, _ = DR.topic_downstream(n, 0, live, c, parent)
    assert orphaned[5] == below[5] and carried[5] == 0


def test_helper_nested_dead_nodes_count_once():
    """A dead node under a dead node, and a dead leaf under a dead parent: only
    the topmost is a cut point, and its sums hold every node once."""
    n, c = 127, 2
    parent = heap_tree(n)
    for dead, top in (([5, 11], 5), ([5, 23, 110], 5), ([62, 125], 62), ([1, 3, 7], 1)):
        live = np.ones(n, dtype=np.uint8)
        live[dead] = 0
        missed, cuts, orphaned, lost, tot, _ = CR.topic_cut(n, 0, live, c, parent)
        size = heap_subtree(top, n, 2)
        assert cuts.sum() == 1 and cuts[top] == 1, dead
        assert orphaned.sum() == orphaned[top] == size - 1
        assert lost.sum() == lost[top] == c * size == missed.sum()
        assert tot == c * (n - 1 - size)
    # two cut points side by side, and one below a live sibling's subtree
    live = np.ones(n, dtype=np.uint8)
    live[[3, 4, 12]] = 0
    missed, cuts, orphaned, lost, tot, _ = CR.topic_cut(n, 0, live, c, parent)
    assert sorted(np.nonzero(cuts)[0]) == [3, 4, 12]
    assert lost.sum() == missed.sum() == c * (n - 1) - tot


def test_helper_identities_against_the_oracles_total():
    rng = np.random.default_rng(5)
    n, root = 300, 3
    parent = random_tree(rng, n, root)
    outside = 299
    parent[parent == outside] = root
    parent[outside] = O.NONE
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    for n_msgs in (1, 65, 130):
        missed, cuts, orphaned, lost, tot, members = CR.topic_cut(n, root, live, n_msgs, parent)
        assert members == n - 1
        assert missed.sum() == n_msgs * (members - 1) - tot > 0  # identity 1
        assert lost.sum() == missed.sum()  # identity 2
        assert not missed[outside] and not cuts[outside] and not missed[root]  # the outsider is no node
        below, carried, _ = DR.topic_downstream(n, root, live, n_msgs, parent)
        at = np.nonzero(cuts)[0]
        assert at.size and np.array_equal(orphaned[at], below[at]) and not carried[at].any()  # identity 3
        assert np.array_equal(lost[at], n_msgs * (1 + orphaned[at]))
        assert (cuts <= 1).all() and not live[at].any()  # on a healthy tree the cut points are dead peers


def test_helper_window_sum():
    rng = np.random.default_rng(7)
    n = 200
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[[4, 9]] = 1
    p0, p1 = random_tree(rng, n, 4), random_tree(rng, n, 9)
    a, b = CR.topic_cut(n, 4, live, 3, p0), CR.topic_cut(n, 9, live, 5, p1)
    w = CR.window_cut(n, live, [(4, 3, p0), (9, 5, p1), (4, 0, p0)])
    for x, y, z in zip(w[:4], a[:4], b[:4]):
        assert x.dtype == np.uint64 and x.shape == (n,) and np.array_equal(x, (y + z).astype(np.uint64))
    assert w[4] == a[4] + b[4] and w[5] == 3 * (n - 1) + 5 * (n - 1)
    assert int(w[0].sum()) == w[5] - w[4] == int(w[3].sum())
