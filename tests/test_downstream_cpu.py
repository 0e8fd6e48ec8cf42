"""ps_peer_downstream / ps_downstream_track / ps_downstream_take without a GPU:
the argument checks that need no engine, the binding and the header, and the
reference helper (tests/downstream_ref.py) against closed forms and the
oracle's own totals.  (With an engine the calls need a device:
tests/test_gpu_downstream.py.)"""
import ctypes as C
import os

import numpy as np

import downstream_ref as DR
import hops_ref as HR
import load_ref as LR
import oracle as O
import psengine as PE
from test_gpu_drain_batch import random_tree

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
FILL = 0xABABABABABABABAB


def outs(n=8):
    a = [np.full(n, FILL, dtype=np.uint64) for _ in range(2)]
    return a, [x.ctypes.data_as(U64P) for x in a]


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    a, (pb, pc) = outs()
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    assert lib.ps_peer_downstream(None, tp, 1, pb, pc) == -1  # PS_E_INVAL
    assert lib.ps_peer_downstream(None, None, 0, pb, pc) == -1
    assert lib.ps_downstream_track(None, tp, 1) == -1
    assert lib.ps_downstream_track(None, None, 0) == -1
    assert lib.ps_downstream_take(None, pb, pc, C.byref(nw), C.byref(nsk)) == -1
    assert lib.ps_downstream_take(None, None, None, None, None) == -1
    assert all((x == FILL).all() for x in a) and nw.value == 0xCCCC and nsk.value == 0xDDDD


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    a, (pb, pc) = outs()
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    assert lib.ps_peer_downstream(h, None, 1, pb, pc) == -1  # topics announced, none given
    assert lib.ps_peer_downstream(h, None, 3, None, pc) == -1
    assert lib.ps_peer_downstream(h, tp, 1, None, None) == -1  # both outputs NULL
    assert lib.ps_peer_downstream(h, None, 0, None, None) == -1
    assert lib.ps_downstream_track(h, None, 1) == -1
    assert lib.ps_downstream_track(h, None, 7) == -1
    assert lib.ps_downstream_take(h, pb, pc, None, C.byref(nsk)) == -1  # no window count
    assert lib.ps_downstream_take(h, pb, pc, C.byref(nw), None) == -1  # no skipped count
    assert lib.ps_downstream_take(h, None, None, None, None) == -1
    assert all((x == FILL).all() for x in a) and nw.value == 0xCCCC and nsk.value == 0xDDDD


def test_prototypes_are_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert len(protos["ps_peer_downstream"][2]) == 5
    assert len(protos["ps_downstream_track"][2]) == 3
    assert len(protos["ps_downstream_take"][2]) == 5
    with open(HEADER) as f:
        text = f.read()
    assert "int ps_peer_downstream(ps_engine* e, const uint32_t* topic, size_t n,\n" in text
    assert "                       uint64_t* below_out, uint64_t* carried_out);" in text
    assert "int ps_downstream_track(ps_engine* e, const uint32_t* topic, size_t n);" in text
    assert "int ps_downstream_take(ps_engine* e, uint64_t* below_out, uint64_t* carried_out," in text
    assert "                       uint64_t* n_windows_out, uint64_t* n_skipped_out);" in text
    # the semantics and the three identities are stated
    for phrase in ("strict descendant", "carried[root_t]", "h * nodes[h]", "h * deliv[h]", "sum of per-window values"):
        assert phrase in text, phrase
    for name in ("peer_downstream", "downstream_track", "downstream_take"):
        assert hasattr(PE.Engine, name), name
    lib = PE.load()
    for name in ("ps_peer_downstream", "ps_downstream_track", "ps_downstream_take"):
        assert getattr(lib, name).restype is C.c_int


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5


# ---- the reference helper ----------------------------------------------------------

def heap_tree(n, w=2):
    parent = ((np.arange(n, dtype=np.int64) - 1) // w).astype(np.uint32)
    parent[0] = O.NONE
    return parent


def heap_subtree(i, n, w):
    """Nodes of the subtree of node i in a complete heap of width w over n
    nodes: level by level, the run [lo, hi] becomes [w * lo + 1, w * hi + w]."""
    lo = hi = i
    size = 0
    while lo < n:
        size += min(hi, n - 1) - lo + 1
        lo, hi = w * lo + 1, w * hi + w
    return size


def test_helper_heap_is_closed_form():
    for n, w, n_msgs in ((2, 2, 1), (64, 2, 3), (100, 3, 7), (1025, 2, 2), (500, 5, 1)):
        below, carried, tot = DR.topic_downstream(n, 0, np.ones(n, dtype=np.uint8), n_msgs, heap_tree(n, w))
        want = np.array([heap_subtree(i, n, w) - 1 for i in range(n)], dtype=np.int64)
        assert np.array_equal(below, want)
        assert np.array_equal(carried, n_msgs * want)  # all live: every node below holds every message
        assert below[0] == n - 1 and carried[0] == tot == n_msgs * (n - 1)


def test_helper_path_is_closed_form():
    n = 300
    parent = np.arange(-1, n - 1).astype(np.uint32)  # peer p's upstream is p - 1
    parent[0] = O.NONE
    live = np.ones(n, dtype=np.uint8)
    below, carried, tot = DR.topic_downstream(n, 0, live, 3, parent)
    assert np.array_equal(below, n - 1 - np.arange(n)) and np.array_equal(carried, 3 * below) and tot == 3 * 299
    live[280] = 0  # nothing arrives from 280 on; the nodes stay
    below, carried, tot = DR.topic_downstream(n, 0, live, 3, parent)
    assert np.array_equal(below, n - 1 - np.arange(n)) and tot == 3 * 279
    assert np.array_equal(carried[:280], 3 * (279 - np.arange(280))) and not carried[279:].any()


def test_helper_dead_subtree_keeps_below_and_loses_carried():
    n, n_msgs = 127, 4
    parent = heap_tree(n)
    live = np.ones(n, dtype=np.uint8)
    full = DR.topic_downstream(n, 0, live, n_msgs, parent)
    live[5] = 0  # the subtree of 5: 5, 11, 12, 23 .. 26, 47 .. 54, 95 .. 110: 31 nodes
    below, carried, tot = DR.topic_downstream(n, 0, live, n_msgs, parent)
    assert np.array_equal(below, full[0]) and below[5] == 30
    sub = [5, 11, 12] + list(range(23, 27)) + list(range(47, 55)) + list(range(95, 111))
    assert not carried[sub].any()
    assert tot == n_msgs * (n - 1 - 31) == carried[0]
    assert carried[2] == full[1][2] - n_msgs * 31 and carried[1] == full[1][1]  # the ancestors of 5 lose its subtree


def test_helper_against_the_oracles_totals_and_the_other_helpers():
    rng = np.random.default_rng(5)
    n, root = 300, 3
    parent = random_tree(rng, n, root)
    outside = 299
    parent[parent == outside] = root
    parent[outside] = O.NONE
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    h = np.arange(HR.COLS, dtype=np.int64)
    for n_msgs in (1, 65, 130):
        below, carried, tot = DR.topic_downstream(n, root, live, n_msgs, parent)
        recv = LR.topic_load(n, root, live, n_msgs, parent=parent)[0]
        nodes, _, deliv, tot_h = HR.topic_hops(n, root, live, n_msgs, parent)
        assert carried[root] == tot == tot_h == recv.sum() > 0
        assert below[root] == n - 2 and below[outside] == carried[outside] == 0  # the outsider is no node
        assert below.sum() == (h * nodes).sum() and carried.sum() == (h * deliv).sum()
        assert (carried <= n_msgs * below).all()
    below, carried, tot = DR.topic_downstream(n, root, live, 0, parent)
    assert not below.any() and not carried.any() and tot == 0  # idle: not even below


def test_helper_window_sum():
    rng = np.random.default_rng(7)
    n = 200
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[[4, 9]] = 1
    p0, p1 = random_tree(rng, n, 4), random_tree(rng, n, 9)
    a, b = DR.topic_downstream(n, 4, live, 3, p0), DR.topic_downstream(n, 9, live, 5, p1)
    wb, wc, wt = DR.window_downstream(n, live, [(4, 3, p0), (9, 5, p1), (4, 0, p0)])
    assert wb.dtype == wc.dtype == np.uint64 and wb.shape == (n,)
    assert np.array_equal(wb, (a[0] + b[0]).astype(np.uint64)) and np.array_equal(wc, (a[1] + b[1]).astype(np.uint64))
    assert wt == a[2] + b[2]
