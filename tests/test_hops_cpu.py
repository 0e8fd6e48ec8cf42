"""ps_topic_hops / ps_hops_track / ps_hops_take without a GPU: the argument
checks that need no engine, the binding and the header, and the reference
helper (tests/hops_ref.py) against the oracle's own totals and closed forms.
(With an engine the calls need a device: tests/test_gpu_hops.py.)"""
import ctypes as C
import os

import numpy as np

import hops_ref as HR
import load_ref as LR
import oracle as O
import psengine as PE
from test_gpu_drain_batch import random_tree

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
FILL = 0xABABABABABABABAB


def outs(n=2):
    a = [np.full(n * PE.MAX_ROUNDS, FILL, dtype=np.uint64) for _ in range(3)]
    return a, [x.ctypes.data_as(U64P) for x in a]


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    a, (pn, pr, pd) = outs()
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    assert lib.ps_topic_hops(None, tp, 1, pn, pr, pd) == -1  # PS_E_INVAL
    assert lib.ps_topic_hops(None, None, 0, pn, pr, pd) == -1
    assert lib.ps_hops_track(None, tp, 1) == -1
    assert lib.ps_hops_track(None, None, 0) == -1
    assert lib.ps_hops_take(None, pn, pr, pd, C.byref(nw), C.byref(nsk)) == -1
    assert lib.ps_hops_take(None, None, None, None, None, None) == -1
    assert all((x == FILL).all() for x in a) and nw.value == 0xCCCC and nsk.value == 0xDDDD


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    a, (pn, pr, pd) = outs()
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    assert lib.ps_topic_hops(h, None, 1, pn, pr, pd) == -1  # topics announced, none given
    assert lib.ps_topic_hops(h, None, 3, None, None, pd) == -1
    assert lib.ps_topic_hops(h, tp, 1, None, None, None) == -1  # all three outputs NULL
    assert lib.ps_topic_hops(h, None, 0, None, None, None) == -1
    assert lib.ps_hops_track(h, None, 1) == -1
    assert lib.ps_hops_track(h, None, 7) == -1
    assert lib.ps_hops_take(h, pn, pr, pd, None, C.byref(nsk)) == -1  # no window count
    assert lib.ps_hops_take(h, pn, pr, pd, C.byref(nw), None) == -1  # no skipped count
    assert lib.ps_hops_take(h, None, None, None, None, None) == -1
    assert all((x == FILL).all() for x in a) and nw.value == 0xCCCC and nsk.value == 0xDDDD


def test_prototypes_are_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert len(protos["ps_topic_hops"][2]) == 6
    assert len(protos["ps_hops_track"][2]) == 3
    assert len(protos["ps_hops_take"][2]) == 6
    with open(HEADER) as f:
        text = f.read()
    assert "int ps_topic_hops(ps_engine* e, const uint32_t* topic, size_t n,\n" in text
    assert "                  uint64_t* nodes_out, uint64_t* reached_out, uint64_t* deliv_out);\n" in text
    assert "int ps_hops_track(ps_engine* e, const uint32_t* topic, size_t n);" in text
    assert "int ps_hops_take(ps_engine* e, uint64_t* nodes_out, uint64_t* reached_out, uint64_t* deliv_out,\n" in text
    assert "                 uint64_t* n_windows_out, uint64_t* n_skipped_out);" in text
    for name in ("topic_hops", "hops_track", "hops_take"):
        assert hasattr(PE.Engine, name), name
    lib = PE.load()
    for name in ("ps_topic_hops", "ps_hops_track", "ps_hops_take"):
        assert getattr(lib, name).restype is C.c_int


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5
    assert HR.COLS == PE.MAX_ROUNDS == 256


# ---- the reference helper ----------------------------------------------------------

def heap_tree(n):
    parent = ((np.arange(n, dtype=np.int64) - 1) // 2).astype(np.uint32)
    parent[0] = O.NONE
    return parent


def test_helper_row_sums_are_the_oracles_and_the_loads():
    rng = np.random.default_rng(5)
    n, root = 300, 3
    parent = random_tree(rng, n, root)
    outside = 299
    parent[parent == outside] = root
    parent[outside] = O.NONE
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    for n_msgs in (1, 65, 130):
        nodes, reached, deliv, tot = HR.topic_hops(n, root, live, n_msgs, parent)
        recv = LR.topic_load(n, root, live, n_msgs, parent=parent)[0]
        assert deliv.sum() == tot == recv.sum() > 0
        assert nodes.sum() == n - 2  # every member but the root; the outsider is none
        assert reached.sum() == (recv > 0).sum() and (reached <= nodes).all()
        assert np.array_equal(deliv, n_msgs * reached)  # a tree row is all or nothing
        assert nodes[0] == reached[0] == deliv[0] == 0
    nodes, reached, deliv, tot = HR.topic_hops(n, root, live, 0, parent)
    assert not nodes.any() and not reached.any() and not deliv.any() and tot == 0  # idle: not even nodes


def test_helper_all_live_heap_is_closed_form():
    for n, n_msgs in ((2, 1), (64, 3), (100, 7), (1025, 2)):
        nodes, reached, deliv, tot = HR.topic_hops(n, 0, np.ones(n, dtype=np.uint8), n_msgs, heap_tree(n))
        want = np.zeros(HR.COLS, dtype=np.int64)
        h, left = 1, n - 1
        while left:
            want[h] = min(2 ** h, left)  # 2^h a level, the last one cut
            left -= want[h]
            h += 1
        assert np.array_equal(nodes, want) and np.array_equal(reached, want)
        assert np.array_equal(deliv, n_msgs * want) and tot == n_msgs * (n - 1)


def test_helper_path_clamps_into_the_last_column():
    n = 300
    parent = np.arange(-1, n - 1).astype(np.uint32)  # peer p's upstream is p - 1
    parent[0] = O.NONE
    live = np.ones(n, dtype=np.uint8)
    nodes, reached, deliv, tot = HR.topic_hops(n, 0, live, 3, parent)
    assert tot == 3 * 299 == deliv.sum() and nodes.sum() == reached.sum() == 299
    assert (nodes[1:255] == 1).all() and nodes[255] == 45  # levels 255 .. 299
    assert np.array_equal(reached, nodes) and np.array_equal(deliv, 3 * nodes)
    live[280] = 0  # cut inside the clamped column
    nodes, reached, deliv, tot = HR.topic_hops(n, 0, live, 3, parent)
    assert nodes[255] == 45 and reached[255] == 25 and deliv[255] == 75 and tot == 3 * 279


def test_helper_window_sum():
    rng = np.random.default_rng(7)
    n, root = 200, 4
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    p0, p1 = random_tree(rng, n, root), random_tree(rng, n, root)
    a, b = HR.topic_hops(n, root, live, 3, p0), HR.topic_hops(n, root, live, 5, p1)
    wn, wr, wd, wt = HR.window_hops(n, live, [(root, 3, p0), (root, 5, p1), (root, 0, p0)])
    assert wn.dtype == wr.dtype == wd.dtype == np.uint64 and wn.shape == (3, HR.COLS)
    for k, w in enumerate((wn, wr, wd)):
        assert np.array_equal(w[0], a[k].astype(np.uint64)) and np.array_equal(w[1], b[k].astype(np.uint64))
        assert not w[2].any()
    assert wt == a[3] + b[3]
