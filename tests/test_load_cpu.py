"""ps_peer_load / ps_load_track / ps_load_take without a GPU: the argument
checks that need no engine, the binding and the header, and the reference
helper (tests/load_ref.py) against the oracle's own totals.  (With an engine
the calls need a device: tests/test_gpu_load.py.)"""
import ctypes as C
import os

import numpy as np

import load_ref as LR
import oracle as O
import psengine as PE
from test_gpu_drain_batch import random_mesh2, random_tree

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
FILL = 0xABABABABABABABAB


def outs(n=4):
    recv = np.full(n, FILL, dtype=np.uint64)
    sent = np.full(n, FILL, dtype=np.uint64)
    return recv, sent, recv.ctypes.data_as(U64P), sent.ctypes.data_as(U64P)


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    recv, sent, rp, sp = outs()
    nw = C.c_uint64(0xCCCC)
    assert lib.ps_peer_load(None, tp, 1, rp, sp) == -1  # PS_E_INVAL
    assert lib.ps_peer_load(None, None, 0, rp, sp) == -1
    assert lib.ps_load_track(None, tp, 1) == -1
    assert lib.ps_load_track(None, None, 0) == -1
    assert lib.ps_load_take(None, rp, sp, C.byref(nw)) == -1
    assert lib.ps_load_take(None, None, None, None) == -1
    assert (recv == FILL).all() and (sent == FILL).all() and nw.value == 0xCCCC


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    recv, sent, rp, sp = outs()
    assert lib.ps_peer_load(h, None, 1, rp, sp) == -1  # topics announced, none given
    assert lib.ps_peer_load(h, None, 3, rp, None) == -1
    assert lib.ps_peer_load(h, tp, 1, None, None) == -1  # both outputs NULL
    assert lib.ps_peer_load(h, None, 0, None, None) == -1
    assert lib.ps_load_track(h, None, 1) == -1
    assert lib.ps_load_track(h, None, 7) == -1
    assert lib.ps_load_take(h, rp, sp, None) == -1  # no window count
    assert lib.ps_load_take(h, None, None, None) == -1
    assert (recv == FILL).all() and (sent == FILL).all()


def test_prototypes_are_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert len(protos["ps_peer_load"][2]) == 5
    assert len(protos["ps_load_track"][2]) == 3
    assert len(protos["ps_load_take"][2]) == 4
    with open(HEADER) as f:
        text = f.read()
    assert "int ps_peer_load(ps_engine* e, const uint32_t* topic, size_t n,\n" in text
    assert "uint64_t* recv_out, uint64_t* sent_out);          /* [n_peers] each, either may be NULL */" in text
    assert "int ps_load_track(ps_engine* e, const uint32_t* topic, size_t n);" in text
    assert "int ps_load_take(ps_engine* e, uint64_t* recv_out, uint64_t* sent_out, /* [n_peers], nullable */" in text
    assert "                 uint64_t* n_windows_out);" in text
    for name in ("peer_load", "load_track", "load_take"):
        assert hasattr(PE.Engine, name), name
    lib = PE.load()
    for name in ("ps_peer_load", "ps_load_track", "ps_load_take"):
        assert getattr(lib, name).restype is C.c_int


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5


# ---- the reference helper ----------------------------------------------------------

def masked(rng, n, root, frac=0.1):
    live = (rng.random(n) > frac).astype(np.uint8)
    live[root] = 1
    return live


def test_helper_tree_sums():
    """Sum recv = the oracle's delivery total; for a tree, what the members
    send to live children is what is received."""
    rng = np.random.default_rng(5)
    n, root = 300, 3
    parent = random_tree(rng, n, root)
    outside = 299
    parent[parent == outside] = root
    parent[outside] = O.NONE
    live = masked(rng, n, root)
    for n_msgs in (1, 65, 130):
        recv, sent, tot = LR.topic_load(n, root, live, n_msgs, parent=parent)
        assert recv.sum() == tot > 0
        assert recv[root] == 0 and recv[outside] == 0 and sent[outside] == 0
        assert set(np.unique(recv)) <= {0, n_msgs}
        assert LR.sent_live(n, root, live, n_msgs, parent=parent).sum() == recv.sum()
        assert sent.sum() >= recv.sum()  # (children count whether live or not)
        rp, _ = O.parents_to_csr(parent)
        assert sent[root] == n_msgs * int(rp[root + 1] - rp[root])
    recv, sent, tot = LR.topic_load(n, root, live, 0, parent=parent)
    assert not recv.any() and not sent.any() and tot == 0


def test_helper_all_live_tree_is_closed_form():
    rng = np.random.default_rng(6)
    n, root = 50, 0
    parent = random_tree(rng, n, root)
    recv, sent, tot = LR.topic_load(n, root, np.ones(n, dtype=np.uint8), 7, parent=parent)
    want = np.full(n, 7)
    want[root] = 0
    assert np.array_equal(recv, want) and tot == 7 * (n - 1)
    kids = np.bincount(parent[parent != O.NONE], minlength=n)
    assert np.array_equal(sent, 7 * kids) and sent.sum() == recv.sum()


def test_helper_mesh_and_window_sum():
    rng = np.random.default_rng(7)
    n, root = 200, 4
    rp, cl = random_mesh2(rng, n, root)
    live = masked(rng, n, root)
    recv, sent, tot = LR.topic_load(n, root, live, 3, csr=(rp, cl))
    assert recv.sum() == tot and recv[root] == 0
    # a mesh node forwards once: the copies written to live children are the
    # deliveries plus the duplicates, so no fewer than the deliveries
    assert LR.sent_live(n, root, live, 3, csr=(rp, cl)).sum() >= recv.sum()
    parent = random_tree(rng, n, root)
    r2, s2, t2 = LR.topic_load(n, root, live, 5, parent=parent)
    wr, ws, wt = LR.window_load(n, live, [(root, 3, None, (rp, cl)), (root, 5, parent, None), (root, 0, parent, None)])
    assert wr.dtype == ws.dtype == np.uint64
    assert np.array_equal(wr, (recv + r2).astype(np.uint64)) and np.array_equal(ws, (sent + s2).astype(np.uint64))
    assert wt == tot + t2
