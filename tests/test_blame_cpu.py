"""ps_topic_blame / ps_blame without a GPU: the argument checks that need no
engine, the binding and the header, and the reference helper
(tests/blame_ref.py) against closed forms and against cut_ref's four sums.
(With an engine the calls need a device: tests/test_gpu_blame.py.)"""
import ctypes as C
import os
import re

import numpy as np

import blame_ref as BR
import cut_ref as CR
import oracle as O
import psengine as PE
from test_cut_cpu import path
from test_downstream_cpu import heap_tree
from test_gpu_drain_batch import random_tree

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
FILL32 = 0xABABABAB
SENTINEL = 0x5A5A5A5A


def lent():
    """ps_topic_blame's seven outputs, preset: the pointers to a sentinel address, the total to a pattern."""
    off = U64P()
    C.cast(C.pointer(off), C.POINTER(C.c_void_p))[0] = SENTINEL
    ptrs = [U32P() for _ in range(5)]
    for p in ptrs:
        C.cast(C.pointer(p), C.POINTER(C.c_void_p))[0] = SENTINEL
    return off, ptrs, C.c_uint64(0xCCCC)


def lent_untouched(off, ptrs, total):
    return (C.cast(off, C.c_void_p).value == SENTINEL and all(C.cast(p, C.c_void_p).value == SENTINEL for p in ptrs) and
            total.value == 0xCCCC)


def outs(n=8):
    a = [np.full(n, FILL32, dtype=np.uint32) for _ in range(4)]
    return a, [x.ctypes.data_as(U32P) for x in a]


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    off, ptrs, total = lent()
    byref = [C.byref(p) for p in ptrs]
    assert lib.ps_topic_blame(None, tp, 1, C.byref(off), *byref, C.byref(total)) == -1  # PS_E_INVAL
    assert lib.ps_topic_blame(None, None, 0, C.byref(off), *byref, C.byref(total)) == -1
    assert lent_untouched(off, ptrs, total)
    a, p = outs()
    assert lib.ps_blame(None, tp, tp, 1, *p) == -1
    assert lib.ps_blame(None, None, None, 0, *p) == -1
    assert all((x == FILL32).all() for x in a)


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    off, ptrs, total = lent()
    byref = [C.byref(p) for p in ptrs]
    assert lib.ps_topic_blame(h, None, 1, C.byref(off), *byref, C.byref(total)) == -1  # topics announced, none given
    assert lib.ps_topic_blame(h, tp, 1, None, *byref, C.byref(total)) == -1  # no rec_off
    assert lib.ps_topic_blame(h, tp, 1, C.byref(off), *byref, None) == -1  # no total
    assert lib.ps_topic_blame(h, None, 0, None, *byref, C.byref(total)) == -1
    assert lib.ps_topic_blame(h, None, 0, C.byref(off), None, None, None, None, None, None) == -1
    assert lent_untouched(off, ptrs, total)
    a, p = outs()
    assert lib.ps_blame(h, None, tp, 1, *p) == -1  # queries announced, no topics
    assert lib.ps_blame(h, tp, None, 1, *p) == -1  # ... no peers
    assert lib.ps_blame(h, tp, tp, 1, None, None, None, None) == -1  # all four outputs NULL
    assert lib.ps_blame(h, None, None, 0, None, None, None, None) == -1
    assert all((x == FILL32).all() for x in a)


def test_prototypes_are_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert len(protos["ps_topic_blame"][2]) == 10
    assert len(protos["ps_blame"][2]) == 8
    with open(HEADER) as f:
        text = f.read()
    assert "int ps_topic_blame(ps_engine* e, const uint32_t* topic, size_t n,\n" in text
    for name in ("rec_off_out", "rec_peer_out", "rec_cut_peer_out", "rec_hop_out", "rec_cut_hop_out", "rec_missed_out"):
        assert re.search(r"const uint(32|64)_t\*\* " + name + r"[,;) ]", text), name
    assert "                   uint64_t* total_out);" in text
    assert "int ps_blame(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n,\n" in text
    assert "             uint32_t* cut_peer_out, uint32_t* hop_out,\n" in text
    assert "             uint32_t* cut_hop_out, uint32_t* missed_out);" in text
    # the C argument kinds against the binding's, one by one
    PP32, PP64 = C.POINTER(U32P), C.POINTER(U64P)
    assert protos["ps_topic_blame"][2][1:] == [U32P, C.c_size_t, PP64, PP32, PP32, PP32, PP32, PP32, U64P]
    assert protos["ps_blame"][2][1:] == [U32P, U32P, C.c_size_t, U32P, U32P, U32P, U32P]
    # the semantics are stated
    flat = " ".join(re.sub(r"\n \*", " ", text).split())  # (the comment's line breaks and stars folded away)
    for phrase in ("u if its parent is full, and else cut(parent(u))", "no clamp at PS_MAX_ROUNDS",
                   "ps_drain_topics' exceptions for the same request", "valid until the next ps_topic_blame or ps_destroy",
                   "There is no tracker and no _begin / _end form"):
        assert phrase in flat, phrase
    for name in ("topic_blame", "blame"):
        assert hasattr(PE.Engine, name), name
    lib = PE.load()
    for name in ("ps_topic_blame", "ps_blame"):
        assert getattr(lib, name).restype is C.c_int


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5


# ---- the reference helper ----------------------------------------------------------

def test_helper_path_one_dead_peer():
    """A path 0-1-...-(n-1) with peer d dead: the records are the peers d..n-1,
    all with cut_peer d, cut_hop d, hop = own index, missed = c."""
    n, c = 300, 3
    parent = path(n)
    for d in (1, 150, 298, 299):
        live = np.ones(n, dtype=np.uint8)
        live[d] = 0
        tab = BR.topic_blame(n, 0, live, c, parent)
        peer, cut_peer, hop, cut_hop, missed = BR.records(tab, np.arange(n))
        assert np.array_equal(peer, np.arange(d, n))
        assert (cut_peer == d).all() and (cut_hop == d).all() and np.array_equal(hop, peer) and (missed == c).all()
        assert all(x.dtype == np.uint32 for x in (peer, cut_peer, hop, cut_hop, missed))
        # the queries: the root and the full rows, the cut point, a peer behind it
        q = BR.queries(tab, [0, d - 1, d, n - 1])
        assert q[0].tolist() == [BR.NONE, BR.NONE, d, d] and q[2].tolist() == [BR.NONE, BR.NONE, d, d]
        assert q[1].tolist() == [0, d - 1, d, n - 1] and q[3].tolist() == [0, 0, c, c]


def test_helper_path_two_dead_peers():
    """Two dead peers a < b on one path: everything from a down blames a, and
    b is no cut point."""
    n, c = 120, 2
    parent = path(n)
    for a, b in ((1, 2), (5, 60), (40, 119), (118, 119)):
        live = np.ones(n, dtype=np.uint8)
        live[[a, b]] = 0
        peer, cut_peer, hop, cut_hop, missed = BR.records(BR.topic_blame(n, 0, live, c, parent), np.arange(n))
        assert np.array_equal(peer, np.arange(a, n)) and np.array_equal(hop, peer)
        assert (cut_peer == a).all() and (cut_hop == a).all() and (missed == c).all()
        assert b in peer and cut_peer[b - a] == a


def test_helper_idle_and_all_live_have_no_records():
    n = 100
    parent = heap_tree(n, 3)
    live = np.ones(n, dtype=np.uint8)
    for tab in (BR.topic_blame(n, 0, live, 5, parent), BR.topic_blame(n, 0, live, 0, parent)):
        assert all(x.size == 0 for x in BR.records(tab, np.arange(n)))
        cut_peer, hop, cut_hop, missed = BR.queries(tab, np.arange(n))
        assert (cut_peer == BR.NONE).all() and (cut_hop == BR.NONE).all() and not missed.any()
        assert hop[0] == 0 and hop[1] == 1 and hop[4] == 2  # the levels stand, idle or not
    live[7] = 0
    assert all(x.size == 0 for x in BR.records(BR.topic_blame(n, 0, live, 0, parent), np.arange(n)))  # idle: nothing missed


def test_helper_a_peer_outside_the_node_space():
    rng = np.random.default_rng(5)
    n, root, outside = 300, 3, 299
    parent = random_tree(rng, n, root)
    parent[parent == outside] = root
    parent[outside] = O.NONE
    live = (rng.random(n) > 0.1).astype(np.uint8)
    live[root] = 1
    tab = BR.topic_blame(n, root, live, 4, parent)
    assert not tab.member[outside] and tab.member.sum() == n - 1
    q = BR.queries(tab, [outside, root])
    assert [int(x[0]) for x in q] == [BR.NONE, BR.NONE, BR.NONE, 0]
    assert [int(x[1]) for x in q] == [BR.NONE, 0, BR.NONE, 0]


def test_helper_against_cut_ref_on_random_trees():
    """The four bincount identities against cut_ref's (missed, cuts, orphaned,
    lost), on random trees under random dead masks."""
    rng = np.random.default_rng(12)
    for case in range(8):
        n = int(rng.integers(50, 600))
        root = int(rng.integers(0, n))
        parent = random_tree(rng, n, root)
        live = (rng.random(n) > (0.02, 0.1, 0.3)[case % 3]).astype(np.uint8)
        live[root] = 1
        c = int(rng.integers(1, 200))
        missed, cuts, orphaned, lost, _, members = CR.topic_cut(n, root, live, c, parent)
        assert members == n
        tab = BR.topic_blame(n, root, live, c, parent)
        order = np.concatenate([[root], np.setdiff1d(np.arange(n), [root])])  # any order that puts the root first
        peer, cut_peer, hop, cut_hop, miss = BR.records(tab, order)
        assert peer.size == int((missed > 0).sum()) > 0
        w = miss.astype(np.int64)
        assert np.array_equal(np.bincount(cut_peer, weights=w, minlength=n).astype(np.int64), lost)
        assert np.array_equal(np.bincount(peer, weights=w, minlength=n).astype(np.int64), missed)
        assert np.array_equal(np.bincount(peer[peer == cut_peer], minlength=n), cuts)
        assert np.array_equal(np.bincount(cut_peer[peer != cut_peer], minlength=n), orphaned)
        assert (cut_hop <= hop).all() and np.array_equal(cut_hop == hop, peer == cut_peer)
        assert np.array_equal(tab.hop[cut_peer], cut_hop)
