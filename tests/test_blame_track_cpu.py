"""ps_blame_track / ps_blame_take without a GPU: the header and the binding, the
argument checks that need no engine, and the reference helper
(tests/blame_track_ref.py) in closed form and against cut_ref summed over the
same windows.  (With an engine the calls need a device:
tests/test_gpu_blame_track.py.)"""
import ctypes as C
import os
import re

import numpy as np

import blame_ref as BR
import blame_track_ref as TR
import cut_ref as CR
import psengine as PE
from test_blame_cpu import SENTINEL, lent
from test_cut_cpu import path
from test_gpu_drain_batch import random_tree

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
COUNTS = (0xC0C0, 0xC1C1, 0xC2C2, 0xC3C3)  # n_windows, n_skipped, total, stored


def take_outs():
    off, ptrs, _ = lent()
    return off, ptrs, [C.c_uint64(v) for v in COUNTS]


def take_untouched(off, ptrs, counts):
    return (C.cast(off, C.c_void_p).value == SENTINEL and all(C.cast(p, C.c_void_p).value == SENTINEL for p in ptrs) and
            [c.value for c in counts] == list(COUNTS))


def test_prototypes_are_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    PP32, PP64 = C.POINTER(U32P), C.POINTER(U64P)
    assert protos["ps_blame_track"][2][1:] == [U32P, C.c_size_t, C.c_size_t]
    assert protos["ps_blame_take"][2][1:] == [PP64, PP32, PP32, PP32, PP32, PP32, U64P, U64P, U64P, U64P]
    with open(HEADER) as f:
        text = f.read()
    assert "int ps_blame_track(ps_engine* e, const uint32_t* topic, size_t n, size_t rec_cap);" in text
    assert "int ps_blame_take(ps_engine* e,\n" in text
    assert "uint64_t* n_windows_out, uint64_t* n_skipped_out,\n                  uint64_t* total_out, uint64_t* stored_out);" in text
    flat = " ".join(re.sub(r"\n \*", " ", text).split())
    for phrase in ("rec_off[w*n + i] .. rec_off[w*n + i + 1]", "Overflow is sticky and leaves a prefix",
                   "total == cap is no overflow", "valid until the next ps_blame_take, ps_blame_track or ps_destroy",
                   "the view is separate from ps_topic_blame's"):
        assert phrase in flat, phrase
    # ps_topic_blame's records have their tracker: what the header still calls missing is something else
    assert "records are variable-size per window, and the sink machinery" not in flat
    assert "its tracker is for one rank only" in flat and "a sharded tracker needs collective exchanges" in flat
    for name in ("blame_track", "blame_take"):
        assert hasattr(PE.Engine, name), name
    lib = PE.load()
    for name in ("ps_blame_track", "ps_blame_take"):
        assert getattr(lib, name).restype is C.c_int


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    assert lib.ps_blame_track(None, t.ctypes.data_as(U32P), 1, 0) == -1  # PS_E_INVAL
    assert lib.ps_blame_track(None, None, 0, 0) == -1
    off, ptrs, counts = take_outs()
    assert lib.ps_blame_take(None, C.byref(off), *(C.byref(p) for p in ptrs), *(C.byref(c) for c in counts)) == -1
    assert take_untouched(off, ptrs, counts)


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    assert lib.ps_blame_track(h, None, 2, 0) == -1  # topics announced, none given
    off, ptrs, counts = take_outs()
    recs = [C.byref(p) for p in ptrs]
    cnt = [C.byref(c) for c in counts]
    assert lib.ps_blame_take(h, None, *recs, *cnt) == -1  # no rec_off
    for i in range(4):  # each count pointer alone
        assert lib.ps_blame_take(h, C.byref(off), *recs, *(None if j == i else c for j, c in enumerate(cnt))) == -1, i
    assert lib.ps_blame_take(h, None, None, None, None, None, None, None, None, None, None) == -1
    assert take_untouched(off, ptrs, counts)


# ---- the reference helper ----------------------------------------------------------

def test_helper_path_with_a_dead_peer_over_three_windows():
    """A path 0-1-...-(n-1), peer d dead, 150 messages through a window of 64:
    three windows of (64, 64, 22).  Each holds the peers d..n-1, cut at d, hop =
    own index, with the window's messages missed."""
    n, d = 50, 17
    parent = path(n)
    live = np.ones(n, dtype=np.uint8)
    live[d] = 0
    counts = (64, 64, 22)
    wins = [TR.window([BR.topic_blame(n, 0, live, c, parent)], [np.arange(n)]) for c in counts]
    r = TR.compose(wins, 1)
    k = n - d
    assert r["rec_off"].dtype == np.uint64 and r["rec_off"].tolist() == [0, k, 2 * k, 3 * k]
    assert (r["n_windows"], r["n_skipped"], r["total"], r["stored"]) == (3, 0, 3 * k, 3 * k)
    assert np.array_equal(r["peer"], np.tile(np.arange(d, n), 3)) and np.array_equal(r["hop"], r["peer"])
    assert (r["cut_peer"] == d).all() and (r["cut_hop"] == d).all()
    assert np.array_equal(r["missed"], np.repeat(counts, k))
    assert all(r[key].dtype == np.uint32 for key in TR.KEYS)
    for w, c in enumerate(counts):
        s = TR.slice_of(r, 1, w, 0)
        assert np.array_equal(s[0], np.arange(d, n)) and (s[4] == c).all()
    # caps: the prefix, and total == cap is no overflow
    for cap, over in ((1, True), (k, True), (3 * k - 1, True), (3 * k, False), (3 * k + 5, False)):
        c, o = TR.capped(r, cap)
        assert o == over and c["stored"] == min(cap, 3 * k) and c["total"] == 3 * k
        assert np.array_equal(c["rec_off"], r["rec_off"]) and all(np.array_equal(c[key], r[key][:c["stored"]]) for key in TR.KEYS)


def test_helper_idle_skipped_and_empty_rows():
    n = 30
    parent = path(n)
    live = np.ones(n, dtype=np.uint8)
    live[20] = 0
    tab = BR.topic_blame(n, 0, live, 3, parent)
    idle = BR.topic_blame(n, 0, live, 0, parent)
    order = [np.arange(n)] * 3
    r = TR.compose([TR.window([None, tab, idle], order), TR.window([idle, None, idle], order),
                    TR.window([tab, tab, None], order)], 3, n_skipped=3)
    assert r["rec_off"].tolist() == [0, 0, 10, 10, 10, 10, 10, 20, 30, 30]
    assert (r["n_windows"], r["n_skipped"], r["total"]) == (3, 3, 30)
    assert all(x.size == 0 for x in TR.slice_of(r, 3, 1, 1))
    empty = TR.compose([], 3)
    assert empty["rec_off"].tolist() == [0] and empty["total"] == 0 and all(empty[k].size == 0 for k in TR.KEYS)


def test_helper_against_cut_ref_summed_over_the_windows():
    """Random trees under random masks, two topics, three windows each: the
    records' bincounts equal cut_ref.window_cut summed over the same windows."""
    rng = np.random.default_rng(19)
    for case in range(6):
        n = int(rng.integers(60, 500))
        roots = [int(rng.integers(0, n)) for _ in range(2)]
        parents = [random_tree(rng, n, r) for r in roots]
        orders = [np.concatenate([[r], np.setdiff1d(np.arange(n), [r])]) for r in roots]  # any order, the root first
        wins = []
        want = [np.zeros(n, dtype=np.uint64) for _ in range(4)]
        for w in range(3):
            live = (rng.random(n) > (0.02, 0.1, 0.3)[(case + w) % 3]).astype(np.uint8)
            live[roots] = 1
            c = [int(rng.integers(0, 90)), int(rng.integers(1, 90))]
            wins.append(TR.window([BR.topic_blame(n, roots[i], live, c[i], parents[i]) for i in (0, 1)], orders))
            cut = CR.window_cut(n, live, [(roots[i], c[i], parents[i]) for i in (0, 1)])
            for acc, x in zip(want, cut[:4]):
                acc += x
        r = TR.compose(wins, 2)
        assert r["total"] == r["peer"].size > 0
        wts = r["missed"].astype(np.int64)
        u64 = lambda x: x.astype(np.uint64)
        own = r["peer"] == r["cut_peer"]
        assert np.array_equal(u64(np.bincount(r["peer"], weights=wts, minlength=n)), want[0])
        assert np.array_equal(u64(np.bincount(r["cut_peer"], weights=wts, minlength=n)), want[3])
        assert np.array_equal(u64(np.bincount(r["peer"][own], minlength=n)), want[1])
        assert int(own.sum()) == int(want[1].sum())
