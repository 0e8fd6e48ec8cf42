"""ps_spread_track / ps_spread_take without a GPU: the reference helper
(tests/spread_track_ref.py) against per-window spread_ref.window_spread, the
bound the tracked pass rests on -- no hop lies beyond the window's last round
-- on every graph the GPU file runs, the header and the binding, and the
argument checks that need no engine.  (With an engine the calls need a device:
tests/test_gpu_spread_track.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_ref as MR
import psengine as PE
import spread_ref as SR
import spread_track_ref as TR

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
E_INVAL = -1
COUNTS = (0xC0C0, 0xC1C1)  # n_windows, n_truncated

BUILDERS = ([("specials", s) for s in (0, 1, 2)] + [("hub", d) for d in (63, 64, 65, 129, 600)] +
            [("detour", k) for k in (8, 40, 300)])


def build(kind, arg):
    if kind == "specials":
        return MR.mesh_with_specials(300, arg)
    return MR.hub_mesh(arg) if kind == "hub" else MR.detour(arg)


def topic_of(g, c, live=None):
    rp, cl, root, lv = g[:4]
    live = lv if live is None else live
    F = MR.flood(rp, cl, root, live)
    return (rp, cl, root, F.level >= 0, c), F


# ---- the reference helper ----------------------------------------------------------

def test_one_window_is_window_spread():
    g = MR.mesh_with_specials(300)
    t, _ = topic_of(g, 70)
    want = SR.window_spread(300, [t])
    got = TR.windows_spread(300, [[t]])
    assert got["n_windows"] == 1
    for name in TR.NAMES:
        assert got[name].dtype == np.uint64 and np.array_equal(got[name], want[name]), name


def test_three_windows_with_differing_counts_and_masks():
    """Two topics over one peer space, three windows: c and the live mask
    differ from window to window, one topic idle in the second."""
    g0, g1 = MR.mesh_with_specials(300), MR.hub_mesh(65)
    n = 300
    rng = np.random.default_rng(7)
    wins, parts = [], []
    for w, (c0, c1) in enumerate(((70, 5), (0, 64), (65, 4136))):
        live = (rng.random(n) > 0.1 * w).astype(np.uint8)
        live[0] = 1
        rp1 = np.concatenate([g1[0], np.full(n - len(g1[3]), g1[0][-1], dtype=g1[0].dtype)])
        t0, _ = topic_of(g0, c0, live)
        F1 = MR.flood(rp1, g1[1], g1[2], live)
        t1 = (rp1, g1[1], g1[2], F1.level >= 0, c1)
        wins.append([t0, t1])
        parts.append(SR.window_spread(n, [t0, t1]))
    got = TR.windows_spread(n, wins)
    assert got["n_windows"] == 3
    for name in TR.NAMES:
        want = sum(p[name].astype(object) for p in parts)
        assert np.array_equal(got[name].astype(object), want % (1 << 64)), name
    # the idle topic's window added nothing to its rows
    alone = TR.windows_spread(n, [wins[0], wins[2]])
    assert np.array_equal(alone["reached"][0], got["reached"][0]) and np.array_equal(alone["unreached"][:1], got["unreached"][:1])
    # stranded and dup are the sums of their parts
    assert np.array_equal(got["stranded"], sum(p["stranded"] for p in parts))
    assert np.array_equal(got["dup"].astype(np.int64), sum(p["dup"].astype(np.int64) for p in parts))
    assert TR.windows_spread(n, [])["n_windows"] == 0


def test_truncated_window_of_a_chain():
    """detour(40) cut after 10 launches: hops 1 .. 10 visited, 11 .. 39
    stranded, the forwarders at hops 0 .. 9 have sent."""
    t, F = topic_of(MR.detour(40), 3)
    r = TR.truncated(t, 10)
    assert r["truncated"] and r["stranded"][0] == 29
    assert (r["reached"][0, 1:11] == 1).all() and not r["reached"][0, 11:].any()
    assert (r["deliv"][0, 1:11] == 3).all() and r["copies"].sum() == 30
    whole = TR.truncated(t, 40)
    want = SR.window_spread(41, [t])
    assert not whole["truncated"]
    for name in TR.NAMES:
        assert np.array_equal(whole[name], want[name]), name
    assert TR.truncated(t, 39)["truncated"] and TR.truncated(t, 39)["stranded"][0] == 0  # (the last forwarder has no child)


# ---- the bound: no hop beyond the window's last round --------------------------------

@pytest.mark.parametrize("kind,arg", BUILDERS)
def test_no_hop_beyond_the_floods_rounds(kind, arg):
    """A forwarder's BFS distance within F is the round the flood reached it
    in, so the deepest hop is the flood's round count; messages started at
    round s arrive s rounds later, and the window runs until the last does."""
    g = build(kind, arg)
    t, F = topic_of(g, 5)
    S = SR.topic_spread(*t)
    assert F.rounds == F.level.max() and S.level.max() <= F.rounds
    assert np.array_equal(S.level[S.level > 0], F.level[S.level > 0]) and S.stranded == 0
    starts = np.arange(8)
    per = F.per_round(starts, length=1024)
    last = int(np.flatnonzero(per).max())
    assert S.level.max() + starts.max() <= last == F.rounds + starts.max()


# ---- header and binding ----------------------------------------------------------------

def test_prototypes_are_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert protos["ps_spread_track"][2][1:] == [U32P, C.c_size_t]
    assert protos["ps_spread_take"][2][1:] == [U64P] * 8
    with open(HEADER) as f:
        text = f.read()
    assert "int ps_spread_track(ps_engine* e, const uint32_t* topic, size_t n);" in text
    assert "int ps_spread_take(ps_engine* e,\n" in text
    assert "uint64_t* n_windows_out, uint64_t* n_truncated_out);" in text
    flat = " ".join(re.sub(r"\n \*", " ", text).split())
    for phrase in ("nothing is refused or skipped for being a mesh", "level launches 0 .. r whole",
                   "There is no n_skipped: nothing is skipped", "0 on a healthy engine, reported and not assumed like stranded",
                   "PSAMD_SPREAD_TRACK_LEVELS=n caps a tracked window's level launches"):
        assert phrase in flat, phrase
    # ps_topic_spread has its tracker now: only the asynchronous blocking form is missing
    assert "There is no tracker and no asynchronous form" not in flat
    assert "There is no asynchronous form of this call" in flat
    for name in ("spread_track", "spread_take"):
        assert hasattr(PE.Engine, name), name
    lib = PE.load()
    for name in ("ps_spread_track", "ps_spread_take"):
        assert getattr(lib, name).restype is C.c_int


def test_abi_version_unchanged():
    with open(HEADER) as f:
        assert "#define PS_ABI_VERSION 5" in " ".join(f.read().split())
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5


def take_args():
    arrays = [np.full(4, 0xAB, dtype=np.uint64) for _ in range(6)]
    return arrays, [C.c_uint64(v) for v in COUNTS]


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    assert lib.ps_spread_track(None, t.ctypes.data_as(U32P), 1) == E_INVAL
    assert lib.ps_spread_track(None, None, 0) == E_INVAL
    arrays, counts = take_args()
    assert lib.ps_spread_take(None, *(a.ctypes.data_as(U64P) for a in arrays), *(C.byref(c) for c in counts)) == E_INVAL
    assert all((a == 0xAB).all() for a in arrays) and [c.value for c in counts] == list(COUNTS)


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    assert lib.ps_spread_track(h, None, 2) == E_INVAL  # topics announced, none given
    arrays, counts = take_args()
    ptrs = [a.ctypes.data_as(U64P) for a in arrays]
    assert lib.ps_spread_take(h, *ptrs, None, C.byref(counts[1])) == E_INVAL
    assert lib.ps_spread_take(h, *ptrs, C.byref(counts[0]), None) == E_INVAL
    assert lib.ps_spread_take(h, None, None, None, None, None, None, None, None) == E_INVAL
    assert all((a == 0xAB).all() for a in arrays) and [c.value for c in counts] == list(COUNTS)
