"""ps_peer_report / ps_report_track / ps_report_take without a GPU: the header
and the binding, the argument checks that need no engine, and the reference
helper (tests/report_ref.py) against the four references' closed forms.  (An
engine needs a device: the checks that need one, PS_E_NOTREADY among them, are
in tests/test_gpu_report.py.)"""
import ctypes as C
import os
import re

import numpy as np

import cut_ref as CR
import downstream_ref as DR
import hops_ref as HR
import load_ref as LR
import oracle as O
import psengine as PE
import report_ref as RR
from test_downstream_cpu import heap_subtree, heap_tree

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
FILL = 0xABABABABABABABAB
SIZE = C.sizeof(PE.Report)


def report(n=8, only=None):
    """A ps_report over eleven filled arrays (only: the names that get a pointer)."""
    arrays = {k: np.full(n, FILL, dtype=np.uint64) for k in RR.NAMES}
    rep = PE.Report()
    for k, a in arrays.items():
        if only is None or k in only:
            setattr(rep, k, a.ctypes.data_as(U64P))
    return arrays, rep


def untouched(arrays):
    return all((a == FILL).all() for a in arrays.values())


def test_header_declares_the_block():
    with open(HEADER) as f:
        text = f.read()
    for line in ("#define PS_REPORT_LOAD       0x1u", "#define PS_REPORT_HOPS       0x2u", "#define PS_REPORT_DOWNSTREAM 0x4u",
                 "#define PS_REPORT_CUT        0x8u", "#define PS_REPORT_ALL        0xFu",
                 "typedef struct ps_report {", "  uint64_t *recv, *sent;", "  uint64_t *nodes, *reached, *deliv;",
                 "  uint64_t *below, *carried;", "  uint64_t *missed, *cuts, *orphaned, *lost;", "} ps_report;",
                 "int ps_peer_report(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what,\n"
                 "                   const ps_report* out, size_t out_size);",
                 "int ps_report_track(ps_engine* e, const uint32_t* topic, size_t n, uint32_t what);",
                 "int ps_report_take(ps_engine* e, const ps_report* out, size_t out_size,\n"
                 "                   uint64_t* n_windows_out, uint64_t* n_skipped_out);"):
        assert line in text, line
    assert "#define PS_ABI_VERSION 5" in " ".join(text.split())
    # the defining property is stated by reference to the four calls, not restated
    flat = " ".join(re.sub(r"\n \*", " ", text).split())
    for phrase in ("every array of a selected section is bit for bit what that call writes",
                   "A pointer of a section that is not selected is not touched",
                   "a NULL pointer inside a selected section is skipped", "out_size is sizeof(ps_report)"):
        assert phrase in flat, phrase


def test_binding_matches_the_header():
    assert (PE.REPORT_LOAD, PE.REPORT_HOPS, PE.REPORT_DOWNSTREAM, PE.REPORT_CUT, PE.REPORT_ALL) == (1, 2, 4, 8, 15)
    assert (RR.LOAD, RR.HOPS, RR.DOWNSTREAM, RR.CUT, RR.ALL) == (1, 2, 4, 8, 15)
    assert [k for k, _ in PE.Report._fields_] == list(RR.NAMES) and SIZE == 11 * C.sizeof(C.c_void_p)
    assert tuple(names for _, names in PE.REPORT_SECTIONS) == tuple(names for _, names in RR.SECTIONS)
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert len(protos["ps_peer_report"][2]) == 6
    assert len(protos["ps_report_track"][2]) == 4
    assert len(protos["ps_report_take"][2]) == 5
    lib = PE.load()
    for name in ("ps_peer_report", "ps_report_track", "ps_report_take"):
        assert getattr(lib, name).restype is C.c_int
    for name in ("peer_report", "report_track", "report_take"):
        assert hasattr(PE.Engine, name), name


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    a, rep = report()
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    assert lib.ps_peer_report(None, tp, 1, PE.REPORT_ALL, C.byref(rep), SIZE) == -1  # PS_E_INVAL
    assert lib.ps_peer_report(None, None, 0, PE.REPORT_LOAD, C.byref(rep), SIZE) == -1
    assert lib.ps_report_track(None, tp, 1, PE.REPORT_ALL) == -1
    assert lib.ps_report_track(None, None, 0, PE.REPORT_ALL) == -1
    assert lib.ps_report_take(None, C.byref(rep), SIZE, C.byref(nw), C.byref(nsk)) == -1
    assert untouched(a) and nw.value == 0xCCCC and nsk.value == 0xDDDD


def test_arguments_are_checked_before_the_engine_is_touched():
    """Any non-NULL engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    a, rep = report()
    nw, nsk = C.c_uint64(0xCCCC), C.c_uint64(0xDDDD)
    assert lib.ps_peer_report(h, tp, 1, 0, C.byref(rep), SIZE) == -1  # what == 0
    assert lib.ps_peer_report(h, tp, 1, 0x10, C.byref(rep), SIZE) == -1  # a bit outside PS_REPORT_ALL
    assert lib.ps_peer_report(h, tp, 1, 0x1F, C.byref(rep), SIZE) == -1
    assert lib.ps_peer_report(h, tp, 1, PE.REPORT_ALL, C.byref(rep), SIZE - 8) == -1  # wrong out_size
    assert lib.ps_peer_report(h, tp, 1, PE.REPORT_ALL, C.byref(rep), SIZE + 8) == -1
    assert lib.ps_peer_report(h, tp, 1, PE.REPORT_ALL, C.byref(rep), 0) == -1
    assert lib.ps_peer_report(h, tp, 1, PE.REPORT_ALL, None, SIZE) == -1  # no struct
    assert lib.ps_peer_report(h, None, 1, PE.REPORT_ALL, C.byref(rep), SIZE) == -1  # topics announced, none given
    # a selected section whose pointers are all NULL, whatever the others hold
    for sec, names in RR.SECTIONS:
        _, part = report(only=[k for k in RR.NAMES if k not in names])
        assert lib.ps_peer_report(h, tp, 1, PE.REPORT_ALL, C.byref(part), SIZE) == -1, names
        assert lib.ps_peer_report(h, tp, 1, sec, C.byref(part), SIZE) == -1, names
    assert lib.ps_peer_report(h, tp, 1, PE.REPORT_ALL, C.byref(PE.Report()), SIZE) == -1
    assert lib.ps_report_track(h, tp, 1, 0) == -1
    assert lib.ps_report_track(h, tp, 1, 0x10) == -1
    assert lib.ps_report_track(h, None, 1, PE.REPORT_ALL) == -1
    assert lib.ps_report_take(h, C.byref(rep), SIZE - 8, C.byref(nw), C.byref(nsk)) == -1
    assert lib.ps_report_take(h, None, SIZE, C.byref(nw), C.byref(nsk)) == -1
    assert lib.ps_report_take(h, C.byref(rep), SIZE, None, C.byref(nsk)) == -1
    assert lib.ps_report_take(h, C.byref(rep), SIZE, C.byref(nw), None) == -1
    assert untouched(a) and nw.value == 0xCCCC and nsk.value == 0xDDDD


# ---- the reference helper ----------------------------------------------------------

def path(n):
    parent = np.arange(-1, n - 1).astype(np.uint32)
    parent[0] = O.NONE
    return parent


def test_helper_path_is_the_four_closed_forms():
    """The 300-peer path cut at depth 150: what each reference gives alone."""
    n, c, j = 300, 3, 150
    live = np.ones(n, dtype=np.uint8)
    live[j] = 0
    r = RR.window_report(n, live, [(0, c, path(n), None)])
    assert set(r) == set(RR.NAMES)
    # load: peers 1 .. j - 1 receive c; all but the last forward to one child (the dead one too is sent to)
    assert (r["recv"][1:j] == c).all() and not r["recv"][j:].any() and r["recv"][0] == 0
    assert (r["sent"][:j] == c).all() and not r["sent"][j:].any()
    # hops: one node a level; the last column takes levels 255 .. 299
    assert (r["nodes"][0, 1:255] == 1).all() and r["nodes"][0, 255] == n - 255 and r["nodes"][0, 0] == 0
    assert (r["reached"][0, 1:j] == 1).all() and not r["reached"][0, j:].any()
    assert np.array_equal(r["deliv"], r["reached"] * c)
    # downstream: peer i has n - 1 - i nodes below; the deliveries among them
    assert np.array_equal(r["below"], np.arange(n - 1, -1, -1).astype(np.uint64))
    assert np.array_equal(r["carried"][:j], (c * np.arange(j - 1, -1, -1)).astype(np.uint64)) and not r["carried"][j:].any()
    # cut: one cut point, the dead peer
    assert r["cuts"].sum() == 1 and r["cuts"][j] == 1 and r["orphaned"][j] == n - 1 - j and r["lost"][j] == c * (n - j)
    assert not r["missed"][:j].any() and (r["missed"][j:] == c).all()
    for k, want in (("recv", LR.window_load(n, live, [(0, c, path(n), None)])[0]),
                    ("below", DR.window_downstream(n, live, [(0, c, path(n))])[0]),
                    ("lost", CR.window_cut(n, live, [(0, c, path(n))])[3]),
                    ("deliv", HR.window_hops(n, live, [(0, c, path(n))])[2])):
        assert r[k].dtype == np.uint64 and np.array_equal(r[k], want), k


def test_helper_heap_with_one_dead_inner_node():
    n, c = 127, 4
    parent = heap_tree(n)
    live = np.ones(n, dtype=np.uint8)
    live[5] = 0  # the subtree of 5 holds 31 nodes
    size = heap_subtree(5, n, 2)
    assert size == 31
    r = RR.window_report(n, live, [(0, c, parent, None)])
    assert int(r["recv"].sum()) == c * (n - 1 - size) == int(r["deliv"].sum())
    assert r["nodes"][0, 1:7].tolist() == [2, 4, 8, 16, 32, 64] and r["reached"][0, 1:7].tolist() == [2, 3, 6, 12, 24, 48]
    assert r["below"][5] == size - 1 and r["carried"][5] == 0 and r["below"][0] == n - 1
    assert r["carried"][0] == c * (n - 1 - size) and r["carried"][2] == c * (heap_subtree(2, n, 2) - 1 - size)
    assert r["cuts"].sum() == 1 and r["cuts"][5] == 1 and r["orphaned"][5] == size - 1 and r["lost"][5] == c * size
    assert int(r["missed"].sum()) == c * size == int(r["lost"].sum())
    assert r["sent"][2] == 2 * c and r["sent"][5] == 0  # the dead child is sent to; it sends nothing


def test_helper_masks_rows_and_meshes():
    n = 64
    parent = heap_tree(n)
    live = np.ones(n, dtype=np.uint8)
    live[3] = 0
    # a diamond beside the tree: 0 -> 1, 2; 1 -> 3; 2 -> 3
    rp = np.zeros(n + 1, dtype=np.uint32)
    rp[1:] = 2
    rp[2:] = 3
    rp[3:] = 4
    mesh = (rp, np.array([1, 2, 3, 3], dtype=np.uint32))
    topics = [(0, 2, None, mesh), (0, 5, parent, None), (0, 0, parent, None)]
    full = RR.window_report(n, live, topics)
    for what in range(1, 16):
        r = RR.window_report(n, live, topics, what)
        assert tuple(r) == RR.names_of(what)
        for k in r:
            assert np.array_equal(r[k], full[k]), (what, k)
    # the mesh feeds the load section alone; its hop row and the idle topic's stay zero
    assert not full["nodes"][0].any() and not full["nodes"][2].any() and full["nodes"][1].any()
    tree_only = RR.window_report(n, live, topics[1:])
    for k in ("below", "carried", "missed", "cuts", "orphaned", "lost"):
        assert np.array_equal(full[k], tree_only[k]), k
    assert int(full["recv"].sum()) > int(tree_only["recv"].sum())
    both = RR.add(RR.add({}, full), full)
    assert all(np.array_equal(both[k], 2 * full[k]) for k in full)
