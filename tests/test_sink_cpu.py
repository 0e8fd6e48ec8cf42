"""ps_sink_set / ps_sink_take without a GPU: the argument checks that need no
engine, the binding and the header.  (With an engine the calls need a
device: tests/test_gpu_sink.py.)"""
import ctypes as C
import os

import numpy as np

import psengine as PE

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def take_outs():
    wp, op, mp = U32P(), U64P(), U32P()
    n_windows, n_lists, total = C.c_uint32(0xAAAA), C.c_uint32(0xBBBB), C.c_uint64(0xCCCC)
    return (wp, op, mp, n_windows, n_lists, total), [C.byref(x) for x in (wp, op, mp, n_windows, n_lists, total)]


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    assert lib.ps_sink_set(None, tp, tp, 1, 0, 0) == -1  # PS_E_INVAL
    assert lib.ps_sink_set(None, None, None, 0, 0, 0) == -1
    _, refs = take_outs()
    assert lib.ps_sink_take(None, *refs) == -1
    assert lib.ps_sink_take(None, None, None, None, None, None, None) == -1


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    assert lib.ps_sink_set(h, None, tp, 1, 0, 0) == -1  # queries announced, no topics
    assert lib.ps_sink_set(h, tp, None, 1, 0, 0) == -1  # ... no peers
    assert lib.ps_sink_set(h, None, None, 3, 8, 8) == -1
    outs, refs = take_outs()
    for missing in range(6):
        args = list(refs)
        args[missing] = None
        assert lib.ps_sink_take(h, *args) == -1, missing
    # nothing was written
    wp, op, mp, n_windows, n_lists, total = outs
    assert not wp and not op and not mp
    assert n_windows.value == 0xAAAA and n_lists.value == 0xBBBB and total.value == 0xCCCC


def test_prototypes_are_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert len(protos["ps_sink_set"][2]) == 6
    assert len(protos["ps_sink_take"][2]) == 7
    with open(HEADER) as f:
        text = f.read()
    assert ("int ps_sink_set(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, size_t list_cap, "
            "size_t id_cap);") in text
    assert "int ps_sink_take(ps_engine* e, const uint32_t** win_list_out, const uint64_t** list_off_out" in text
    assert hasattr(PE.Engine, "sink_set") and hasattr(PE.Engine, "sink_take")
    lib = PE.load()
    assert lib.ps_sink_set.restype is C.c_int and lib.ps_sink_take.restype is C.c_int


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5
