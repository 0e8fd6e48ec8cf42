"""ps_drain_shared without a GPU: the argument checks that need no engine,
the binding and the header.  (With an engine the call needs a device:
tests/test_gpu_drain_shared.py.)"""
import ctypes as C
import os

import numpy as np

import psengine as PE

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def call(lib, h, t, p, n, lists, off, n_lists, total):
    def u32(a):
        return a.ctypes.data_as(U32P) if a is not None else None

    return lib.ps_drain_shared(h, u32(t), u32(p), n, u32(lists), off.ctypes.data_as(U64P) if off is not None else None,
                               0, None, 0, C.byref(n_lists) if n_lists is not None else None,
                               C.byref(total) if total is not None else None)


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    lists = np.zeros(1, dtype=np.uint32)
    off = np.zeros(1, dtype=np.uint64)
    assert call(lib, None, t, t, 1, lists, off, C.c_uint32(), C.c_uint64()) == -1  # PS_E_INVAL
    assert lib.ps_drain_shared(None, None, None, 0, None, None, 0, None, 0, None, None) == -1


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    lists = np.full(1, 0x55555555, dtype=np.uint32)
    off = np.full(1, 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    n_lists, total = C.c_uint32(0xBBBB), C.c_uint64(0xCCCC)
    assert call(lib, h, t, t, 1, lists, None, n_lists, total) == -1  # no list_off_out
    assert call(lib, h, t, t, 1, lists, off, None, total) == -1  # no n_lists_out
    assert call(lib, h, t, t, 1, lists, off, n_lists, None) == -1  # no total_out
    assert call(lib, h, None, t, 1, lists, off, n_lists, total) == -1  # queries announced, no topics
    assert call(lib, h, t, None, 1, lists, off, n_lists, total) == -1  # ... no peers
    assert call(lib, h, t, t, 1, None, off, n_lists, total) == -1  # ... no list_out
    # a capacity without a buffer
    assert lib.ps_drain_shared(h, t.ctypes.data_as(U32P), t.ctypes.data_as(U32P), 1, lists.ctypes.data_as(U32P),
                               off.ctypes.data_as(U64P), 0, None, 8, C.byref(n_lists), C.byref(total)) == -1
    # nothing was written
    assert lists[0] == 0x55555555 and off[0] == 0xAAAAAAAAAAAAAAAA
    assert n_lists.value == 0xBBBB and total.value == 0xCCCC


def test_prototype_is_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert "ps_drain_shared" in protos
    assert len(protos["ps_drain_shared"][2]) == 11
    with open(HEADER) as f:
        assert "int ps_drain_shared(ps_engine* e" in f.read()
    assert hasattr(PE.Engine, "drain_shared")


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5
