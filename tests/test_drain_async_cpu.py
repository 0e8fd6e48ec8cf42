"""ps_drain_begin / ps_drain_end without a GPU: the argument checks that need
no engine, the binding and the header.  (With an engine the calls need a
device: tests/test_gpu_drain_async.py.)"""
import ctypes as C
import os

import numpy as np

import psengine as PE

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    assert lib.ps_drain_begin(None, t.ctypes.data_as(u32p), t.ctypes.data_as(u32p), 1) == -1  # PS_E_INVAL
    assert lib.ps_drain_begin(None, None, None, 0) == -1
    off, ids, total = u64p(), u32p(), C.c_uint64()
    assert lib.ps_drain_end(None, C.byref(off), C.byref(ids), C.byref(total)) == -1
    assert lib.ps_drain_end(None, None, None, None) == -1


def test_null_outputs_are_invalid():
    """The outputs are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    off, ids, total = u64p(), u32p(), C.c_uint64()
    assert lib.ps_drain_end(h, None, C.byref(ids), C.byref(total)) == -1
    assert lib.ps_drain_end(h, C.byref(off), None, C.byref(total)) == -1
    assert lib.ps_drain_end(h, C.byref(off), C.byref(ids), None) == -1
    assert lib.ps_drain_begin(h, None, None, 1) == -1  # queries announced, none given


def test_prototypes_are_bound_and_declared():
    names = {p[0] for p in PE.PROTOTYPES}
    with open(HEADER) as f:
        text = f.read()
    for name in ("ps_drain_begin", "ps_drain_end"):
        assert name in names
        assert f"int {name}(ps_engine* e" in text
    assert hasattr(PE.Engine, "drain_begin") and hasattr(PE.Engine, "drain_end")


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5
