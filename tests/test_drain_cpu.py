"""ps_drain without a GPU: the argument checks that need no engine.  (With
an engine the call needs a device: tests/test_gpu_drain_batch.py.)"""
import ctypes as C

import numpy as np

import psengine as PE


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    off = np.zeros(2, dtype=np.uint64)
    total = C.c_uint64()
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = lib.ps_drain(None, t.ctypes.data_as(u32p), t.ctypes.data_as(u32p), 1, off.ctypes.data_as(u64p), None, 0,
                      C.byref(total))
    assert rc == -1  # PS_E_INVAL
    assert lib.ps_drain(None, None, None, 0, None, None, 0, None) == -1


def test_prototype_is_bound():
    assert "ps_drain" in {p[0] for p in PE.PROTOTYPES}
