"""ps_drain_topics_begin / ps_drain_topics_end without a GPU: the argument
checks that need no engine, the binding and the header.  (With an engine the
calls need a device: tests/test_gpu_drain_topics_async.py.)"""
import ctypes as C
import os

import numpy as np

import psengine as PE
from test_drain_topics_cpu import Outs, U32P

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")


def fake_engine():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (4 KiB of zeros nobody reads)."""
    buf = C.create_string_buffer(4096)
    return buf, C.cast(buf, C.c_void_p)


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    assert lib.ps_drain_topics_begin(None, t.ctypes.data_as(U32P), 1, 0, 0, 0) == -1  # PS_E_INVAL
    assert lib.ps_drain_topics_begin(None, None, 0, 0, 0, 0) == -1
    o = Outs()
    assert lib.ps_drain_topics_end(None, *o.args()) == -1
    assert o.untouched()
    assert lib.ps_drain_topics_end(None, *([None] * 10)) == -1


def test_null_outputs_are_invalid():
    lib = PE.load()
    keep, h = fake_engine()
    for drop in range(10):  # each output in turn
        o = Outs()
        assert lib.ps_drain_topics_end(h, *o.args(drop)) == -1
        assert o.untouched()
    assert keep.raw == bytes(4096)


def test_topics_announced_but_not_given():
    lib = PE.load()
    keep, h = fake_engine()
    assert lib.ps_drain_topics_begin(h, None, 1, 0, 0, 0) == -1
    assert lib.ps_drain_topics_begin(h, None, 3, 10, 10, 10) == -1
    assert keep.raw == bytes(4096)


def test_prototypes_are_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert len(protos["ps_drain_topics_begin"][2]) == 6
    assert len(protos["ps_drain_topics_end"][2]) == 11
    with open(HEADER) as f:
        text = f.read()
    assert "int ps_drain_topics_begin(ps_engine* e, const uint32_t* topic, size_t n, size_t exc_cap, size_t list_cap," in text
    assert "int ps_drain_topics_end(ps_engine* e," in text
    lib = PE.load()
    assert lib.ps_drain_topics_begin.argtypes == protos["ps_drain_topics_begin"][2]
    assert lib.ps_drain_topics_end.argtypes == protos["ps_drain_topics_end"][2]


def test_engine_methods_exist():
    import inspect

    sig = inspect.signature(PE.Engine.drain_topics_begin)
    assert list(sig.parameters) == ["self", "topics", "exc_cap", "list_cap", "id_cap"]
    assert [sig.parameters[k].default for k in ("exc_cap", "list_cap", "id_cap")] == [0, 0, 0]
    sig = inspect.signature(PE.Engine.drain_topics_end)
    assert list(sig.parameters) == ["self", "copy"] and sig.parameters["copy"].default is True


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5
