"""ps_sink_set_topics / ps_sink_take_topics without a GPU: the argument checks
that need no engine, the binding and the header.  (With an engine the calls
need a device: tests/test_gpu_sink_topics.py.)"""
import ctypes as C
import os

import numpy as np

import psengine as PE

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def take_outs():
    tl, nn, nf, eo, ep, el, lo, mp = U32P(), U64P(), U64P(), U64P(), U32P(), U32P(), U64P(), U32P()
    n_windows, n_lists, total = C.c_uint32(0xAAAA), C.c_uint32(0xBBBB), C.c_uint64(0xCCCC)
    outs = (tl, nn, nf, eo, ep, el, lo, mp, n_windows, n_lists, total)
    return outs, [C.byref(x) for x in outs]


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    tp = t.ctypes.data_as(U32P)
    assert lib.ps_sink_set_topics(None, tp, 1, 0, 0, 0) == -1  # PS_E_INVAL
    assert lib.ps_sink_set_topics(None, None, 0, 0, 0, 0) == -1
    outs, refs = take_outs()
    assert lib.ps_sink_take_topics(None, *refs) == -1
    assert lib.ps_sink_take_topics(None, *([None] * 11)) == -1
    assert not any(bool(p) for p in outs[:8])
    assert (outs[8].value, outs[9].value, outs[10].value) == (0xAAAA, 0xBBBB, 0xCCCC)


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    assert lib.ps_sink_set_topics(h, None, 1, 0, 0, 0) == -1  # topics announced, none given
    assert lib.ps_sink_set_topics(h, None, 3, 8, 8, 8) == -1
    outs, refs = take_outs()
    for missing in range(11):
        args = list(refs)
        args[missing] = None
        assert lib.ps_sink_take_topics(h, *args) == -1, missing
    # nothing was written
    assert not any(bool(p) for p in outs[:8])
    assert (outs[8].value, outs[9].value, outs[10].value) == (0xAAAA, 0xBBBB, 0xCCCC)


def test_prototypes_are_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert len(protos["ps_sink_set_topics"][2]) == 6
    assert len(protos["ps_sink_take_topics"][2]) == 12
    with open(HEADER) as f:
        text = f.read()
    assert ("int ps_sink_set_topics(ps_engine* e, const uint32_t* topic, size_t n, size_t exc_cap, size_t list_cap, "
            "size_t id_cap);") in text
    assert "int ps_sink_take_topics(ps_engine* e," in text
    assert "uint32_t* n_windows_out, uint32_t* n_lists_out, uint64_t* total_out);" in text
    assert hasattr(PE.Engine, "sink_set_topics") and hasattr(PE.Engine, "sink_take_topics")
    lib = PE.load()
    assert lib.ps_sink_set_topics.restype is C.c_int and lib.ps_sink_take_topics.restype is C.c_int


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5
