"""ps_drain_topics without a GPU: the argument checks that need no engine,
the binding and the header.  (With an engine the call needs a device:
tests/test_gpu_drain_topics.py.)"""
import ctypes as C
import os

import numpy as np

import psengine as PE

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psengine.h")
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
SENT = 0x5555


class Outs:
    """The ten outputs, each preset to a sentinel address / value."""

    def __init__(self):
        self.p32 = [U32P() for _ in range(4)]  # topic_list, exc_peer, exc_list, msg
        self.p64 = [U64P() for _ in range(4)]  # n_nodes, n_full, exc_off, list_off
        self.n_lists, self.total = C.c_uint32(SENT), C.c_uint64(SENT)

    def args(self, drop=None):
        a = [C.byref(self.p32[0]), C.byref(self.p64[0]), C.byref(self.p64[1]), C.byref(self.p64[2]),
             C.byref(self.p32[1]), C.byref(self.p32[2]), C.byref(self.p64[3]), C.byref(self.p32[3]),
             C.byref(self.n_lists), C.byref(self.total)]
        if drop is not None:
            a[drop] = None
        return a

    def untouched(self):
        return (not any(bool(p) for p in self.p32 + self.p64)) and self.n_lists.value == SENT and self.total.value == SENT


def test_null_engine_is_invalid():
    lib = PE.load()
    t = np.zeros(1, dtype=np.uint32)
    o = Outs()
    assert lib.ps_drain_topics(None, t.ctypes.data_as(U32P), 1, *o.args()) == -1  # PS_E_INVAL
    assert o.untouched()
    assert lib.ps_drain_topics(None, None, 0, *([None] * 10)) == -1


def test_null_arguments_are_invalid():
    """The arguments are checked before the engine is touched: any non-NULL
    engine pointer will do (here 4 KiB of zeros nobody reads)."""
    lib = PE.load()
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    t = np.zeros(1, dtype=np.uint32)
    for drop in range(10):  # each output in turn
        o = Outs()
        assert lib.ps_drain_topics(h, t.ctypes.data_as(U32P), 1, *o.args(drop)) == -1
        assert o.untouched()
    o = Outs()
    assert lib.ps_drain_topics(h, None, 1, *o.args()) == -1  # topics announced, none given
    assert o.untouched()


def test_prototype_is_bound_and_declared():
    protos = {p[0]: p for p in PE.PROTOTYPES}
    assert "ps_drain_topics" in protos
    assert len(protos["ps_drain_topics"][2]) == 13
    with open(HEADER) as f:
        text = f.read()
    assert "int ps_drain_topics(ps_engine* e" in text
    assert "ps_topic_get_parents gives PS_NONE" in text  # who is not part of the answer
    assert hasattr(PE.Engine, "drain_topics")


def test_abi_version_unchanged():
    assert PE.load().ps_abi_version() == 5
    assert PE.ABI_VERSION == 5
