"""ctypes binding of libpsengine.so (include/psengine.h).

This is plumbing for tests and bench.py: every call goes straight into the
C ABI, whose hot path runs only as HIP kernels on the GPU.  There is no CPU
fallback: if the library or a GPU is missing, construction fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _build

NONE = 0xFFFFFFFF
HOP_NONE = 0xFF
MAX_ROUNDS = 256

PS_OK = 0
ERRORS = {
    -1: "PS_E_INVAL", -2: "PS_E_NOMEM", -3: "PS_E_STATE", -4: "PS_E_NOPARENT",
    -5: "PS_E_UNREACHABLE", -6: "PS_E_DEVICE", -7: "PS_E_RANGE", -8: "PS_E_NOTREADY",
}
PART_PEER = 0
PART_SUBTREE = 1
F_RECORD_HOPS = 0x1
F_TIME_KERNELS = 0x2
F_NO_LAZY_SEEN = 0x4
F_COMPACT = 0x8
MODE_COMPACT, MODE_LEVEL_PULL, MODE_FLOOD = 0, 2, 3
# ps_stats.expand_mode -> the kernel that ran the window's rounds
# ps_stats.round_kernel: the launch kind that wrote each round
K_NONE, K_FLOOD, K_PULL, K_PAIR, K_PAIR2, K_EXPAND, K_CHAIN, K_CHAIN2 = 0, 1, 2, 3, 4, 5, 6, 7
ROUND_KERNEL = {K_FLOOD: "k_flood", K_PULL: "k_pull", K_PAIR: "k_pull_pair", K_PAIR2: "k_pull_pair",
                K_EXPAND: "k_expand", K_CHAIN: "k_pull_chain", K_CHAIN2: "k_pull_chain"}
MODE_KERNEL = {MODE_COMPACT: "k_expand", MODE_LEVEL_PULL: "k_pull", MODE_FLOOD: "k_flood"}

# C prototypes exported by libpsengine.so: (name, restype, argtypes)
_P = C.c_void_p
_u32 = C.c_uint32
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)


class Config(C.Structure):
    _fields_ = [("n_peers", C.c_uint32), ("n_topics", C.c_uint32), ("tree_width", C.c_uint32),
                ("tree_max_width", C.c_uint32), ("msg_window", C.c_uint32), ("device", C.c_int32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [("deliveries", C.c_uint64), ("duplicates", C.c_uint64),
                ("frontier_entries", C.c_uint64), ("child_visits", C.c_uint64),
                ("edge_words", C.c_uint64), ("expand_bytes", C.c_uint64),
                ("windows", C.c_uint64), ("rounds", C.c_uint64), ("expand_launches", C.c_uint64),
                ("run_ms", C.c_double), ("expand_ms", C.c_double), ("host_ms", C.c_double),
                ("expand_mode", C.c_uint32), ("flood_rounds", C.c_uint32),
                ("deliveries_per_round", C.c_uint64 * MAX_ROUNDS),
                ("expand_ms_per_round", C.c_float * MAX_ROUNDS),
                ("frontier_per_round", C.c_uint32 * MAX_ROUNDS),
                ("expand_bytes_per_round", C.c_uint64 * MAX_ROUNDS),
                ("round_kernel", C.c_uint8 * MAX_ROUNDS),
                ("plan_max_rounds", C.c_uint32), ("prefix_rounds", C.c_uint32),
                ("overlapped", C.c_uint32), ("xchg_path", C.c_uint32),
                ("xchg_rounds", C.c_uint64), ("xchg_bytes", C.c_uint64),
                ("level_aligned", C.c_uint32), ("reserved2", C.c_uint32)]

    PER_ROUND = ("deliveries_per_round", "expand_ms_per_round", "frontier_per_round", "expand_bytes_per_round",
                 "round_kernel")

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in self.PER_ROUND}
        n = int(self.rounds) + 1 if self.windows == 1 else MAX_ROUNDS
        for k in self.PER_ROUND:
            per = list(getattr(self, k))[:min(n, MAX_ROUNDS)]
            while per and per[-1] == 0:
                per.pop()
            d[k] = per
        return d


class DistConfig(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("partition", C.c_uint32),
                ("split_depth", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class Report(C.Structure):
    """ps_report (include/psengine.h): eleven nullable output pointers."""
    _fields_ = [(k, C.POINTER(C.c_uint64)) for k in
                ("recv", "sent", "nodes", "reached", "deliv", "below", "carried", "missed", "cuts", "orphaned", "lost")]


REPORT_LOAD, REPORT_HOPS, REPORT_DOWNSTREAM, REPORT_CUT, REPORT_ALL = 0x1, 0x2, 0x4, 0x8, 0xF
REPORT_DIST = 0x7  # LOAD | HOPS | DOWNSTREAM: the sections ps_dist_report answers
# the arrays of each section, in ps_report's order
REPORT_SECTIONS = ((REPORT_LOAD, ("recv", "sent")), (REPORT_HOPS, ("nodes", "reached", "deliv")),
                   (REPORT_DOWNSTREAM, ("below", "carried")), (REPORT_CUT, ("missed", "cuts", "orphaned", "lost")))

DIST_F_COPY = 0x1  # loopback: copy the records into the receive buffer (the RCCL data path)
DIST_F_INPLACE = 0x2  # loopback: ghost-fed nodes read the owner's rows in place (no records)
XCHG_NONE, XCHG_ZERO_COPY, XCHG_COPY, XCHG_IN_PLACE = 0, 1, 2, 3  # ps_stats.xchg_path


class PlanOpts(C.Structure):
    """ps_plan_opts (include/psengine.h): the launch-plan knobs."""
    _fields_ = [("flood_top_bytes", C.c_uint64), ("overlap_min_bytes", C.c_uint64),
                ("launch_bytes", C.c_uint64), ("flood", C.c_uint32), ("chain_max", C.c_uint32),
                ("chain_max_groups", C.c_uint32), ("chain_tail", C.c_uint32), ("chain_words", C.c_uint32),
                ("flood_words", C.c_uint32), ("pad_words", C.c_uint32), ("overlap", C.c_uint32),
                ("overlap_min_rounds", C.c_uint32), ("xchg_overlap", C.c_int32), ("gpu_build", C.c_uint32),
                ("flood_spin_ticks", C.c_uint32), ("chain_nt", C.c_uint32), ("chain_waves", C.c_uint32),
                ("flood_min_rounds", C.c_uint32), ("align_groups", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class MessageC(C.Structure):
    """ps_message (include/psengine.h): pubsub.go:146-153 Message."""
    _fields_ = [("type", C.c_int32), ("data", _u8p), ("data_len", C.c_size_t),
                ("peers", C.POINTER(C.c_char_p)), ("n_peers", C.c_size_t),
                ("tree_width", C.c_int64), ("tree_max_width", C.c_int64), ("num_peers", C.c_int64)]


class MessageBuf(C.Structure):
    """ps_message_buf: caller-owned decode target."""
    _fields_ = [("type", C.c_int32), ("reserved", C.c_int32), ("data", _u8p),
                ("data_cap", C.c_size_t), ("data_len", C.c_size_t), ("peers", C.c_char_p),
                ("peers_cap", C.c_size_t), ("peers_len", C.c_size_t), ("n_peers", C.c_size_t),
                ("tree_width", C.c_int64), ("tree_max_width", C.c_int64), ("num_peers", C.c_int64)]


ABI_VERSION = 5  # PS_ABI_VERSION of include/psengine.h this binding mirrors

PROTOTYPES = [
    ("ps_version", C.c_char_p, []),
    ("ps_abi_version", C.c_uint32, []),
    ("ps_abi_check", C.c_int, [C.c_uint32, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    ("ps_create", C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    ("ps_destroy", None, [_P]),
    ("ps_last_error", C.c_char_p, [_P]),
    ("ps_topic_create", C.c_int, [_P, _u32, _u32, _u32, _u32]),
    ("ps_topic_close", C.c_int, [_P, _u32]),
    ("ps_topic_join", C.c_int, [_P, _u32, _u32p, C.c_size_t, _i32p]),
    ("ps_topic_leave", C.c_int, [_P, _u32, _u32p, C.c_size_t]),
    ("ps_topic_drop", C.c_int, [_P, _u32, _u32p, C.c_size_t]),
    ("ps_topic_set_tree", C.c_int, [_P, _u32, _u32, _u32p]),
    ("ps_topic_set_children", C.c_int, [_P, _u32, _u32, _u32p, _u32p]),
    ("ps_topic_get_parents", C.c_int, [_P, _u32, _u32p]),
    ("ps_topic_depth", C.c_int, [_P, _u32, _u32p, _u32p]),
    ("ps_set_live", C.c_int, [_P, _u8p]),
    ("ps_set_flags", C.c_int, [_P, _u32]),
    ("ps_plan_opts_default", C.c_int, [C.POINTER(PlanOpts)]),
    ("ps_get_plan_opts", C.c_int, [_P, C.POINTER(PlanOpts)]),
    ("ps_set_plan_opts", C.c_int, [_P, C.POINTER(PlanOpts)]),
    ("ps_publish", C.c_int, [_P, _u32p, C.c_size_t, _u32p]),
    ("ps_publish_at", C.c_int, [_P, _u32p, _u32p, C.c_size_t, _u32p]),
    ("ps_run", C.c_int, [_P, C.POINTER(Stats)]),
    ("ps_run_async", C.c_int, [_P]),
    ("ps_wait", C.c_int, [_P, C.POINTER(Stats)]),
    ("ps_read_hops", C.c_int, [_P, _u32, _u8p]),
    ("ps_read_delivered", C.c_int, [_P, _u32, _u8p]),
    ("ps_read_peer_messages", C.c_int, [_P, _u32, _u32, _u32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ps_drain", C.c_int, [_P, _u32p, _u32p, C.c_size_t, _u64p, _u32p, C.c_size_t, _u64p]),
    ("ps_drain_shared", C.c_int, [_P, _u32p, _u32p, C.c_size_t, _u32p, _u64p, C.c_size_t, _u32p, C.c_size_t, _u32p,
                                  _u64p]),
    ("ps_drain_begin", C.c_int, [_P, _u32p, _u32p, C.c_size_t]),
    ("ps_drain_end", C.c_int, [_P, C.POINTER(_u64p), C.POINTER(_u32p), _u64p]),
    ("ps_drain_shared_begin", C.c_int, [_P, _u32p, _u32p, C.c_size_t, C.c_size_t, C.c_size_t]),
    ("ps_drain_shared_end", C.c_int, [_P, C.POINTER(_u32p), C.POINTER(_u64p), C.POINTER(_u32p), _u32p, _u64p]),
    ("ps_sink_set", C.c_int, [_P, _u32p, _u32p, C.c_size_t, C.c_size_t, C.c_size_t]),
    ("ps_sink_take", C.c_int, [_P, C.POINTER(_u32p), C.POINTER(_u64p), C.POINTER(_u32p), _u32p, _u32p, _u64p]),
    ("ps_drain_topics", C.c_int, [_P, _u32p, C.c_size_t, C.POINTER(_u32p), C.POINTER(_u64p), C.POINTER(_u64p),
                                  C.POINTER(_u64p), C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_u64p),
                                  C.POINTER(_u32p), _u32p, _u64p]),
    ("ps_drain_topics_begin", C.c_int, [_P, _u32p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    ("ps_drain_topics_end", C.c_int, [_P, C.POINTER(_u32p), C.POINTER(_u64p), C.POINTER(_u64p), C.POINTER(_u64p),
                                      C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_u64p), C.POINTER(_u32p), _u32p,
                                      _u64p]),
    ("ps_sink_set_topics", C.c_int, [_P, _u32p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    ("ps_sink_take_topics", C.c_int, [_P, C.POINTER(_u32p), C.POINTER(_u64p), C.POINTER(_u64p), C.POINTER(_u64p),
                                      C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_u64p), C.POINTER(_u32p), _u32p,
                                      _u32p, _u64p]),
    ("ps_peer_load", C.c_int, [_P, _u32p, C.c_size_t, _u64p, _u64p]),
    ("ps_load_track", C.c_int, [_P, _u32p, C.c_size_t]),
    ("ps_load_take", C.c_int, [_P, _u64p, _u64p, _u64p]),
    ("ps_topic_hops", C.c_int, [_P, _u32p, C.c_size_t, _u64p, _u64p, _u64p]),
    ("ps_hops_track", C.c_int, [_P, _u32p, C.c_size_t]),
    ("ps_hops_take", C.c_int, [_P, _u64p, _u64p, _u64p, _u64p, _u64p]),
    ("ps_peer_downstream", C.c_int, [_P, _u32p, C.c_size_t, _u64p, _u64p]),
    ("ps_downstream_track", C.c_int, [_P, _u32p, C.c_size_t]),
    ("ps_downstream_take", C.c_int, [_P, _u64p, _u64p, _u64p, _u64p]),
    ("ps_peer_cut", C.c_int, [_P, _u32p, C.c_size_t, _u64p, _u64p, _u64p, _u64p]),
    ("ps_cut_track", C.c_int, [_P, _u32p, C.c_size_t]),
    ("ps_cut_take", C.c_int, [_P, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p]),
    ("ps_topic_blame", C.c_int, [_P, _u32p, C.c_size_t, C.POINTER(_u64p), C.POINTER(_u32p), C.POINTER(_u32p),
                                 C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_u32p), _u64p]),
    ("ps_blame", C.c_int, [_P, _u32p, _u32p, C.c_size_t, _u32p, _u32p, _u32p, _u32p]),
    ("ps_blame_track", C.c_int, [_P, _u32p, C.c_size_t, C.c_size_t]),
    ("ps_blame_take", C.c_int, [_P, C.POINTER(_u64p), C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_u32p),
                                C.POINTER(_u32p), C.POINTER(_u32p), _u64p, _u64p, _u64p, _u64p]),
    ("ps_peer_report", C.c_int, [_P, _u32p, C.c_size_t, C.c_uint32, C.POINTER(Report), C.c_size_t]),
    ("ps_report_track", C.c_int, [_P, _u32p, C.c_size_t, C.c_uint32]),
    ("ps_report_take", C.c_int, [_P, C.POINTER(Report), C.c_size_t, _u64p, _u64p]),
    ("ps_dist_report", C.c_int, [_P, _u32p, C.c_size_t, C.c_uint32, C.POINTER(Report), C.c_size_t]),
    ("ps_dist_cut", C.c_int, [_P, _u32p, C.c_size_t, _u64p, _u64p, _u64p, _u64p]),
    ("ps_dist_blame", C.c_int, [_P, _u32p, C.c_size_t, C.POINTER(_u64p), C.POINTER(_u32p), C.POINTER(_u32p),
                                C.POINTER(_u32p), C.POINTER(_u32p), C.POINTER(_u32p), _u64p]),
    ("ps_topic_spread", C.c_int, [_P, _u32p, C.c_size_t, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p]),
    ("ps_spread_track", C.c_int, [_P, _u32p, C.c_size_t]),
    ("ps_spread_take", C.c_int, [_P, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p]),
    ("ps_seen_digest", C.c_int, [_P, _u64p]),
    ("ps_overlapped_windows", C.c_int, [_P, _u64p]),
    ("ps_chain_fill_launches", C.c_int, [_P, _u64p]),
    ("ps_msg_encode", C.c_int, [C.POINTER(MessageC), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ps_msg_decode", C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(MessageBuf), C.POINTER(C.c_size_t)]),
    ("ps_dist_unique_id", C.c_int, [C.POINTER(C.c_uint8)]),
    ("ps_dist_init", C.c_int, [_P, C.POINTER(DistConfig), C.POINTER(C.c_uint8)]),
    ("ps_device_count", C.c_int, [_i32p]),
    ("ps_dist_ipc_id", C.c_int, [C.POINTER(C.c_uint8)]),
    ("ps_dist_init_ipc", C.c_int, [_P, C.POINTER(DistConfig), C.POINTER(C.c_uint8)]),
    ("ps_loopback_create", C.c_int, [C.c_int32, C.POINTER(_P)]),
    ("ps_loopback_destroy", None, [_P]),
    ("ps_dist_init_loopback", C.c_int, [_P, C.POINTER(DistConfig), _P]),
    ("ps_partition_owner", C.c_int, [_u32, _u32, _u32p, _u32, C.POINTER(DistConfig), _i32p]),
]

# ps_graph_get tables (include/psengine_plan.h, bound by psengine.plan): test
# support, not the drop-in boundary
G_NODE_PEER, G_NODE_PARENT, G_NODE_TOPIC, G_NODE_FLAGS, G_ROW_PTR, G_COL, G_TOPIC, G_BUILD = range(8)
NODE_LIVE, NODE_INTERNAL, NODE_SPLIT = 1, 2, 4
BUILD_FIELDS = ("gpu_builds", "host_builds", "fallback_stall", "fallback_attempts", "fallback_capacity",
                "fallback_depth", "redo_grid", "redo_order", "redo_depth", "last_kind", "last_attempts")
BUILD_KINDS = {0: None, 1: "gpu", 2: "host"}


def graph_get(L, h, what: int, index: int = 0) -> np.ndarray:
    """ps_graph_get(what, index) of engine handle h as a uint64 array."""
    n = C.c_size_t()
    rc = L.ps_graph_get(h, what, index, None, 0, C.byref(n))
    if rc not in (PS_OK, -7):
        raise EngineError(rc, (L.ps_last_error(h) or b"ps_graph_get").decode())
    out = np.zeros(max(1, n.value), dtype=np.uint64)
    rc = L.ps_graph_get(h, what, index, _p(out, C.c_uint64), out.shape[0], C.byref(n))
    if rc != PS_OK:
        raise EngineError(rc, (L.ps_last_error(h) or b"ps_graph_get").decode())
    return out[:n.value]


def graph_topic(v) -> dict:
    """PS_GRAPH_TOPIC's values by name."""
    d = {k: int(x) for k, x in zip(("exists", "nbase", "n_nodes", "depth", "max_deg", "top_levels"), v)}
    depth = d["depth"]
    d["level_off"] = v[6:6 + depth + 2].astype(np.int64)
    d["level_internal"] = v[6 + depth + 2:6 + 2 * depth + 3].astype(np.int64)
    return d


def build_report(v) -> dict:
    """PS_GRAPH_BUILD's values by name; last_kind as "gpu" / "host" / None;
    "fallbacks" and "redos" are the sums over their reasons."""
    d = {k: int(x) for k, x in zip(BUILD_FIELDS, v)}
    d["last_kind"] = BUILD_KINDS[d["last_kind"]]
    d["fallbacks"] = sum(d[k] for k in BUILD_FIELDS if k.startswith("fallback_"))
    d["redos"] = sum(d[k] for k in BUILD_FIELDS if k.startswith("redo_"))
    return d

_lib = None


def lib_path() -> str:
    return _build.LIB


def load(build_if_missing: bool = False):
    """Loads libpsengine.so and binds every prototype (raises if absent)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_build.LIB):
            if not build_if_missing:
                raise FileNotFoundError(
                    f"{_build.LIB} missing: run __graft_entry__.build() (no CPU fallback exists)")
            _build.build()
        # (A/B tools: another build of the library, only under PSAMD_AB=1)
        ab = os.environ.get("PSENGINE_LIB_AB") if os.environ.get("PSAMD_AB") == "1" else None
        L = C.CDLL(ab or _build.LIB)
        for name, res, args in PROTOTYPES:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        # the structs this module declares must match the library's layouts
        rc = L.ps_abi_check(ABI_VERSION, C.sizeof(Config), C.sizeof(Stats), C.sizeof(PlanOpts),
                            C.sizeof(DistConfig))
        if rc != 0:
            raise RuntimeError(f"libpsengine ABI mismatch: {L.ps_last_error(None).decode()}")
        _lib = L
    return _lib


class EngineError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


def _u32arr(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _queries(topics, peers):
    """A drain's queries as the C calls take them: the two contiguous uint32
    arrays (kept alive by the caller) and their pointers."""
    t = np.ascontiguousarray(topics, dtype=np.uint32)
    p = np.ascontiguousarray(peers, dtype=np.uint32)
    if t.ndim != 1 or t.shape != p.shape:
        raise ValueError("topics and peers must be 1-d arrays of one length")
    return t, p, _p(t, C.c_uint32), _p(p, C.c_uint32)


def _view(ptr, shape, dtype) -> np.ndarray:
    """The engine's memory at ptr as an array of `shape` (an int: 1-d); an
    empty array of `dtype` where it holds no element (ptr is not read)."""
    shape = shape if isinstance(shape, tuple) else (shape,)
    return np.ctypeslib.as_array(ptr, shape=shape) if all(shape) else np.empty(shape, dtype=dtype)


class Engine:
    """One engine = one GPU's worth of topics (NewTopicManager, pubsub.go:26-31)."""

    _pub_arr = None  # the last uint32 array published and its ctypes pointer
    _pub_ptr = None

    def __init__(self, n_peers: int, n_topics: int = 1, tree_width: int = 2,
                 tree_max_width: int = 5, msg_window: int = 65536, device: int = 0,
                 record_hops: bool = False, time_kernels: bool = False, seed: int = 1,
                 flags: int = 0, plan: dict | None = None):
        """plan: launch-plan options to set right away (ps_set_plan_opts)."""
        L = load()
        self.n_peers = n_peers
        self.n_topics = n_topics
        self.seed = seed
        f = flags | (F_RECORD_HOPS if record_hops else 0) | (F_TIME_KERNELS if time_kernels else 0)
        cfg = Config(n_peers, n_topics, tree_width, tree_max_width, msg_window, device, f, 0, seed)
        self.flags = f
        h = _P()
        rc = L.ps_create(C.byref(cfg), C.byref(h))
        if rc != PS_OK:
            raise EngineError(rc, "ps_create failed (is a GPU visible?)")
        self._h = h
        self._L = L
        self._drain_n = []  # (kind: 0 plain, 1 shared, 2 topics; entries) of the drains begun and not ended
        self._sink_n = 0  # standing queries (sink_set)
        self._hops_n = 0  # standing topics (hops_track): the rows hops_take's arrays hold
        self._spread_n = 0  # standing topics (spread_track): the rows spread_take's arrays hold
        if plan:
            self.set_plan(**plan)

    def close(self):
        if getattr(self, "_h", None):
            self._L.ps_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int) -> int:
        if rc < 0:
            raise EngineError(rc, self._L.ps_last_error(self._h).decode())
        return rc

    @staticmethod
    def topic_seed(seed: int, topic: int) -> int:
        """Redirect tie-break seed of a topic created with ps_topic_create."""
        return (seed ^ (0xA5A5A5A5 * (topic + 1))) & ((1 << 64) - 1)

    # topics
    def topic_create(self, topic: int, root: int, tree_width: int = 0, tree_max_width: int = 0):
        self._check(self._L.ps_topic_create(self._h, topic, root, tree_width, tree_max_width))

    def topic_close(self, topic: int):
        self._check(self._L.ps_topic_close(self._h, topic))

    def join(self, topic: int, peers, check: bool = True) -> np.ndarray:
        p = _u32arr(peers)
        st = np.zeros(p.shape[0], dtype=np.int32)
        rc = self._L.ps_topic_join(self._h, topic, _p(p, C.c_uint32), p.shape[0],
                                   _p(st, C.c_int32))
        if check:
            self._check(rc)
        return st

    def leave(self, topic: int, peers):
        p = _u32arr(peers)
        self._check(self._L.ps_topic_leave(self._h, topic, _p(p, C.c_uint32), p.shape[0]))

    def drop(self, topic: int, peers):
        p = _u32arr(peers)
        self._check(self._L.ps_topic_drop(self._h, topic, _p(p, C.c_uint32), p.shape[0]))

    def set_tree(self, topic: int, root: int, parent):
        par = _u32arr(parent)
        assert par.shape[0] == self.n_peers
        self._check(self._L.ps_topic_set_tree(self._h, topic, root, _p(par, C.c_uint32)))

    def set_children(self, topic: int, root: int, row_ptr, col):
        rp, cl = _u32arr(row_ptr), _u32arr(col)
        assert rp.shape[0] == self.n_peers + 1
        if cl.shape[0] == 0:
            cl = np.zeros(1, dtype=np.uint32)
        self._check(self._L.ps_topic_set_children(self._h, topic, root, _p(rp, C.c_uint32),
                                                  _p(cl, C.c_uint32)))

    def parents(self, topic: int) -> np.ndarray:
        out = np.empty(self.n_peers, dtype=np.uint32)
        self._check(self._L.ps_topic_get_parents(self._h, topic, _p(out, C.c_uint32)))
        return out

    def depth(self, topic: int) -> tuple[int, int]:
        d, n = C.c_uint32(), C.c_uint32()
        self._check(self._L.ps_topic_depth(self._h, topic, C.byref(d), C.byref(n)))
        return d.value, n.value

    def set_flags(self, flags: int):
        """Replaces the PS_F_* flags for the next runs (ps_set_flags)."""
        self._check(self._L.ps_set_flags(self._h, flags))
        self.flags = flags

    def plan_opts(self) -> dict:
        """The effective launch-plan options (ps_get_plan_opts)."""
        o = PlanOpts()
        self._check(self._L.ps_get_plan_opts(self._h, C.byref(o)))
        return o.as_dict()

    def set_plan(self, **kw) -> dict:
        """Changes launch-plan options by name (ps_set_plan_opts), e.g.
        set_plan(flood=0, chain_max=2); returns the effective options."""
        o = PlanOpts()
        self._check(self._L.ps_get_plan_opts(self._h, C.byref(o)))
        for k, v in kw.items():
            if k not in dict(PlanOpts._fields_):
                raise KeyError(f"no plan option {k!r}")
            setattr(o, k, int(v))
        self._check(self._L.ps_set_plan_opts(self._h, C.byref(o)))
        return self.plan_opts()

    def set_time_kernels(self, on: bool):
        self.set_flags((self.flags & ~F_TIME_KERNELS) | (F_TIME_KERNELS if on else 0))

    def set_live(self, live):
        lv = np.ascontiguousarray(live, dtype=np.uint8)
        assert lv.shape[0] == self.n_peers
        self._check(self._L.ps_set_live(self._h, _p(lv, C.c_uint8)))

    # hot path
    def publish(self, topics, start_rounds=None) -> int:
        # (the same uint32 array again, the usual batch loop: its pointer is
        # reused -- ndarray.ctypes costs microseconds per call)
        if topics is self._pub_arr:
            t, tp = topics, self._pub_ptr
        else:
            t = _u32arr(topics)
            tp = _p(t, C.c_uint32)
            if t is topics:
                self._pub_arr, self._pub_ptr = t, tp
        first = C.c_uint32()
        if start_rounds is None:
            self._check(self._L.ps_publish(self._h, tp, t.shape[0], C.byref(first)))
        else:
            s = _u32arr(start_rounds)
            assert s.shape == t.shape
            self._check(self._L.ps_publish_at(self._h, tp, _p(s, C.c_uint32),
                                              t.shape[0], C.byref(first)))
        return first.value

    def run(self) -> Stats:
        st = Stats()
        self._check(self._L.ps_run(self._h, C.byref(st)))
        return st

    def run_async(self):
        """Enqueues the run (ps_run_async); ps_wait / wait() completes it."""
        self._check(self._L.ps_run_async(self._h))

    def wait(self) -> Stats:
        st = Stats()
        self._check(self._L.ps_wait(self._h, C.byref(st)))
        return st

    def hops(self, msg: int) -> np.ndarray:
        out = np.empty(self.n_peers, dtype=np.uint8)
        self._check(self._L.ps_read_hops(self._h, msg, _p(out, C.c_uint8)))
        return out

    def delivered(self, msg: int) -> np.ndarray:
        out = np.empty(self.n_peers, dtype=np.uint8)
        self._check(self._L.ps_read_delivered(self._h, msg, _p(out, C.c_uint8)))
        return out

    def peer_messages(self, topic: int, peer: int) -> np.ndarray:
        """Message ids `peer`'s client.Messages() yields for `topic` from the
        last window, in arrival order (ps_read_peer_messages)."""
        n = C.c_size_t()
        cap = 1024
        while True:
            out = np.empty(cap, dtype=np.uint32)
            rc = self._L.ps_read_peer_messages(self._h, topic, peer, _p(out, C.c_uint32), cap, C.byref(n))
            if rc == -7 and n.value > cap:
                cap = n.value
                continue
            self._check(rc)
            return out[:n.value].copy()

    def drain(self, topics, peers):
        """client.Messages() of many subscribers at once (ps_drain): query q =
        (topics[q], peers[q]); returns (off: uint64[n + 1], ids: uint32[total]),
        query q's message ids, in arrival order, being ids[off[q]:off[q + 1]]."""
        t, p, tp, pp = _queries(topics, peers)
        n = t.size
        off = np.empty(n + 1, dtype=np.uint64)
        total = C.c_uint64()
        op = _p(off, C.c_uint64)
        rc = self._L.ps_drain(self._h, tp, pp, n, op, None, 0, C.byref(total))  # the sizing call
        if rc != -7 or total.value == 0:
            self._check(rc)
            return off, np.empty(0, dtype=np.uint32)
        ids = np.empty(total.value, dtype=np.uint32)
        self._check(self._L.ps_drain(self._h, tp, pp, n, op, _p(ids, C.c_uint32), ids.size, C.byref(total)))
        return off, ids

    def drain_shared(self, topics, peers):
        """drain(topics, peers) with equal lists stored once (ps_drain_shared):
        returns (list_of_query: uint32[n], list_off: uint64[n_lists + 1],
        ids: uint32[total]); query q's ids are list l = list_of_query[q],
        ids[list_off[l]:list_off[l + 1]], or nothing when l == NONE."""
        t, p, tp, pp = _queries(topics, peers)
        n = t.size
        lists = np.empty(n, dtype=np.uint32)
        off = np.zeros(1, dtype=np.uint64)
        n_lists, total = C.c_uint32(), C.c_uint64()
        lp = _p(lists, C.c_uint32)
        rc = self._L.ps_drain_shared(self._h, tp, pp, n, lp, _p(off, C.c_uint64), 0, None, 0, C.byref(n_lists),
                                     C.byref(total))  # the sizing call
        if rc != -7 or n_lists.value == 0:
            self._check(rc)
            return lists, off, np.empty(0, dtype=np.uint32)
        off = np.empty(n_lists.value + 1, dtype=np.uint64)
        ids = np.empty(total.value, dtype=np.uint32)
        self._check(self._L.ps_drain_shared(self._h, tp, pp, n, lp, _p(off, C.c_uint64), n_lists.value,
                                            _p(ids, C.c_uint32) if ids.size else None, ids.size, C.byref(n_lists),
                                            C.byref(total)))
        return lists, off, ids

    def drain_begin(self, topics, peers):
        """Enqueues drain(topics, peers) of the last window of the last run
        enqueued (ps_drain_begin) and returns without waiting for it; at most
        two may be outstanding.  drain_end() completes the oldest."""
        t, p, tp, pp = _queries(topics, peers)
        self._check(self._L.ps_drain_begin(self._h, tp, pp, t.size))
        self._drain_n.append((0, t.size))

    def drain_end(self, copy: bool = True):
        """(off, ids) of the oldest drain_begin, as drain() returns them
        (ps_drain_end).  copy=False: views of the engine's pinned memory,
        valid until the next drain_begin."""
        op, mp, total = _u64p(), _u32p(), C.c_uint64()
        rc = self._L.ps_drain_end(self._h, C.byref(op), C.byref(mp), C.byref(total))
        # (no slot was completed: PS_E_NOTREADY, or the oldest drain is of another kind)
        if rc != -8 and self._drain_n and self._drain_n[0][0] == 0:
            n = self._drain_n.pop(0)[1]
        self._check(rc)
        off, ids = _view(op, n + 1, np.uint64), _view(mp, total.value, np.uint32)
        return (off.copy(), ids.copy()) if copy else (off, ids)

    def drain_shared_begin(self, topics, peers, list_cap: int = 0, id_cap: int = 0):
        """Enqueues drain_shared(topics, peers) of the last window of the last
        run enqueued (ps_drain_shared_begin) and returns without waiting for
        it; it shares drain_begin's two slots.  list_cap = id_cap = 0: the
        engine's caps, the size of the answer.  drain_shared_end() completes
        the oldest."""
        t, p, tp, pp = _queries(topics, peers)
        self._check(self._L.ps_drain_shared_begin(self._h, tp, pp, t.size, list_cap, id_cap))
        self._drain_n.append((1, t.size))

    def drain_shared_end(self, copy: bool = True):
        """(list_of_query, list_off, ids) of the oldest drain_shared_begin, as
        drain_shared() returns them (ps_drain_shared_end).  copy=False: views
        of the engine's pinned memory, valid until the next begin of either
        kind."""
        lp, op, mp = _u32p(), _u64p(), _u32p()
        n_lists, total = C.c_uint32(), C.c_uint64()
        rc = self._L.ps_drain_shared_end(self._h, C.byref(lp), C.byref(op), C.byref(mp), C.byref(n_lists),
                                         C.byref(total))
        # (no slot was completed: PS_E_NOTREADY, or the oldest drain is of another kind)
        if rc != -8 and self._drain_n and self._drain_n[0][0] == 1:
            n = self._drain_n.pop(0)[1]
        self._check(rc)
        lists = _view(lp, n, np.uint32)
        off, ids = _view(op, n_lists.value + 1, np.uint64), _view(mp, total.value, np.uint32)
        return (lists.copy(), off.copy(), ids.copy()) if copy else (lists, off, ids)

    def sink_set(self, topics, peers, list_cap: int = 0, id_cap: int = 0):
        """Registers standing queries (ps_sink_set): from now on every window
        of every run is drained for them, one result per run (sink_take).  No
        query clears the sink; results not yet taken are discarded."""
        t, p, tp, pp = _queries(topics, peers)
        self._check(self._L.ps_sink_set(self._h, tp, pp, t.size, list_cap, id_cap))
        self._sink_n = t.size

    def sink_take(self, copy: bool = True):
        """(win_list[n_windows, n], list_off, ids) of the oldest run not yet
        taken (ps_sink_take): query q's list in window w, or PS_NONE; list l
        is ids[list_off[l]:list_off[l + 1]].  copy=False: views of the
        engine's pinned memory, valid until the second run after its own."""
        wp, op, mp = _u32p(), _u64p(), _u32p()
        n_windows, n_lists, total = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._check(self._L.ps_sink_take(self._h, C.byref(wp), C.byref(op), C.byref(mp), C.byref(n_windows),
                                         C.byref(n_lists), C.byref(total)))
        n, nw = self._sink_n, n_windows.value
        wl = _view(wp, (nw, n), np.uint32)
        off, ids = _view(op, n_lists.value + 1, np.uint64), _view(mp, total.value, np.uint32)
        return (wl.copy(), off.copy(), ids.copy()) if copy else (wl, off, ids)

    def drain_topics(self, topics) -> dict:
        """Each named topic's whole audience in the last window, with no query
        per subscriber (ps_drain_topics): a dict of numpy copies --
        topic_list[n], n_nodes[n], n_full[n], exc_off[n + 1], exc_peer[E],
        exc_list[E], list_off[n_lists + 1], ids[total].  Entry i's shared list
        is topic_list[i] (or NONE), held by n_full[i] of its n_nodes[i]
        non-root nodes; the others are exc_peer / exc_list[exc_off[i]:
        exc_off[i + 1]], in node order; list l is ids[list_off[l]:
        list_off[l + 1]]."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        n = t.size
        tl, ep, el, mp = _u32p(), _u32p(), _u32p(), _u32p()
        nn, nf, eo, lo = _u64p(), _u64p(), _u64p(), _u64p()
        n_lists, total = C.c_uint32(), C.c_uint64()
        self._check(self._L.ps_drain_topics(self._h, _p(t, C.c_uint32), n, C.byref(tl), C.byref(nn), C.byref(nf),
                                            C.byref(eo), C.byref(ep), C.byref(el), C.byref(lo), C.byref(mp),
                                            C.byref(n_lists), C.byref(total)))

        def arr(p, k, dt):
            return _view(p, k, dt).copy()

        exc_off = arr(eo, n + 1, np.uint64)
        n_exc = int(exc_off[n])
        return {"topic_list": arr(tl, n, np.uint32), "n_nodes": arr(nn, n, np.uint64), "n_full": arr(nf, n, np.uint64),
                "exc_off": exc_off, "exc_peer": arr(ep, n_exc, np.uint32), "exc_list": arr(el, n_exc, np.uint32),
                "list_off": arr(lo, n_lists.value + 1, np.uint64), "ids": arr(mp, total.value, np.uint32)}

    def drain_topics_begin(self, topics, exc_cap: int = 0, list_cap: int = 0, id_cap: int = 0):
        """Enqueues drain_topics(topics) of the last window of the last run
        enqueued (ps_drain_topics_begin) and returns without waiting for it;
        it shares drain_begin's two slots.  A cap of 0: the engine's own.
        drain_topics_end() completes the oldest."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        self._check(self._L.ps_drain_topics_begin(self._h, _p(t, C.c_uint32), t.size, exc_cap, list_cap, id_cap))
        self._drain_n.append((2, t.size))

    def drain_topics_end(self, copy: bool = True) -> dict:
        """The oldest drain_topics_begin's answer, the dict drain_topics()
        returns (ps_drain_topics_end).  copy=False: views of the engine's
        pinned memory, valid until the next begin of any kind.  When the
        answer exceeded a cap the EngineError (PS_E_RANGE) carries `partial`:
        n_nodes, n_full and exc_off, exact whatever the caps, and n_lists and
        total, exact when the exceptions and the lists fit."""
        tl, ep, el, mp = _u32p(), _u32p(), _u32p(), _u32p()
        nn, nf, eo, lo = _u64p(), _u64p(), _u64p(), _u64p()
        n_lists, total = C.c_uint32(), C.c_uint64()
        rc = self._L.ps_drain_topics_end(self._h, C.byref(tl), C.byref(nn), C.byref(nf), C.byref(eo), C.byref(ep),
                                         C.byref(el), C.byref(lo), C.byref(mp), C.byref(n_lists), C.byref(total))
        # (no slot was completed: PS_E_NOTREADY, or the oldest drain is of another kind)
        done = rc != -8 and self._drain_n and self._drain_n[0][0] == 2
        if done:
            n = self._drain_n.pop(0)[1]

        def arr(p, k, dt):
            v = _view(p, k, dt)
            return v.copy() if copy else v

        if rc == -7 and done and tl:
            err = EngineError(rc, self._L.ps_last_error(self._h).decode())
            err.partial = {"n_nodes": _view(nn, n, np.uint64).copy(), "n_full": _view(nf, n, np.uint64).copy(),
                           "exc_off": _view(eo, n + 1, np.uint64).copy(),
                           # (exact when the exceptions and the lists fit)
                           "n_lists": n_lists.value, "total": total.value}
            raise err
        self._check(rc)
        exc_off = arr(eo, n + 1, np.uint64)
        n_exc = int(exc_off[n])
        return {"topic_list": arr(tl, n, np.uint32), "n_nodes": arr(nn, n, np.uint64), "n_full": arr(nf, n, np.uint64),
                "exc_off": exc_off, "exc_peer": arr(ep, n_exc, np.uint32), "exc_list": arr(el, n_exc, np.uint32),
                "list_off": arr(lo, n_lists.value + 1, np.uint64), "ids": arr(mp, total.value, np.uint32)}

    def sink_set_topics(self, topics, exc_cap: int = 0, list_cap: int = 0, id_cap: int = 0):
        """Registers standing topics (ps_sink_set_topics): from now on every
        window of every run is drained for them as drain_topics does, one
        result per run (sink_take_topics).  It replaces a query sink; no topic
        clears the sink; results not yet taken are discarded.  A cap of 0: the
        engine's own, summed over the run's windows."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        self._check(self._L.ps_sink_set_topics(self._h, _p(t, C.c_uint32), t.size, exc_cap, list_cap, id_cap))
        self._sink_n = t.size

    def sink_take_topics(self, copy: bool = True) -> dict:
        """The oldest run not yet taken (ps_sink_take_topics): drain_topics'
        dict over the run's windows plus n_windows -- topic_list, n_nodes and
        n_full as [n_windows, n] arrays, exc_off[n_windows * n + 1] cumulative
        over the run, exc_peer / exc_list, list_off and ids run-wide.
        copy=False: views of the engine's pinned memory, valid until the
        second run after its own.  When the answer exceeded a cap the
        EngineError (PS_E_RANGE) carries `partial`: n_windows, n_nodes, n_full
        and exc_off, exact whatever the caps, and n_lists and total."""
        tl, ep, el, mp = _u32p(), _u32p(), _u32p(), _u32p()
        nn, nf, eo, lo = _u64p(), _u64p(), _u64p(), _u64p()
        n_windows, n_lists, total = C.c_uint32(), C.c_uint32(), C.c_uint64()
        rc = self._L.ps_sink_take_topics(self._h, C.byref(tl), C.byref(nn), C.byref(nf), C.byref(eo), C.byref(ep),
                                         C.byref(el), C.byref(lo), C.byref(mp), C.byref(n_windows), C.byref(n_lists),
                                         C.byref(total))
        n, nw = self._sink_n, n_windows.value

        def arr(p, k, dt):
            v = _view(p, k, dt)
            return v.copy() if copy else v

        if rc == -7 and tl:
            err = EngineError(rc, self._L.ps_last_error(self._h).decode())
            err.partial = {"n_windows": nw, "n_nodes": _view(nn, (nw, n), np.uint64).copy(),
                           "n_full": _view(nf, (nw, n), np.uint64).copy(),
                           "exc_off": _view(eo, nw * n + 1, np.uint64).copy(),
                           # (exact for the windows before the first that overflowed)
                           "topic_list": _view(tl, (nw, n), np.uint32).copy(),
                           "n_lists": n_lists.value, "total": total.value}
            # the first k records / list offsets / ids, for a caller who knows its caps
            ptrs = {"exc_peer": (ep, np.uint32), "exc_list": (el, np.uint32), "list_off": (lo, np.uint64),
                    "ids": (mp, np.uint32)}
            err.partial["head"] = lambda name, k: _view(ptrs[name][0], int(k), ptrs[name][1]).copy()
            raise err
        self._check(rc)
        exc_off = arr(eo, nw * n + 1, np.uint64)
        n_exc = int(exc_off[nw * n])
        return {"n_windows": nw, "topic_list": arr(tl, (nw, n), np.uint32), "n_nodes": arr(nn, (nw, n), np.uint64),
                "n_full": arr(nf, (nw, n), np.uint64), "exc_off": exc_off, "exc_peer": arr(ep, n_exc, np.uint32),
                "exc_list": arr(el, n_exc, np.uint32), "list_off": arr(lo, n_lists.value + 1, np.uint64),
                "ids": arr(mp, total.value, np.uint32)}

    def peer_load(self, topics) -> tuple[np.ndarray, np.ndarray]:
        """Per-peer traffic of the last window over the named distinct topics
        (ps_peer_load): (recv, sent), uint64 [n_peers] each -- the messages a
        peer received as a non-root node, and the copies it wrote to its
        children (live or not)."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        recv = np.empty(self.n_peers, dtype=np.uint64)
        sent = np.empty(self.n_peers, dtype=np.uint64)
        self._check(self._L.ps_peer_load(self._h, _p(t, C.c_uint32), t.size, _p(recv, C.c_uint64), _p(sent, C.c_uint64)))
        return recv, sent

    def load_track(self, topics):
        """Registers standing topics (ps_load_track): from now on every window
        of every run adds its per-peer traffic over them into totals on the
        device (load_take).  No topic clears the tracking; setting or clearing
        zeroes the totals."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        self._check(self._L.ps_load_track(self._h, _p(t, C.c_uint32), t.size))

    def load_take(self) -> tuple[np.ndarray, np.ndarray, int]:
        """The totals since the last take or track call (ps_load_take):
        (recv, sent, n_windows); the totals and the count start again at 0."""
        recv = np.empty(self.n_peers, dtype=np.uint64)
        sent = np.empty(self.n_peers, dtype=np.uint64)
        nw = C.c_uint64()
        self._check(self._L.ps_load_take(self._h, _p(recv, C.c_uint64), _p(sent, C.c_uint64), C.byref(nw)))
        return recv, sent, nw.value

    def topic_hops(self, topics) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Deliveries by hop of the last window for the named distinct tree
        topics (ps_topic_hops): (nodes, reached, deliv), uint64 [n, MAX_ROUNDS]
        each, row i for topics[i] -- per BFS level the topic's nodes, those the
        window reached, and the messages they received; the last column holds
        every level from MAX_ROUNDS - 1 on."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        out = [np.zeros((t.size, MAX_ROUNDS), dtype=np.uint64) for _ in range(3)]
        self._check(self._L.ps_topic_hops(self._h, _p(t, C.c_uint32), t.size, *(_p(a, C.c_uint64) for a in out)))
        return out[0], out[1], out[2]

    def hops_track(self, topics):
        """Registers standing tree topics (ps_hops_track): from now on every
        window of every run adds its deliveries by hop over them into totals on
        the device (hops_take).  No topic clears the tracking; setting or
        clearing zeroes the totals."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        self._check(self._L.ps_hops_track(self._h, _p(t, C.c_uint32), t.size))
        self._hops_n = int(t.size)

    def hops_take(self) -> tuple[np.ndarray, np.ndarray, np.ndarray, int, int]:
        """The totals since the last take or track call (ps_hops_take):
        (nodes, reached, deliv, n_windows, n_skipped), the arrays uint64
        [n_tracked, MAX_ROUNDS]; n_skipped counts the (topic, window) pairs
        left out because the topic was a mesh there.  The totals and both
        counts start again at 0.  (The arrays are sized by the last hops_track
        made through this object: track through it, not through the raw
        library handle.)"""
        n = self._hops_n
        out = [np.zeros((n, MAX_ROUNDS), dtype=np.uint64) for _ in range(3)]
        nw, nsk = C.c_uint64(), C.c_uint64()
        self._check(self._L.ps_hops_take(self._h, *(_p(a, C.c_uint64) for a in out), C.byref(nw), C.byref(nsk)))
        return out[0], out[1], out[2], nw.value, nsk.value

    def peer_downstream(self, topics) -> tuple[np.ndarray, np.ndarray]:
        """The audience behind each peer in the last window over the named
        distinct tree topics (ps_peer_downstream): (below, carried), uint64
        [n_peers] each -- the nodes strictly below the peer's nodes, live or
        not, and the window messages delivered to them: what would have been
        lost had the peer dropped."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        below = np.empty(self.n_peers, dtype=np.uint64)
        carried = np.empty(self.n_peers, dtype=np.uint64)
        self._check(self._L.ps_peer_downstream(self._h, _p(t, C.c_uint32), t.size, _p(below, C.c_uint64),
                                               _p(carried, C.c_uint64)))
        return below, carried

    def downstream_track(self, topics):
        """Registers standing tree topics (ps_downstream_track): from now on
        every window of every run adds the audience behind each peer over them
        into totals on the device (downstream_take).  No topic clears the
        tracking; setting or clearing zeroes the totals."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        self._check(self._L.ps_downstream_track(self._h, _p(t, C.c_uint32), t.size))

    def downstream_take(self) -> tuple[np.ndarray, np.ndarray, int, int]:
        """The totals since the last take or track call (ps_downstream_take):
        (below, carried, n_windows, n_skipped); below is a sum of per-window
        values, n_skipped counts the (topic, window) pairs left out because the
        topic was a mesh there.  The totals and both counts start again at 0."""
        below = np.empty(self.n_peers, dtype=np.uint64)
        carried = np.empty(self.n_peers, dtype=np.uint64)
        nw, nsk = C.c_uint64(), C.c_uint64()
        self._check(self._L.ps_downstream_take(self._h, _p(below, C.c_uint64), _p(carried, C.c_uint64), C.byref(nw),
                                               C.byref(nsk)))
        return below, carried, nw.value, nsk.value

    def peer_cut(self, topics) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """What the last window lost over the named distinct tree topics, and
        where the trees were cut (ps_peer_cut): (missed, cuts, orphaned, lost),
        uint64 [n_peers] each -- the messages the peer's own nodes lack; its
        cut points (nodes that lack messages under a full parent); the nodes
        behind them, live or not; and the deliveries that did not happen at
        and behind them."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        out = [np.empty(self.n_peers, dtype=np.uint64) for _ in range(4)]
        self._check(self._L.ps_peer_cut(self._h, _p(t, C.c_uint32), t.size, *(_p(a, C.c_uint64) for a in out)))
        return out[0], out[1], out[2], out[3]

    def cut_track(self, topics):
        """Registers standing tree topics (ps_cut_track): from now on every
        window of every run adds its losses and cut points over them into
        totals on the device (cut_take).  No topic clears the tracking;
        setting or clearing zeroes the totals."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        self._check(self._L.ps_cut_track(self._h, _p(t, C.c_uint32), t.size))

    def cut_take(self) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, int, int]:
        """The totals since the last take or track call (ps_cut_take):
        (missed, cuts, orphaned, lost, n_windows, n_skipped); n_skipped counts
        the (topic, window) pairs left out because the topic was a mesh there.
        The totals and both counts start again at 0."""
        out = [np.empty(self.n_peers, dtype=np.uint64) for _ in range(4)]
        nw, nsk = C.c_uint64(), C.c_uint64()
        self._check(self._L.ps_cut_take(self._h, *(_p(a, C.c_uint64) for a in out), C.byref(nw), C.byref(nsk)))
        return out[0], out[1], out[2], out[3], nw.value, nsk.value

    def topic_blame(self, topics) -> dict:
        """Every non-root node of the named distinct tree topics that lacks
        messages of the last window, with the cut point to blame
        (ps_topic_blame): a dict of numpy copies -- rec_off[n + 1], and per
        record, in node order, peer, cut_peer (the peer of the nearest node on
        the way up that lacks messages under a full parent), hop and cut_hop
        (their BFS levels) and missed.  Topic i's records are
        [rec_off[i], rec_off[i + 1])."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        off = _u64p()
        ptrs = [_u32p() for _ in range(5)]
        total = C.c_uint64()
        self._check(self._L.ps_topic_blame(self._h, _p(t, C.c_uint32), t.size, C.byref(off), *(C.byref(p) for p in ptrs),
                                           C.byref(total)))
        out = {"rec_off": _view(off, t.size + 1, np.uint64).copy()}
        for k, p in zip(("peer", "cut_peer", "hop", "cut_hop", "missed"), ptrs):
            out[k] = _view(p, total.value, np.uint32).copy()
        return out

    def blame(self, topics, peers) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """topic_blame's facts for explicit (topic, peer) queries, repeats and
        any order allowed (ps_blame): (cut_peer, hop, cut_hop, missed), uint32
        [n] each.  The root, a peer with a full row and any node of a topic
        idle in the window: cut_peer = cut_hop = NONE, missed 0, hop its level;
        a peer outside the topic's node space: NONE, NONE, NONE, 0."""
        t, p, tp, pp = _queries(topics, peers)
        out = [np.empty(t.size, dtype=np.uint32) for _ in range(4)]
        self._check(self._L.ps_blame(self._h, tp, pp, t.size, *(_p(a, C.c_uint32) for a in out)))
        return out[0], out[1], out[2], out[3]

    def blame_track(self, topics, rec_cap: int = 0):
        """Registers standing tree topics (ps_blame_track): from now on every
        window of every run appends topic_blame's records over them on the
        device (blame_take).  No topic clears the tracking; setting or clearing
        discards what was not taken.  rec_cap: the records kept between two
        takes at most; 0: the engine's own cap, summed as the windows come."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        self._check(self._L.ps_blame_track(self._h, _p(t, C.c_uint32), t.size, rec_cap))
        self._blame_n = t.size

    def blame_take(self) -> dict:
        """Everything since the last take or track call (ps_blame_take): a
        dict of numpy copies -- rec_off[n_windows * n + 1], cumulative, window
        w's records of request position i at [rec_off[w * n + i],
        rec_off[w * n + i + 1]); peer, cut_peer, hop, cut_hop and missed, the
        first `stored` records each; n_windows, n_skipped, total and stored.
        When the records exceeded the cap the EngineError (PS_E_RANGE) carries
        that dict as `partial`: rec_off and the counts exact, the arrays the
        prefix that was kept."""
        off = _u64p()
        ptrs = [_u32p() for _ in range(5)]
        nw, nsk, total, stored = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = self._L.ps_blame_take(self._h, C.byref(off), *(C.byref(p) for p in ptrs), C.byref(nw), C.byref(nsk),
                                   C.byref(total), C.byref(stored))
        if rc != -7 or not off:
            self._check(rc)
        out = {"rec_off": _view(off, nw.value * getattr(self, "_blame_n", 0) + 1, np.uint64).copy()}
        for k, p in zip(("peer", "cut_peer", "hop", "cut_hop", "missed"), ptrs):
            out[k] = _view(p, stored.value, np.uint32).copy()
        out.update(n_windows=nw.value, n_skipped=nsk.value, total=total.value, stored=stored.value)
        if rc:
            err = EngineError(rc, self._L.ps_last_error(self._h).decode())
            err.partial = out
            raise err
        return out

    def _report_arrays(self, n_topics: int, what: int) -> tuple[dict, Report]:
        """The selected sections' arrays (hop arrays [n_topics, MAX_ROUNDS],
        the others [n_peers]) and the ps_report that points at them."""
        arrays, rep = {}, Report()
        for sec, names in REPORT_SECTIONS:
            if not what & sec:
                continue
            for k in names:
                shape = (n_topics, MAX_ROUNDS) if sec == REPORT_HOPS else (self.n_peers,)
                arrays[k] = np.zeros(shape, dtype=np.uint64)
                setattr(rep, k, _p(arrays[k], C.c_uint64))
        return arrays, rep

    def peer_report(self, topics, what: int = REPORT_ALL) -> dict:
        """The last window's load, hops, downstream and cut answers over the
        named distinct topics from one pass (ps_peer_report): a dict of the
        arrays of the sections selected in `what` (REPORT_*), each what that
        section's own call returns (peer_load, topic_hops, peer_downstream,
        peer_cut)."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        arrays, rep = self._report_arrays(t.size, what)
        self._check(self._L.ps_peer_report(self._h, _p(t, C.c_uint32), t.size, what, C.byref(rep), C.sizeof(Report)))
        return arrays

    def dist_report(self, topics, what: int = REPORT_DIST) -> dict:
        """This rank's share of peer_report's load, hop and downstream sections
        over the named distinct topics (ps_dist_report), on an engine of any
        rank count: a dict of the arrays of the sections selected in `what`
        (within REPORT_DIST).  The ranks' arrays add up to a one-rank engine's
        peer_report.  With REPORT_DOWNSTREAM on a multi-rank engine the call is
        collective: every rank makes it, with the same topics and `what`."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        arrays, rep = self._report_arrays(t.size, what)
        self._check(self._L.ps_dist_report(self._h, _p(t, C.c_uint32), t.size, what, C.byref(rep), C.sizeof(Report)))
        return arrays

    def dist_cut(self, topics) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """This rank's share of peer_cut over the named distinct tree topics
        (ps_dist_cut), on an engine of any rank count: (missed, cuts,
        orphaned, lost), uint64 [n_peers] each, for the nodes this rank owns --
        the subtree behind a cut point counted on whatever rank it lies.  The
        ranks' arrays add up to a one-rank engine's peer_cut.  On a multi-rank
        engine the call is collective whenever topics are named: every rank
        makes it, with the same topics in the same order."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        out = [np.empty(self.n_peers, dtype=np.uint64) for _ in range(4)]
        self._check(self._L.ps_dist_cut(self._h, _p(t, C.c_uint32), t.size, *(_p(a, C.c_uint64) for a in out)))
        return out[0], out[1], out[2], out[3]

    def dist_blame(self, topics) -> dict:
        """This rank's share of topic_blame over the named distinct tree topics
        (ps_dist_blame), on an engine of any rank count: topic_blame's dict --
        rec_off[n + 1], and per record peer, cut_peer, hop, cut_hop and missed
        -- for the missed non-root nodes this rank owns, in its own node
        order; the cut point may lie on any rank.  Keyed by (request position,
        peer) the ranks' records together are a one-rank engine's topic_blame.
        On a multi-rank engine the call is collective whenever topics are
        named: every rank makes it, with the same topics in the same order."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        off = _u64p()
        ptrs = [_u32p() for _ in range(5)]
        total = C.c_uint64()
        self._check(self._L.ps_dist_blame(self._h, _p(t, C.c_uint32), t.size, C.byref(off), *(C.byref(p) for p in ptrs),
                                          C.byref(total)))
        out = {"rec_off": _view(off, t.size + 1, np.uint64).copy()}
        for k, p in zip(("peer", "cut_peer", "hop", "cut_hop", "missed"), ptrs):
            out[k] = _view(p, total.value, np.uint32).copy()
        return out

    def topic_spread(self, topics) -> dict:
        """Hops and duplicate copies of the last window for the named distinct
        topics, meshes and trees alike (ps_topic_spread): a dict of reached and
        deliv, uint64 [n, MAX_ROUNDS], row i for topics[i] -- per hop the
        forwarders the window reached and the messages they hold; unreached and
        stranded, uint64 [n] -- the non-root nodes whose rows hold nothing, and
        those that hold messages no forwarder's child entry leads to; copies
        and dup, uint64 [n_peers] -- the copies sent to each peer and those
        beyond what it received."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        out = {"reached": np.zeros((t.size, MAX_ROUNDS), dtype=np.uint64), "deliv": np.zeros((t.size, MAX_ROUNDS), dtype=np.uint64),
               "unreached": np.zeros(t.size, dtype=np.uint64), "stranded": np.zeros(t.size, dtype=np.uint64),
               "copies": np.empty(self.n_peers, dtype=np.uint64), "dup": np.empty(self.n_peers, dtype=np.uint64)}
        self._check(self._L.ps_topic_spread(self._h, _p(t, C.c_uint32), t.size, *(_p(a, C.c_uint64) for a in out.values())))
        return out

    def spread_track(self, topics):
        """Registers standing topics, meshes and trees alike (ps_spread_track):
        from now on every window of every run adds topic_spread's answer over
        them into totals on the device (spread_take).  No topic clears the
        tracking; setting or clearing zeroes the totals."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        self._check(self._L.ps_spread_track(self._h, _p(t, C.c_uint32), t.size))
        self._spread_n = int(t.size)

    def spread_take(self) -> dict:
        """The totals since the last take or track call (ps_spread_take):
        topic_spread's six arrays, row i for the i-th standing topic, summed
        over the windows, with n_windows and n_truncated -- the windows whose
        BFS was cut short with a frontier left (0 on a healthy engine).  The
        totals and both counts start again at 0."""
        n = self._spread_n
        out = {"reached": np.zeros((n, MAX_ROUNDS), dtype=np.uint64), "deliv": np.zeros((n, MAX_ROUNDS), dtype=np.uint64),
               "unreached": np.zeros(n, dtype=np.uint64), "stranded": np.zeros(n, dtype=np.uint64),
               "copies": np.empty(self.n_peers, dtype=np.uint64), "dup": np.empty(self.n_peers, dtype=np.uint64)}
        nw, nt = C.c_uint64(), C.c_uint64()
        self._check(self._L.ps_spread_take(self._h, *(_p(a, C.c_uint64) for a in out.values()), C.byref(nw), C.byref(nt)))
        out["n_windows"] = nw.value
        out["n_truncated"] = nt.value
        return out

    def report_track(self, topics, what: int = REPORT_ALL):
        """Registers standing topics and sections (ps_report_track): from now on
        every window of every run adds the selected sections over them into
        totals on the device (report_take), one pass a window.  No topic clears
        the tracking; setting or clearing zeroes the totals."""
        t = np.ascontiguousarray(topics, dtype=np.uint32)
        if t.ndim != 1:
            raise ValueError("topics must be a 1-d array")
        self._check(self._L.ps_report_track(self._h, _p(t, C.c_uint32), t.size, what))
        self._report = (int(t.size), int(what)) if t.size else None

    def report_take(self) -> tuple[dict, int, int]:
        """The totals since the last take or track call (ps_report_take):
        (dict of the tracked sections' arrays, n_windows, n_skipped); n_skipped
        counts the (topic, window) pairs left out of the tree sections because
        the topic was a mesh there.  The totals and both counts start again at 0."""
        n, what = getattr(self, "_report", None) or (0, REPORT_ALL)
        arrays, rep = self._report_arrays(n, what)
        nw, nsk = C.c_uint64(), C.c_uint64()
        self._check(self._L.ps_report_take(self._h, C.byref(rep), C.sizeof(Report), C.byref(nw), C.byref(nsk)))
        return arrays, nw.value, nsk.value

    def seen_digest(self) -> int:
        d = C.c_uint64()
        self._check(self._L.ps_seen_digest(self._h, C.byref(d)))
        return d.value

    # the node space (tests): ps_graph_get
    def graph(self, what: int, index: int = 0) -> np.ndarray:
        """One table of the node space, brought up to date as the next run
        would (ps_graph_get; G_* above)."""
        from . import plan

        return graph_get(plan.lib(), self._h, what, index)

    def graph_topic(self, topic: int) -> dict:
        return graph_topic(self.graph(G_TOPIC, topic))

    def build_report(self) -> dict:
        """Which build produced the node spaces so far: counters since
        creation and the last build's kind and GPU attempts."""
        return build_report(self.graph(G_BUILD))

    def overlapped_windows(self) -> int:
        """Pipelined windows whose prefix ran beside the previous window."""
        d = C.c_uint64()
        self._check(self._L.ps_overlapped_windows(self._h, C.byref(d)))
        return d.value

    def chain_fill_launches(self) -> int:
        """Chain launch slots whose whole rows were written by reach + fill."""
        d = C.c_uint64()
        self._check(self._L.ps_chain_fill_launches(self._h, C.byref(d)))
        return d.value

    # multi-GPU
    def dist_init(self, rank: int, world: int, unique_id: bytes, partition: int = PART_PEER,
                  split_depth: int = 0):
        """RCCL-backed sharding: this engine owns a hash partition of every topic."""
        dc = DistConfig(rank, world, partition, split_depth)
        uid = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self._L.ps_dist_init(self._h, C.byref(dc), uid))

    def dist_init_ipc(self, rank: int, world: int, group_id: bytes, partition: int = PART_PEER,
                      split_depth: int = 0, copy: bool = False, inplace: bool = False):
        """Process-shared sharding (ps_dist_init_ipc): one process per rank on
        one node, device memory mapped across processes (several ranks may
        share a GPU); group_id from ipc_group_id() on one rank.  copy / inplace
        as for dist_init_loopback."""
        flags = (DIST_F_COPY if copy else 0) | (DIST_F_INPLACE if inplace else 0)
        dc = DistConfig(rank, world, partition, split_depth, flags, 0)
        gid = (C.c_uint8 * 128).from_buffer_copy(group_id)
        self._check(self._L.ps_dist_init_ipc(self._h, C.byref(dc), gid))

    def dist_init_loopback(self, group: "Loopback", rank: int, partition: int = PART_PEER,
                           split_depth: int = 0, copy: bool = False, inplace: bool = False):
        """copy: the records go through the receive buffer (PS_DIST_F_COPY), the
        RCCL transport's data path, instead of being read in place.  inplace:
        no records below the roots -- ghost-fed nodes read their parents' rows
        in the owner's row set (PS_DIST_F_INPLACE)."""
        flags = (DIST_F_COPY if copy else 0) | (DIST_F_INPLACE if inplace else 0)
        dc = DistConfig(rank, group.world, partition, split_depth, flags, 0)
        self._check(self._L.ps_dist_init_loopback(self._h, C.byref(dc), group._h))


def unique_id() -> bytes:
    buf = (C.c_uint8 * 128)()
    rc = load().ps_dist_unique_id(buf)
    if rc != PS_OK:
        raise EngineError(rc, "ps_dist_unique_id")
    return bytes(buf)


def device_count() -> int:
    """GPUs visible to this process, through the engine's own HIP runtime."""
    n = C.c_int32()
    load().ps_device_count(C.byref(n))
    return int(n.value)


def ipc_group_id() -> bytes:
    """A fresh group id for ps_dist_init_ipc (host only; ship it to every rank)."""
    buf = (C.c_uint8 * 128)()
    rc = load().ps_dist_ipc_id(buf)
    if rc != PS_OK:
        raise EngineError(rc, "ps_dist_ipc_id")
    return bytes(buf)


class Loopback:
    """In-process transport: `world` engines (one thread each) exchange
    frontier regions through device copies -- the multi-GPU path on one GPU."""

    def __init__(self, world: int):
        self.world = world
        h = _P()
        rc = load().ps_loopback_create(world, C.byref(h))
        if rc != PS_OK:
            raise EngineError(rc, "ps_loopback_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            load().ps_loopback_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def partition_owner(parent, root: int, topic: int, world: int, partition: int = PART_PEER,
                    split_depth: int = 0) -> np.ndarray:
    """Host-only: owner rank of every peer of a tree (-1 outside the tree)."""
    par = _u32arr(parent)
    out = np.empty(par.shape[0], dtype=np.int32)
    dc = DistConfig(0, world, partition, split_depth)
    rc = load().ps_partition_owner(par.shape[0], root, _p(par, C.c_uint32), topic, C.byref(dc),
                                   _p(out, C.c_int32))
    if rc != PS_OK:
        raise EngineError(rc, "ps_partition_owner")
    return out


def default_plan_opts() -> dict:
    """ps_plan_opts_default: the options every engine starts from."""
    o = PlanOpts()
    rc = load().ps_plan_opts_default(C.byref(o))
    if rc != PS_OK:
        raise EngineError(rc, "ps_plan_opts_default")
    return o.as_dict()


def version() -> str:
    return load().ps_version().decode()
