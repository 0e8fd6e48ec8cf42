#!/usr/bin/env python3
"""The delivery sink measured: one batched drain (ps_drain) against a loop of
ps_read_peer_messages, on a workload of psengine/workloads.py after one step.

  (a) one ps_drain over --queries random subscribed (topic, peer) pairs, its
      count / scan / emit / copy phases timed apart with HIP events
      (PSAMD_DRAIN_TIMING=1: the phases run one after the other, each
      synchronised), with the LDS-staged and with the direct-scatter emit; and
      the same call untimed (slab copies beside the next slab's emit), wall clock
  (b) ps_read_peer_messages over the first --loop-queries of the same pairs,
      scaled to --queries: the unchanged one-subscriber path

Prints one JSON line and, with --out DIR, writes DIR/drain_bench.json.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))

import psengine as PE  # noqa: E402
from psengine import workloads as WL  # noqa: E402


def pick_queries(wl, n, seed):
    """n (topic, peer) pairs drawn uniformly from all subscriptions."""
    rng = np.random.default_rng(seed)
    sizes = np.array([ts.join_order.size for ts in wl.topics], dtype=np.float64)
    qt = rng.choice(len(wl.topics), size=n, p=sizes / sizes.sum()).astype(np.uint32)
    qp = np.array([wl.topics[t].join_order[rng.integers(0, wl.topics[t].join_order.size)] for t in qt], dtype=np.uint32)
    return qt, qp


class StderrCapture:
    """The library's stderr lines (file descriptor 2) of the enclosed calls."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        return False


def stepped_engine(wl, env):
    for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING", "PSAMD_DRAIN_EMIT"):
        os.environ.pop(k, None)
    os.environ.update(env)
    eng = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed)
    WL.build_engine_topics(eng, wl)
    eng.publish(wl.msg_topics)
    st = eng.run()
    return eng, st


def raw_drain(eng, qt, qp, off, ids):
    total = C.c_uint64()
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = eng._L.ps_drain(eng._h, qt.ctypes.data_as(u32p), qp.ctypes.data_as(u32p), qt.size, off.ctypes.data_as(u64p),
                         ids.ctypes.data_as(u32p) if ids is not None else None, 0 if ids is None else ids.size,
                         C.byref(total))
    return rc, total.value


def timed_phases(wl, qt, qp, emit, reps):
    eng, _ = stepped_engine(wl, {"PSAMD_AB": "1", "PSAMD_DRAIN_TIMING": "1", "PSAMD_DRAIN_EMIT": emit})
    with eng:
        off = np.empty(qt.size + 1, dtype=np.uint64)
        rc, total = raw_drain(eng, qt, qp, off, None)
        assert rc in (0, -7), rc
        ids = np.empty(max(total, 1), dtype=np.uint32)
        rows = []
        for _ in range(reps + 1):  # (the first call builds the window's tables and allocates)
            with StderrCapture() as cap:
                rc, _ = raw_drain(eng, qt, qp, off, ids)
            assert rc == 0, rc
            m = re.search(r"psamd drain: .*", cap.text)
            assert m, cap.text
            rows.append({k: float(v) for k, v in re.findall(r"(\w+_ms) ([0-9.]+)", m.group(0))})
            rows[-1]["slabs"] = int(re.search(r"slabs (\d+)", m.group(0)).group(1))
            rows[-1]["segments"] = int(re.search(r"segments (\d+)", m.group(0)).group(1))
        best = min(rows[1:], key=lambda r: r["count_ms"] + r["emit_ms"])
        return total, best, ids[:total].copy(), off.copy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="cfg3", choices=sorted(WL.CONFIGS))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--loop-queries", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    wl = WL.scaled(a.workload, a.scale) if a.scale != 1.0 else WL.CONFIGS[a.workload]()
    qt, qp = pick_queries(wl, a.queries, a.seed)
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "queries": a.queries}

    total, lds, ids_lds, off_lds = timed_phases(wl, qt, qp, "lds", a.reps)
    total_d, direct, ids_dir, off_dir = timed_phases(wl, qt, qp, "direct", a.reps)
    assert total == total_d and np.array_equal(ids_lds, ids_dir) and np.array_equal(off_lds, off_dir)
    res.update(ids=total, id_bytes=4 * total, phases_lds=lds, phases_direct=direct)

    # untimed: the shipped path, wall clock of the full call (sizing known)
    eng, st = stepped_engine(wl, {})
    with eng:
        res.update(step_run_ms=st.run_ms, step_deliveries=st.deliveries)  # (the first, cold step)
        off = np.empty(qt.size + 1, dtype=np.uint64)
        ids = np.empty(max(total, 1), dtype=np.uint32)
        walls = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            rc, _ = raw_drain(eng, qt, qp, off, ids)
            walls.append(time.perf_counter() - t0)
            assert rc == 0, rc
        assert np.array_equal(ids[:total], ids_lds) and np.array_equal(off, off_lds)
        res["drain_wall_ms"] = 1e3 * min(walls[1:])
        res["drain_first_call_wall_ms"] = 1e3 * walls[0]  # with the window's table build
        t0 = time.perf_counter()
        off2, ids2 = eng.drain(qt, qp)
        res["drain_sized_and_read_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        # (b) the one-subscriber loop over a subset, scaled
        k = min(a.loop_queries, a.queries)
        t0 = time.perf_counter()
        got = [eng.peer_messages(int(t), int(p)) for t, p in zip(qt[:k], qp[:k])]
        loop = time.perf_counter() - t0
        for q in range(k):
            assert np.array_equal(got[q], ids[int(off[q]):int(off[q + 1])]), q
        loop_ids = int(off[k])
        res.update(loop_queries=k, loop_wall_ms=1e3 * loop, loop_ids=loop_ids,
                   loop_scaled_ms=1e3 * loop * a.queries / k)
    res["drain_ids_per_s"] = total / (res["drain_wall_ms"] / 1e3)
    res["loop_ids_per_s"] = loop_ids / loop
    res["speedup_wall"] = res["loop_scaled_ms"] / res["drain_wall_ms"]
    faster = "lds" if lds["emit_ms"] <= direct["emit_ms"] else "direct"
    best = lds if faster == "lds" else direct
    res["faster_emit"] = faster
    res["count_plus_emit_over_copy"] = (best["count_ms"] + best["emit_ms"]) / best["copy_ms"] if best["copy_ms"] else None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "drain_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
