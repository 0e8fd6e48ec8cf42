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

--pipelined: the drain in two halves (ps_drain_begin / ps_drain_end) inside the
pipelined step loop, for 256, 1024 and 4096 pairs (--pipelined-queries), wall
ms/step over --steps timed steps after --warmup:
  (i)   publish, ps_run_async, ps_wait of the previous: no drain (bench.py's loop)
  (ii)  ps_run then ps_drain, every step: the serial sink
  (iii) publish, ps_run_async, ps_drain_begin, ps_wait and ps_drain_end of the
        previous; the view copied out of device memory (copy) and emitted
        straight into mapped pinned memory (mapped)
with the host time inside ps_drain_begin, ps_overlapped_windows(), the link
time of the view's bytes (the copy phase of a timed ps_drain in the same
process), the host phases of the first synchronous drain after a window and
the device time of k_drain_tables and its check.  Writes
DIR/drain_async_bench.json.

--shared: ps_drain_shared (equal lists stored once) against ps_drain on the
same pairs of one window, for the counts of --pipelined-queries: the classify /
count / scan / emit / copy phases, the wall clock of the untimed calls, ids and
bytes moved to the host and the ratio of the two calls; then --large-queries
pairs through ps_drain_shared alone (ps_drain is skipped there because of its
output size), with classify's algorithmic bytes over its device time against
the HBM spec.  Writes DIR/drain_shared_bench.json.

--pipelined --shared: the shared drain in two halves (ps_drain_shared_begin /
ps_drain_shared_end) inside the pipelined step loop, in one process beside
loop (i) and loop (iii) (copy) above: wall ms/step, the host time inside the
begin call, ps_overlapped_windows() and the view's bytes; then, on a quiet
engine with PSAMD_DRAIN_TIMING=1, the device time of its classify / list
assignment / count / scan / emit passes for the counts of --pipelined-queries
and --large-queries.  Writes DIR/drain_shared_async_bench.json.

--sink: the sink (ps_sink_set / ps_sink_take) in the pipelined loop against
the loop of --pipelined --shared, the two alternating in one process, --reps
timings each: wall ms/step, the host time of ps_run_async (with the begin call
in the other loop), ps_overlapped_windows(); one case with msg_window cut so
that the largest topic takes three windows per step; the host time of the sink
per run from PSAMD_DRAIN_TIMING's clock.  Writes DIR/sink_bench.json.

--topics: ps_drain_topics (each topic's audience as one list plus exceptions)
over every topic of one window, --reps timings: its wall clock and its classify
/ scan / emit / lists / copy phases, the row bytes the classify pass covers
over its device time against the HBM spec; against (a) ps_drain_shared over
every subscription in the node space as explicit queries -- both wall clocks,
the host share of each, and that the expanded answers agree -- and (b) the
device time of k_digest (ps_seen_digest), which reads the same rows once under
the same generation test.  Writes DIR/drain_topics_bench.json.

--pipelined --topics: the audience drain in two halves (ps_drain_topics_begin /
ps_drain_topics_end) over every topic inside the pipelined step loop, three
loops alternating in one process, --reps timings each: (i) no drain, (ii)
ps_run then ps_drain_topics, (iii) publish, ps_run_async,
ps_drain_topics_begin, ps_wait and ps_drain_topics_end of the previous; wall
ms/step, the host time inside the begin call, the view's and the upload's
bytes, ps_overlapped_windows(), the answers of (ii) and (iii) compared entry
for entry, and whether (iii) beats (ii) by more than (ii)'s own spread; then,
on a quiet engine with PSAMD_DRAIN_TIMING=1, the device time of the passes.
Writes DIR/drain_topics_async_bench.json.

--pipelined --topics --sink: the audience sink (ps_sink_set_topics /
ps_sink_take_topics) over every topic: the sink-topics loop -- publish,
ps_run_async, ps_wait and ps_sink_take_topics of the previous -- beside loops
(i) and (iii) of --pipelined --topics, the three alternating in one process,
--reps timings each: wall ms/step, the host time inside ps_run_async (with the
begin call in loop (iii)), ps_overlapped_windows(), the results of the two
drained loops compared entry for entry, and whether the sink loop is slower
than loop (iii) by more than loop (iii)'s own spread; the sink's host time and
whether the strips were kept, per run, from PSAMD_DRAIN_TIMING's line; one
case with msg_window cut so that the largest topic takes three windows per
step.  Writes DIR/sink_topics_bench.json.

--load: per-peer load (ps_peer_load) over every topic after one step, --reps
repetitions in one process: its wall and device phases (classify, load, copy)
beside ps_drain_topics' phases; the derivation a caller has without it --
ps_drain_topics + ps_topic_get_parents per topic + numpy -- and its wall, the
two answers compared array for array; then the pipelined step with every
topic tracked (ps_load_track, one ps_load_take per loop) against the step with
the audience sink over the same topics and the plain step, the three
alternating in one process.  Writes DIR/load_bench.json.

--hops: deliveries by hop per topic (ps_topic_hops) over every topic after one
step, --reps repetitions in one process: its wall and device phases (classify,
hops, sum, copy) beside ps_peer_load's and ps_drain_topics' phases and walls;
the derivation a caller has without it -- ps_drain_topics +
ps_topic_get_parents per topic + numpy depths -- and its wall, the two answers
compared array for array; then the pipelined step plain, with hops tracked
(ps_hops_track, one ps_hops_take per loop), with load tracked, with both and
with the audience sink beside both, the five alternating in one process, the
totals against steps x the blocking answer.  Writes DIR/hops_bench.json.

--downstream: the audience behind each peer (ps_peer_downstream) over every
topic after one step, --reps repetitions in one process: its device phases
(classify, weights, levels + top, copy) with k_audience_load's in the same
process as the yardstick, and its wall; the derivation a caller has without it
-- ps_drain_topics + ps_topic_get_parents per topic + numpy depths and a
bottom-up sum level by level -- and its wall, the two answers compared array
for array; then the pipelined step plain, with downstream tracked
(ps_downstream_track, one ps_downstream_take per loop) and beside hops and
load tracking, the three alternating in one process, with the overlapped
windows of each, the totals against steps x the blocking answer.  Writes
DIR/downstream_bench.json.

--cut: the losses blamed on their cut points (ps_peer_cut) over every topic
after one step under a live mask with about 1 % of the peers dead (--seed; an
all-live window has no cut point and exercises nothing), --reps repetitions in
one process: its device phases (classify, weights, missed, levels + top, copy)
with ps_peer_downstream's under the same mask in the same process as the
yardstick, and its wall; the derivation a caller has without it --
ps_drain_topics + ps_topic_get_parents per topic + numpy depths, cut points
and a bottom-up sum -- and its wall, the two answers compared array for array;
then the pipelined step plain, with cuts tracked (ps_cut_track, one ps_cut_take
per loop) and beside load, hop and downstream tracking, the three alternating
in one process, the totals against steps x the blocking answer.  Writes
DIR/cut_bench.json.

--blame: each missed subscriber and its cut point (ps_topic_blame) over every
topic after one step under --cut's live mask, --reps repetitions alternating in
one process with its two yardsticks: (a) ps_peer_cut on the same window -- the
device phases of both (PSAMD_DRAIN_TIMING; ps_topic_blame's: classify, weights,
sweep, count + scan, emit, copy) and the walls --, and (b) the derivation a
caller has without it -- ps_drain_topics + ps_topic_get_parents per topic + a
numpy walk from the root down -- and its wall, the two answers compared record
for record on every repetition; the records, the bytes copied, and one ps_blame
over the records' own (topic, peer) pairs against them.  Writes
DIR/blame_bench.json.

--blame-track: the blame records behind every window (ps_blame_track /
ps_blame_take) over every topic under --cut's live mask, rec_cap set to the
records of --take-every steps.  The tracked step -- ps_run_async / ps_wait,
pipelined, one take every --take-every steps -- against the loop it replaces,
ps_run + ps_topic_blame every step, and against the untracked pipelined step,
the three alternating in one process: wall per step, the overlapped windows,
and the records of every take compared with the blocking call's, entry for
entry.  The device phases of one tracked window and of one ps_topic_blame
(PSAMD_DRAIN_TIMING: the tracked window's classify, weights, sweep, count +
scan, commit + emit; the take's wall with its copies) alternate in a second
engine.  Writes DIR/blame_track_bench.json.

--report: the four answers from one pass (ps_peer_report, all sections) over
every topic after one step under --cut's live mask, --reps repetitions
alternating in one process with the sequence ps_peer_load + ps_topic_hops +
ps_peer_downstream + ps_peer_cut: the device phases of each call
(PSAMD_DRAIN_TIMING) and the walls, the answers compared array for array; then
the pipelined step plain, with the report tracked (ps_report_track, all
sections, one ps_report_take per loop) and with the four trackers together,
the three alternating in one process, with the overlapped windows of each, the
totals against steps x the blocking answer.  Writes DIR/report_bench.json.
--report-once: one step and one ps_peer_report, nothing else (for a kernel
trace of one pass).

--dist-report: a rank's share of the report (ps_dist_report, what = 0x7).  One
rank: over every topic after one step under --cut's live mask, --reps
repetitions alternating in one process with ps_peer_report of the same
sections -- the yardstick --: the device phases of both (PSAMD_DRAIN_TIMING)
and the walls, the answers compared array for array.  Then 2 and 4 loopback
ranks on a cfg4-shaped run under the peer hash (one GPU: the ranks are threads
of this process): the collective call's wall per rank, its exchanges, the bytes
a rank ships in them and the bytes of its send and receive records, the ranks'
sum compared with the one-rank answer.  Writes DIR/dist_report_bench.json.

--dist-cut: a rank's share of the cut (ps_dist_cut).  One rank: over every
topic after one step under --cut's live mask, --reps repetitions alternating in
one process with ps_peer_cut -- the yardstick --: the device phases of both
(PSAMD_DRAIN_TIMING) and the walls, the answers compared array for array.  Then
2 and 4 loopback ranks on --dist-report's cfg4-shaped run, alternating with
ps_dist_report(PS_REPORT_DOWNSTREAM) -- the yardstick there --: the wall per
rank, the exchanges, the bytes a rank ships in them and the bytes of its
records and words, the ranks' sum compared with the one-rank answer on every
call.  Writes DIR/dist_cut_bench.json.

--dist-blame: a rank's share of the blame (ps_dist_blame).  One rank: over
every topic after one step under --cut's live mask, --reps repetitions
alternating in one process with ps_topic_blame -- the yardstick --: the device
phases of both (PSAMD_DRAIN_TIMING) and the walls, the answers compared entry
for entry.  Then 2 and 4 loopback ranks on --dist-report's cfg4-shaped run,
alternating with ps_dist_cut -- the yardstick there --: the wall per rank, the
exchanges, the bytes a rank ships in them and the bytes of its pairs, the
records and the bytes copied; the ranks' union, keyed by peer, compared with
the one-rank ps_topic_blame on every call.  Writes DIR/dist_blame_bench.json.

--spread: hops and duplicate copies of a mesh (ps_topic_spread).  The tool
builds its own mesh -- --spread-peers peers (default 2^20), random out-degree
0..6, 3 % dead, one topic, 1,024 messages -- and a second shape with one hub of
--spread-hub children below the root.  Per shape: the device phases of the
call (PSAMD_DRAIN_TIMING: classify, nodes, levels with their launch count, sum,
copy) beside ps_peer_load's on the same window -- the yardstick: the same
front, comparable work per node -- with a frontier node walked by its wave
from 0, 16 (the default), 64 and never (PSAMD_AB=1 PSAMD_SPREAD_WIDE); then the
walls of ps_topic_spread, ps_peer_load and the same answer derived on the host
(ps_peer_load's recv, the child lists, a frontier BFS in numpy), --reps
repetitions alternating in one process, the answers compared array for array.
Writes DIR/spread_bench.json.

--spread-track: that answer behind every window (ps_spread_track), on
--spread's own mesh in its random and hub shapes.  Per shape: the device
phases (PSAMD_DRAIN_TIMING) of a tracked window, of its take and of the
blocking call, alternating in one process, with the level launches of each;
then three loops of --steps steps alternating in one process, --reps times:
(a) the untracked pipelined step, (b) ps_run + ps_topic_spread every step,
(c) the tracked pipelined step with one ps_spread_take every --take-every
steps, every take compared array for array with the sum of (b)'s answers.
Writes DIR/spread_track_bench.json.
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


def norm(ids):
    """Message ids relative to the step's first (every step publishes the same batch under new ids)."""
    return ids - ids.min() if ids.size else ids


def fresh_engine(wl, env):
    for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING", "PSAMD_DRAIN_EMIT", "PSAMD_DRAIN_ASYNC_OUT"):
        os.environ.pop(k, None)
    os.environ.update(env)
    eng = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed)
    WL.build_engine_topics(eng, wl)
    for k in env:
        os.environ.pop(k, None)
    return eng


def loop_plain(eng, wl, n):
    eng.publish(wl.msg_topics)
    for i in range(n):
        eng.run_async()
        if i + 1 < n:
            eng.publish(wl.msg_topics)
        if i:
            eng.wait()
    eng.wait()


def loop_serial(eng, wl, n, qt, qp, off, ids):
    for _ in range(n):
        eng.publish(wl.msg_topics)
        eng.run()
        rc, _ = raw_drain(eng, qt, qp, off, ids)
        assert rc == 0, rc


def loop_async(eng, wl, n, qt, qp, begin_s):
    """Returns the last view (a copy).  begin_s: host seconds inside ps_drain_begin, appended per step."""
    L, h = eng._L, eng._h
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    tp, pp = qt.ctypes.data_as(u32p), qp.ctypes.data_as(u32p)
    op, mp, total = u64p(), u32p(), C.c_uint64()
    eng.publish(wl.msg_topics)
    for i in range(n):
        eng.run_async()
        t0 = time.perf_counter()
        rc = L.ps_drain_begin(h, tp, pp, qt.size)
        begin_s.append(time.perf_counter() - t0)
        assert rc == 0, rc
        if i + 1 < n:
            eng.publish(wl.msg_topics)
        if i:
            eng.wait()
            rc = L.ps_drain_end(h, C.byref(op), C.byref(mp), C.byref(total))
            assert rc == 0, rc
    eng.wait()
    rc = L.ps_drain_end(h, C.byref(op), C.byref(mp), C.byref(total))
    assert rc == 0, rc
    off = np.ctypeslib.as_array(op, shape=(qt.size + 1,)).copy()
    ids = np.ctypeslib.as_array(mp, shape=(max(total.value, 1),))[:total.value].copy()
    return off, ids


def pipelined_main(a, wl):
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "steps": a.steps,
           "warmup": a.warmup, "rows": []}
    counts = [int(x) for x in a.pipelined_queries.split(",")]
    queries = {n: pick_queries(wl, n, a.seed) for n in counts}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0) / a.steps

    # the timing engine: link time of each view's bytes, the first-call host
    # split and the device table build (every phase synchronised: not a wall figure)
    link, first_call, tables_dev, want = {}, {}, {}, {}
    eng = fresh_engine(wl, {"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        for n in counts:
            qt, qp = queries[n]
            eng.publish(wl.msg_topics)
            eng.run()
            off = np.empty(n + 1, dtype=np.uint64)
            with StderrCapture() as cap:
                t0 = time.perf_counter()
                rc, total = raw_drain(eng, qt, qp, off, None)
                wall = 1e3 * (time.perf_counter() - t0)
            if "engine_first_drain_sizing_call" not in res:  # (node-space mirrors and peer maps built here)
                m = re.search(r"psamd drain: .*", cap.text)
                cold = {k: float(v) for k, v in re.findall(r"(host_\w+_ms) ([0-9.]+)", m.group(0))} if m else {}
                cold.update(wall_ms=wall, queries=n)
                res["engine_first_drain_sizing_call"] = cold
            ids = np.empty(max(total, 1), dtype=np.uint32)
            eng.publish(wl.msg_topics)
            eng.run()
            rows = []
            for _ in range(a.reps + 1):  # (the first call after the window builds its tables)
                with StderrCapture() as cap:
                    t0 = time.perf_counter()
                    rc, _ = raw_drain(eng, qt, qp, off, ids)
                    wall = 1e3 * (time.perf_counter() - t0)
                assert rc == 0, rc
                m = re.search(r"psamd drain: .*", cap.text)
                rows.append({k: float(v) for k, v in re.findall(r"(\w+_ms) ([0-9.]+)", m.group(0))})
                rows[-1]["wall_ms"] = wall
            first_call[n] = rows[0]
            link[n] = min(r["copy_ms"] for r in rows[1:])
            want[n] = (off.copy(), ids[:total].copy())
            eng.publish(wl.msg_topics)
            eng.run()
            with StderrCapture() as cap:
                eng.drain_begin(qt, qp)
                eng.drain_end()
            m = re.search(r"psamd drain tables: .*device_ms ([0-9.]+)", cap.text)
            tables_dev[n] = {"device_ms": float(m.group(1)), "line": m.group(0)}
    res["first_sync_drain_after_a_window"] = {str(n): first_call[n] for n in counts}
    res["k_drain_tables_plus_check"] = {str(n): tables_dev[n] for n in counts}

    eng = fresh_engine(wl, {})
    with eng:
        loop_plain(eng, wl, a.warmup)
        o0 = eng.overlapped_windows()
        res["plain_ms_per_step"] = timed(lambda: loop_plain(eng, wl, a.steps))
        res["plain_overlapped_windows"] = eng.overlapped_windows() - o0
        serial = {}
        for n in counts:
            qt, qp = queries[n]
            off = np.empty(n + 1, dtype=np.uint64)
            ids = np.empty(max(want[n][1].size, 1), dtype=np.uint32)
            loop_serial(eng, wl, a.warmup, qt, qp, off, ids)
            serial[n] = timed(lambda: loop_serial(eng, wl, a.steps, qt, qp, off, ids))
            assert np.array_equal(off, want[n][0]) and np.array_equal(norm(ids[:want[n][1].size]), norm(want[n][1]))
    asyn = {}
    for variant in ("copy", "mapped"):
        eng = fresh_engine(wl, {"PSAMD_AB": "1", "PSAMD_DRAIN_ASYNC_OUT": variant})
        with eng:
            for n in counts:
                qt, qp = queries[n]
                loop_async(eng, wl, a.warmup, qt, qp, [])
                o0 = eng.overlapped_windows()
                begin_s = []
                t0 = time.perf_counter()
                off, ids = loop_async(eng, wl, a.steps, qt, qp, begin_s)
                ms = 1e3 * (time.perf_counter() - t0) / a.steps
                assert np.array_equal(off, want[n][0]) and np.array_equal(norm(ids), norm(want[n][1]))
                asyn[(variant, n)] = {"ms_per_step": ms, "begin_host_us_median": 1e6 * float(np.median(begin_s)),
                                      "begin_host_us_max": 1e6 * float(np.max(begin_s)),
                                      "overlapped_windows": eng.overlapped_windows() - o0}
    for n in counts:
        best = min(("copy", "mapped"), key=lambda v: asyn[(v, n)]["ms_per_step"])
        floor = max(res["plain_ms_per_step"], link[n])
        res["rows"].append({
            "queries": n, "ids": int(want[n][1].size), "id_bytes": 4 * int(want[n][1].size),
            "link_ms": link[n], "serial_ms_per_step": serial[n],
            "async_copy": asyn[("copy", n)], "async_mapped": asyn[("mapped", n)], "faster": best,
            "floor_ms": floor, "floor_is": "plain step" if res["plain_ms_per_step"] >= link[n] else "link time",
            "async_over_floor": asyn[(best, n)]["ms_per_step"] / floor,
            "serial_over_async": serial[n] / asyn[(best, n)]["ms_per_step"]})
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "drain_async_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def loop_shared_async(eng, wl, n, qt, qp, begin_s):
    """Loop (iii) with ps_drain_shared_begin / _end.  Returns the last view (copies)."""
    L, h = eng._L, eng._h
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    tp, pp = qt.ctypes.data_as(u32p), qp.ctypes.data_as(u32p)
    lp, op, mp, n_lists, total = u32p(), u64p(), u32p(), C.c_uint32(), C.c_uint64()
    end = lambda: L.ps_drain_shared_end(h, C.byref(lp), C.byref(op), C.byref(mp), C.byref(n_lists), C.byref(total))
    eng.publish(wl.msg_topics)
    for i in range(n):
        eng.run_async()
        t0 = time.perf_counter()
        rc = L.ps_drain_shared_begin(h, tp, pp, qt.size, 0, 0)
        begin_s.append(time.perf_counter() - t0)
        assert rc == 0, rc
        if i + 1 < n:
            eng.publish(wl.msg_topics)
        if i:
            eng.wait()
            rc = end()
            assert rc == 0, rc
    eng.wait()
    rc = end()
    assert rc == 0, rc
    lists = np.ctypeslib.as_array(lp, shape=(qt.size,)).copy()
    off = np.ctypeslib.as_array(op, shape=(n_lists.value + 1,)).copy()
    ids = np.ctypeslib.as_array(mp, shape=(max(total.value, 1),))[:total.value].copy()
    return lists, off, ids


def pipelined_shared_main(a, wl):
    counts = [int(x) for x in a.pipelined_queries.split(",")]
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "steps": a.steps,
           "warmup": a.warmup, "rows": [], "device_phases": []}
    queries = {n: pick_queries(wl, n, a.seed) for n in counts + [a.large_queries]}

    # the quiet timing engine: the synchronous call's answer (the reference of
    # the loops below) and the device time of every pass of the new call
    want = {}
    eng, _ = stepped_engine(wl, {"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        for n in counts + [a.large_queries]:
            qt, qp = queries[n]
            want[n] = eng.drain_shared(qt, qp)
            rows = []
            for _ in range(a.reps + 1):  # (the first call allocates)
                with StderrCapture() as cap:
                    eng.drain_shared_begin(qt, qp)
                    got = eng.drain_shared_end()
                assert all(np.array_equal(x, y) for x, y in zip(got, want[n]))
                row = phase_line(cap.text, "drain_shared_begin")
                for k in ("list_cap", "id_cap", "seg_bound", "view_bytes"):
                    row[k] = int(re.search(rf"\b{k} (\d+)", cap.text).group(1))
                rows.append(row)
            best = min(rows[1:], key=lambda r: r["classify_ms"] + r["assign_ms"])
            with StderrCapture() as cap:
                eng.drain_shared(qt, qp)
            sync = [phase_line(x, "drain_shared") for x in cap.text.splitlines() if "psamd drain_shared:" in x][-1]
            print(f"device phases, {n} pairs: done", file=sys.stderr, flush=True)
            res["device_phases"].append({"queries": n, "begin": best, "synchronous": sync,
                                         "assign_over_classify": best["assign_ms"] / best["classify_ms"]
                                         if best["classify_ms"] else None})

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0) / a.steps

    eng = fresh_engine(wl, {})
    with eng:
        loop_plain(eng, wl, a.warmup)
        o0 = eng.overlapped_windows()
        res["plain_ms_per_step"] = timed(lambda: loop_plain(eng, wl, a.steps))
        res["plain_overlapped_windows"] = eng.overlapped_windows() - o0
    for n in counts:
        qt, qp = queries[n]
        row = {"queries": n, "n_lists": int(want[n][1].size - 1), "shared_ids": int(want[n][2].size)}
        eng = fresh_engine(wl, {})
        with eng:
            loop_async(eng, wl, a.warmup, qt, qp, [])
            o0 = eng.overlapped_windows()
            begin_s = []
            t0 = time.perf_counter()
            off, ids = loop_async(eng, wl, a.steps, qt, qp, begin_s)
            row["drain_begin"] = {"ms_per_step": 1e3 * (time.perf_counter() - t0) / a.steps,
                                  "begin_host_us_median": 1e6 * float(np.median(begin_s)),
                                  "overlapped_windows": eng.overlapped_windows() - o0,
                                  "bytes_to_host": 8 * (n + 2) + 4 * int(ids.size)}
        eng = fresh_engine(wl, {})
        with eng:
            loop_shared_async(eng, wl, a.warmup, qt, qp, [])
            o0 = eng.overlapped_windows()
            begin_s = []
            t0 = time.perf_counter()
            lists, loff, lids = loop_shared_async(eng, wl, a.steps, qt, qp, begin_s)
            ms = 1e3 * (time.perf_counter() - t0) / a.steps
            assert np.array_equal(lists, want[n][0]) and np.array_equal(loff, want[n][1])
            assert np.array_equal(norm(lids), norm(want[n][2]))
            assert same_answer(lists, loff, lids, off, ids)
            row["drain_shared_begin"] = {"ms_per_step": ms, "begin_host_us_median": 1e6 * float(np.median(begin_s)),
                                         "begin_host_us_max": 1e6 * float(np.max(begin_s)),
                                         "overlapped_windows": eng.overlapped_windows() - o0}
        print(f"pipelined loops, {n} pairs: done", file=sys.stderr, flush=True)
        row["shared_over_plain"] = row["drain_shared_begin"]["ms_per_step"] / res["plain_ms_per_step"]
        row["drain_begin_over_shared"] = row["drain_begin"]["ms_per_step"] / row["drain_shared_begin"]["ms_per_step"]
        res["rows"].append(row)
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "drain_shared_async_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def loop_sink(eng, wl, n, run_s):
    """publish; ps_run_async; ps_wait of the previous; ps_sink_take of the
    previous (a sink is set).  Returns the last view (copies)."""
    view = None
    eng.publish(wl.msg_topics)
    for i in range(n):
        t0 = time.perf_counter()
        eng.run_async()
        run_s.append(time.perf_counter() - t0)
        if i + 1 < n:
            eng.publish(wl.msg_topics)
        if i:
            eng.wait()
            view = eng.sink_take(copy=False)
    eng.wait()
    view = eng.sink_take(copy=False)
    return tuple(x.copy() for x in view)


def loop_shared_async_timed(eng, wl, n, qt, qp, run_s):
    """loop_shared_async with the host time of ps_run_async + ps_drain_shared_begin per step."""
    eng.publish(wl.msg_topics)
    for i in range(n):
        t0 = time.perf_counter()
        eng.run_async()
        eng.drain_shared_begin(qt, qp)
        run_s.append(time.perf_counter() - t0)
        if i + 1 < n:
            eng.publish(wl.msg_topics)
        if i:
            eng.wait()
            eng.drain_shared_end(copy=False)
    eng.wait()
    return eng.drain_shared_end()


def sink_main(a, wl):
    """--sink: the pipelined loop with a sink set (publish; ps_run_async;
    ps_wait and ps_sink_take of the previous) against the loop of
    --pipelined --shared (ps_drain_shared_begin / _end behind every run), both
    in this process and alternating, --reps timings each; one multi-window
    case (msg_window cut so that the largest topic takes three windows); the
    host time of the sink per run from PSAMD_DRAIN_TIMING's host clock."""
    counts = [int(x) for x in a.pipelined_queries.split(",")]
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "steps": a.steps,
           "warmup": a.warmup, "reps": a.reps, "rows": []}
    queries = {n: pick_queries(wl, n, a.seed) for n in counts}

    def engine(env, msg_window=65536):
        os.environ.update(env)
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=msg_window)
        WL.build_engine_topics(e, wl)
        for k in env:
            os.environ.pop(k, None)
        return e

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return 1e3 * (time.perf_counter() - t0) / a.steps, out

    with engine({}) as plain:
        loop_plain(plain, wl, a.warmup)
        res["plain_ms_per_step"] = [timed(lambda: loop_plain(plain, wl, a.steps))[0] for _ in range(a.reps)]
    for n in counts:
        qt, qp = queries[n]
        row = {"queries": n, "shared_begin_ms_per_step": [], "sink_ms_per_step": []}
        with engine({}) as par, engine({}) as snk:
            snk.sink_set(qt, qp)
            loop_shared_async_timed(par, wl, a.warmup, qt, qp, [])
            loop_sink(snk, wl, a.warmup, [])
            o_par, o_snk = par.overlapped_windows(), snk.overlapped_windows()
            host_par, host_snk = [], []
            for _ in range(a.reps):
                ms, want = timed(lambda: loop_shared_async_timed(par, wl, a.steps, qt, qp, host_par))
                row["shared_begin_ms_per_step"].append(ms)
                ms, got = timed(lambda: loop_sink(snk, wl, a.steps, host_snk))
                row["sink_ms_per_step"].append(ms)
                assert got[0].shape == (1, n) and np.array_equal(got[0][0], want[0]) and np.array_equal(got[1], want[1])
                assert np.array_equal(norm(got[2]), norm(want[2]))
            row["n_lists"] = int(want[1].size - 1)
            row["ids"] = int(want[2].size)
            row["shared_begin_overlapped_windows"] = par.overlapped_windows() - o_par
            row["sink_overlapped_windows"] = snk.overlapped_windows() - o_snk
            row["run_async_plus_begin_host_us_median"] = 1e6 * float(np.median(host_par))
            row["run_async_with_sink_host_us_median"] = 1e6 * float(np.median(host_snk))
        sp, ss = row["shared_begin_ms_per_step"], row["sink_ms_per_step"]
        row["sink_median_over_shared_begin_median"] = float(np.median(ss) / np.median(sp))
        row["sink_median_within_shared_begin_spread"] = bool(min(sp) <= np.median(ss) <= max(sp))
        with engine({"PSAMD_DRAIN_TIMING": "1"}) as tim:
            tim.sink_set(qt, qp)
            with StderrCapture() as cap:
                loop_sink(tim, wl, 8, [])
                tim.publish(wl.msg_topics)
                tim.run()
                tim.drain_shared(qt, qp)
            us = [float(x) for x in re.findall(r"psamd sink: .*host_us ([0-9.]+)", cap.text)]
            row["sink_host_us_per_run_median"] = float(np.median(us[2:]))
            row["view_bytes"] = int(re.findall(r"psamd sink: .*view_bytes (\d+)", cap.text)[-1])
            m = re.findall(r"psamd drain_shared: .*copy_ms ([0-9.]+)", cap.text)
            row["link_ms_of_the_ids"] = float(m[-1]) if m else None
        print(f"sink loops, {n} pairs: done", file=sys.stderr, flush=True)
        res["rows"].append(row)

    # three windows per step: the largest topic's messages over three windows
    most = int(np.bincount(wl.msg_topics).max())
    cap3 = ((most + 2) // 3 + 63) // 64 * 64
    qt, qp = queries[counts[-1]]
    multi = {"queries": counts[-1], "msg_window": cap3, "largest_topic_msgs": most}
    with engine({}, cap3) as plain, engine({}, cap3) as snk:
        snk.sink_set(qt, qp)
        loop_plain(plain, wl, a.warmup)
        loop_sink(snk, wl, a.warmup, [])
        o_plain, o_snk = plain.overlapped_windows(), snk.overlapped_windows()
        multi["plain_ms_per_step"], multi["sink_ms_per_step"] = [], []
        for _ in range(a.reps):
            multi["plain_ms_per_step"].append(timed(lambda: loop_plain(plain, wl, a.steps))[0])
            ms, got = timed(lambda: loop_sink(snk, wl, a.steps, []))
            multi["sink_ms_per_step"].append(ms)
        multi["windows_per_step"] = int(got[0].shape[0])
        multi["n_lists"] = int(got[1].size - 1)
        multi["ids"] = int(got[2].size)
        multi["plain_overlapped_windows"] = plain.overlapped_windows() - o_plain
        multi["sink_overlapped_windows"] = snk.overlapped_windows() - o_snk
    res["three_windows"] = multi
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "sink_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


HBM_SPEC_BYTES_PER_S = 8e12


def all_subscriptions(eng, n_topics):
    """(topic, peer) of every non-root node, topic by topic in node order; the first query of each topic."""
    node_peer = eng.graph(PE.G_NODE_PEER)
    parts, first = [], [0]
    for t in range(n_topics):
        g = eng.graph_topic(t)
        lo, hi = g["nbase"] + 1, g["nbase"] + g["n_nodes"]
        parts.append(node_peer[lo:max(lo, hi)].astype(np.uint32) if g["exists"] else np.empty(0, dtype=np.uint32))
        first.append(first[-1] + parts[-1].size)
    qt = np.repeat(np.arange(n_topics, dtype=np.uint32), np.diff(first))
    return qt, np.concatenate(parts), first


def topics_agree(r, first, n_peers, qp, lists, loff, lids):
    """ps_drain_topics' answer r expanded per subscription equals ps_drain_shared's (lists, loff, lids)."""
    ours = np.empty(qp.size, dtype=np.uint32)
    at = np.zeros(n_peers, dtype=np.int64)
    for i in range(len(first) - 1):
        q = qp[first[i]:first[i + 1]]
        ours[first[i]:first[i + 1]] = r["topic_list"][i]
        at[q] = np.arange(first[i], first[i + 1])
        e0, e1 = int(r["exc_off"][i]), int(r["exc_off"][i + 1])
        ours[at[r["exc_peer"][e0:e1]]] = r["exc_list"][e0:e1]
    if not np.array_equal(ours == PE.NONE, lists == PE.NONE):
        return False
    keep = ours != PE.NONE
    pairs = np.unique(np.stack([ours[keep], lists[keep]]), axis=1)
    return all(np.array_equal(r["ids"][int(r["list_off"][a]):int(r["list_off"][a + 1])], lids[int(loff[b]):int(loff[b + 1])])
               for a, b in pairs.T)


def topics_main(a, wl):
    nt = len(wl.topics)
    topics = np.arange(nt, dtype=np.uint32)
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": nt, "reps": a.reps}
    eng, _ = stepped_engine(wl, {"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        qt, qp, first = all_subscriptions(eng, nt)
        res["subscriptions_in_the_node_space"] = int(qt.size)
        rows = []
        for _ in range(a.reps + 1):  # (the first call builds the window's tables and allocates)
            with StderrCapture() as cap:
                r = eng.drain_topics(topics)
            row = phase_line(cap.text, "drain_topics")
            for k in ("strips", "nodes", "row_bytes", "exceptions"):
                row[k] = int(re.search(rf"\b{k} (\d+)", cap.text).group(1))
            rows.append(row)
        res["topics_phases"] = rows[1:]
        lists, loff, lids, n_lists, total = shared_sizes(eng, qt, qp)
        rows = []
        for _ in range(a.reps + 1):
            with StderrCapture() as cap:
                rc, _, _ = raw_shared(eng, qt, qp, lists, loff, lids)
            assert rc == 0, rc
            rows.append(phase_line(cap.text, "drain_shared"))
        res["shared_phases"] = rows[1:]
        res["answers_agree"] = bool(topics_agree(r, first, wl.n_peers, qp, lists, loff, lids[:total]))
        assert res["answers_agree"]
        res.update(n_full=int(r["n_full"].sum()), exceptions=int(r["exc_peer"].size), lists=int(r["list_off"].size - 1),
                   ids=int(r["ids"].size), shared_lists=n_lists, shared_ids=total)
        digest = []
        for _ in range(a.reps + 1):
            with StderrCapture() as cap:
                eng.seen_digest()
            digest.append(float(re.search(r"psamd digest: device_ms ([0-9.]+)", cap.text).group(1)))
        res["k_digest_device_ms"] = digest[1:]
    eng, _ = stepped_engine(wl, {})
    with eng:
        walls = {"topics": [], "shared": [], "digest": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            eng.drain_topics(topics)
            walls["topics"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            rc, _, _ = raw_shared(eng, qt, qp, lists, loff, lids)
            walls["shared"].append(1e3 * (time.perf_counter() - t0))
            assert rc == 0, rc
            t0 = time.perf_counter()
            eng.seen_digest()
            walls["digest"].append(1e3 * (time.perf_counter() - t0))
    res["topics_wall_ms"], res["shared_wall_ms"], res["digest_wall_ms"] = (walls[k][1:] for k in ("topics", "shared", "digest"))
    tp, sp = res["topics_phases"], res["shared_phases"]
    res["topics_host_ms"] = [p["host_strips_ms"] + p["host_lists_ms"] for p in tp]
    res["shared_host_ms"] = [p["host_queries_ms"] + p["host_lists_ms"] for p in sp]
    res["shared_over_topics_wall"] = float(np.median(res["shared_wall_ms"]) / np.median(res["topics_wall_ms"]))
    cls, dig = [p["classify_ms"] for p in tp], res["k_digest_device_ms"]
    res["classify_ms"] = cls
    res["classify_over_digest"] = float(np.median(cls) / np.median(dig))
    res["digest_spread_ms"] = max(dig) - min(dig)
    res["classify_within_digest_plus_spread"] = bool(np.median(cls) <= np.median(dig) + max(max(dig) - min(dig), max(cls) - min(cls)))
    res["classify_vs_hbm_spec"] = tp[0]["row_bytes"] / (float(np.median(cls)) / 1e3) / HBM_SPEC_BYTES_PER_S
    res["digest_vs_hbm_spec"] = tp[0]["row_bytes"] / (float(np.median(dig)) / 1e3) / HBM_SPEC_BYTES_PER_S
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "drain_topics_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

TOPIC_KEYS = ("topic_list", "n_nodes", "n_full", "exc_off", "exc_peer", "exc_list", "list_off")


def loop_topics_serial(eng, wl, n, topics):
    r = None
    for _ in range(n):
        eng.publish(wl.msg_topics)
        eng.run()
        r = eng.drain_topics(topics)
    return r


def loop_topics_async(eng, wl, n, topics, exc_cap, begin_s):
    """Loop (iii) with ps_drain_topics_begin / _end.  Returns the last view (copies)."""
    L, h = eng._L, eng._h
    tp = topics.ctypes.data_as(C.POINTER(C.c_uint32))
    r = None
    eng.publish(wl.msg_topics)
    for i in range(n):
        eng.run_async()
        t0 = time.perf_counter()
        rc = L.ps_drain_topics_begin(h, tp, topics.size, exc_cap, 0, 0)
        begin_s.append(time.perf_counter() - t0)
        assert rc == 0, rc
        eng._drain_n.append((2, topics.size))
        if i + 1 < n:
            eng.publish(wl.msg_topics)
        if i:
            eng.wait()
            r = eng.drain_topics_end(copy=False)
    eng.wait()
    r = eng.drain_topics_end()
    return r


def pipelined_topics_main(a, wl):
    topics = np.arange(len(wl.topics), dtype=np.uint32)
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": int(topics.size),
           "steps": a.steps, "warmup": a.warmup, "reps": a.reps}
    # the passes' device time, each run apart and waited for (not a wall figure)
    eng = fresh_engine(wl, {"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        eng.publish(wl.msg_topics)
        eng.run()
        with StderrCapture():
            exc_cap = max(int(eng.drain_topics(topics)["exc_off"][-1]), 1)  # (every step publishes the same batch)
        rows = []
        for _ in range(a.reps + 1):  # (the first call allocates; each builds its window's tables)
            eng.publish(wl.msg_topics)
            eng.run()
            with StderrCapture() as cap:
                eng.drain_topics_begin(topics, exc_cap=exc_cap)
                want = eng.drain_topics_end()
            row = phase_line(cap.text, "drain_topics_begin")
            for k in ("strips", "nodes", "row_bytes", "exc_cap", "list_cap", "id_cap", "seg_bound", "upload_bytes", "view_bytes"):
                row[k] = int(re.search(rf"\b{k} (\d+)", cap.text).group(1))
            row["host_us"] = float(re.search(r"host_us ([0-9.]+)", cap.text).group(1))
            rows.append(row)
        res["device_phases"] = rows[1:]
        with StderrCapture():
            sync = eng.drain_topics(topics)
        assert all(np.array_equal(want[k], sync[k]) for k in TOPIC_KEYS) and np.array_equal(want["ids"], sync["ids"])
    res.update(exceptions=int(want["exc_off"][-1]), lists=int(want["list_off"].size - 1), ids=int(want["ids"].size),
               view_bytes=rows[-1]["view_bytes"], upload_bytes=rows[-1]["upload_bytes"])
    eng = fresh_engine(wl, {})
    with eng:
        loop_plain(eng, wl, a.warmup)
        loop_topics_serial(eng, wl, a.warmup, topics)
        loop_topics_async(eng, wl, a.warmup, topics, exc_cap, [])
        plain, serial, asyn, begin_us, over = [], [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            loop_plain(eng, wl, a.steps)
            plain.append(1e3 * (time.perf_counter() - t0) / a.steps)
            t0 = time.perf_counter()
            rs = loop_topics_serial(eng, wl, a.steps, topics)
            serial.append(1e3 * (time.perf_counter() - t0) / a.steps)
            o0 = eng.overlapped_windows()
            begin_s = []
            t0 = time.perf_counter()
            ra = loop_topics_async(eng, wl, a.steps, topics, exc_cap, begin_s)
            asyn.append(1e3 * (time.perf_counter() - t0) / a.steps)
            over.append(eng.overlapped_windows() - o0)
            begin_us.append({"median": 1e6 * float(np.median(begin_s)), "max": 1e6 * float(np.max(begin_s))})
            # entry for entry (every step publishes the same batch under new ids)
            assert all(np.array_equal(ra[k], rs[k]) for k in TOPIC_KEYS), "loop (iii) differs from loop (ii)"
            assert np.array_equal(norm(ra["ids"]), norm(rs["ids"])), "loop (iii) differs from loop (ii)"
    res.update(plain_ms_per_step=plain, serial_ms_per_step=serial, async_ms_per_step=asyn, begin_host_us=begin_us,
               async_overlapped_windows=over, answers_agree=True)
    res["serial_spread_ms"] = max(serial) - min(serial)
    res["serial_minus_async_ms"] = float(np.median(serial) - np.median(asyn))
    res["async_faster_than_serial_by_more_than_its_spread"] = bool(res["serial_minus_async_ms"] > res["serial_spread_ms"])
    res["async_minus_plain_ms"] = float(np.median(asyn) - np.median(plain))
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "drain_topics_async_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def loop_sink_topics(eng, wl, n, run_s):
    """publish; ps_run_async; ps_wait of the previous; ps_sink_take_topics of
    the previous (a topics sink is set).  Returns the last view (copies)."""
    view = None
    eng.publish(wl.msg_topics)
    for i in range(n):
        t0 = time.perf_counter()
        eng.run_async()
        run_s.append(time.perf_counter() - t0)
        if i + 1 < n:
            eng.publish(wl.msg_topics)
        if i:
            eng.wait()
            view = eng.sink_take_topics(copy=False)
    eng.wait()
    view = eng.sink_take_topics(copy=False)
    return {k: (v.copy() if k != "n_windows" else v) for k, v in view.items()}


def loop_topics_async_timed(eng, wl, n, topics, exc_cap, run_s):
    """loop_topics_async with the host time of ps_run_async + ps_drain_topics_begin per step."""
    r = None
    eng.publish(wl.msg_topics)
    for i in range(n):
        t0 = time.perf_counter()
        eng.run_async()
        eng.drain_topics_begin(topics, exc_cap=exc_cap)
        run_s.append(time.perf_counter() - t0)
        if i + 1 < n:
            eng.publish(wl.msg_topics)
        if i:
            eng.wait()
            r = eng.drain_topics_end(copy=False)
    eng.wait()
    r = eng.drain_topics_end()
    return r


def sink_topics_main(a, wl):
    topics = np.arange(len(wl.topics), dtype=np.uint32)
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": int(topics.size),
           "steps": a.steps, "warmup": a.warmup, "reps": a.reps}

    def engine(env, msg_window=65536):
        os.environ.update(env)
        e = PE.Engine(wl.n_peers, len(wl.topics), seed=wl.seed, msg_window=msg_window)
        WL.build_engine_topics(e, wl)
        for k in env:
            os.environ.pop(k, None)
        return e

    def us(xs):
        return {"median": 1e6 * float(np.median(xs)), "max": 1e6 * float(np.max(xs))}

    with engine({}) as eng:
        eng.publish(wl.msg_topics)
        eng.run()
        exc_cap = max(int(eng.drain_topics(topics)["exc_off"][-1]), 1)  # (every step publishes the same batch)
        loop_plain(eng, wl, a.warmup)
        loop_topics_async_timed(eng, wl, a.warmup, topics, exc_cap, [])
        eng.sink_set_topics(topics, exc_cap=exc_cap)
        loop_sink_topics(eng, wl, a.warmup, [])
        eng.sink_set_topics([])
        plain, asyn, sink, asyn_us, sink_us, over_a, over_s = [], [], [], [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            loop_plain(eng, wl, a.steps)
            plain.append(1e3 * (time.perf_counter() - t0) / a.steps)
            o0, run_s = eng.overlapped_windows(), []
            t0 = time.perf_counter()
            ra = loop_topics_async_timed(eng, wl, a.steps, topics, exc_cap, run_s)
            asyn.append(1e3 * (time.perf_counter() - t0) / a.steps)
            over_a.append(eng.overlapped_windows() - o0)
            asyn_us.append(us(run_s))
            eng.sink_set_topics(topics, exc_cap=exc_cap)
            o0, run_s = eng.overlapped_windows(), []
            t0 = time.perf_counter()
            rk = loop_sink_topics(eng, wl, a.steps, run_s)
            sink.append(1e3 * (time.perf_counter() - t0) / a.steps)
            over_s.append(eng.overlapped_windows() - o0)
            sink_us.append(us(run_s))
            eng.sink_set_topics([])
            # entry for entry (one window a step; every step publishes the same batch under new ids)
            assert rk["n_windows"] == 1
            for k in TOPIC_KEYS:
                got = rk[k][0] if k in ("topic_list", "n_nodes", "n_full") else rk[k]
                assert np.array_equal(got, ra[k]), ("the sink-topics loop differs from loop (iii)", k)
            assert np.array_equal(norm(rk["ids"]), norm(ra["ids"])), "the sink-topics loop differs from loop (iii)"
        res.update(exc_cap=exc_cap, exceptions=int(rk["exc_off"][-1]), lists=int(rk["list_off"].size - 1),
                   ids=int(rk["ids"].size))
    res.update(plain_ms_per_step=plain, async_ms_per_step=asyn, sink_ms_per_step=sink, async_run_host_us=asyn_us,
               sink_run_host_us=sink_us, async_overlapped_windows=over_a, sink_overlapped_windows=over_s, answers_agree=True)
    res["async_spread_ms"] = max(asyn) - min(asyn)
    res["sink_minus_async_ms"] = float(np.median(sink) - np.median(asyn))
    res["sink_slower_than_async_by_more_than_its_spread"] = bool(res["sink_minus_async_ms"] > res["async_spread_ms"])
    res["sink_minus_plain_ms"] = float(np.median(sink) - np.median(plain))

    # the sink's own host time and upload per run (PSAMD_DRAIN_TIMING's line; the timed build of the
    # tables waits in no sink window), and three windows a step for the record
    def timed_runs(msg_window, runs):
        rows = []
        with engine({"PSAMD_DRAIN_TIMING": "1"}, msg_window) as eng:
            eng.sink_set_topics(topics, exc_cap=exc_cap * 3)
            for _ in range(runs):
                eng.publish(wl.msg_topics)
                with StderrCapture() as cap:
                    eng.run()
                    r = eng.sink_take_topics(copy=False)
                m = re.search(r"psamd sink_topics: .*", cap.text).group(0)
                rows.append({"windows": int(re.search(r"windows (\d+)", m).group(1)),
                             "strips": re.search(r"strips (\w+)", m).group(1),
                             "upload_bytes": int(re.search(r"upload_bytes (\d+)", m).group(1)),
                             "view_bytes": int(re.search(r"view_bytes (\d+)", m).group(1)),
                             "host_us": float(re.search(r"host_us ([0-9.]+)", m).group(1)),
                             "lists": int(r["list_off"].size - 1), "ids": int(r["ids"].size)})
        return rows

    res["sink_runs_timed"] = timed_runs(65536, a.reps + 2)
    res["three_windows_runs_timed"] = timed_runs(7040, a.reps + 2)
    with engine({}, 7040) as eng:
        loop_plain(eng, wl, a.warmup)
        eng.sink_set_topics(topics, exc_cap=exc_cap * 3)
        loop_sink_topics(eng, wl, a.warmup, [])
        t0 = time.perf_counter()
        rk = loop_sink_topics(eng, wl, a.steps, [])
        t_sink = 1e3 * (time.perf_counter() - t0) / a.steps
        eng.sink_set_topics([])
        t0 = time.perf_counter()
        loop_plain(eng, wl, a.steps)
        res["three_windows"] = {"msg_window": 7040, "windows_per_step": int(rk["n_windows"]), "sink_ms_per_step": t_sink,
                                "plain_ms_per_step": 1e3 * (time.perf_counter() - t0) / a.steps,
                                "lists": int(rk["list_off"].size - 1), "ids": int(rk["ids"].size)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "sink_topics_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def host_peer_load(eng, wl, topics):
    """Per-peer load as a caller derives it without ps_peer_load: the audience
    answer, every topic's parent array, numpy.  (A Join topic's parents name
    the members: a peer with no upstream is outside the node space.)"""
    r = eng.drain_topics(topics)
    n = wl.n_peers
    recv = np.zeros(n, dtype=np.uint64)
    sent = np.zeros(n, dtype=np.uint64)
    sizes = np.diff(r["list_off"]).astype(np.uint64)
    c_all = np.bincount(wl.msg_topics, minlength=len(wl.topics))
    for i, t in enumerate(topics):
        c = int(c_all[t])
        if not c:
            continue
        par = eng.parents(int(t))
        kid = np.nonzero(par != 0xFFFFFFFF)[0]
        n_child = np.bincount(par[kid], minlength=n).astype(np.uint64)
        k = np.zeros(n, dtype=np.uint64)
        k[kid] = c
        lo, hi = int(r["exc_off"][i]), int(r["exc_off"][i + 1])
        if hi > lo:  # the nodes that are not full: their private list's length, or nothing
            el = r["exc_list"][lo:hi].astype(np.int64)
            have = el != 0xFFFFFFFF
            ke = np.zeros(hi - lo, dtype=np.uint64)
            ke[have] = sizes[el[have]]
            k[r["exc_peer"][lo:hi]] = ke
        root = wl.topics[int(t)].root
        k[root] = 0
        recv += k
        sent += k * n_child
        sent[root] += np.uint64(c) * n_child[root]
    return recv, sent


def loop_track(eng, wl, n):
    """publish; ps_run_async; ps_wait of the previous (topics are tracked);
    one ps_load_take behind the last."""
    loop_plain(eng, wl, n)
    return eng.load_take()


def load_main(a, wl):
    """--load: ps_peer_load over every topic after one step: its phases
    (PSAMD_DRAIN_TIMING) beside ps_drain_topics' in one process, its wall
    against the host derivation (ps_drain_topics + ps_topic_get_parents per
    topic + numpy), the two answers compared array for array; then the step
    of the pipelined loop with every topic tracked (ps_load_track) against
    the step with the audience sink over the same topics and the plain step,
    alternating in one process.  Writes DIR/load_bench.json."""
    nt = len(wl.topics)
    topics = np.arange(nt, dtype=np.uint32)
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": nt, "reps": a.reps,
           "steps": a.steps, "warmup": a.warmup}
    eng, st = stepped_engine(wl, {"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        rows = []
        for _ in range(a.reps + 1):  # (the first call builds the window's tables and allocates)
            with StderrCapture() as cap:
                recv, sent = eng.peer_load(topics)
            row = phase_line(cap.text, "peer_load")
            for k in ("strips", "nodes", "row_bytes"):
                row[k] = int(re.search(rf"\b{k} (\d+)", cap.text).group(1))
            rows.append(row)
        res["load_phases"] = rows[1:]
        rows = []
        for _ in range(a.reps + 1):
            with StderrCapture() as cap:
                eng.drain_topics(topics)
            rows.append(phase_line(cap.text, "drain_topics"))
        res["topics_phases"] = rows[1:]
        assert int(recv.sum()) == st.deliveries, (int(recv.sum()), st.deliveries)
        res.update(deliveries=int(st.deliveries), recv_sum=int(recv.sum()), sent_sum=int(sent.sum()),
                   peers_receiving=int((recv > 0).sum()), peers_sending=int((sent > 0).sum()),
                   sent_max=int(sent.max()), recv_max=int(recv.max()))
    eng, _ = stepped_engine(wl, {})
    with eng:
        walls = {"load": [], "host": [], "topics": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            got = eng.peer_load(topics)
            walls["load"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            want = host_peer_load(eng, wl, topics)
            walls["host"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            eng.drain_topics(topics)
            walls["topics"].append(1e3 * (time.perf_counter() - t0))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "ps_peer_load differs from the host derivation"
    res["load_wall_ms"], res["host_derivation_wall_ms"], res["topics_wall_ms"] = (walls[k][1:] for k in ("load", "host", "topics"))
    res["answers_agree"] = True
    res["host_over_load_wall"] = float(np.median(res["host_derivation_wall_ms"]) / np.median(res["load_wall_ms"]))
    lp = res["load_phases"]
    res["load_over_classify_device"] = float(np.median([p["load_ms"] for p in lp]) / np.median([p["classify_ms"] for p in lp]))

    # tracking in the pipelined loop, beside the audience sink and the plain step
    for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING"):
        os.environ.pop(k, None)
    eng = PE.Engine(wl.n_peers, nt, seed=wl.seed)
    WL.build_engine_topics(eng, wl)
    with eng:
        eng.publish(wl.msg_topics)
        eng.run()
        exc_cap = max(int(eng.drain_topics(topics)["exc_off"][-1]), 1)
        loop_plain(eng, wl, a.warmup)
        eng.sink_set_topics(topics, exc_cap=exc_cap)
        loop_sink_topics(eng, wl, a.warmup, [])
        eng.sink_set_topics([])
        eng.load_track(topics)
        loop_track(eng, wl, a.warmup)
        eng.load_track([])
        plain, sink, track, over = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            loop_plain(eng, wl, a.steps)
            plain.append(1e3 * (time.perf_counter() - t0) / a.steps)
            eng.sink_set_topics(topics, exc_cap=exc_cap)
            t0 = time.perf_counter()
            loop_sink_topics(eng, wl, a.steps, [])
            sink.append(1e3 * (time.perf_counter() - t0) / a.steps)
            eng.sink_set_topics([])
            eng.load_track(topics)
            o0 = eng.overlapped_windows()
            t0 = time.perf_counter()
            r, s, nw = loop_track(eng, wl, a.steps)
            track.append(1e3 * (time.perf_counter() - t0) / a.steps)
            over.append(eng.overlapped_windows() - o0)
            eng.load_track([])
            assert nw == a.steps and np.array_equal(r, recv * np.uint64(a.steps)) and np.array_equal(s, sent * np.uint64(a.steps))
    res.update(plain_ms_per_step=plain, sink_topics_ms_per_step=sink, track_ms_per_step=track, track_overlapped_windows=over,
               track_minus_plain_ms=float(np.median(track) - np.median(plain)),
               sink_minus_plain_ms=float(np.median(sink) - np.median(plain)), tracked_totals_agree=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "load_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def host_topic_hops(eng, wl, topics):
    """Deliveries by hop as a caller derives them without ps_topic_hops: the
    audience answer, every topic's parent array, depths by numpy (level d + 1 =
    the peers whose upstream stands at level d)."""
    r = eng.drain_topics(topics)
    n, cols = wl.n_peers, PE.MAX_ROUNDS
    out = [np.zeros((len(topics), cols), dtype=np.uint64) for _ in range(3)]
    sizes = np.diff(r["list_off"]).astype(np.uint64)
    c_all = np.bincount(wl.msg_topics, minlength=len(wl.topics))
    for i, t in enumerate(topics):
        c = int(c_all[t])
        if not c:
            continue
        par = eng.parents(int(t))
        root = wl.topics[int(t)].root
        kid = np.nonzero(par != 0xFFFFFFFF)[0]
        kid = kid[kid != root]
        depth = np.full(n, -1, dtype=np.int64)
        depth[root] = 0
        todo, d = kid, 0
        while todo.size:
            at = depth[par[todo]] == d
            if not at.any():
                break
            d += 1
            depth[todo[at]] = d
            todo = todo[~at]
        k = np.zeros(n, dtype=np.uint64)
        k[kid] = c
        lo, hi = int(r["exc_off"][i]), int(r["exc_off"][i + 1])
        if hi > lo:  # the nodes that are not full: their private list's length, or nothing
            el = r["exc_list"][lo:hi].astype(np.int64)
            have = el != 0xFFFFFFFF
            ke = np.zeros(hi - lo, dtype=np.uint64)
            ke[have] = sizes[el[have]]
            k[r["exc_peer"][lo:hi]] = ke
        k[root] = 0
        m = kid[depth[kid] > 0]
        col = np.minimum(depth[m], cols - 1)
        out[0][i] = np.bincount(col, minlength=cols).astype(np.uint64)
        out[1][i] = np.bincount(col[k[m] > 0], minlength=cols).astype(np.uint64)
        out[2][i] = np.bincount(col, weights=k[m].astype(np.float64), minlength=cols).astype(np.uint64)
    return tuple(out)


def hops_main(a, wl):
    """--hops (see the module text).  Writes DIR/hops_bench.json."""
    nt = len(wl.topics)
    topics = np.arange(nt, dtype=np.uint32)
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": nt, "reps": a.reps,
           "steps": a.steps, "warmup": a.warmup}
    eng, st = stepped_engine(wl, {"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        for tag, call, key in (("topic_hops", eng.topic_hops, "hops_phases"), ("peer_load", eng.peer_load, "load_phases"),
                               ("drain_topics", eng.drain_topics, "topics_phases")):
            rows = []
            for _ in range(a.reps + 1):  # (the first call builds the window's tables and allocates)
                with StderrCapture() as cap:
                    got = call(topics)
                row = phase_line(cap.text, tag)
                for k in ("strips", "nodes", "row_bytes", "partials"):
                    m = re.search(rf"\b{k} (\d+)", cap.text)
                    if m:
                        row[k] = int(m.group(1))
                rows.append(row)
            res[key] = rows[1:]
            if tag == "topic_hops":
                blocking = got
        assert int(blocking[2].sum()) == st.deliveries, (int(blocking[2].sum()), st.deliveries)
        depth = [int(np.nonzero(blocking[0][i])[0].max()) if blocking[0][i].any() else 0 for i in range(nt)]
        res.update(deliveries=int(st.deliveries), deliv_sum=int(blocking[2].sum()), nodes_sum=int(blocking[0].sum()),
                   reached_sum=int(blocking[1].sum()), max_depth=max(depth),
                   deliv_by_hop=blocking[2].sum(axis=0)[:max(depth) + 1].tolist())
    eng, _ = stepped_engine(wl, {})
    with eng:
        walls = {"hops": [], "host": [], "topics": [], "load": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            got = eng.topic_hops(topics)
            walls["hops"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            want = host_topic_hops(eng, wl, topics)
            walls["host"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            eng.drain_topics(topics)
            walls["topics"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            eng.peer_load(topics)
            walls["load"].append(1e3 * (time.perf_counter() - t0))
            for g, w, name in zip(got, want, ("nodes", "reached", "deliv")):
                assert np.array_equal(g, w), f"ps_topic_hops {name} differs from the host derivation"
    res["hops_wall_ms"], res["host_derivation_wall_ms"], res["topics_wall_ms"], res["load_wall_ms"] = \
        (walls[k][1:] for k in ("hops", "host", "topics", "load"))
    res["answers_agree"] = True
    res["host_over_hops_wall"] = float(np.median(res["host_derivation_wall_ms"]) / np.median(res["hops_wall_ms"]))
    hp, lp = res["hops_phases"], res["load_phases"]
    res["hops_kernels_over_load_kernel"] = float(np.median([p["hops_ms"] + p["sum_ms"] for p in hp]) /
                                                 np.median([p["load_ms"] for p in lp]))

    # tracking in the pipelined loop: plain, hops, load, both
    for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING"):
        os.environ.pop(k, None)
    eng = PE.Engine(wl.n_peers, nt, seed=wl.seed)
    WL.build_engine_topics(eng, wl)
    none = np.zeros(0, dtype=np.uint32)
    # (hops tracked, load tracked, the audience sink set)
    modes = {"plain": (False, False, False), "hops": (True, False, False), "load": (False, True, False),
             "both": (True, True, False), "all_three": (True, True, True)}

    def timed(hops, load, sink, steps):
        eng.hops_track(topics if hops else none)
        eng.load_track(topics if load else none)
        if sink:
            eng.sink_set_topics(topics, exc_cap=exc_cap)
        o0 = eng.overlapped_windows()
        t0 = time.perf_counter()
        if sink:
            loop_sink_topics(eng, wl, steps, [])
        else:
            loop_plain(eng, wl, steps)
        th = eng.hops_take() if hops else None
        tl = eng.load_take() if load else None
        ms = 1e3 * (time.perf_counter() - t0) / steps
        if sink:
            eng.sink_set_topics([])
        return ms, eng.overlapped_windows() - o0, th, tl

    with eng:
        eng.publish(wl.msg_topics)
        eng.run()
        load0 = eng.peer_load(topics)
        exc_cap = max(int(eng.drain_topics(topics)["exc_off"][-1]), 1)
        for mode in modes.values():
            timed(*mode, a.warmup)
        ms = {k: [] for k in modes}
        over = {k: [] for k in modes}
        for _ in range(a.reps):
            for name, (hops, load, sink) in modes.items():
                t, o, th, tl = timed(hops, load, sink, a.steps)
                ms[name].append(t)
                over[name].append(int(o))
                if hops:
                    assert th[3:] == (a.steps, 0)
                    for g, w in zip(th[:3], blocking):
                        assert np.array_equal(g, w * np.uint64(a.steps)), "tracked hop totals differ"
                if load:
                    assert tl[2] == a.steps and np.array_equal(tl[0], load0[0] * np.uint64(a.steps))
        eng.hops_track(none)
        eng.load_track(none)
    res.update(ms_per_step=ms, overlapped_windows=over, tracked_totals_agree=True,
               hops_minus_plain_ms=float(np.median(ms["hops"]) - np.median(ms["plain"])),
               load_minus_plain_ms=float(np.median(ms["load"]) - np.median(ms["plain"])),
               both_minus_plain_ms=float(np.median(ms["both"]) - np.median(ms["plain"])),
               all_three_minus_plain_ms=float(np.median(ms["all_three"]) - np.median(ms["plain"])))
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "hops_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def host_peer_downstream(eng, wl, topics):
    """The audience behind each peer as a caller derives it without
    ps_peer_downstream: the audience answer, every topic's parent array, depths
    by numpy as in host_topic_hops, then each level's (1, k) pairs added into
    the parents', the deepest level first."""
    n = wl.n_peers
    below = np.zeros(n, dtype=np.uint64)
    carried = np.zeros(n, dtype=np.uint64)
    for c, par, root, k, depth, levels in host_topic_trees(eng, wl, topics):
        w_n = (depth >= 0).astype(np.uint64)
        w_k = k.copy()
        for at in reversed(levels):
            np.add.at(w_n, par[at], w_n[at])
            np.add.at(w_k, par[at], w_k[at])
        member = depth >= 0
        below[member] += w_n[member] - np.uint64(1)
        carried[member] += w_k[member] - k[member]
    return below, carried


def host_topic_trees(eng, wl, topics, with_exc=False):
    """What the host derivations over subtrees start from, per topic with
    messages: (c, parents, root, k per peer -- the root's and every
    non-member's 0 --, depth per peer, the peers of levels 1 ..), from the
    audience answer and ps_topic_get_parents.  with_exc: the topic's position
    in the request and the peers of its exceptions, in the audience answer's
    order, behind them."""
    r = eng.drain_topics(topics)
    n = wl.n_peers
    sizes = np.diff(r["list_off"]).astype(np.uint64)
    c_all = np.bincount(wl.msg_topics, minlength=len(wl.topics))
    for i, t in enumerate(topics):
        c = int(c_all[t])
        if not c:
            continue
        par = eng.parents(int(t))
        root = wl.topics[int(t)].root
        kid = np.nonzero(par != 0xFFFFFFFF)[0]
        kid = kid[kid != root]
        depth = np.full(n, -1, dtype=np.int64)
        depth[root] = 0
        todo, levels = kid, []
        while todo.size:
            at = depth[par[todo]] == len(levels)
            if not at.any():
                break
            levels.append(todo[at])
            depth[todo[at]] = len(levels)
            todo = todo[~at]
        k = np.zeros(n, dtype=np.uint64)
        k[kid] = c
        lo, hi = int(r["exc_off"][i]), int(r["exc_off"][i + 1])
        if hi > lo:  # the nodes that are not full: their private list's length, or nothing
            el = r["exc_list"][lo:hi].astype(np.int64)
            have = el != 0xFFFFFFFF
            ke = np.zeros(hi - lo, dtype=np.uint64)
            ke[have] = sizes[el[have]]
            k[r["exc_peer"][lo:hi]] = ke
        k[root] = 0
        k[depth < 0] = 0
        if with_exc:
            yield c, par, root, k, depth, levels, i, r["exc_peer"][lo:hi]
        else:
            yield c, par, root, k, depth, levels


def downstream_main(a, wl):
    """--downstream (see the module text).  Writes DIR/downstream_bench.json."""
    nt = len(wl.topics)
    topics = np.arange(nt, dtype=np.uint32)
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": nt, "reps": a.reps,
           "steps": a.steps, "warmup": a.warmup}
    eng, st = stepped_engine(wl, {"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        for tag, call, key in (("peer_downstream", eng.peer_downstream, "downstream_phases"),
                               ("peer_load", eng.peer_load, "load_phases")):
            rows = []
            for _ in range(a.reps + 1):  # (the first call builds the window's tables and allocates)
                with StderrCapture() as cap:
                    got = call(topics)
                row = phase_line(cap.text, tag)
                for k in ("strips", "nodes", "row_bytes", "work", "launches"):
                    m = re.search(rf"\b{k} (\d+)", cap.text)
                    if m:
                        row[k] = int(m.group(1))
                rows.append(row)
            res[key] = rows[1:]
            if tag == "peer_downstream":
                blocking = got
        roots = np.array([ts.root for ts in wl.topics])
        res.update(deliveries=int(st.deliveries), below_sum=int(blocking[0].sum()), carried_sum=int(blocking[1].sum()),
                   below_max=int(blocking[0].max()), carried_max=int(blocking[1].max()),
                   peers_with_audience=int((blocking[0] > 0).sum()), carried_at_roots=int(blocking[1][np.unique(roots)].sum()))
    eng, _ = stepped_engine(wl, {})
    with eng:
        walls = {"downstream": [], "host": [], "load": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            got = eng.peer_downstream(topics)
            walls["downstream"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            want = host_peer_downstream(eng, wl, topics)
            walls["host"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            eng.peer_load(topics)
            walls["load"].append(1e3 * (time.perf_counter() - t0))
            for g, w, name in zip(got, want, ("below", "carried")):
                assert np.array_equal(g, w), f"ps_peer_downstream {name} differs from the host derivation"
            for g, w in zip(got, blocking):
                assert np.array_equal(g, w)
    res["downstream_wall_ms"], res["host_derivation_wall_ms"], res["load_wall_ms"] = \
        (walls[k][1:] for k in ("downstream", "host", "load"))
    res["answers_agree"] = True
    res["host_over_downstream_wall"] = float(np.median(res["host_derivation_wall_ms"]) / np.median(res["downstream_wall_ms"]))
    dp, lp = res["downstream_phases"], res["load_phases"]
    res["downstream_kernels_over_load_kernel"] = float(np.median([p["weights_ms"] + p["levels_ms"] for p in dp]) /
                                                       np.median([p["load_ms"] for p in lp]))

    # tracking in the pipelined loop: plain, downstream, beside hops and load
    for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING"):
        os.environ.pop(k, None)
    eng = PE.Engine(wl.n_peers, nt, seed=wl.seed)
    WL.build_engine_topics(eng, wl)
    none = np.zeros(0, dtype=np.uint32)
    modes = {"plain": (False, False), "downstream": (True, False), "beside_hops_and_load": (True, True)}

    def timed(down, others, steps):
        eng.downstream_track(topics if down else none)
        eng.hops_track(topics if others else none)
        eng.load_track(topics if others else none)
        o0 = eng.overlapped_windows()
        t0 = time.perf_counter()
        loop_plain(eng, wl, steps)
        td = eng.downstream_take() if down else None
        th = eng.hops_take() if others else None
        tl = eng.load_take() if others else None
        return 1e3 * (time.perf_counter() - t0) / steps, eng.overlapped_windows() - o0, td, th, tl

    with eng:
        eng.publish(wl.msg_topics)
        eng.run()
        load0, hops0 = eng.peer_load(topics), eng.topic_hops(topics)
        for mode in modes.values():
            timed(*mode, a.warmup)
        ms = {k: [] for k in modes}
        over = {k: [] for k in modes}
        for _ in range(a.reps):
            for name, (down, others) in modes.items():
                t, o, td, th, tl = timed(down, others, a.steps)
                ms[name].append(t)
                over[name].append(int(o))
                if down:
                    assert td[2:] == (a.steps, 0)
                    for g, w in zip(td[:2], blocking):
                        assert np.array_equal(g, w * np.uint64(a.steps)), "tracked downstream totals differ"
                if others:
                    assert th[3:] == (a.steps, 0) and np.array_equal(th[2], hops0[2] * np.uint64(a.steps))
                    assert tl[2] == a.steps and np.array_equal(tl[0], load0[0] * np.uint64(a.steps))
        eng.downstream_track(none)
        eng.hops_track(none)
        eng.load_track(none)
    res.update(ms_per_step=ms, overlapped_windows=over, tracked_totals_agree=True,
               downstream_minus_plain_ms=float(np.median(ms["downstream"]) - np.median(ms["plain"])),
               beside_minus_plain_ms=float(np.median(ms["beside_hops_and_load"]) - np.median(ms["plain"])))
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "downstream_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def host_peer_cut(eng, wl, topics):
    """The losses and their cut points as a caller derives them without
    ps_peer_cut: host_topic_trees' k per peer, miss = c - k for the non-root
    members, a cut point where a member lacks messages under a full parent, and
    each level's (1, miss) pairs added into the parents', the deepest first."""
    n = wl.n_peers
    out = [np.zeros(n, dtype=np.uint64) for _ in range(4)]
    for c, par, root, k, depth, levels in host_topic_trees(eng, wl, topics):
        member = depth > 0
        miss = np.where(member, np.uint64(c) - k, np.uint64(0))
        w_n = (depth >= 0).astype(np.uint64)
        w_m = miss.copy()
        for at in reversed(levels):
            np.add.at(w_n, par[at], w_n[at])
            np.add.at(w_m, par[at], w_m[at])
        up = np.where(member, par, root).astype(np.int64)
        cut = member & (miss > 0) & (miss[up] == 0)
        out[0] += miss
        out[1] += cut.astype(np.uint64)
        out[2][cut] += w_n[cut] - np.uint64(1)
        out[3][cut] += w_m[cut]
    return tuple(out)


def cut_main(a, wl):
    """--cut (see the module text).  Writes DIR/cut_bench.json."""
    nt = len(wl.topics)
    topics = np.arange(nt, dtype=np.uint32)
    live = (np.random.default_rng(a.seed).random(wl.n_peers) >= 0.01).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": nt, "reps": a.reps,
           "steps": a.steps, "warmup": a.warmup, "mask_seed": a.seed, "dead_peers": int((live == 0).sum())}

    def masked_engine(env):
        for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING", "PSAMD_DRAIN_EMIT"):
            os.environ.pop(k, None)
        os.environ.update(env)
        eng = PE.Engine(wl.n_peers, nt, seed=wl.seed)
        WL.build_engine_topics(eng, wl)
        eng.set_live(live)
        eng.publish(wl.msg_topics)
        return eng, eng.run()

    eng, st = masked_engine({"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        for tag, call, key in (("peer_cut", eng.peer_cut, "cut_phases"),
                               ("peer_downstream", eng.peer_downstream, "downstream_phases")):
            rows = []
            for _ in range(a.reps + 1):  # (the first call builds the window's tables and allocates)
                with StderrCapture() as cap:
                    got = call(topics)
                row = phase_line(cap.text, tag)
                for k in ("strips", "nodes", "row_bytes", "work", "launches"):
                    m = re.search(rf"\b{k} (\d+)", cap.text)
                    if m:
                        row[k] = int(m.group(1))
                rows.append(row)
            res[key] = rows[1:]
            if tag == "peer_cut":
                blocking = got
        res.update(deliveries=int(st.deliveries), missed_sum=int(blocking[0].sum()), cut_points=int(blocking[1].sum()),
                   orphaned_sum=int(blocking[2].sum()), lost_sum=int(blocking[3].sum()),
                   peers_with_a_cut=int((blocking[1] > 0).sum()), lost_max=int(blocking[3].max()))
        assert res["lost_sum"] == res["missed_sum"] and res["cut_points"] > 0
    eng, _ = masked_engine({})
    with eng:
        walls = {"cut": [], "host": [], "downstream": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            got = eng.peer_cut(topics)
            walls["cut"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            want = host_peer_cut(eng, wl, topics)
            walls["host"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            eng.peer_downstream(topics)
            walls["downstream"].append(1e3 * (time.perf_counter() - t0))
            for g, w, name in zip(got, want, ("missed", "cuts", "orphaned", "lost")):
                assert np.array_equal(g, w), f"ps_peer_cut {name} differs from the host derivation"
            for g, w in zip(got, blocking):
                assert np.array_equal(g, w)
    res["cut_wall_ms"], res["host_derivation_wall_ms"], res["downstream_wall_ms"] = \
        (walls[k][1:] for k in ("cut", "host", "downstream"))
    res["answers_agree"] = True
    res["host_over_cut_wall"] = float(np.median(res["host_derivation_wall_ms"]) / np.median(res["cut_wall_ms"]))
    res["cut_over_downstream_wall"] = float(np.median(res["cut_wall_ms"]) / np.median(res["downstream_wall_ms"]))
    cp, dp = res["cut_phases"], res["downstream_phases"]
    res["cut_levels_over_downstream_levels"] = float(np.median([p["levels_ms"] for p in cp]) /
                                                     np.median([p["levels_ms"] for p in dp]))

    # tracking in the pipelined loop: plain, cut, beside load, hops and downstream
    for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING"):
        os.environ.pop(k, None)
    eng = PE.Engine(wl.n_peers, nt, seed=wl.seed)
    WL.build_engine_topics(eng, wl)
    eng.set_live(live)
    none = np.zeros(0, dtype=np.uint32)
    modes = {"plain": (False, False), "cut": (True, False), "beside_load_hops_and_downstream": (True, True)}

    def timed(cut, others, steps):
        eng.cut_track(topics if cut else none)
        eng.downstream_track(topics if others else none)
        eng.hops_track(topics if others else none)
        eng.load_track(topics if others else none)
        o0 = eng.overlapped_windows()
        t0 = time.perf_counter()
        loop_plain(eng, wl, steps)
        tc = eng.cut_take() if cut else None
        td = eng.downstream_take() if others else None
        th = eng.hops_take() if others else None
        tl = eng.load_take() if others else None
        return 1e3 * (time.perf_counter() - t0) / steps, eng.overlapped_windows() - o0, tc, td, th, tl

    with eng:
        eng.publish(wl.msg_topics)
        eng.run()
        load0, hops0, down0 = eng.peer_load(topics), eng.topic_hops(topics), eng.peer_downstream(topics)
        for mode in modes.values():
            timed(*mode, a.warmup)
        ms = {k: [] for k in modes}
        over = {k: [] for k in modes}
        for _ in range(a.reps):
            for name, (cut, others) in modes.items():
                t, o, tc, td, th, tl = timed(cut, others, a.steps)
                ms[name].append(t)
                over[name].append(int(o))
                if cut:
                    assert tc[4:] == (a.steps, 0)
                    for g, w in zip(tc[:4], blocking):
                        assert np.array_equal(g, w * np.uint64(a.steps)), "tracked cut totals differ"
                if others:
                    assert td[2:] == (a.steps, 0) and np.array_equal(td[1], down0[1] * np.uint64(a.steps))
                    assert th[3:] == (a.steps, 0) and np.array_equal(th[2], hops0[2] * np.uint64(a.steps))
                    assert tl[2] == a.steps and np.array_equal(tl[0], load0[0] * np.uint64(a.steps))
        for track in (eng.cut_track, eng.downstream_track, eng.hops_track, eng.load_track):
            track(none)
    res.update(ms_per_step=ms, overlapped_windows=over, tracked_totals_agree=True,
               cut_minus_plain_ms=float(np.median(ms["cut"]) - np.median(ms["plain"])),
               beside_minus_plain_ms=float(np.median(ms["beside_load_hops_and_downstream"]) - np.median(ms["plain"])))
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "cut_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def host_topic_blame(eng, wl, topics):
    """Each missed subscriber and its cut point as a caller derives them
    without ps_topic_blame: host_topic_trees' k per peer and levels, the cut
    point and its level handed down level by level from the root, and the
    records in the order of the audience answer's exceptions."""
    n = wl.n_peers
    recs = [[np.empty(0, dtype=np.uint32)] for _ in range(5)]
    off = np.zeros(len(topics) + 1, dtype=np.uint64)
    for c, par, root, k, depth, levels, i, exc in host_topic_trees(eng, wl, topics, with_exc=True):
        miss = np.where(depth > 0, np.uint64(c) - k, np.uint64(0)).astype(np.int64)
        cut_peer = np.full(n, -1, dtype=np.int64)
        cut_hop = np.full(n, -1, dtype=np.int64)
        for d, at in enumerate(levels, 1):
            up = par[at].astype(np.int64)
            lacks, full_parent = miss[at] > 0, miss[up] == 0
            cut_peer[at] = np.where(lacks, np.where(full_parent, at, cut_peer[up]), -1)
            cut_hop[at] = np.where(lacks, np.where(full_parent, d, cut_hop[up]), -1)
        q = exc[miss[exc] > 0].astype(np.int64)
        off[i + 1] = q.size
        for out, x in zip(recs, (q, cut_peer[q], depth[q], cut_hop[q], miss[q])):
            out.append(x.astype(np.uint32))
    return {"rec_off": np.cumsum(off, dtype=np.uint64), **{k: np.concatenate(x) for k, x in zip(BLAME_KEYS, recs)}}


BLAME_KEYS = ("peer", "cut_peer", "hop", "cut_hop", "missed")


def blame_main(a, wl):
    """--blame (see the module text).  Writes DIR/blame_bench.json."""
    nt = len(wl.topics)
    topics = np.arange(nt, dtype=np.uint32)
    live = (np.random.default_rng(a.seed).random(wl.n_peers) >= 0.01).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": nt, "reps": a.reps,
           "mask_seed": a.seed, "dead_peers": int((live == 0).sum())}

    def masked_engine(env):
        for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING", "PSAMD_DRAIN_EMIT"):
            os.environ.pop(k, None)
        os.environ.update(env)
        eng = PE.Engine(wl.n_peers, nt, seed=wl.seed)
        WL.build_engine_topics(eng, wl)
        eng.set_live(live)
        eng.publish(wl.msg_topics)
        return eng, eng.run()

    # the device phases, alternating with yardstick (a): ps_peer_cut's on the same window
    eng, st = masked_engine({"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        rows = {"topic_blame": [], "peer_cut": []}
        for _ in range(a.reps + 1):  # (the first calls build the window's tables and allocate)
            for tag, call in (("topic_blame", eng.topic_blame), ("peer_cut", eng.peer_cut)):
                with StderrCapture() as cap:
                    got = call(topics)
                row = phase_line(cap.text, tag)
                for k in ("strips", "nodes", "row_bytes", "work", "launches", "records", "copied_bytes"):
                    m = re.search(rf"\b{k} (\d+)", cap.text)
                    if m:
                        row[k] = int(m.group(1))
                rows[tag].append(row)
                if tag == "topic_blame":
                    blocking = got
        res["blame_phases"], res["cut_phases"] = rows["topic_blame"][1:], rows["peer_cut"][1:]
        total = int(blocking["rec_off"][-1])
        res.update(deliveries=int(st.deliveries), records=total, copied_bytes=(nt + 1) * 8 + 5 * 4 * total,
                   cut_points=int((blocking["peer"] == blocking["cut_peer"]).sum()),
                   missed_sum=int(blocking["missed"].astype(np.uint64).sum()),
                   deepest_record=int(blocking["hop"].max()) if total else 0,
                   farthest_cut=int((blocking["hop"] - blocking["cut_hop"]).max()) if total else 0)
        assert total > 0
    # the walls, alternating with both yardsticks: (a) ps_peer_cut, (b) the host derivation
    eng, _ = masked_engine({})
    with eng:
        walls = {"blame": [], "host": [], "cut": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            got = eng.topic_blame(topics)
            walls["blame"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            want = host_topic_blame(eng, wl, topics)
            walls["host"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            eng.peer_cut(topics)
            walls["cut"].append(1e3 * (time.perf_counter() - t0))
            for k in ("rec_off",) + BLAME_KEYS:
                assert np.array_equal(got[k], want[k]), f"ps_topic_blame {k} differs from the host derivation"
                assert np.array_equal(got[k], blocking[k]), k
        # ps_blame over the records' own (topic, peer) pairs: ps_topic_blame expanded
        qt = np.repeat(topics, np.diff(got["rec_off"]).astype(np.int64))
        t0 = time.perf_counter()
        q = eng.blame(qt, got["peer"])
        res["blame_queries"], res["blame_queries_wall_ms"] = int(qt.size), 1e3 * (time.perf_counter() - t0)
        for g, k in zip(q, ("cut_peer", "hop", "cut_hop", "missed")):
            assert np.array_equal(g, got[k]), f"ps_blame {k} differs from ps_topic_blame"
    res["blame_wall_ms"], res["host_derivation_wall_ms"], res["cut_wall_ms"] = (walls[k][1:] for k in ("blame", "host", "cut"))
    res["answers_agree"] = True
    res["host_over_blame_wall"] = float(np.median(res["host_derivation_wall_ms"]) / np.median(res["blame_wall_ms"]))
    res["blame_over_cut_wall"] = float(np.median(res["blame_wall_ms"]) / np.median(res["cut_wall_ms"]))
    bp, cp = res["blame_phases"], res["cut_phases"]
    res["blame_sweep_over_cut_levels"] = float(np.median([p["sweep_ms"] for p in bp]) / np.median([p["levels_ms"] for p in cp]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "blame_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def blame_track_main(a, wl):
    """--blame-track (see the module text).  Writes DIR/blame_track_bench.json."""
    nt = len(wl.topics)
    topics = np.arange(nt, dtype=np.uint32)
    none = np.zeros(0, dtype=np.uint32)
    live = (np.random.default_rng(a.seed).random(wl.n_peers) >= 0.01).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    k = max(1, min(a.take_every, a.steps))
    steps = a.steps // k * k
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": nt, "reps": a.reps,
           "steps": steps, "warmup": a.warmup, "take_every": k, "mask_seed": a.seed, "dead_peers": int((live == 0).sum())}

    def masked_engine(env):
        eng = fresh_engine(wl, env)
        eng.set_live(live)
        eng.publish(wl.msg_topics)
        return eng, eng.run()

    def agree(t, blocking, windows):
        assert (t["n_windows"], t["n_skipped"], t["stored"]) == (windows, 0, t["total"]), "the tracker's counts"
        assert t["total"] == windows * blocking["peer"].size
        off = blocking["rec_off"].astype(np.int64)
        want = np.concatenate([[0], (off[1:][None, :] + off[-1] * np.arange(windows)[:, None]).ravel()])
        assert np.array_equal(t["rec_off"].astype(np.int64), want), "tracked rec_off differs"
        for key in BLAME_KEYS:
            assert np.array_equal(t[key], np.tile(blocking[key], windows)), f"tracked {key} differs from ps_topic_blame"

    # the device phases: one tracked window and one blocking call, alternating
    eng, st = masked_engine({"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        assert st.windows == 1
        blocking = eng.topic_blame(topics)
        total = int(blocking["rec_off"][-1])
        assert total > 0
        rows = {"blame_track": [], "topic_blame": [], "blame_take": []}
        eng.blame_track(topics, total)
        for _ in range(a.reps + 1):  # (the first pass allocates)
            eng.publish(wl.msg_topics)
            with StderrCapture() as cap:
                eng.run()
            row = phase_line(cap.text, "blame_track")
            for key in ("strips", "nodes", "row_bytes", "work", "launches"):
                m = re.search(rf"psamd blame_track: .*\b{key} (\d+)", cap.text)
                if m:
                    row[key] = int(m.group(1))
            rows["blame_track"].append(row)
            with StderrCapture() as cap:
                t = eng.blame_take()
            agree(t, blocking, 1)
            row = phase_line(cap.text, "blame_take")
            row["copied_bytes"] = int(re.search(r"copied_bytes (\d+)", cap.text).group(1))
            rows["blame_take"].append(row)
            with StderrCapture() as cap:
                got = eng.topic_blame(topics)
            rows["topic_blame"].append(phase_line(cap.text, "topic_blame"))
            for key in ("rec_off",) + BLAME_KEYS:
                assert np.array_equal(got[key], blocking[key]), key
        eng.blame_track(none)
        res.update(records=total, deliveries=int(st.deliveries), tracked_phases=rows["blame_track"][1:],
                   take_phases=rows["blame_take"][1:], blocking_phases=rows["topic_blame"][1:])
        dev = lambda rs, skip=(): float(np.median([sum(v for q, v in r.items() if q.endswith("_ms") and q not in skip) for r in rs]))
        res["tracked_window_device_ms"] = dev(res["tracked_phases"], ("host_ms",))
        res["blocking_call_device_ms"] = dev(res["blocking_phases"], ("host_strips_ms", "copy_ms"))
        res["blocking_call_copy_ms"] = float(np.median([r["copy_ms"] for r in res["blocking_phases"]]))

    # the walls: the tracked pipelined step, the loop it replaces, the untracked pipelined step
    eng, _ = masked_engine({})

    def tracked(n):
        eng.blame_track(topics, total * k)
        o0 = eng.overlapped_windows()
        t0 = time.perf_counter()
        takes = []
        for _ in range(n // k):
            loop_plain(eng, wl, k)
            takes.append(eng.blame_take())
        ms = 1e3 * (time.perf_counter() - t0) / n
        over = eng.overlapped_windows() - o0
        for t in takes:  # (outside the timed part)
            agree(t, blocking, k)
        eng.blame_track(none)
        return ms, over

    def blocking_loop(n):
        o0 = eng.overlapped_windows()
        t0 = time.perf_counter()
        for _ in range(n):
            eng.publish(wl.msg_topics)
            eng.run()
            got = eng.topic_blame(topics)
        ms = 1e3 * (time.perf_counter() - t0) / n
        for key in ("rec_off",) + BLAME_KEYS:
            assert np.array_equal(got[key], blocking[key]), key
        return ms, eng.overlapped_windows() - o0

    def plain(n):
        o0 = eng.overlapped_windows()
        t0 = time.perf_counter()
        for _ in range(n // k):
            loop_plain(eng, wl, k)
        return 1e3 * (time.perf_counter() - t0) / n, eng.overlapped_windows() - o0

    modes = {"tracked": tracked, "run_plus_topic_blame": blocking_loop, "plain": plain}
    with eng:
        for f in modes.values():
            f(max(a.warmup // k, 1) * k)
        ms = {name: [] for name in modes}
        over = {name: [] for name in modes}
        for _ in range(a.reps):
            for name, f in modes.items():
                t, o = f(steps)
                ms[name].append(t)
                over[name].append(int(o))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    res.update(ms_per_step=ms, overlapped_windows=over, records_agree=True, rec_cap=total * k,
               tracked_minus_plain_ms=med["tracked"] - med["plain"],
               blocking_loop_over_tracked=med["run_plus_topic_blame"] / med["tracked"])
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "blame_track_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


REPORT_CALLS = (("peer_load", "peer_load", ("recv", "sent")), ("topic_hops", "topic_hops", ("nodes", "reached", "deliv")),
                ("peer_downstream", "peer_downstream", ("below", "carried")),
                ("peer_cut", "peer_cut", ("missed", "cuts", "orphaned", "lost")))


def four_calls(eng, topics):
    out = {}
    for _, method, names in REPORT_CALLS:
        out.update(zip(names, getattr(eng, method)(topics)))
    return out


def report_main(a, wl):
    """--report, --report-once (see the module text).  Writes DIR/report_bench.json."""
    nt = len(wl.topics)
    topics = np.arange(nt, dtype=np.uint32)
    live = (np.random.default_rng(a.seed).random(wl.n_peers) >= 0.01).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": nt, "reps": a.reps,
           "steps": a.steps, "warmup": a.warmup, "mask_seed": a.seed, "dead_peers": int((live == 0).sum())}

    def masked_engine(env):
        for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING", "PSAMD_DRAIN_EMIT"):
            os.environ.pop(k, None)
        os.environ.update(env)
        eng = PE.Engine(wl.n_peers, nt, seed=wl.seed)
        WL.build_engine_topics(eng, wl)
        eng.set_live(live)
        eng.publish(wl.msg_topics)
        return eng, eng.run()

    if a.report_once:
        eng, st = masked_engine({})
        with eng:
            got = eng.peer_report(topics)
            print(json.dumps({"deliveries": int(st.deliveries), "recv_sum": int(got["recv"].sum()),
                              "cut_points": int(got["cuts"].sum())}))
        return

    # the device phases, the report and the four calls alternating
    eng, st = masked_engine({"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        phases = {"peer_report": []}
        phases.update({tag: [] for tag, _, _ in REPORT_CALLS})
        for _ in range(a.reps + 1):  # (the first calls build the window's tables and allocate)
            with StderrCapture() as cap:
                got = eng.peer_report(topics)
            row = phase_line(cap.text, "peer_report")
            for k in ("strips", "nodes", "partials", "work", "launches"):
                m = re.search(rf"\b{k} (\d+)", cap.text)
                if m:
                    row[k] = int(m.group(1))
            phases["peer_report"].append(row)
            for tag, method, names in REPORT_CALLS:
                with StderrCapture() as cap:
                    want = getattr(eng, method)(topics)
                phases[tag].append(phase_line(cap.text, tag))
                for k, w in zip(names, want):
                    assert np.array_equal(got[k], w), f"ps_peer_report {k} differs from ps_{tag}"
        res["phases"] = {k: v[1:] for k, v in phases.items()}

        def device_ms(rows):
            return float(np.median([sum(v for k, v in r.items() if k.endswith("_ms") and k != "host_strips_ms") for r in rows]))

        res["report_device_ms"] = device_ms(res["phases"]["peer_report"])
        res["four_calls_device_ms"] = float(sum(device_ms(res["phases"][tag]) for tag, _, _ in REPORT_CALLS))
        res.update(deliveries=int(st.deliveries), recv_sum=int(got["recv"].sum()), cut_points=int(got["cuts"].sum()),
                   lost_sum=int(got["lost"].sum()), missed_sum=int(got["missed"].sum()))
        assert res["recv_sum"] == res["deliveries"] and res["lost_sum"] == res["missed_sum"] and res["cut_points"] > 0
    # the walls, untimed
    eng, _ = masked_engine({})
    with eng:
        walls = {"report": [], "four_calls": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            got = eng.peer_report(topics)
            walls["report"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            blocking = four_calls(eng, topics)
            walls["four_calls"].append(1e3 * (time.perf_counter() - t0))
            for k in got:
                assert np.array_equal(got[k], blocking[k]), k
    res["report_wall_ms"], res["four_calls_wall_ms"] = walls["report"][1:], walls["four_calls"][1:]
    res["answers_agree"] = True
    res["four_calls_over_report_wall"] = float(np.median(res["four_calls_wall_ms"]) / np.median(res["report_wall_ms"]))

    # tracking in the pipelined loop: plain, the report, the four trackers
    eng = PE.Engine(wl.n_peers, nt, seed=wl.seed)
    WL.build_engine_topics(eng, wl)
    eng.set_live(live)
    none = np.zeros(0, dtype=np.uint32)
    modes = ("plain", "report", "four_trackers")
    trackers = (eng.load_track, eng.hops_track, eng.downstream_track, eng.cut_track)
    takes = (("load", eng.load_take, ("recv", "sent")), ("hops", eng.hops_take, ("nodes", "reached", "deliv")),
             ("downstream", eng.downstream_take, ("below", "carried")), ("cut", eng.cut_take, ("missed", "cuts", "orphaned", "lost")))

    def timed(mode, steps):
        eng.report_track(topics if mode == "report" else none)
        for track in trackers:
            track(topics if mode == "four_trackers" else none)
        o0 = eng.overlapped_windows()
        t0 = time.perf_counter()
        loop_plain(eng, wl, steps)
        totals, windows = {}, []
        if mode == "report":
            totals, nw, nsk = eng.report_take()
            windows = [nw]
            assert nsk == 0
        elif mode == "four_trackers":
            for _, take, names in takes:
                r = take()
                totals.update(zip(names, r))
                windows.append(r[len(names)])
        return 1e3 * (time.perf_counter() - t0) / steps, eng.overlapped_windows() - o0, totals, windows

    with eng:
        for mode in modes:
            timed(mode, a.warmup)
        ms = {k: [] for k in modes}
        over = {k: [] for k in modes}
        for _ in range(a.reps):
            for mode in modes:
                t, o, totals, windows = timed(mode, a.steps)
                ms[mode].append(t)
                over[mode].append(int(o))
                assert all(w == a.steps for w in windows), (mode, windows)
                for k, g in totals.items():
                    assert np.array_equal(g, blocking[k] * np.uint64(a.steps)), f"{mode}: tracked {k} totals differ"
                assert mode == "plain" or o > 0, f"{mode}: no overlapped window"
        eng.report_track(none)
        for track in trackers:
            track(none)
    four = ms["four_trackers"]
    res.update(ms_per_step=ms, overlapped_windows=over, tracked_totals_agree=True,
               report_minus_plain_ms=float(np.median(ms["report"]) - np.median(ms["plain"])),
               four_trackers_minus_plain_ms=float(np.median(four) - np.median(ms["plain"])),
               four_trackers_spread_ms=float(max(four) - min(four)),
               four_trackers_minus_report_ms=float(np.median(four) - np.median(ms["report"])))
    res["report_below_four_trackers_by_more_than_their_spread"] = bool(
        res["four_trackers_minus_report_ms"] > res["four_trackers_spread_ms"])
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "report_bench.json"), "w") as f:  # (a line per key, a line per phase row)
            rows = [f" {json.dumps(k)}: {json.dumps(v)}" for k, v in res.items() if k != "phases"]
            rows.append(' "phases": {\n' + ",\n".join(
                f"  {json.dumps(k)}: [\n   " + ",\n   ".join(json.dumps(r) for r in v) + "]" for k, v in res["phases"].items()) + "}")
            f.write("{\n" + ",\n".join(rows) + "\n}\n")


def dist_report_main(a, wl):
    """--dist-report (see the module text).  Writes DIR/dist_report_bench.json."""
    import threading

    what = PE.REPORT_DIST
    nt = len(wl.topics)
    topics = np.arange(nt, dtype=np.uint32)
    live = (np.random.default_rng(a.seed).random(wl.n_peers) >= 0.01).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": nt, "reps": a.reps,
           "what": what, "mask_seed": a.seed, "dead_peers": int((live == 0).sum())}

    def masked_engine(env):
        for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING", "PSAMD_DRAIN_EMIT"):
            os.environ.pop(k, None)
        os.environ.update(env)
        eng = PE.Engine(wl.n_peers, nt, seed=wl.seed)
        WL.build_engine_topics(eng, wl)
        eng.set_live(live)
        eng.publish(wl.msg_topics)
        return eng, eng.run()

    def counts(text, row, keys):
        for k in keys:
            m = re.search(rf"\b{k} (\d+)", text)
            if m:
                row[k] = int(m.group(1))
        return row

    # 1. one rank: the device phases, the two calls alternating
    eng, st = masked_engine({"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        phases = {"peer_report": [], "dist_report": []}
        for _ in range(a.reps + 1):  # (the first calls build the window's tables and allocate)
            with StderrCapture() as cap:
                want = eng.peer_report(topics, what)
            phases["peer_report"].append(counts(cap.text, phase_line(cap.text, "peer_report"), ("strips", "nodes", "work", "launches")))
            with StderrCapture() as cap:
                got = eng.dist_report(topics, what)
            phases["dist_report"].append(counts(cap.text, phase_line(cap.text, "dist_report"), ("strips", "nodes", "work", "launches")))
            for k in want:
                assert np.array_equal(got[k], want[k]), f"ps_dist_report {k} differs from ps_peer_report"
        res["phases"] = {k: v[1:] for k, v in phases.items()}

        def device_ms(rows):
            return float(np.median([sum(v for k, v in r.items() if k.endswith("_ms") and not k.startswith("host_")) for r in rows]))

        res["peer_report_device_ms"] = device_ms(res["phases"]["peer_report"])
        res["dist_report_device_ms"] = device_ms(res["phases"]["dist_report"])
        res["peer_report_levels_ms"] = float(np.median([r["levels_ms"] for r in res["phases"]["peer_report"]]))
        res["dist_report_sweep_ms"] = float(np.median([r["sweep_ms"] for r in res["phases"]["dist_report"]]))
        res.update(deliveries=int(st.deliveries), recv_sum=int(got["recv"].sum()))
        assert res["recv_sum"] == res["deliveries"]
    eng, _ = masked_engine({})
    with eng:
        walls = {"peer_report": [], "dist_report": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            want = eng.peer_report(topics, what)
            walls["peer_report"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            got = eng.dist_report(topics, what)
            walls["dist_report"].append(1e3 * (time.perf_counter() - t0))
            for k in want:
                assert np.array_equal(got[k], want[k]), k
    res["peer_report_wall_ms"], res["dist_report_wall_ms"] = walls["peer_report"][1:], walls["dist_report"][1:]
    res["dist_over_peer_report_wall"] = float(np.median(res["dist_report_wall_ms"]) / np.median(res["peer_report_wall_ms"]))
    res["answers_agree"] = True

    # 2. loopback ranks, cfg4-shaped, the peer hash
    w4 = WL.cfg4(200_000, 300)
    live4 = (np.random.default_rng(a.seed).random(w4.n_peers) >= 0.03).astype(np.uint8)
    live4[0] = 1
    with PE.Engine(w4.n_peers, 1, seed=w4.seed) as one:
        WL.build_engine_topics(one, w4)
        one.set_live(live4)
        one.publish(w4.msg_topics)
        one.run()
        whole = one.peer_report([0], what)
    res["ranks"] = {"workload": "cfg4-shaped: 200000 peers, 300 messages, one topic", "partition": "peer hash", "worlds": {}}

    def threads(fn, world):
        out, errs = [None] * world, []

        def go(r):
            try:
                out[r] = fn(r)
            except Exception as ex:  # noqa: BLE001
                errs.append((r, ex))

        th = [threading.Thread(target=go, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in th) and not errs, errs
        return out

    def ranks_up(world, timed):
        os.environ.pop("PSAMD_DRAIN_TIMING", None)
        if timed:
            os.environ["PSAMD_DRAIN_TIMING"] = "1"
        lb = PE.Loopback(world)
        engines = [PE.Engine(w4.n_peers, 1, seed=w4.seed) for _ in range(world)]
        os.environ.pop("PSAMD_DRAIN_TIMING", None)
        for r, e in enumerate(engines):
            e.dist_init_loopback(lb, r)
            WL.build_engine_topics(e, w4)
            e.set_live(live4)
            e.publish(w4.msg_topics)
        threads(lambda r: engines[r].run(), world)
        return lb, engines

    for world in (2, 4):
        # the sweep's shape and device phases from engines under PSAMD_DRAIN_TIMING, the walls from plain ones
        lb, engines = ranks_up(world, True)
        shape = []
        for _ in range(2):  # (the first call builds the slot tables and allocates)
            with StderrCapture() as cap:
                out = threads(lambda r: engines[r].dist_report([0], what), world)
        for r in range(world):
            m = re.search(rf"psamd dist_report: rank {r} .*", cap.text)
            assert m, cap.text
            row = {k: float(v) for k, v in re.findall(r"(\w+_ms) ([0-9.]+)", m.group(0))}
            shape.append(counts(m.group(0), row, ("strips", "nodes", "launches", "exchanges", "sent_bytes", "slot_bytes")))
        for e in engines:
            e.close()
        lb.close()
        lb, engines = ranks_up(world, False)

        def timed_call(r):
            t0 = time.perf_counter()
            got = engines[r].dist_report([0], what)
            return 1e3 * (time.perf_counter() - t0), got

        walls = []
        for _ in range(a.reps + 1):
            out = threads(timed_call, world)
            total = {k: sum(o[1][k] for o in out) for k in whole}
            for k in whole:
                assert np.array_equal(total[k], whole[k]), f"{world} ranks: the sum of {k} differs from one rank's"
            walls.append([o[0] for o in out])
        res["ranks"]["worlds"][str(world)] = {"per_rank": shape, "first_call_wall_ms": walls[0], "wall_ms": walls[1:]}
        for e in engines:
            e.close()
        lb.close()
    res["ranks"]["sums_agree"] = True
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "dist_report_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def dist_cut_main(a, wl):
    """--dist-cut (see the module text).  Writes DIR/dist_cut_bench.json."""
    import threading

    names = ("missed", "cuts", "orphaned", "lost")
    nt = len(wl.topics)
    topics = np.arange(nt, dtype=np.uint32)
    live = (np.random.default_rng(a.seed).random(wl.n_peers) >= 0.01).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": nt, "reps": a.reps,
           "mask_seed": a.seed, "dead_peers": int((live == 0).sum())}

    def masked_engine(env):
        for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING", "PSAMD_DRAIN_EMIT"):
            os.environ.pop(k, None)
        os.environ.update(env)
        eng = PE.Engine(wl.n_peers, nt, seed=wl.seed)
        WL.build_engine_topics(eng, wl)
        eng.set_live(live)
        eng.publish(wl.msg_topics)
        return eng, eng.run()

    def counts(text, row, keys):
        for k in keys:
            m = re.search(rf"\b{k} (\d+)", text)
            if m:
                row[k] = int(m.group(1))
        return row

    # 1. one rank: the device phases, the two calls alternating
    eng, st = masked_engine({"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        phases = {"peer_cut": [], "dist_cut": []}
        for _ in range(a.reps + 1):  # (the first calls build the window's tables and allocate)
            with StderrCapture() as cap:
                want = eng.peer_cut(topics)
            phases["peer_cut"].append(counts(cap.text, phase_line(cap.text, "peer_cut"), ("strips", "nodes", "work", "launches")))
            with StderrCapture() as cap:
                got = eng.dist_cut(topics)
            phases["dist_cut"].append(counts(cap.text, phase_line(cap.text, "dist_cut"), ("strips", "nodes", "work", "launches")))
            for k, g, w in zip(names, got, want):
                assert np.array_equal(g, w), f"ps_dist_cut {k} differs from ps_peer_cut"
        res["phases"] = {k: v[1:] for k, v in phases.items()}

        def device_ms(rows):
            return float(np.median([sum(v for k, v in r.items() if k.endswith("_ms") and not k.startswith("host_")) for r in rows]))

        res["peer_cut_device_ms"] = device_ms(res["phases"]["peer_cut"])
        res["dist_cut_device_ms"] = device_ms(res["phases"]["dist_cut"])
        res["peer_cut_levels_ms"] = float(np.median([r["levels_ms"] for r in res["phases"]["peer_cut"]]))
        res["dist_cut_sweep_ms"] = float(np.median([r["sweep_ms"] for r in res["phases"]["dist_cut"]]))
        res["dist_minus_peer_cut_device_ms"] = res["dist_cut_device_ms"] - res["peer_cut_device_ms"]
        res.update(deliveries=int(st.deliveries), cut_points=int(got[1].sum()), missed_sum=int(got[0].sum()))
        assert int(got[3].sum()) == res["missed_sum"] and res["cut_points"] > 0
    eng, _ = masked_engine({})
    with eng:
        walls = {"peer_cut": [], "dist_cut": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            want = eng.peer_cut(topics)
            walls["peer_cut"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            got = eng.dist_cut(topics)
            walls["dist_cut"].append(1e3 * (time.perf_counter() - t0))
            for k, g, w in zip(names, got, want):
                assert np.array_equal(g, w), k
    res["peer_cut_wall_ms"], res["dist_cut_wall_ms"] = walls["peer_cut"][1:], walls["dist_cut"][1:]
    res["dist_over_peer_cut_wall"] = float(np.median(res["dist_cut_wall_ms"]) / np.median(res["peer_cut_wall_ms"]))
    res["answers_agree"] = True

    # 2. loopback ranks, cfg4-shaped, the peer hash; the yardstick there: ps_dist_report(PS_REPORT_DOWNSTREAM)
    w4 = WL.cfg4(200_000, 300)
    live4 = (np.random.default_rng(a.seed).random(w4.n_peers) >= 0.03).astype(np.uint8)
    live4[0] = 1
    with PE.Engine(w4.n_peers, 1, seed=w4.seed) as one:
        WL.build_engine_topics(one, w4)
        one.set_live(live4)
        one.publish(w4.msg_topics)
        one.run()
        whole = one.peer_cut([0])
        whole_down = one.peer_report([0], PE.REPORT_DOWNSTREAM)
    res["ranks"] = {"workload": "cfg4-shaped: 200000 peers, 300 messages, one topic", "partition": "peer hash",
                    "cut_points": int(whole[1].sum()), "worlds": {}}

    def threads(fn, world):
        out, errs = [None] * world, []

        def go(r):
            try:
                out[r] = fn(r)
            except Exception as ex:  # noqa: BLE001
                errs.append((r, ex))

        th = [threading.Thread(target=go, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in th) and not errs, errs
        return out

    def ranks_up(world, timed):
        os.environ.pop("PSAMD_DRAIN_TIMING", None)
        if timed:
            os.environ["PSAMD_DRAIN_TIMING"] = "1"
        lb = PE.Loopback(world)
        engines = [PE.Engine(w4.n_peers, 1, seed=w4.seed) for _ in range(world)]
        os.environ.pop("PSAMD_DRAIN_TIMING", None)
        for r, e in enumerate(engines):
            e.dist_init_loopback(lb, r)
            WL.build_engine_topics(e, w4)
            e.set_live(live4)
            e.publish(w4.msg_topics)
        threads(lambda r: engines[r].run(), world)
        return lb, engines

    calls = {"dist_cut": lambda e: e.dist_cut([0]), "dist_report": lambda e: e.dist_report([0], PE.REPORT_DOWNSTREAM)}
    for world in (2, 4):
        # the pass's shape and device phases from engines under PSAMD_DRAIN_TIMING, the walls from plain ones
        lb, engines = ranks_up(world, True)
        shape = {}
        for tag, call in calls.items():
            for _ in range(2):  # (the first call builds the slot tables and allocates)
                with StderrCapture() as cap:
                    threads(lambda r: call(engines[r]), world)
            shape[tag] = []
            for r in range(world):
                m = re.search(rf"psamd {tag}: rank {r} .*", cap.text)
                assert m, cap.text
                row = {k: float(v) for k, v in re.findall(r"(\w+_ms) ([0-9.]+)", m.group(0))}
                shape[tag].append(counts(m.group(0), row, ("strips", "nodes", "launches", "exchanges", "sent_bytes", "slot_bytes")))
        for e in engines:
            e.close()
        lb.close()
        lb, engines = ranks_up(world, False)
        walls = {tag: [] for tag in calls}
        for _ in range(a.reps + 1):
            for tag, call in calls.items():  # (alternating)

                def timed_call(r):
                    t0 = time.perf_counter()
                    got = call(engines[r])
                    return 1e3 * (time.perf_counter() - t0), got

                out = threads(timed_call, world)
                if tag == "dist_cut":
                    for i, k in enumerate(names):
                        assert np.array_equal(sum(o[1][i] for o in out), whole[i]), f"{world} ranks: the sum of {k} differs from one rank's"
                else:
                    for k in whole_down:
                        assert np.array_equal(sum(o[1][k] for o in out), whole_down[k]), f"{world} ranks: the sum of {k} differs"
                walls[tag].append([o[0] for o in out])
        med = {tag: float(np.median(np.array(w[1:]))) for tag, w in walls.items()}
        res["ranks"]["worlds"][str(world)] = {
            "per_rank": shape, "first_call_wall_ms": {tag: w[0] for tag, w in walls.items()},
            "wall_ms": {tag: w[1:] for tag, w in walls.items()}, "median_wall_ms": med,
            "dist_cut_over_dist_report_wall": med["dist_cut"] / med["dist_report"]}
        for e in engines:
            e.close()
        lb.close()
    res["ranks"]["sums_agree"] = True
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "dist_cut_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def dist_blame_main(a, wl):
    """--dist-blame (see the module text).  Writes DIR/dist_blame_bench.json."""
    import threading

    keys = ("peer", "cut_peer", "hop", "cut_hop", "missed")
    nt = len(wl.topics)
    topics = np.arange(nt, dtype=np.uint32)
    live = (np.random.default_rng(a.seed).random(wl.n_peers) >= 0.01).astype(np.uint8)
    live[[ts.root for ts in wl.topics]] = 1
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "topics": nt, "reps": a.reps,
           "mask_seed": a.seed, "dead_peers": int((live == 0).sum())}

    def masked_engine(env):
        for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING", "PSAMD_DRAIN_EMIT"):
            os.environ.pop(k, None)
        os.environ.update(env)
        eng = PE.Engine(wl.n_peers, nt, seed=wl.seed)
        WL.build_engine_topics(eng, wl)
        eng.set_live(live)
        eng.publish(wl.msg_topics)
        return eng, eng.run()

    def counts(text, row, keys):
        for k in keys:
            m = re.search(rf"\b{k} (\d+)", text)
            if m:
                row[k] = int(m.group(1))
        return row

    def device_ms(rows):
        return float(np.median([sum(v for k, v in r.items() if k.endswith("_ms") and not k.startswith("host_")) for r in rows]))

    # 1. one rank: the device phases, the two calls alternating
    shape_keys = ("strips", "nodes", "work", "launches", "records", "copied_bytes")
    eng, st = masked_engine({"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        phases = {"topic_blame": [], "dist_blame": []}
        for _ in range(a.reps + 1):  # (the first calls build the window's tables and allocate)
            with StderrCapture() as cap:
                want = eng.topic_blame(topics)
            phases["topic_blame"].append(counts(cap.text, phase_line(cap.text, "topic_blame"), shape_keys))
            with StderrCapture() as cap:
                got = eng.dist_blame(topics)
            phases["dist_blame"].append(counts(cap.text, phase_line(cap.text, "dist_blame"), shape_keys))
            for k in ("rec_off",) + keys:
                assert np.array_equal(got[k], want[k]), f"ps_dist_blame {k} differs from ps_topic_blame"
        res["phases"] = {k: v[1:] for k, v in phases.items()}
        res["topic_blame_device_ms"] = device_ms(res["phases"]["topic_blame"])
        res["dist_blame_device_ms"] = device_ms(res["phases"]["dist_blame"])
        res["topic_blame_sweep_ms"] = float(np.median([r["sweep_ms"] for r in res["phases"]["topic_blame"]]))
        res["dist_blame_sweep_ms"] = float(np.median([r["sweep_ms"] for r in res["phases"]["dist_blame"]]))
        res["dist_over_topic_blame_device"] = res["dist_blame_device_ms"] / res["topic_blame_device_ms"]
        res.update(deliveries=int(st.deliveries), records=int(got["peer"].size),
                   cut_points=int((got["peer"] == got["cut_peer"]).sum()))
        assert res["records"] > res["cut_points"] > 0
    eng, _ = masked_engine({})
    with eng:
        walls = {"topic_blame": [], "dist_blame": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            want = eng.topic_blame(topics)
            walls["topic_blame"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            got = eng.dist_blame(topics)
            walls["dist_blame"].append(1e3 * (time.perf_counter() - t0))
            for k in ("rec_off",) + keys:
                assert np.array_equal(got[k], want[k]), k
    res["topic_blame_wall_ms"], res["dist_blame_wall_ms"] = walls["topic_blame"][1:], walls["dist_blame"][1:]
    res["dist_over_topic_blame_wall"] = float(np.median(res["dist_blame_wall_ms"]) / np.median(res["topic_blame_wall_ms"]))
    res["answers_agree"] = True

    # 2. loopback ranks, cfg4-shaped, the peer hash; the yardstick there: ps_dist_cut
    w4 = WL.cfg4(200_000, 300)
    live4 = (np.random.default_rng(a.seed).random(w4.n_peers) >= 0.03).astype(np.uint8)
    live4[0] = 1
    with PE.Engine(w4.n_peers, 1, seed=w4.seed) as one:
        WL.build_engine_topics(one, w4)
        one.set_live(live4)
        one.publish(w4.msg_topics)
        one.run()
        whole = one.topic_blame([0])
        whole_cut = one.peer_cut([0])
    by_peer = np.argsort(whole["peer"], kind="stable")
    whole_keyed = {k: whole[k][by_peer] for k in keys}
    res["ranks"] = {"workload": "cfg4-shaped: 200000 peers, 300 messages, one topic", "partition": "peer hash",
                    "records": int(whole["peer"].size), "cut_points": int((whole["peer"] == whole["cut_peer"]).sum()),
                    "worlds": {}}

    def threads(fn, world):
        out, errs = [None] * world, []

        def go(r):
            try:
                out[r] = fn(r)
            except Exception as ex:  # noqa: BLE001
                errs.append((r, ex))

        th = [threading.Thread(target=go, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in th) and not errs, errs
        return out

    def ranks_up(world, timed):
        os.environ.pop("PSAMD_DRAIN_TIMING", None)
        if timed:
            os.environ["PSAMD_DRAIN_TIMING"] = "1"
        lb = PE.Loopback(world)
        engines = [PE.Engine(w4.n_peers, 1, seed=w4.seed) for _ in range(world)]
        os.environ.pop("PSAMD_DRAIN_TIMING", None)
        for r, e in enumerate(engines):
            e.dist_init_loopback(lb, r)
            WL.build_engine_topics(e, w4)
            e.set_live(live4)
            e.publish(w4.msg_topics)
        threads(lambda r: engines[r].run(), world)
        return lb, engines

    calls = {"dist_blame": lambda e: e.dist_blame([0]), "dist_cut": lambda e: e.dist_cut([0])}
    for world in (2, 4):
        # the pass's shape and device phases from engines under PSAMD_DRAIN_TIMING, the walls from plain ones
        lb, engines = ranks_up(world, True)
        shape = {}
        for tag, call in calls.items():
            for _ in range(2):  # (the first call builds the slot tables and allocates)
                with StderrCapture() as cap:
                    threads(lambda r: call(engines[r]), world)
            shape[tag] = []
            for r in range(world):
                m = re.search(rf"psamd {tag}: rank {r} .*", cap.text)
                assert m, cap.text
                row = {k: float(v) for k, v in re.findall(r"(\w+_ms) ([0-9.]+)", m.group(0))}
                shape[tag].append(counts(m.group(0), row, ("strips", "nodes", "launches", "exchanges", "sent_bytes", "slot_bytes",
                                                           "records", "copied_bytes")))
        for e in engines:
            e.close()
        lb.close()
        lb, engines = ranks_up(world, False)
        walls = {tag: [] for tag in calls}
        for _ in range(a.reps + 1):
            for tag, call in calls.items():  # (alternating)

                def timed_call(r):
                    t0 = time.perf_counter()
                    got = call(engines[r])
                    return 1e3 * (time.perf_counter() - t0), got

                out = threads(timed_call, world)
                if tag == "dist_blame":  # the union, keyed by peer, against the one-rank answer
                    peer = np.concatenate([o[1]["peer"] for o in out])
                    at = np.argsort(peer, kind="stable")
                    for k in keys:
                        got = np.concatenate([o[1][k] for o in out])[at]
                        assert np.array_equal(got, whole_keyed[k]), f"{world} ranks: the union's {k} differs from one rank's"
                else:
                    for i in range(4):
                        assert np.array_equal(sum(o[1][i] for o in out), whole_cut[i]), f"{world} ranks: the cut's sum differs"
                walls[tag].append([o[0] for o in out])
        med = {tag: float(np.median(np.array(w[1:]))) for tag, w in walls.items()}
        res["ranks"]["worlds"][str(world)] = {
            "per_rank": shape, "first_call_wall_ms": {tag: w[0] for tag, w in walls.items()},
            "wall_ms": {tag: w[1:] for tag, w in walls.items()}, "median_wall_ms": med,
            "dist_blame_over_dist_cut_wall": med["dist_blame"] / med["dist_cut"]}
        for e in engines:
            e.close()
        lb.close()
    res["ranks"]["unions_agree"] = True
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "dist_blame_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def raw_shared(eng, qt, qp, lists, off, ids):
    n_lists, total = C.c_uint32(), C.c_uint64()
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = eng._L.ps_drain_shared(eng._h, qt.ctypes.data_as(u32p), qp.ctypes.data_as(u32p), qt.size,
                                lists.ctypes.data_as(u32p), off.ctypes.data_as(u64p), off.size - 1,
                                ids.ctypes.data_as(u32p) if ids is not None else None, 0 if ids is None else ids.size,
                                C.byref(n_lists), C.byref(total))
    return rc, n_lists.value, total.value


def phase_line(text, tag):
    m = re.search(rf"psamd {tag}: .*", text)
    assert m, text
    row = {k: float(v) for k, v in re.findall(r"(\w+_ms) ([0-9.]+)", m.group(0))}
    for k in ("classified", "waves", "lists", "segments", "ids"):
        mm = re.search(rf"\b{k} (\d+)", m.group(0))
        if mm:
            row[k] = int(mm.group(1))
    return row


def shared_sizes(eng, qt, qp):
    lists = np.empty(qt.size, dtype=np.uint32)
    rc, n_lists, total = raw_shared(eng, qt, qp, lists, np.empty(1, dtype=np.uint64), None)
    assert rc in (0, -7), rc
    return lists, np.empty(n_lists + 1, dtype=np.uint64), np.empty(max(total, 1), dtype=np.uint32), n_lists, total


def same_answer(lists, loff, lids, off, ids):
    """The shared result expanded is ps_drain's, query by query."""
    for q in range(lists.size):
        want = ids[int(off[q]):int(off[q + 1])]
        got = lids[int(loff[lists[q]]):int(loff[lists[q] + 1])] if lists[q] != PE.NONE else lids[:0]
        if not np.array_equal(got, want):
            return False
    return True


def shared_main(a, wl):
    """ps_drain_shared against ps_drain on the same queries of one window, in
    one process: the phases (PSAMD_DRAIN_TIMING=1: run apart, each
    synchronised), the wall clock of the untimed calls, the bytes that cross
    the link; and one batch ps_drain is not asked to serve."""
    counts = [int(x) for x in a.pipelined_queries.split(",")]
    res = {"workload": wl.name, "scale": a.scale, "n_peers": wl.n_peers, "n_msgs": wl.n_msgs, "rows": []}
    queries = {n: pick_queries(wl, n, a.seed) for n in counts + [a.large_queries]}
    words = {}  # row words under the message mask, per topic: ceil(window messages / 64)
    for t in range(len(wl.topics)):
        words[t] = -(-int(np.sum(wl.msg_topics == t)) // 64)
    phases, sizes = {}, {}
    eng, _ = stepped_engine(wl, {"PSAMD_DRAIN_TIMING": "1"})
    with eng:
        for n in counts + [a.large_queries]:
            qt, qp = queries[n]
            lists, loff, lids, n_lists, total = shared_sizes(eng, qt, qp)
            rows = []
            for _ in range(a.reps + 1):  # (the first call allocates; the very first builds the window's tables)
                with StderrCapture() as cap:
                    rc, _, _ = raw_shared(eng, qt, qp, lists, loff, lids)
                assert rc == 0, rc
                rows.append(phase_line(cap.text, "drain_shared"))
            sh = min(rows[1:], key=lambda r: r["classify_ms"])
            sizes[n] = (n_lists, total)
            row = {"queries": n, "shared_phases": sh, "n_lists": n_lists, "shared_ids": total,
                   "shared_bytes_to_host": 4 * n + 8 * (n_lists + 2) + 4 * total,
                   "shared_bound_bytes": 8 * n + 8 * (n_lists + 1) + 4 * total}
            # classify's algorithmic bytes: every classified row's words, the sorted query (8 B), the
            # generation byte, the verdict (4 B); each queried topic's mask words once
            alg = int(sum(8 * words[int(t)] for t in qt)) + 13 * n + 8 * sum(words[int(t)] for t in set(qt.tolist()))
            row["classify_algorithmic_bytes"] = alg
            row["classify_vs_hbm_spec"] = alg / (sh["classify_ms"] / 1e3) / HBM_SPEC_BYTES_PER_S if sh["classify_ms"] else None
            if n == a.large_queries:
                row["ps_drain"] = "skipped: its output would be %.1f GB of ids" % (
                    4e-9 * sum(64.0 * words[int(t)] for t in qt))
            else:
                off = np.empty(n + 1, dtype=np.uint64)
                rc, dtotal = raw_drain(eng, qt, qp, off, None)
                assert rc in (0, -7), rc
                ids = np.empty(max(dtotal, 1), dtype=np.uint32)
                rows = []
                for _ in range(a.reps + 1):
                    with StderrCapture() as cap:
                        rc, _ = raw_drain(eng, qt, qp, off, ids)
                    assert rc == 0, rc
                    rows.append(phase_line(cap.text, "drain"))
                row["drain_phases"] = min(rows[1:], key=lambda r: r["count_ms"] + r["emit_ms"] + r["copy_ms"])
                row.update(drain_ids=dtotal, drain_bytes_to_host=8 * (row["drain_phases"]["segments"] + 1) + 4 * dtotal)
                assert same_answer(lists, loff, lids, off, ids)
            phases[n] = row
    eng, _ = stepped_engine(wl, {})
    with eng:
        for n in counts + [a.large_queries]:
            qt, qp = queries[n]
            row = phases[n]
            lists = np.empty(n, dtype=np.uint32)
            loff = np.empty(sizes[n][0] + 1, dtype=np.uint64)
            lids = np.empty(max(sizes[n][1], 1), dtype=np.uint32)
            walls = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                rc, _, _ = raw_shared(eng, qt, qp, lists, loff, lids)
                walls.append(time.perf_counter() - t0)
                assert rc == 0, rc
            row["shared_wall_ms"] = 1e3 * min(walls[1:])
            if n != a.large_queries:
                off = np.empty(n + 1, dtype=np.uint64)
                ids = np.empty(max(row["drain_ids"], 1), dtype=np.uint32)
                walls = []
                for _ in range(a.reps + 1):
                    t0 = time.perf_counter()
                    rc, _ = raw_drain(eng, qt, qp, off, ids)
                    walls.append(time.perf_counter() - t0)
                    assert rc == 0, rc
                row["drain_wall_ms"] = 1e3 * min(walls[1:])
                row["drain_over_shared_wall"] = row["drain_wall_ms"] / row["shared_wall_ms"]
                row["bytes_ratio"] = row["drain_bytes_to_host"] / row["shared_bytes_to_host"]
            res["rows"].append(row)
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "drain_shared_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def spread_graph(n, hub, seed):
    """(row_ptr, col, root, live): out-degree uniform in 0..6, children uniform
    over the peers but the root; the root has six; 3 % dead.  hub > 0: peer 1, a
    child of the root, lists `hub` distinct peers instead."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 7, size=n)
    deg[0] = 6
    if hub:
        deg[1] = hub
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rp[1:])
    col = rng.integers(1, n, size=int(rp[-1]))
    if hub:
        col[rp[0]] = 1
        col[rp[1]:rp[2]] = rng.choice(np.arange(2, n), size=hub, replace=False)
    live = (rng.random(n) >= 0.03).astype(np.uint8)
    live[:2] = 1
    return rp.astype(np.uint32), col.astype(np.uint32), 0, live


def host_topic_spread(eng, rp, cl, root, c):
    """The answer as a caller derives it without ps_topic_spread: who holds
    the messages from ps_peer_load, then a frontier BFS over the child lists in
    numpy (the rows of this workload are full or empty: k is c or 0)."""
    recv, _ = eng.peer_load([0])
    n = recv.size
    rp = rp.astype(np.int64)
    in_f = recv > 0
    in_f[root] = True
    member = np.zeros(n, dtype=bool)  # named by a child entry of a member: the node space
    level = np.full(n, -1, dtype=np.int64)
    level[root] = 0
    copies = np.zeros(n, dtype=np.int64)
    cur, h = np.array([root], dtype=np.int64), 0
    while cur.size:
        h += 1
        lo, ln = rp[cur], rp[cur + 1] - rp[cur]
        idx = np.repeat(lo - np.concatenate([[0], np.cumsum(ln)[:-1]]), ln) + np.arange(int(ln.sum()))
        tgt = cl[idx].astype(np.int64)
        tgt = tgt[in_f[tgt]]
        copies += np.bincount(tgt, minlength=n) * c
        new = np.unique(tgt[level[tgt] < 0])
        level[new] = h
        cur = new
    # the node space: everything the root reaches over all child lists
    member[root] = True
    cur = np.array([root], dtype=np.int64)
    while cur.size:
        lo, ln = rp[cur], rp[cur + 1] - rp[cur]
        idx = np.repeat(lo - np.concatenate([[0], np.cumsum(ln)[:-1]]), ln) + np.arange(int(ln.sum()))
        new = np.unique(cl[idx].astype(np.int64))
        new = new[~member[new]]
        member[new] = True
        cur = new
    vis = level > 0
    cols = np.minimum(level[vis], PE.MAX_ROUNDS - 1)
    reached = np.bincount(cols, minlength=PE.MAX_ROUNDS).astype(np.uint64)
    out = {"reached": reached[None, :], "deliv": (reached * np.uint64(c))[None, :],
           "unreached": np.array([int(member.sum()) - 1 - int((recv > 0).sum())], dtype=np.uint64),
           "stranded": np.array([int(((recv > 0) & (level < 0)).sum())], dtype=np.uint64),
           "copies": copies.astype(np.uint64), "dup": (copies - recv.astype(np.int64)).astype(np.uint64)}
    return out


def spread_main(a):
    """--spread (see above).  Writes DIR/spread_bench.json."""
    c = 1024
    res = {"n_peers": a.spread_peers, "n_msgs": c, "reps": a.reps, "hub": a.spread_hub, "shapes": {}}

    def engine(env, g):
        for k in ("PSAMD_AB", "PSAMD_DRAIN_TIMING", "PSAMD_SPREAD_WIDE"):
            os.environ.pop(k, None)
        os.environ.update(env)
        eng = PE.Engine(a.spread_peers, 1)
        eng.set_children(0, g[2], g[0], g[1])
        eng.set_live(g[3])
        eng.publish(np.zeros(c))
        return eng, eng.run()

    for shape, hub in (("random", 0), ("hub", a.spread_hub)):
        g = spread_graph(a.spread_peers, hub, a.seed)
        row = {"edges": int(g[1].size), "wide": {}}
        for wide in (16, 0, 64, 1 << 20):
            env = {"PSAMD_DRAIN_TIMING": "1"}
            if wide != 16:
                env.update(PSAMD_AB="1", PSAMD_SPREAD_WIDE=str(wide))
            eng, st = engine(env, g)
            with eng:
                rows = []
                for _ in range(a.reps + 1):  # (the first call builds the window's tables and allocates)
                    with StderrCapture() as cap:
                        got = eng.topic_spread([0])
                    r = phase_line(cap.text, "topic_spread")
                    for k in ("strips", "nodes", "row_bytes", "level_launches"):
                        r[k] = int(re.search(rf"\b{k} (\d+)", cap.text).group(1))
                    rows.append(r)
                row["wide"][str(wide)] = rows[1:]
                if wide == 16:
                    lrows = []
                    for _ in range(a.reps + 1):
                        with StderrCapture() as cap:
                            eng.peer_load([0])
                        lrows.append(phase_line(cap.text, "peer_load"))
                    row["load_phases"] = lrows[1:]
                    assert int(got["deliv"].sum()) == st.deliveries and int(got["dup"].astype(np.int64).sum()) == st.duplicates
                    row.update(deliveries=int(st.deliveries), duplicates=int(st.duplicates), rounds=int(st.rounds),
                               run_ms=float(st.run_ms), reached=int(got["reached"].sum()), unreached=int(got["unreached"][0]),
                               stranded=int(got["stranded"][0]), depth=int(np.nonzero(got["reached"][0])[0].max()),
                               dup_peers=int((got["dup"] > 0).sum()), dup_max=int(got["dup"].max()))
        eng, _ = engine({}, g)
        with eng:
            walls = {"spread": [], "load": [], "host": []}
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                got = eng.topic_spread([0])
                walls["spread"].append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                eng.peer_load([0])
                walls["load"].append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                want = host_topic_spread(eng, g[0], g[1], g[2], c)
                walls["host"].append(1e3 * (time.perf_counter() - t0))
                for k in want:
                    assert np.array_equal(got[k], want[k]), f"ps_topic_spread {k} differs from the host derivation"
        row["spread_wall_ms"], row["load_wall_ms"], row["host_derivation_wall_ms"] = (walls[k][1:] for k in ("spread", "load", "host"))
        row["answers_agree"] = True
        row["host_over_spread_wall"] = float(np.median(row["host_derivation_wall_ms"]) / np.median(row["spread_wall_ms"]))
        row["spread_over_load_wall"] = float(np.median(row["spread_wall_ms"]) / np.median(row["load_wall_ms"]))
        res["shapes"][shape] = row
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "spread_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


SPREAD_NAMES = ("reached", "deliv", "unreached", "stranded", "copies", "dup")


def spread_track_main(a):
    """--spread-track (see the module text).  Writes DIR/spread_track_bench.json."""
    c = 1024
    k = max(1, min(a.take_every, a.steps))
    steps = a.steps // k * k
    res = {"n_peers": a.spread_peers, "n_msgs": c, "reps": a.reps, "hub": a.spread_hub, "steps": steps, "warmup": a.warmup,
           "take_every": k, "shapes": {}}
    batch = np.zeros(c)

    def engine(env, g):
        for key in ("PSAMD_AB", "PSAMD_DRAIN_TIMING", "PSAMD_SPREAD_WIDE", "PSAMD_SPREAD_TRACK_LEVELS"):
            os.environ.pop(key, None)
        os.environ.update(env)
        eng = PE.Engine(a.spread_peers, 1)
        for key in env:
            os.environ.pop(key, None)
        eng.set_children(0, g[2], g[0], g[1])
        eng.set_live(g[3])
        eng.publish(batch)
        return eng, eng.run()

    def pipelined(eng, n):
        eng.publish(batch)
        for i in range(n):
            eng.run_async()
            if i + 1 < n:
                eng.publish(batch)
            if i:
                eng.wait()
        eng.wait()

    def summed(parts):
        tot = {name: np.zeros_like(parts[0][name]) for name in SPREAD_NAMES}
        with np.errstate(over="ignore"):
            for p in parts:
                for name in SPREAD_NAMES:
                    tot[name] += p[name]
        return tot

    def agree(take, parts, what):
        want = summed(parts)
        assert take["n_windows"] == len(parts) and take["n_truncated"] == 0, (what, take["n_windows"], take["n_truncated"])
        for name in SPREAD_NAMES:
            assert np.array_equal(take[name], want[name]), f"{what}: tracked {name} differs from the sum of ps_topic_spread"

    for shape, hub in (("random", 0), ("hub", a.spread_hub)):
        g = spread_graph(a.spread_peers, hub, a.seed)
        row = {"edges": int(g[1].size)}
        # the device phases: one tracked window, its take and one blocking call, alternating
        eng, st = engine({"PSAMD_DRAIN_TIMING": "1"}, g)
        with eng:
            assert st.windows == 1
            blocking = eng.topic_spread([0])
            rows = {"spread_track": [], "spread_take": [], "topic_spread": []}
            eng.spread_track([0])
            for _ in range(a.reps + 1):  # (the first pass allocates and uploads the strips)
                eng.publish(batch)
                with StderrCapture() as cap:
                    eng.run()
                r = phase_line(cap.text, "spread_track")
                for key in ("strips", "nodes", "row_bytes", "rounds", "level_launches", "staged_bytes", "kept"):
                    r[key] = int(re.search(rf"psamd spread_track: .*\b{key} (\d+)", cap.text).group(1))
                rows["spread_track"].append(r)
                with StderrCapture() as cap:
                    t = eng.spread_take()
                agree(t, [blocking], shape + " timed")
                r = phase_line(cap.text, "spread_take")
                r["copied_bytes"] = int(re.search(r"copied_bytes (\d+)", cap.text).group(1))
                rows["spread_take"].append(r)
                with StderrCapture() as cap:
                    got = eng.topic_spread([0])
                r = phase_line(cap.text, "topic_spread")
                r["level_launches"] = int(re.search(r"psamd topic_spread: .*\blevel_launches (\d+)", cap.text).group(1))
                rows["topic_spread"].append(r)
                for name in SPREAD_NAMES:
                    assert np.array_equal(got[name], blocking[name]), name
            eng.spread_track([])
        dev = lambda rs, skip=(): float(np.median([sum(v for q, v in r.items() if q.endswith("_ms") and q not in skip) for r in rs]))
        row.update(deliveries=int(st.deliveries), duplicates=int(st.duplicates), rounds=int(st.rounds),
                   depth=int(np.nonzero(blocking["reached"][0])[0].max()), tracked_phases=rows["spread_track"][1:],
                   take_phases=rows["spread_take"][1:], blocking_phases=rows["topic_spread"][1:])
        row["tracked_window_device_ms"] = dev(row["tracked_phases"], ("host_ms",))
        row["blocking_call_device_ms"] = dev(row["blocking_phases"], ("host_strips_ms", "copy_ms"))
        row["blocking_call_copy_ms"] = float(np.median([r["copy_ms"] for r in row["blocking_phases"]]))
        row["tracked_level_launches"] = row["tracked_phases"][-1]["level_launches"]
        row["blocking_level_launches"] = row["blocking_phases"][-1]["level_launches"]

        # the walls: (a) the untracked pipelined step, (b) ps_run + ps_topic_spread every step, (c) tracked, a take every k steps
        eng, _ = engine({}, g)

        def plain(n):
            t0 = time.perf_counter()
            for _ in range(n // k):
                pipelined(eng, k)
            return 1e3 * (time.perf_counter() - t0) / n

        def blocking_loop(n):
            parts = []
            t0 = time.perf_counter()
            for _ in range(n):
                eng.publish(batch)
                eng.run()
                parts.append(eng.topic_spread([0]))
            ms = 1e3 * (time.perf_counter() - t0) / n
            blocking_loop.parts = parts
            return ms

        def tracked(n):
            eng.spread_track([0])
            takes = []
            t0 = time.perf_counter()
            for _ in range(n // k):
                pipelined(eng, k)
                takes.append(eng.spread_take())
            ms = 1e3 * (time.perf_counter() - t0) / n
            for i, t in enumerate(takes):  # (outside the timed part; (b) ran the same steps just before)
                agree(t, blocking_loop.parts[i * k:(i + 1) * k], shape)
            eng.spread_track([])
            return ms

        modes = {"plain": plain, "run_plus_topic_spread": blocking_loop, "tracked": tracked}
        with eng:
            for f in modes.values():
                f(max(a.warmup // k, 1) * k)
            ms = {name: [] for name in modes}
            for _ in range(a.reps):
                for name, f in modes.items():
                    ms[name].append(f(steps))
        med = {name: float(np.median(v)) for name, v in ms.items()}
        row.update(ms_per_step=ms, median_ms_per_step=med, takes_agree=True, tracked_minus_plain_ms=med["tracked"] - med["plain"],
                   blocking_loop_over_tracked=med["run_plus_topic_spread"] / med["tracked"])
        res["shapes"][shape] = row
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "spread_track_bench.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="cfg3", choices=sorted(WL.CONFIGS))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--loop-queries", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pipelined", action="store_true", help="the drain inside the pipelined step loop (see above)")
    ap.add_argument("--pipelined-queries", default="256,1024,4096")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shared", action="store_true", help="ps_drain_shared against ps_drain (see above)")
    ap.add_argument("--large-queries", type=int, default=262144)
    ap.add_argument("--sink", action="store_true", help="the sink in the pipelined loop against ps_drain_shared_begin's")
    ap.add_argument("--topics", action="store_true", help="ps_drain_topics against ps_drain_shared and k_digest (see above)")
    ap.add_argument("--load", action="store_true", help="ps_peer_load against the host derivation; tracking in the pipelined loop")
    ap.add_argument("--hops", action="store_true", help="ps_topic_hops against the host derivation; tracking in the pipelined loop")
    ap.add_argument("--downstream", action="store_true",
                    help="ps_peer_downstream against the host derivation; tracking in the pipelined loop")
    ap.add_argument("--cut", action="store_true",
                    help="ps_peer_cut against ps_peer_downstream and the host derivation; tracking in the pipelined loop")
    ap.add_argument("--blame", action="store_true", help="ps_topic_blame against ps_peer_cut and the host derivation")
    ap.add_argument("--blame-track", action="store_true",
                    help="ps_blame_track in the pipelined loop against ps_run + ps_topic_blame every step")
    ap.add_argument("--take-every", type=int, default=10, help="--blame-track, --spread-track: steps between two takes")
    ap.add_argument("--report", action="store_true",
                    help="ps_peer_report against the four calls in sequence; report tracking against the four trackers")
    ap.add_argument("--report-once", action="store_true", help="one step and one ps_peer_report (for a kernel trace)")
    ap.add_argument("--dist-report", action="store_true",
                    help="ps_dist_report against ps_peer_report on one rank; the collective call on 2 and 4 loopback ranks")
    ap.add_argument("--dist-cut", action="store_true",
                    help="ps_dist_cut against ps_peer_cut on one rank; against ps_dist_report's downstream on 2 and 4 loopback ranks")
    ap.add_argument("--dist-blame", action="store_true",
                    help="ps_dist_blame against ps_topic_blame on one rank; against ps_dist_cut on 2 and 4 loopback ranks")
    ap.add_argument("--spread", action="store_true", help="ps_topic_spread on a mesh of its own against ps_peer_load and the host derivation")
    ap.add_argument("--spread-track", action="store_true",
                    help="ps_spread_track in the pipelined loop against ps_run + ps_topic_spread every step, on --spread's meshes")
    ap.add_argument("--spread-peers", type=int, default=1 << 20)
    ap.add_argument("--spread-hub", type=int, default=4096)
    a = ap.parse_args()
    if a.spread_track:
        return spread_track_main(a)
    if a.spread:
        return spread_main(a)
    wl = WL.scaled(a.workload, a.scale) if a.scale != 1.0 else WL.CONFIGS[a.workload]()
    if a.dist_report:
        return dist_report_main(a, wl)
    if a.dist_cut:
        return dist_cut_main(a, wl)
    if a.dist_blame:
        return dist_blame_main(a, wl)
    if a.report or a.report_once:
        return report_main(a, wl)
    if a.blame_track:
        return blame_track_main(a, wl)
    if a.blame:
        return blame_main(a, wl)
    if a.cut:
        return cut_main(a, wl)
    if a.downstream:
        return downstream_main(a, wl)
    if a.hops:
        return hops_main(a, wl)
    if a.load:
        return load_main(a, wl)
    if a.topics and a.sink:
        return sink_topics_main(a, wl)
    if a.pipelined and a.topics:
        return pipelined_topics_main(a, wl)
    if a.topics:
        return topics_main(a, wl)
    if a.sink:
        return sink_main(a, wl)
    if a.pipelined and a.shared:
        return pipelined_shared_main(a, wl)
    if a.pipelined:
        return pipelined_main(a, wl)
    if a.shared:
        return shared_main(a, wl)
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
