"""GPU: bench.py's command line on one GPU.  A plain run prints the headline
line and runs no other leg; --dump-outputs writes the last timed step's
outputs; --full adds the legs beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import psengine as PE
from psengine import dump as D

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_LEGS = ("roofline", "sustained", "general_path", "cpu_baseline")
SMALL = ["--gpus", "1", "--workload", "cfg3", "--scale", "0.05", "--steps", "4", "--warmup", "1"]


def bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + SMALL + list(extra),
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1  # one JSON line
    return json.loads(lines[0])


def test_plain_run_headline_only_and_dump(tmp_path):
    """The plain line holds the headline figure (value over the timed steps,
    ms_per_step) and none of the --full legs; the dumped arrays are float32 /
    float64, under 64 MB, and say what the line says: every step's deliveries,
    no duplicates on a tree, each sampled message at every subscriber of its
    topic."""
    out = str(tmp_path / "dump")
    line = bench("--dump-outputs", out)
    assert line["steps"] == 4 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "deliveries/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    per_step = line["config"]["deliveries_per_step"]
    assert line["value"] == pytest.approx(per_step / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert not set(FULL_LEGS) & set(line)
    arrays = {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    assert set(arrays) == {"counters", "deliveries_per_round", "frontier_per_round", "seen_digest",
                           "sample_messages", "sample_peers", "delivered_sample", "delivered_counts"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64 << 20
    deliveries, duplicates, rounds, windows = arrays["counters"]
    assert deliveries == per_step and duplicates == 0 and rounds > 0 and windows >= 1
    assert arrays["deliveries_per_round"].shape == (PE.MAX_ROUNDS,)
    assert arrays["deliveries_per_round"].sum() == per_step
    # the sample is the seeded draw, and each sampled message reached exactly
    # its topic's subscribers (the workload is rebuilt here from its seed)
    from psengine import workloads as WL

    wl = WL.scaled("cfg3", 0.05)
    msgs, peers = D.sample(wl.n_msgs, wl.n_peers)
    assert peers is None and np.array_equal(arrays["sample_messages"], msgs)
    assert arrays["delivered_sample"].shape == (msgs.shape[0], wl.n_peers)
    for k, m in enumerate(msgs):
        members = np.zeros(wl.n_peers, dtype=np.float32)
        members[wl.topics[int(wl.msg_topics[m])].join_order] = 1.0
        assert np.array_equal(arrays["delivered_sample"][k], members), int(m)
        assert arrays["delivered_counts"][k] == members.sum()


def test_full_run_adds_the_legs():
    line = bench("--full", "--sustain", "0.2", "--cpu-budget", "0.6")
    assert set(FULL_LEGS) <= set(line)
    assert line["roofline"]["achieved"] > 0 and line["sustained"]["steps"] >= 100
    assert line["general_path"]["compaction"]["value"] > 0
    assert line["cpu_baseline"]["value"] > 0
    assert line["value"] > 0 and line["ms_per_step"] > 0
