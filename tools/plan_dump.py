#!/usr/bin/env python3
"""Text dump of the planner probe's plans for the workload configurations,
to compare two builds of the library byte for byte (no GPU needed):

    python tools/plan_dump.py a.txt
    PSAMD_AB=1 PSENGINE_LIB_AB=<other libpsengine.so> python tools/plan_dump.py b.txt
    cmp a.txt b.txt

Per configuration (cfg2 full size, cfg3 / cfg4 / cfg5 at scale 0.1; trees from
the oracle's join protocol) and per option set: info(), schedule(), the round
kinds and every round's pull chunks, pair chunks and chain.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

import oracle as O  # noqa: E402
import psengine as PE  # noqa: E402
from psengine import plan as PL  # noqa: E402
from psengine import workloads as WL  # noqa: E402

CONFIGS = (("cfg2", 1.0), ("cfg3", 0.1), ("cfg4", 0.1), ("cfg5", 0.1))
OPTION_SETS = ({}, {"chain_max": 2}, {"flood": 0}, {"overlap": 0, "align_groups": 0})


def parents_of(wl):
    par = np.full((len(wl.topics), wl.n_peers), O.NONE, dtype=np.uint32)
    for t, ts in enumerate(wl.topics):
        tree = O.Tree(wl.n_peers, ts.root, ts.width, ts.max_width, PE.Engine.topic_seed(wl.seed, t))
        tree.join_all(ts.join_order)
        par[t] = tree.parents()
    return par


def dump(out, p):
    def line(name, v):
        out.write(f"{name} {' '.join(str(int(x)) for x in v)}\n")

    info = p.info()
    line("info", p.get(PL.INFO))
    line("schedule", p.get(PL.SCHEDULE))
    kind = p.get(PL.ROUND_KIND)
    line("round_kind", kind)
    # (the pair table of a round is read only where a pair launch starts, the
    # chain table only where a chain starts: elsewhere their ranges index the
    # other array)
    for q in range(1, info["rounds"] + 1):
        line(f"pull[{q}]", p.get(PL.PULL, q))
        if q < len(kind) and kind[q] == PE.K_PAIR:
            line(f"pair[{q}]", p.get(PL.PAIR, q))
        if q < len(kind) and kind[q] == PE.K_CHAIN:
            line(f"chain[{q}]", p.get(PL.CHAIN, q))


def main():
    with open(sys.argv[1], "w") as out:
        for name, scale in CONFIGS:
            wl = WL.CONFIGS[name]() if scale == 1.0 else WL.scaled(name, scale)
            par = parents_of(wl)
            roots = [ts.root for ts in wl.topics]
            for opts in OPTION_SETS:
                p = PL.Plan(par, roots, plan=opts)
                p.window(wl.msg_topics)
                out.write(f"== {name} x{scale} {sorted(opts.items())}\n")
                dump(out, p)
                p.close()


if __name__ == "__main__":
    main()
