"""bench.py --dump-outputs: what a caller of the timed path holds after its
last step, one .npy per array (float32 / float64), so that two builds of the
library can be compared output for output on the same (seeded) inputs.

  counters              ps_stats of the last step: deliveries, duplicates,
                        rounds, windows (the counters; no timings)
  deliveries_per_round  ps_stats.deliveries_per_round, PS_MAX_ROUNDS entries
  frontier_per_round    ps_stats.frontier_per_round, PS_MAX_ROUNDS entries
  seen_digest           ps_seen_digest of the final seen state, as four 16-bit
                        limbs (least significant first; exact in float64)
  sample_messages       the sampled messages' indices within the last batch
  sample_peers          the sampled peers
  delivered_sample      [message, peer] 1.0 where the message was delivered
                        (ps_read_delivered), float32
  delivered_counts      peers each sampled message reached (all peers)

The sample is fixed: SAMPLE_MSGS messages of the last batch drawn with a seeded
generator, every peer up to SAMPLE_PEERS of them (a seeded draw above that), so
the files stay under 64 MB whatever the workload; the ranks of a multi-process
run write their own nodes' share each (names ending in _rank<r>) and split
SAMPLE_PEERS among them.
"""
from __future__ import annotations

import os

import numpy as np

from . import MAX_ROUNDS, EngineError

SAMPLE_MSGS = 8
SAMPLE_PEERS = 1_500_000  # 8 x 1.5M float32 = 48 MB
SAMPLE_SEED = 0xD0_0D


def _per_round(per) -> np.ndarray:
    out = np.zeros(MAX_ROUNDS, dtype=np.float64)
    out[:len(per)] = per
    return out


def sample(n_msgs: int, n_peers: int, ranks: int = 1):
    """(message indices within the batch, peers or None for every peer): the
    same draw on every run and on each of `ranks` ranks."""
    rng = np.random.default_rng(SAMPLE_SEED)
    msgs = np.sort(rng.choice(n_msgs, min(SAMPLE_MSGS, n_msgs), replace=False))
    peers = None
    cap = SAMPLE_PEERS // max(1, ranks)
    if n_peers > cap:
        peers = np.sort(rng.choice(n_peers, cap, replace=False))
    return msgs, peers


def dump_outputs(dirname: str, eng, st, first: int, n_msgs: int, suffix: str = "", extra: dict | None = None,
                 ranks: int = 1):
    """Writes the arrays above into `dirname` for the engine's last run: `st`
    its ps_stats, `first` the id of its first message, `n_msgs` its batch
    size.  `suffix` goes behind every name (a rank of a multi-process run of
    `ranks` ranks); `extra` adds float arrays of the caller's own."""
    os.makedirs(dirname, exist_ok=True)
    d = st.as_dict()
    digest = eng.seen_digest()
    msgs, peers = sample(n_msgs, eng.n_peers, ranks)
    width = eng.n_peers if peers is None else peers.shape[0]
    deliv = np.zeros((msgs.shape[0], width), dtype=np.float32)
    counts = np.zeros(msgs.shape[0], dtype=np.float64)
    for k, m in enumerate(msgs):
        try:
            got = eng.delivered(first + int(m))
        except EngineError as exc:
            if exc.code != -8:  # PS_E_NOTREADY: the message ran in an earlier window of the batch
                raise
            deliv[k] = -1.0
            counts[k] = -1.0
            continue
        counts[k] = float(got.sum(dtype=np.int64))
        deliv[k] = got if peers is None else got[peers]
    arrays = {
        "counters": np.array([st.deliveries, st.duplicates, st.rounds, st.windows], dtype=np.float64),
        "deliveries_per_round": _per_round(d["deliveries_per_round"]),
        "frontier_per_round": _per_round(d["frontier_per_round"]),
        "seen_digest": np.array([(digest >> (16 * i)) & 0xFFFF for i in range(4)], dtype=np.float64),
        "sample_messages": msgs.astype(np.float64),
        "sample_peers": (np.arange(eng.n_peers) if peers is None else peers).astype(np.float64),
        "delivered_sample": deliv,
        "delivered_counts": counts,
    }
    for k, v in (extra or {}).items():
        arrays[k] = np.asarray(v, dtype=np.float64)
    for k, v in arrays.items():
        np.save(os.path.join(dirname, f"{k}{suffix}.npy"), v)
