"""Per-phase host time of a sharded round (LocalShards on one GPU, cfg 5 schedule at H = 16384):
where the per-round cost of the exchange layer goes, call by call. The rounds are the driver's own
(sidecar_amd.dist.ShardRounds.run_rounds); Engine's sharded-round calls are wrapped on the class to
wait for their device work and take the time. Gossip rounds (no push-pull, no storm), then one
push-pull round.

  python profiles/shard_phase_times.py [G] [H]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import sidecar_amd.dist as dist_mod  # noqa: E402
from sidecar_amd.abi import load_product  # noqa: E402

GOSSIP = ("round_send", "outbox_sizes_async", "outbox_pack", "inbox_unpack", "round_merge", "round_gossip_begin",
          "round_gossip_end", "round_end")
PUSH_PULL = ("lock_census", "ae_skip_locked", "ae_bytes", "ae_pack", "ae_merge_local", "ae_delta_bytes",
             "ae_delta_pack", "ae_return_bytes", "ae_return_pack", "ae_merge")

G = int(sys.argv[1]) if len(sys.argv) > 1 else 8
kw = dict(bench.CONFIGS["cfg5"]["p"])
kw["n_hosts"] = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
sh = dist_mod.LocalShards(load_product(), G, device="cuda:0", **kw)
sh.run_rounds(11)  # past the first push-pull round and the storm


def timed_rounds(n):
    """n rounds of the driver with every sharded-round call timed; ({call: [seconds]}, wall seconds)."""
    T = {}
    orig = {name: getattr(dist_mod.Engine, name) for name in GOSSIP + PUSH_PULL}
    for name, f in orig.items():
        def wrap(self, *a, _f=f, _n=name):
            t0 = time.perf_counter()
            r = _f(self, *a)
            torch.cuda.synchronize()
            T.setdefault(_n, []).append(time.perf_counter() - t0)
            return r
        setattr(dist_mod.Engine, name, wrap)
    try:
        a = time.perf_counter()
        sh.run_rounds(n)
        torch.cuda.synchronize()
        return T, time.perf_counter() - a
    finally:
        for name, f in orig.items():
            setattr(dist_mod.Engine, name, f)


T = {}
rounds = 0
while rounds < 8:
    if sh.shards[0].e.is_ae_round():
        sh.run_rounds(1)
        continue
    for k, v in timed_rounds(1)[0].items():
        T.setdefault(k, []).extend(v)
    rounds += 1
# per shard round: a call made once per shard and round counts its mean
out = {k: round(1e6 * float(np.sum(v)) / (G * rounds), 1) for k, v in T.items()}
# a push-pull round: whole-round wall time through the driver, then its phases
while not sh.shards[0].e.is_ae_round():
    sh.run_rounds(1)
TA, ae_wall = timed_rounds(1)
ae = {k: round(1e3 * float(np.sum(v)) / G, 3) for k, v in TA.items() if k in PUSH_PULL}
print(json.dumps({"G": G, "H": kw["n_hosts"], "us_per_call": out,
                  "us_per_shard_round": round(sum(out.values()), 1),
                  "push_pull_round": {"round": sh.shards[0].e.round - 1, "wall_ms_all_shards": round(1e3 * ae_wall, 2),
                                      "ms_per_shard_by_call": ae}}), flush=True)
