"""Device time of one shard's planned gossip round at G shards of the cfg 5 schedule (the method of
profiles/r05/shard_round.py: HIP events around each shard's gx_round_gossip_begin and
gx_round_gossip_end, LocalShards on one GPU), for several builds of the engine in ONE process,
alternating (as profiles/r04/ab_kernels.py does), with probe_piggyback off or on. Each repetition
makes fresh engines, runs `--start` rounds untimed and times `--rounds` gossip rounds.

With --fill it also counts, per round, the slots the plan reserved and the slots that carry a packet
(the rest are padding: sender key GX_SLOT_EMPTY).

    python profiles/probe_shards/shard_probe_ab.py --libs parent.so sidecar_amd/libgx.so --reps 4
    python profiles/probe_shards/shard_probe_ab.py --libs sidecar_amd/libgx.so --probe 1 --fill --reps 2

One JSON line per (rep, lib), then a summary line: per lib the median per-shard round time of each
repetition, their median and spread (max - min).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def one_run(lib, a, kw, torch):
    from sidecar_amd.dist import LocalShards, _ptr
    stream = torch.cuda.current_stream()
    sh = LocalShards(lib, a.G, device="cuda:0", **kw)
    sh.run_rounds(a.start)
    torch.cuda.synchronize()
    G = a.G
    bufs = sh._planned_bufs()
    slot = 16 + 16 * sh.shards[0].e.params.packet_cap
    begin_us, end_us, planned, filled = [], [], [], []
    for _ in range(a.rounds):
        plan = np.zeros(G * G, dtype=np.uint64)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(2 * G)]
        for g, (s, b) in enumerate(zip(sh.shards, bufs)):
            ev[g][0].record(stream)
            s.e.round_gossip_begin(plan, _ptr(b), b.numel())
            ev[g][1].record(stream)
        m = plan.reshape(G, G)
        planned.append(int(m.sum()) // slot)
        if a.fill:
            n = 0
            for src in range(G):
                hdr = bufs[src][:int(m[src].sum())].view(-1, slot)[:, :4]
                n += int((hdr != 255).any(1).sum())
            filled.append(n)
        ae = False
        for dst, s in enumerate(sh.shards):
            x = torch.cat([bufs[src][int(m[src][:dst].sum()):int(m[src][:dst + 1].sum())] for src in range(G)])
            ev[G + dst][0].record(stream)
            ae = s.e.round_gossip_end(_ptr(x), x.numel())
            ev[G + dst][1].record(stream)
        if ae:
            raise SystemExit("a push-pull round in the stretch: pick gossip-only rounds")
        torch.cuda.synchronize()
        begin_us.append([1e3 * p.elapsed_time(q) for p, q in ev[:G]])
        end_us.append([1e3 * p.elapsed_time(q) for p, q in ev[G:]])
    B, E = np.array(begin_us), np.array(end_us)
    out = {"per_shard_begin_us": [round(float(x), 1) for x in B.mean(axis=1)],
           "per_shard_end_us": [round(float(x), 1) for x in E.mean(axis=1)],
           "per_shard_us": [round(float(x), 1) for x in (B + E).mean(axis=1)],
           "slots_planned": planned, "paths": dict(sh.exchange_paths)}
    if a.fill:
        out["slots_filled"] = filled
    if a.probe:
        out["probe_cross"] = list(sh.probe_cross())
    st = sh.stats()
    out["check"] = {k: st[k] for k in ("round", "packets", "gossip_merges", "lost_packets")}
    for s in sh.shards:
        s.e.close()
    del sh
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--config", default="cfg5")
    ap.add_argument("--start", type=int, default=51)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--probe", type=int, default=0)
    ap.add_argument("--fill", action="store_true")
    ap.add_argument("--libs", nargs="+", required=True)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import bench
    from sidecar_amd.abi import load_library
    libs = [(p, load_library(p)) for p in a.libs]
    kw = dict(bench.CONFIGS[a.config]["p"], seed=0x5EED, lock_model=1, probe_piggyback=a.probe)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    med = {p: [] for p, _ in libs}
    for rep in range(a.reps):
        for p, lib in libs:
            r = one_run(lib, a, kw, torch)
            med[p].append(statistics.median(r["per_shard_us"]))
            emit(dict(rep=rep, lib=p, config=a.config, G=a.G, probe=a.probe, rounds=[a.start, a.start + a.rounds - 1],
                      **r))
    emit({"summary": {p: {"rep_medians_us": v, "median_us": round(statistics.median(v), 2),
                          "spread_us": round(max(v) - min(v), 2)} for p, v in med.items()}})


if __name__ == "__main__":
    main()
