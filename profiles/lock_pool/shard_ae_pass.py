"""Stream time of a sharded push-pull pass with and without lock_readers (gx.h), G LocalShards on one
GPU: H hosts x S services on the lock_readers test schedule (tests/lock_pool_cases.py BASE) scaled up.
HIP events on the engines' stream bracket each round's push-pull steps (ShardRounds._push_pull: the
chain's kernels of all G shards one after another, the in-process exchanges, and the stream's idle
time while the host reads sizes back) and, inside them, the slot arbitration (_claim_slots: G
k_ae_want launches, the fold, G k_ae_claim_set launches and the local k_ae_rox). Per round: the pass,
the arbitration, and the read-locked exchanges the round carried (oracle-free: the shards' counters).

    python profiles/lock_pool/shard_ae_pass.py [--G 8] [--hosts 4096] [--services 16] [--rounds 40]
    python profiles/lock_pool/shard_ae_pass.py --libs parent.so sidecar_amd/libgx.so --reps 4
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def run(lib, G, kw, rounds, lock_readers):
    import torch
    from sidecar_amd.dist import LocalShards
    sh = LocalShards(lib, G, device="cuda:0", lock_readers=lock_readers, **kw)
    stream = torch.cuda.current_stream()
    rows, claim_ev = [], []
    push_pull, claim = sh._push_pull, sh._claim_slots

    def timed_claim():
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record(stream)
        claim()
        ev[1].record(stream)
        claim_ev.append(ev)

    def timed_push_pull():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        before = (sh.ro_counts(), sh.stats()) if lock_readers else None
        del claim_ev[:]
        t0.record(stream)
        push_pull()
        t1.record(stream)
        torch.cuda.synchronize()
        row = {"round": sh.engines[0].round - 1, "pass_us": round(1e3 * t0.elapsed_time(t1), 1)}
        if lock_readers:
            ro, st = sh.ro_counts(), sh.stats()
            row["claim_us"] = [round(1e3 * a.elapsed_time(b), 1) for a, b in claim_ev]
            row["cross_ro_exchanges"] = ro["cross_exchanges"] - before[0]["cross_exchanges"]
            row["deferred"] = st["ae_deferred"] - before[1]["ae_deferred"]
            row["lost"] = st["ae_defer_lost"] - before[1]["ae_defer_lost"]
        rows.append(row)

    sh._push_pull, sh._claim_slots = timed_push_pull, timed_claim
    sh.run_rounds(rounds)
    st = sh.stats()
    for e in sh.engines:
        e.close()
    return {"lock_readers": lock_readers, "skipped": sh.ae_skipped, "rounds": rows,
            "stats": {k: st[k] for k in ("ae_exchanges", "ae_locked", "ae_deferred", "ae_defer_lost")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--hosts", type=int, default=4096)
    ap.add_argument("--services", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--libs", nargs="+", default=None, help="builds of the engine to alternate (A/B), with --reps")
    ap.add_argument("--reps", type=int, default=4)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from sidecar_amd.abi import INIT_OWN, load_library, load_product
    kw = dict(n_hosts=a.hosts, n_services=a.services, fanout=1, packet_cap=1, init_mode=INIT_OWN, churn_ppm=100000,
              alive_interval_rounds=2, tombstone_interval_rounds=7, ae_period_rounds=1, queue_cap=4096, storm_round=5)
    if not a.libs:
        lib = load_product()
        out = {"G": a.G, "hosts": a.hosts, "services": a.services,
               "runs": [run(lib, a.G, kw, a.rounds, lr) for lr in (0, 1)]}
        print(json.dumps(out), flush=True)
        return
    # A/B: the builds in one process, alternating; per (rep, build, lock_readers) the median pass over
    # the rounds that ran the chain, then per build the median and spread (max - min) of those medians
    libs = [(p, load_library(p)) for p in a.libs]
    med = {p: {0: [], 1: []} for p, _ in libs}
    for rep in range(a.reps):
        for p, lib in libs:
            for lr in (0, 1):
                r = run(lib, a.G, kw, a.rounds, lr)
                m = statistics.median(x["pass_us"] for x in r["rounds"])
                med[p][lr].append(m)
                print(json.dumps({"rep": rep, "lib": p, "G": a.G, "hosts": a.hosts, "services": a.services,
                                  "lock_readers": lr, "median_pass_us": m, "skipped": r["skipped"],
                                  "stats": r["stats"]}), flush=True)
    print(json.dumps({"summary": {p: {f"lock_readers_{lr}": {"rep_medians_us": v, "median_us": statistics.median(v),
                                                             "spread_us": round(max(v) - min(v), 1)}
                                      for lr, v in by.items()} for p, by in med.items()}}), flush=True)


if __name__ == "__main__":
    main()
