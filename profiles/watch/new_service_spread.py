"""How long one new version takes to reach every view, round by round, at the BASELINE sizes: the
figure Sidecar's "a few seconds" claim describes, measured with the record watch
(include/gx_watch.h) instead of streaming every view (gx_view_minmax).

HIP engine only. A warm cluster (every view holds every record) with a small churn, and a fixed,
seeded sample of record keys, one watch entry each. After every round the owners' words
(gx_owner_words, into a device tensor) show which sampled keys' owners stamped a new version in
that round; those entries are set to that version (watch_set) and count from the next round end. A
version's latency is the rounds from the round it was stamped in to the first round at whose end
every live view holds it (sidecar_amd.spread.spread_rounds; the watch first counts it one round
after its birth, so the least latency seen is 1). A version its owner replaced before it got
everywhere is `superseded`, one still on its way at the end `unfinished`. One JSON line per size
and lock model, with the run's queue_drops beside it (0: every round was the reference's queue).

    python profiles/watch/new_service_spread.py [--sizes cfg2,cfg3,cfg4,cfg5] [--rounds 600] [--sample 1024]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from sidecar_amd.abi import TS_SHIFT, WATCH_MAX, Engine, default_params, load_product  # noqa: E402
from sidecar_amd.spread import spread_rounds  # noqa: E402

# BASELINE.json configs[1..4]: hosts x services (fanout 3, 32 records per message, push-pull every 10 rounds)
SIZES = {"cfg2": (4096, 16), "cfg3": (16384, 16), "cfg4": (8192, 64), "cfg5": (32768, 16)}
ROUND_S = 0.2


def params(lib, size, lock_model, churn_ppm, seed):
    H, S = SIZES[size]
    return default_params(lib, n_hosts=H, n_services=S, fanout=3, packet_cap=32, pending_cap=100, queue_cap=16384,
                          list_slots=32, init_mode=2, ae_period_rounds=10, churn_ppm=churn_ppm, lock_model=lock_model,
                          seed=seed)


def run(lib, size, lock_model, a):
    e = Engine(params(lib, size, lock_model, a.churn_ppm, a.seed), lib=lib)
    try:
        R = e.H * e.S
        dev = torch.device("cuda:0")
        n = min(a.sample, WATCH_MAX, R)
        keys = np.sort(np.random.default_rng(a.seed).choice(R, size=n, replace=False)).astype(np.uint32)
        kdev = torch.from_numpy(keys.astype(np.int64)).to(dev)
        own = torch.empty(R, dtype=torch.int64, device=dev)
        e.run_rounds(a.warmup)
        e.owner_words(own.data_ptr())
        prev = own[kdev].clone()
        e.watch_arm(n, a.rounds)
        st0 = e.stats()
        segs = []  # (entry, born round, first counted round) of every version watched, in order per entry
        t0 = time.time()
        for _ in range(a.rounds):
            r = e.round
            e.run_rounds(1)
            e.owner_words(own.data_ptr())
            cur = own[kdev]
            # stamped by the owner itself in round r: its word changed and carries that round's time or later
            now_r = e.params.t0_ns - e.epoch + r * e.params.round_ns
            new = ((cur != prev) & (slot_ts(cur) >= now_r) & ((cur & 7) != 7)).nonzero().flatten().cpu().numpy()
            prev = cur
            if len(new):
                ts = slot_ts(cur).cpu().numpy()[new] + e.epoch
                for lo, hi in runs(new):  # consecutive entries in one call
                    e.watch_set(int(new[lo]), keys[new[lo:hi]], ts[lo:hi])
                segs += [(int(i), r, r + 1) for i in new]
        wall = time.time() - t0
        counts, live, first_round, n_logged, missed = e.watch_read()
        st1 = e.stats()
        lat, superseded, unfinished = latencies(segs, counts, live, first_round, n_logged)
        out = {"size": size, "hosts": e.H, "services": e.S, "lock_model": lock_model, "churn_ppm": a.churn_ppm,
               "watched_keys": n, "rounds": [first_round, first_round + n_logged - 1], "versions_born": len(segs),
               "versions_spread": len(lat), "superseded": superseded, "unfinished": unfinished,
               "queue_drops": st1["queue_drops"] - st0["queue_drops"], "missed_rounds": missed,
               "wall_s_per_round": round(wall / a.rounds, 6), "round_s": ROUND_S}
        if lat:
            q = np.percentile(np.array(lat, dtype=np.float64), [50, 99])
            out.update({"p50_rounds": float(q[0]), "p99_rounds": float(q[1]), "max_rounds": int(max(lat)),
                        "p50_s": round(float(q[0]) * ROUND_S, 2), "p99_s": round(float(q[1]) * ROUND_S, 2),
                        "max_s": round(max(lat) * ROUND_S, 2)})
        return out
    finally:
        e.close()


def slot_ts(w):
    """Slot time of packed words held in int64 (a logical shift)."""
    return (w >> TS_SHIFT) & ((1 << 61) - 1)


def runs(idx):
    """[lo, hi) ranges of consecutive values in a sorted index array."""
    cut = np.flatnonzero(np.diff(idx) != 1) + 1
    b = np.concatenate([[0], cut, [len(idx)]])
    return list(zip(b[:-1], b[1:]))


def latencies(segs, counts, live, first_round, n_logged):
    """Each watched version's rounds to every live view, from the rows that counted it: from the
    round after its birth to the round before the entry's next version was set."""
    nxt = {}
    lat, superseded, unfinished = [], 0, 0
    for i, born, start in reversed(segs):
        replaced = i in nxt
        end = nxt[i] if replaced else first_round + n_logged  # first round counted with the entry's next version
        nxt[i] = start
        a, b = start - first_round, end - first_round
        full, _ = spread_rounds(counts[a:b, i:i + 1], live[a:b], start, born)
        if full[0] is not None:
            lat.append(full[0])
        elif replaced:
            superseded += 1
        else:
            unfinished += 1
    return lat, superseded, unfinished


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="cfg2,cfg3,cfg4,cfg5")
    ap.add_argument("--rounds", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sample", type=int, default=1024)
    ap.add_argument("--churn-ppm", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    lib = load_product()
    for size in a.sizes.split(","):
        for lock_model in (0, 1):
            line = json.dumps(run(lib, size, lock_model, a))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
