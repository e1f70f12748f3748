"""What the record watch costs per round at 32768 x 16 (include/gx_watch.h, k_watch), against the two
yardsticks of profiles/watch/README.md: the gx_view_minmax call it replaces, and the gather ceiling
of DESIGN.md §6 (gather_run16: 3.99e10 128-B view lines per second).

k_watch is timed with the engine's own HIP events (gx_enable_timing: the launch's class is
"converge", which nothing else in gx_run_rounds uses), over --rounds rounds after a warm-up, for
W = 64 and W = 1024 entries on distinct sampled keys; whole rounds without and then with a watch, two
adjacent stretches of --rounds rounds, by the host clock around gx_run_rounds (it returns when the
device is done); gx_view_minmax by the host clock around the call (it waits for the device too).
One JSON line.

    python profiles/watch/watch_cost.py [--hosts 32768] [--services 16] [--rounds 200]
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

from sidecar_amd.abi import WATCH_ANY, Engine, default_params, load_product  # noqa: E402

LINE_CEILING_PER_S = 6.379e11 / 16  # bench.py: gather_run16, 128-B view lines per second


def timed_rounds(e, n):
    t0 = time.perf_counter()
    e.run_rounds(n)
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=32768)
    ap.add_argument("--services", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=600)
    ap.add_argument("--seed", type=int, default=0x5EED)
    a = ap.parse_args()
    lib = load_product()
    # the cfg 5 engine of bench.py without its partition and storm: steady gossip rounds
    e = Engine(default_params(lib, n_hosts=a.hosts, n_services=a.services, fanout=3, packet_cap=32, pending_cap=100,
                              queue_cap=20480, list_slots=32, init_mode=2, ae_period_rounds=10, seed=a.seed), lib=lib)
    R = e.H * e.S
    out = {"hosts": e.H, "services": e.S, "rounds": a.rounds, "view_bytes": 8 * e.H * R}
    e.run_rounds(a.warmup)
    rng = np.random.default_rng(a.seed)
    for w in (64, 1024):
        e.watch_arm(0)
        ms_plain = timed_rounds(e, a.rounds)  # the rounds just before the watched ones: the engine's state drifts
        keys = rng.choice(R, size=w, replace=False).astype(np.uint32)
        e.watch_arm(w, a.rounds + 8)
        e.watch_set(0, keys, np.full(w, WATCH_ANY, dtype=np.int64))
        e.run_rounds(8)  # first launches
        t0 = e.timing()["converge"]
        e.enable_timing(True)
        e.run_rounds(a.rounds)
        t1 = e.timing()["converge"]
        e.enable_timing(False)
        n = t1["launches"] - t0["launches"]
        us = (t1["ms"] - t0["ms"]) * 1e3 / n
        counts, live, *_ = e.watch_read()
        every = bool(n == a.rounds and (live == e.H).all() and (counts[:, :, 0] == e.H).all())  # warm: every slot present
        e.watch_arm(w, a.rounds)
        e.watch_set(0, keys, np.full(w, WATCH_ANY, dtype=np.int64))
        ms_round = timed_rounds(e, a.rounds)
        lines = e.H * w
        out[f"w{w}"] = {"k_watch_us": round(us, 2), "gathers": lines, "gather_bytes": 8 * lines,
                        "lines_per_s": round(lines / (us * 1e-6), 0),
                        "ceiling_us": round(lines / LINE_CEILING_PER_S * 1e6, 2),
                        "of_gather_ceiling": round(lines / LINE_CEILING_PER_S * 1e6 / us, 4),
                        "round_ms_no_watch": round(ms_plain, 4), "round_ms_with_watch": round(ms_round, 4),
                        "every_view_counted": every}
    e.watch_arm(0)
    dev = torch.device("cuda:0")
    mn = torch.empty(R, dtype=torch.int64, device=dev)
    mx = torch.empty(R, dtype=torch.int64, device=dev)
    e.view_minmax(mn.data_ptr(), mx.data_ptr())
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        e.view_minmax(mn.data_ptr(), mx.data_ptr())
        ts.append((time.perf_counter() - t0) * 1e3)
    out["view_minmax_ms"] = [round(x, 3) for x in ts]
    out["view_minmax_ms_median"] = round(float(np.median(ts)), 3)
    for w in (64, 1024):
        out[f"w{w}"]["view_minmax_over_k_watch"] = round(out["view_minmax_ms_median"] * 1e3 / out[f"w{w}"]["k_watch_us"], 1)
    print(json.dumps(out), flush=True)
    e.close()


if __name__ == "__main__":
    main()
