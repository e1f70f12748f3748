"""Kernel time per shard round from a rocprofv3 kernel trace of shard_probe_ab.py --probe 1 --reps 1
(the rocpd database `<dir>/run_results.db`): the window from the first k_probe launch of the timed
rounds (the last rounds x G launches) to the end of the run, summed per kernel.

    python profiles/probe_shards/trace_rounds.py prof_out/trace/run_results.db [--G 8] [--rounds 9]
"""
import argparse
import json
import re
import sqlite3

ap = argparse.ArgumentParser()
ap.add_argument("db")
ap.add_argument("--G", type=int, default=8)
ap.add_argument("--rounds", type=int, default=9)
a = ap.parse_args()
rows = list(sqlite3.connect(a.db).execute("select name, start, end from kernels order by start"))
n = a.G * a.rounds
probes = [i for i, r in enumerate(rows) if "k_probe" in r[0]]
agg = {}
for name, s, e in rows[probes[-n]:]:
    k = agg.setdefault(re.sub(r"\(.*", "", name)[:60], [0, 0.0])
    k[0] += 1
    k[1] += (e - s) / 1e3
tot = sum(v[1] for v in agg.values())
print(json.dumps({"window": f"the last {n} k_probe launches to the end of the run",
                  "kernels": {k: {"launches": v[0], "total_us": round(v[1], 1), "per_launch_us": round(v[1] / v[0], 2)}
                              for k, v in sorted(agg.items(), key=lambda x: -x[1][1])},
                  "kernel_us_per_shard_round": round(tot / n, 2)}, indent=1))
