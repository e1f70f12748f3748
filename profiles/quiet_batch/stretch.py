"""The quiet stretch of cfg 5 (every host locked, pipelines full): rounds 102..301 as one gx_run_rounds
call after 102 rounds, µs per round by the host clock around the call, with the launches per kernel
class and the send class's algorithmic bytes. One JSON line.

Run from the root of the tree whose library is measured (another checkout for the parent):
  [GX_QUIET_BATCH=1] python <path to>/profiles/quiet_batch/stretch.py LABEL"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from sidecar_amd.abi import load_product  # noqa: E402

FIRST, N = 102, 200

if __name__ == "__main__":
    lib = load_product()
    e = bench.make_engine(lib, "cfg5", 0x5EED, 0)
    e.run_rounds(FIRST)
    t0 = e.timing()
    a = time.perf_counter()
    e.run_rounds(N)
    dt = time.perf_counter() - a
    t1 = e.timing()
    launches = {k: t1[k]["launches"] - t0[k]["launches"] for k in t1 if t1[k]["launches"] != t0[k]["launches"]}
    print(json.dumps({"lib": sys.argv[1], "quiet_batch_env": os.environ.get("GX_QUIET_BATCH"),
                      "rounds": f"{FIRST}..{FIRST + N - 1}", "us_per_round": round(dt * 1e6 / N, 2), "launches": launches,
                      "send_bytes": t1["send"]["bytes"] - t0["send"]["bytes"],
                      "send_units": t1["send"]["units"] - t0["send"]["units"]}))
