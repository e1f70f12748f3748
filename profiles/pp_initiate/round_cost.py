"""One-GPU LocalShards timing of a sharded push-pull round, matching beside GX_PP_INITIATE (cfg 2
parameters, G = 4): wall time of each push-pull step with the device drained around it, and the
device time of its merge launches from the engine's timers in a second run.
  python profiles/pp_initiate/round_cost.py [out.json]   (default prof_out/pp_round_cost.json)"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bench import CONFIGS  # noqa: E402
from sidecar_amd.abi import load_product  # noqa: E402
from sidecar_amd.dist import LocalShards  # noqa: E402

gx = load_product()
base = dict(CONFIGS["cfg2"]["p"])
G, ROUNDS = 4, 41
out = {"G": G, "params": base, "rounds": ROUNDS, "modes": {}}


def run(kw, timing):
    sh = LocalShards(gx, G, device="cuda:0", **kw)
    if timing:
        for e in sh.engines:
            e.enable_timing(True)
    rows = []
    inner = sh._push_pull

    def timed():
        torch.cuda.synchronize()
        b0 = sh.ae_batches_run
        a0 = sum(e.timing()["ae"]["ms"] for e in sh.engines) if timing else 0.0
        t0 = time.perf_counter()
        inner()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        a1 = sum(e.timing()["ae"]["ms"] for e in sh.engines) if timing else 0.0
        rows.append({"round": sh.engines[0].round - 1, "wall_ms": (t1 - t0) * 1e3, "batches": sh.ae_batches_run - b0,
                     "ae_kernel_ms": a1 - a0})
    sh._push_pull = timed
    sh.run_rounds(ROUNDS)
    torch.cuda.synchronize()
    return rows, sh.stats(), sh.wire.as_dict(), sh.ae_skipped


for mode in (0, 1):
    kw = dict(base, push_pull_mode=mode)
    run(kw, False)  # code objects loaded, allocator warm
    wall, st, wire, skipped = run(kw, False)
    dev, _, _, _ = run(kw, True)
    out["modes"]["initiate" if mode else "matching"] = {
        "push_pull_rounds": [dict(w, ae_kernel_ms=d["ae_kernel_ms"]) for w, d in zip(wall, dev)],
        "ae_exchanges": st["ae_exchanges"], "ae_locked": st["ae_locked"], "skipped": skipped, "wire": wire}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "prof_out", "pp_round_cost.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
for m, v in out["modes"].items():
    print(m, json.dumps(v["push_pull_rounds"]), v["ae_exchanges"], v["ae_locked"], v["skipped"])
