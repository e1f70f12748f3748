"""GX_K_AE launch time of the two pools of waiting push-pull merges (gx.h lock_readers 1 and 2) on a
schedule where neither loses a merge, so both do the same work: the lock_readers test schedule at
n_hosts 4096, n_services 16 with a slot per host. One unmeasured window per policy at the measured
shape first (code objects, allocator), then fresh engines, alternating: rounds 0 to ROUNDS (most
exchanges with a read-locked side come in the rounds around the storm, round 5) between two
gx_timing_get reads. Writes one JSON object: per policy the window's ae ms / launches / bytes of every repeat, and the window's counters.

  python profiles/lock_pool/ae_ro_timing.py OUT.json [n_hosts n_services [repeats]]"""
import json
import sys

from sidecar_amd.abi import INIT_OWN, Engine, default_params, load_product

WARM, ROUNDS = 0, 60
COUNTERS = ("ae_exchanges", "ae_locked", "ae_deferred", "ae_defer_lost", "ae_merges")


def window(lib, policy, n_hosts, n_services):
    kw = dict(n_hosts=n_hosts, n_services=n_services, fanout=1, packet_cap=1, init_mode=INIT_OWN, churn_ppm=100000,
              alive_interval_rounds=2, tombstone_interval_rounds=7, ae_period_rounds=1, queue_cap=4096,
              storm_round=5, lock_readers=policy, lock_defer_slots=min(n_hosts, 4096), device=0)
    e = Engine(default_params(lib, **kw), lib=lib)
    e.enable_timing(True)
    if WARM:
        e.run_rounds(WARM)
    t0, s0 = e.timing()["ae"], e.stats()
    e.run_rounds(ROUNDS)
    t1, s1 = e.timing()["ae"], e.stats()
    out = {k: t1[k] - t0[k] for k in ("ms", "launches", "bytes")}
    out.update({k: s1[k] - s0[k] for k in COUNTERS})
    out["digest"] = int(e.digests().sum()) & 0xFFFFFFFFFFFF
    e.close()
    return out


def main():
    path = sys.argv[1]
    n_hosts, n_services = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (4096, 16)
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    lib = load_product()
    window(lib, 1, n_hosts, n_services)  # code objects loaded, allocator warm
    window(lib, 2, n_hosts, n_services)
    res = {"n_hosts": n_hosts, "n_services": n_services, "warm_rounds": WARM, "rounds": ROUNDS, "runs": []}
    for r in range(repeats):
        for policy in ((1, 2) if r % 2 == 0 else (2, 1)):
            w = window(lib, policy, n_hosts, n_services)
            w["lock_readers"], w["repeat"] = policy, r
            res["runs"].append(w)
            print(json.dumps(w), flush=True)
    for policy in (1, 2):
        ms = sorted(w["ms"] for w in res["runs"] if w["lock_readers"] == policy)
        res[f"ae_ms_lock_readers_{policy}"] = {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}
    same = {tuple(w[k] for k in COUNTERS + ("digest",)) for w in res["runs"]}
    res["same_work"] = len(same) == 1
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))


if __name__ == "__main__":
    main()
