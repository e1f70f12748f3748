"""Wall-clock latency of single-host ABI calls on a 128 x 16 engine, one library against another.

    python profiles/abi_guard/call_latency.py --libs parent.so sidecar_amd/libgx.so --calls 3000 --reps 3

Each repetition makes a fresh engine (schedule h128 of tests/quiet_cases.py, 20 rounds in), then times
every call of gx_is_new_service (a reader) and of gx_expire_server (a mutating call; the owner is
expired by the first call, the rest find nothing to do) with time.perf_counter_ns around the ctypes
call. The libraries alternate: A B B A A B ... One JSON line per (library, entry, repetition)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sidecar_amd.abi import ALIVE, Engine, default_params, load_library, svc_array  # noqa: E402
from tests import quiet_cases  # noqa: E402


def timed(fn, n):
    t = np.empty(n, dtype=np.int64)
    for i in range(n):
        a = time.perf_counter_ns()
        rc = fn()
        t[i] = time.perf_counter_ns() - a
        assert rc == 0
    return t / 1e3


def one(lib, calls):
    e = Engine(default_params(lib, **quiet_cases.SCHEDULES["h128"]), lib=lib)
    e.run_rounds(20)
    rec, out, x = svc_array([(3, 5, e.now(), ALIVE)]), C.c_int(), C.c_int()
    res = {"gx_is_new_service": timed(lambda: lib.gx_is_new_service(e.h, 7, rec, C.byref(out)), calls),
           "gx_expire_server": timed(lambda: lib.gx_expire_server(e.h, 7, 100, C.byref(x)), calls)}
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs=2, required=True, metavar=("A", "B"))
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    libs = [load_library(p) for p in a.libs]
    order = [0, 1, 1, 0] * a.reps
    done = [0, 0]
    for k in order[:2 * a.reps]:
        for entry, us in one(libs[k], a.calls).items():
            print(json.dumps({"lib": a.libs[k], "entry": entry, "rep": done[k], "calls": a.calls,
                              "median_us": round(float(np.median(us)), 3), "p10_us": round(float(np.percentile(us, 10)), 3),
                              "p90_us": round(float(np.percentile(us, 90)), 3), "mean_us": round(float(us.mean()), 3)}),
                  flush=True)
        done[k] += 1


if __name__ == "__main__":
    main()
