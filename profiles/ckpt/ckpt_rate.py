"""Rate of the checkpoint view coder (include/gx_ckpt.h) beside gx_view_minmax, the existing kernel
that streams the same views once, at the BASELINE sizes, on two states of each configuration: the
engine as created and the engine after the bench window (bench.py's default 2 + 100 rounds).

    python profiles/ckpt/ckpt_rate.py [--config cfg2 cfg3 cfg4 cfg5] [--reps 3] [--out FILE] [--dir DIR]

Per state it alternates gx_view_minmax and gx_ckpt_save, `reps` times each, both timed with events on
the stream the kernels run on: the engine is put on a torch stream and gx_view_minmax bracketed by
torch events there; the coder's times are gx_ckpt_info's (HIP events around the base reduction, the
count and scans, the emit, summed over the chunks). The host wall time of each call is reported
beside them. One JSON line per state: the medians, the stored and raw bytes per section, the view
section's ratio.
Files go to --dir, by default to /dev/null (the coder's device times do not depend on where the bytes
land; the save's wall time does, and is reported as such)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from sidecar_amd.abi import CK_SRVT, CK_VIEW, load_product  # noqa: E402


def measure(e, stream, state, cfg, reps, path, out_file=None):
    R = e.H * e.S
    mn = torch.empty(R, dtype=torch.int64, device="cuda:0")
    mx = torch.empty(R, dtype=torch.int64, device="cuda:0")
    minmax, minmax_wall, base, count, emit, wall, info = [], [], [], [], [], [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(stream)
        e.view_minmax(mn.data_ptr(), mx.data_ptr())  # returns when the device is done
        b.record(stream)
        b.synchronize()
        minmax_wall.append((time.perf_counter() - t0) * 1e3)
        minmax.append(a.elapsed_time(b))
        t0 = time.perf_counter()
        info = e.ckpt_save(path)
        wall.append(time.perf_counter() - t0)
        base.append(info["base_ms"])
        count.append(info["count_ms"])
        emit.append(info["emit_ms"])
    med = statistics.median
    v = info["sections"][CK_VIEW]
    out = {
        "config": cfg, "state": state, "round": e.round, "hosts": e.H, "services": e.S, "reps": reps,
        "view_minmax_ms": round(med(minmax), 3), "view_minmax_ms_wall": round(med(minmax_wall), 3),
        "coder_ms": {"base": round(med(base), 3), "count_scan": round(med(count), 3), "emit": round(med(emit), 3),
                     "total": round(med(base) + med(count) + med(emit), 3)},
        "coder_over_minmax": round((med(base) + med(count) + med(emit)) / med(minmax), 2),
        "save_wall_s": round(med(wall), 3), "file": path,
        "views": {"raw_bytes": v["raw_bytes"], "stored_bytes": v["stored_bytes"],
                  "ratio": round(v["stored_bytes"] / v["raw_bytes"], 6), "views_raw": info["views_raw"],
                  "chunks": info["chunks"]},
        "server_times_bytes": info["sections"].get(CK_SRVT, {}).get("stored_bytes"),
        "total": {"raw_bytes": info["raw_bytes"], "stored_bytes": info["stored_bytes"]},
        "sections": {str(k): s["stored_bytes"] for k, s in info["sections"].items()},
    }
    print(json.dumps(out), flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write(json.dumps(out) + "\n")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["cfg2", "cfg3", "cfg4", "cfg5"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=102, help="the bench window: warmup + steps")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--dir", help="write real files here (default: /dev/null)")
    a = ap.parse_args()
    lib = load_product()
    stream = torch.cuda.Stream(device="cuda:0")
    for cfg in a.config:
        path = os.path.join(a.dir, f"{cfg}.gxck") if a.dir else "/dev/null"
        e = bench.make_engine(lib, cfg, 0x5EED, 0)
        e.set_stream(stream.cuda_stream, False)
        measure(e, stream, "created", cfg, a.reps, path, a.out)
        e.run_rounds(a.rounds)
        measure(e, stream, "after_bench_window", cfg, a.reps, path, a.out)
        e.close()


if __name__ == "__main__":
    main()
