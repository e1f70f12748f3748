"""k_send over the bench window, by instance, from the kernel trace of plain
`bench.py --steps 100 --warmup 2` (rocprofv3 --kernel-trace --output-format csv): launches and total
µs of every k_send launch after the two warm-up rounds' (one launch each), and of the other round
kernels after the second warm-up round's k_send. One JSON line.

  python profiles/quiet_batch/trace_sum.py LABEL run_kernel_trace.csv"""
import csv
import json
import re
import sys

OTHERS = ("k_lock_append", "k_merge_seg", "k_ae_chunk", "k_ae_locked_note", "k_storm_p2")


def short(name):
    m = re.search(r"(k_\w+)(<[^>]*>)?", name)
    return (m.group(1), (m.group(1) + (m.group(2) or ""))) if m else (name, name)


if __name__ == "__main__":
    rows = []
    with open(sys.argv[2]) as f:
        for r in csv.DictReader(f):
            base, inst = short(r["Kernel_Name"])
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), base, inst))
    rows.sort()
    sends = [r for r in rows if r[2] == "k_send"]
    t_win = sends[2][0]  # the window's first k_send
    out = {"lib": sys.argv[1], "k_send_launches_in_process": len(sends), "k_send": {"launches": 0, "us": 0.0}, "k_send_instances": {}}
    for a, b, base, inst in rows:
        if a < t_win:
            continue
        us = (b - a) / 1e3
        if base == "k_send":
            out["k_send"]["launches"] += 1
            out["k_send"]["us"] += us
            i = out["k_send_instances"].setdefault(inst, {"launches": 0, "us": 0.0})
            i["launches"] += 1
            i["us"] += us
        elif base in OTHERS:
            o = out.setdefault(base, {"launches": 0, "us": 0.0})
            o["launches"] += 1
            o["us"] += us
    for v in [out["k_send"], *out["k_send_instances"].values(), *(out[k] for k in OTHERS if k in out)]:
        v["us"] = round(v["us"], 1)
        v["us_per_launch"] = round(v["us"] / max(1, v["launches"]), 2)
    out["window_us"] = round((max(r[1] for r in rows) - t_win) / 1e3, 1)
    print(json.dumps(out))
