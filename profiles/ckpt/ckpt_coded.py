"""Coded checkpoints (include/gx_ckpt.h gx_ckpt_save_coded: server times in the ROW CODING, FIFOs as
their stored windows) beside the plain save of the same engine, at the BASELINE sizes, on two states
of each configuration: the engine as created and the engine after the bench window (bench.py's
default 2 + 100 rounds).

    python profiles/ckpt/ckpt_coded.py [--config cfg3 cfg5] [--reps 2] [--out FILE] [--dir DIR] [--max-file-gb 90]
                                        [--states created after_bench_window] [--rounds 102] [--hosts N]

Saves. Per state it alternates gx_ckpt_save (code = 0: the yardstick) and gx_ckpt_save_coded (both
sections coded) on the same engine, `reps` times each, all to /dev/null as profiles/ckpt/ckpt_rate.py
does (the wall time is the coders, the copy to the host and the checksum, not a file system's rate),
and reports per section the stored bytes of both files, the coders' device times (gx_ckpt_info,
gx_ckpt_coded_info: HIP events around the kernels) and the median wall time of each save.

Loads, one file on disk at a time, in --dir (default: a fresh temporary directory, removed at the
end). The saving engine's fingerprint is taken: counters, gx_view_minmax, the queue digests of every
host (each covers the host's whole stored window), state.LastChanged and the server times of 256
evenly spaced views, hashed. Then the raw file is written (its wall time is reported apart), the
engine is closed (two cfg5 engines do not fit one device), the file is loaded, timed from the call to
the restored engine (gx_create included), fingerprinted and removed; the restored engine, equal to the
saving one by its fingerprint, writes the coded file, is closed, and the coded file is loaded, timed,
fingerprinted and removed. A file is written only when it is at most --max-file-gb and the directory
has room for it and 8 GiB more; otherwise its load is null with the reason beside it, and the coded
file is written by the saving engine itself."""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from sidecar_amd.abi import (CK_FIFO, CK_SRVT, CK_VIEW, CKPT_CODE_FIFO, CKPT_CODE_SRVT, Engine,  # noqa: E402
                             load_product)

BOTH = CKPT_CODE_SRVT | CKPT_CODE_FIFO
CODES = (("raw", 0), ("coded", BOTH))


def say(*a):
    print("#", *a, flush=True)


def fingerprint(e):
    R = e.H * e.S
    mn = torch.empty(R, dtype=torch.int64, device="cuda:0")
    mx = torch.empty(R, dtype=torch.int64, device="cuda:0")
    e.view_minmax(mn.data_ptr(), mx.data_ptr())
    torch.cuda.synchronize()
    h = hashlib.sha256()
    h.update(mn.cpu().numpy().tobytes())
    h.update(mx.cpu().numpy().tobytes())
    h.update(e.digests().tobytes())
    h.update(e.last_changed().tobytes())
    for v in np.linspace(e.lo, e.hi - 1, 256).astype(int):
        h.update(e.server_times(int(v)).tobytes())
    return {"round": e.round, "stats": e.stats(), "sha256": h.hexdigest()}


def sections(info):
    return {"views": info["sections"][CK_VIEW]["stored_bytes"], "server_times": info["sections"][CK_SRVT]["stored_bytes"],
            "fifo": info["sections"][CK_FIFO]["stored_bytes"],
            "rest": info["stored_bytes"] - sum(info["sections"][k]["stored_bytes"] for k in (CK_VIEW, CK_SRVT, CK_FIFO)),
            "total": info["stored_bytes"]}


def fits(nbytes, where, max_bytes):
    """None if a file of nbytes may be written to `where`, else the reason it may not."""
    if nbytes > max_bytes:
        return f"the file ({nbytes} B) is above --max-file-gb"
    free = shutil.disk_usage(where).free
    if free < nbytes + (8 << 30):
        return f"the directory has {free} B free, the file needs {nbytes} B and 8 GiB of margin"
    return None


def save_file(e, path, code):
    t0 = time.perf_counter()
    e.ckpt_save(path, code)
    return round(time.perf_counter() - t0, 3)


def load_file(lib, path, want):
    """(the restored engine, its line of the result)"""
    t0 = time.perf_counter()
    b = Engine.from_checkpoint(path, lib=lib)
    dt = time.perf_counter() - t0
    return b, {"wall_s": round(dt, 3), "equals_saving_engine": fingerprint(b) == want,
               "view_coder_ms": round(b.ckpt_info["coder_ms"], 3)}


def measure(lib, e, state, cfg, reps, where, max_bytes, out_file):
    med = statistics.median
    wall, infos = {"raw": [], "coded": []}, {}
    for kind, code in CODES:  # warm-up, and the sizes
        infos[kind] = e.ckpt_save("/dev/null", code)
    for _ in range(reps):
        for kind, code in CODES:
            t0 = time.perf_counter()
            infos[kind] = e.ckpt_save("/dev/null", code)
            wall[kind].append(time.perf_counter() - t0)
    say(cfg, state, "saves timed")
    want = fingerprint(e)
    H, S, rnd = e.H, e.S, e.round
    path = {k: os.path.join(where, f"{cfg}_{state}_{k}.gxck") for k in ("raw", "coded")}
    why = {k: fits(infos[k]["stored_bytes"], where, max_bytes) for k in ("raw", "coded")}
    loads, file_wall = {"raw": None, "coded": None}, {"raw": None, "coded": None}
    src = e  # the engine that writes the next file
    if why["raw"] is None:
        file_wall["raw"] = save_file(e, path["raw"], 0)
        e.close()
        src, loads["raw"] = load_file(lib, path["raw"], want)
        os.remove(path["raw"])
        say(cfg, state, "raw file loaded", loads["raw"])
        why["coded"] = fits(infos["coded"]["stored_bytes"], where, max_bytes)
    if why["coded"] is None:
        file_wall["coded"] = save_file(src, path["coded"], BOTH)
        src.close()
        b, loads["coded"] = load_file(lib, path["coded"], want)
        loads["coded"]["written_by"] = "the engine restored from the raw file" if src is not e else "the saving engine"
        b.close()
        os.remove(path["coded"])
        say(cfg, state, "coded file loaded", loads["coded"])
    else:
        src.close()
    c = infos["coded"]["coded"]
    out = {
        "config": cfg, "state": state, "round": rnd, "hosts": H, "services": S, "reps": reps,
        "stored_bytes": {k: sections(infos[k]) for k in ("raw", "coded")},
        "save_wall_s": {k: round(med(wall[k]), 3) for k in wall},
        "view_coder_ms": {k: round(infos[k]["coder_ms"], 3) for k in infos},
        "srvt_coder_ms": {"base": round(c["srvt_base_ms"], 3), "count_scan": round(c["srvt_count_ms"], 3),
                          "emit": round(c["srvt_emit_ms"], 3), "total": round(c["srvt_ms"], 3)},
        "fifo_pack_ms": round(c["fifo_ms"], 3),
        "srvt_rows_raw": c["srvt_rows_raw"], "srvt_chunks": c["srvt_chunks"], "fifo_chunks": c["fifo_chunks"],
        "fifo_jobs": c["fifo_jobs"], "save_to_file_wall_s": file_wall, "load": loads,
        "not_loaded_because": {k: v for k, v in why.items() if v},
    }
    print(json.dumps(out), flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write(json.dumps(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["cfg3", "cfg5"])
    ap.add_argument("--states", nargs="+", default=["created", "after_bench_window"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=102, help="the bench window: warmup + steps")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--dir", help="write the files here (default: a temporary directory)")
    ap.add_argument("--max-file-gb", type=float, default=90.0)
    ap.add_argument("--hosts", type=int, help="the configuration's schedule at another n_hosts")
    a = ap.parse_args()
    lib = load_product()
    where = a.dir or tempfile.mkdtemp(prefix="gxck_")
    say("files in", where, "free", shutil.disk_usage(where).free)
    try:
        for cfg in a.config:
            for state in a.states:
                over = {"n_hosts": a.hosts} if a.hosts else {}
                e = bench.make_engine(lib, cfg, 0x5EED, 0, **over)  # (measure closes it: a fresh engine per state)
                if state != "created":
                    e.run_rounds(a.rounds)
                measure(lib, e, state, cfg, a.reps, where, int(a.max_file_gb * (1 << 30)), a.out)
    finally:
        if not a.dir:
            shutil.rmtree(where, ignore_errors=True)


if __name__ == "__main__":
    main()
