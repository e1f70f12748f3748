"""Batches of quiet rounds in one k_send launch: the schedules of tests/quiet_cases.py
and tests/quiet_send_cases.py together, and the runs that tests/test_gpu_quiet_batch.py makes of them
on the HIP engine, here so that a fresh process can make them too (the cap on a batch, GX_QUIET_BATCH,
is read when an engine is created).

The send class (gx_timing.launches) counts one launch per round, and one per batch."""
import json
import sys

from sidecar_amd.abi import Engine, default_params
from tests import quiet_cases, quiet_send_cases

ROUNDS = quiet_cases.ROUNDS
CHECK_ROUNDS = quiet_cases.CHECK_ROUNDS
SCHEDULES = {**quiet_cases.SCHEDULES, **quiet_send_cases.SCHEDULES}
MIN_PREDICTED = {**quiet_cases.MIN_PREDICTED, **quiet_send_cases.MIN_PREDICTED}
CHUNKS = (ROUNDS, 10, 7)  # one call; calls of 10; calls of 7, ragged against the push-pull period and the partition's end


def oracle_trace(name):
    return (quiet_cases if name in quiet_cases.SCHEDULES else quiet_send_cases).oracle_trace(name)


def send_launches(e):
    return e.timing()["send"]["launches"]


def engine(lib, name):
    return Engine(default_params(lib, **SCHEDULES[name]), lib=lib)


def run_parity(lib, name, chunk):
    """Schedule `name` in calls of `chunk` rounds beside the oracle's snapshots (at round 150 for one
    call, else at CHECK_ROUNDS); returns the send and merge launches."""
    from tests.test_gpu_quiet_rounds import assert_snap, merge_launches, run_checked
    t = oracle_trace(name)
    g = engine(lib, name)
    if chunk == ROUNDS:
        g.run_rounds(ROUNDS)
        assert_snap(g, t["snaps"][ROUNDS], f"{name} one call")
    else:
        run_checked(g, chunk, t["snaps"], f"{name} calls of {chunk}")
    return {"send_launches": send_launches(g), "merge_launches": merge_launches(g)}


def run_calls(lib, name, chunk=10):
    """Schedule `name` in calls of `chunk` rounds; quiet_send_cases.fingerprint at round ROUNDS with the
    send launches beside it."""
    g = engine(lib, name)
    while g.round < ROUNDS:
        g.run_rounds(min(chunk, ROUNDS - g.round))
    fp = quiet_send_cases.fingerprint(g)
    fp["send_launches"] = send_launches(g)
    return fp


if __name__ == "__main__":  # python -m tests.quiet_batch_cases parity|calls NAME: one JSON line (the tests' child process)
    from sidecar_amd.abi import load_product
    mode, name = sys.argv[1], sys.argv[2]
    lib = load_product()
    if mode == "parity":
        print(json.dumps({str(c): run_parity(lib, name, c) for c in CHUNKS}))
    else:
        print(json.dumps(run_calls(lib, name)))
