"""Schedules for k_send's lean quiet-round instance, beside tests/quiet_cases.py: the
paths of a quiet round's sends that the schedules there do not reach, and what the CPU oracle says
about them, computed once per process (tests/test_quiet_send_cpu.py, tests/test_gpu_quiet_send.py).

Each is quiet_cases._STORM (S = 16, warm start, storm at round 1, partition [0, 50), push-pull every
10 rounds, queue_cap 4096) plus overrides:
  h130_cap8_pend4  a ragged last block and wave; every EXPIRE batch of 16 leaves records pending in a
                   dropped packet (packet_cap 8) and the ring is cut (pending_cap 4)
  h128_s64         S = 64: the owner ticks are a separate k_owner, so the peers are sampled in k_send's
                   prologue; batches of 64 against the default packet_cap
  h128_s4          S = 4: another owner-tick class of the fused launch
  h192_s8_f5       S = 8, fanout 5: a third class, more peers than team lanes"""
import functools
import hashlib
import json
import sys

import numpy as np

from sidecar_amd.abi import Engine, default_params
from tests import quiet_cases
from tests.oracle_lib import load_oracle
from tests.parity import snapshot

ROUNDS = quiet_cases.ROUNDS
CHECK_ROUNDS = quiet_cases.CHECK_ROUNDS

SCHEDULES = {
    "h130_cap8_pend4": dict(quiet_cases._STORM, n_hosts=130, lock_buffer=32, packet_cap=8, pending_cap=4),
    "h128_s64": dict(quiet_cases._STORM, n_hosts=128, n_services=64, lock_buffer=64),
    "h128_s4": dict(quiet_cases._STORM, n_hosts=128, n_services=4, lock_buffer=16),
    "h192_s8_f5": dict(quiet_cases._STORM, n_hosts=192, n_services=8, lock_buffer=32, fanout=5),
}
# rounds covered by a bound taken at an earlier round, on the oracle over 150 rounds (quiet rounds:
# 51, 45, 62, 53); the tests ask for 5 fewer
PREDICTED = {"h130_cap8_pend4": 45, "h128_s64": 38, "h128_s4": 55, "h192_s8_f5": 47}
MIN_PREDICTED = {k: v - 5 for k, v in PREDICTED.items()}
# the schedules whose dropped packets leave batch records pending and cut the ring in predicted rounds
PENDING = ("h130_cap8_pend4", "h128_s64")


@functools.lru_cache(maxsize=None)
def oracle_trace(name):
    """Runs the oracle over schedule `name` round by round. Returns quiet (set of rounds), predicted
    (rounds a bound taken at an earlier quiet round covers), pending_drops_predicted (the growth of
    stats.pending_drops inside predicted rounds), the final stats and the parity snapshots at
    CHECK_ROUNDS. The snapshots are shared: nobody changes them."""
    kw = SCHEDULES[name]
    lib = load_oracle()
    p = default_params(lib, **kw)
    o = Engine(p, lib=lib)
    k = p.fanout * max(1, p.gossip_messages)
    cap = p.lock_buffer
    quiet, predicted, snaps = set(), set(), {}
    until, pdrop = 0, 0
    for n in range(ROUNDS):
        hosts = list(o.hosts())
        covered = n < until
        if covered:
            predicted.add(n)
        if quiet_cases.is_quiet(hosts, n, cap):
            quiet.add(n)
            until = max(until, min(quiet_cases.host_bound(h, n, k, cap) for h in hosts))
        before = o.stats()["pending_drops"] if covered else 0
        o.run_rounds(1)
        if covered:
            pdrop += o.stats()["pending_drops"] - before
        if o.round in CHECK_ROUNDS:
            snaps[o.round] = snapshot(o)
    return dict(quiet=quiet, predicted=predicted, pending_drops_predicted=pdrop, stats=o.stats(), snaps=snaps,
                params=kw)


def fingerprint(e):
    """An engine's parity snapshot and its send class's algorithmic bytes and units (gx_timing) in a
    form that compares across processes: JSON values, the arrays as SHA-256 of their bytes."""
    s = snapshot(e)
    t = e.timing()["send"]
    fp = {"round": e.round, "stats": s["stats"], "hosts": [list(h) for h in s["hosts"]],
          "send_bytes": t["bytes"], "send_units": t["units"], "merge_launches": e.timing()["merge"]["launches"]}
    for k in ("views", "digests", "last_changed", "times"):
        fp[k] = hashlib.sha256(np.ascontiguousarray(s[k]).tobytes()).hexdigest()
    return json.loads(json.dumps(fp))


def run_product(name):
    """Schedule `name` on the HIP engine in calls of 1 round (every bound is seen before the next
    round, so the quiet path is taken wherever it is predicted); its fingerprint at round ROUNDS."""
    from sidecar_amd.abi import load_product
    lib = load_product()
    g = Engine(default_params(lib, **SCHEDULES[name]), lib=lib)
    for _ in range(ROUNDS):
        g.run_rounds(1)
    return fingerprint(g)


if __name__ == "__main__":  # python -m tests.quiet_send_cases NAME: one JSON line (the tests' child process)
    print(json.dumps(run_product(sys.argv[1])))
