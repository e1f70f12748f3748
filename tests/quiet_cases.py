"""Quiet rounds: the schedules of tests/test_quiet_rounds_cpu.py and
tests/test_gpu_quiet_rounds.py, and what the CPU oracle says about them, computed once per process.

A round is quiet when, at its start, every host holds the ServicesState lock for it and its inbound
pipeline is full. From a quiet round n the bound

    B(n) = n + min over hosts of ceil((max over set looper flags of (nil_pos - fifo_head) + 1) / K)

(K = fanout x max(1, gossip_messages) dequeues per round at most) says that every round in [n, B(n))
is quiet; rounds (n, B(n)) are the ones predicted ahead."""
import functools

from sidecar_amd.abi import INIT_OWN, INIT_WARM, LOCK_BUF_SHIFT, Engine, default_params
from tests.oracle_lib import load_oracle
from tests.parity import snapshot

ROUNDS = 150
CHECK_ROUNDS = (10, 50, 51, 100, 150)

_STORM = dict(n_services=16, init_mode=INIT_WARM, storm_round=1, partition_start=0, partition_end=50,
              ae_period_rounds=10, queue_cap=4096)
SCHEDULES = {
    "h128": dict(_STORM, n_hosts=128, lock_buffer=32),
    "h256": dict(_STORM, n_hosts=256, lock_buffer=64),
}
# no storm, no partition: no host's pipeline ever fills while it is locked
COLD = dict(n_hosts=128, n_services=16, init_mode=INIT_OWN, ae_period_rounds=10, queue_cap=4096, lock_buffer=32)
MIN_PREDICTED = {"h128": 30, "h256": 80}


def host_bound(h, n, k, cap):
    """Host state h at the start of round n: the first round for which the host may stop being locked
    with a full pipeline, or 0 when it is not so in round n."""
    if not (h.lock >> (n & 1)) & 1 or not h.flags & 3 or (h.lock >> LOCK_BUF_SHIFT) < cap:
        return 0
    dist = max(((pos - h.fifo_head) & 0xFFFFFFFF) for bit, pos in ((1, h.nil_pos_bs), (2, h.nil_pos_bt))
               if h.flags & bit)
    return n + (dist + 1 + k - 1) // k


def is_quiet(hosts, n, cap):
    return all((h.lock >> (n & 1)) & 1 and (h.lock >> LOCK_BUF_SHIFT) >= cap for h in hosts)


@functools.lru_cache(maxsize=None)
def oracle_trace(name):
    """Runs the oracle over schedule `name` round by round. Returns quiet (set of rounds), predicted
    (rounds a bound taken at an earlier quiet round covers), unlocks (host unlock events) and the
    parity snapshots at CHECK_ROUNDS. The snapshots are shared: nobody changes them."""
    kw = COLD if name == "cold" else SCHEDULES[name]
    lib = load_oracle()
    p = default_params(lib, **kw)
    o = Engine(p, lib=lib)
    k = p.fanout * max(1, p.gossip_messages)
    cap = p.lock_buffer
    quiet, predicted, snaps = set(), set(), {}
    unlocks, until = 0, 0
    prev = None
    for n in range(ROUNDS):
        hosts = list(o.hosts())
        locked = [(h.lock >> (n & 1)) & 1 for h in hosts]
        if prev is not None:
            unlocks += sum(1 for a, b in zip(prev, locked) if a and not b)
        prev = locked
        if n < until:
            predicted.add(n)
        if is_quiet(hosts, n, cap):
            quiet.add(n)
            until = max(until, min(host_bound(h, n, k, cap) for h in hosts))
        o.run_rounds(1)
        if o.round in CHECK_ROUNDS:
            snaps[o.round] = snapshot(o)
    return dict(quiet=quiet, predicted=predicted, unlocks=unlocks, snaps=snaps, params=kw)
