"""Schedules shared by tests/test_lock_pool_cpu.py and tests/test_gpu_lock_pool.py (gx.h lock_readers
= 2, the claimed pool): the lock_readers test schedule with one change each and the pool size the
claimed pool runs it with, and the reference for a pool that loses nothing: the oracle's
direct-mapped pool with lock_defer_slots = n_hosts (v % P = v, so no two hosts share a slot)."""
from sidecar_amd.abi import INIT_OWN, LOCK_DEFER_MERGE, LOCK_READERS_MAPPED, Engine, default_params

BASE = dict(n_hosts=32, n_services=4, fanout=1, packet_cap=1, init_mode=INIT_OWN, churn_ppm=100000,
            alive_interval_rounds=2, tombstone_interval_rounds=7, ae_period_rounds=1, queue_cap=4096,
            storm_round=5)

# name -> (the change to BASE, pool size; 0 = the default 64)
SCHEDULES = {
    "matching": ({}, 8),
    "initiate": (dict(push_pull_mode=1), 8),
    "fd": (dict(fd_enable=1), 8),
    "odd_rows": (dict(n_hosts=33, n_services=3), 8),
    "gm4": (dict(gossip_messages=4), 8),
    "pp2_cap4": (dict(ae_period_rounds=2, packet_cap=4), 8),
    "h128": (dict(n_hosts=128), 16),
    "h128_initiate": (dict(n_hosts=128, push_pull_mode=1), 16),
    "h512": (dict(n_hosts=512), 0),
}
# the schedules on which the direct-mapped pool of the same size loses merges
CONTRAST = ("matching", "initiate", "gm4", "h128", "h512")
CHUNKS = (1, 4, 10, 35, 50, 100, 100)
ROUNDS = sum(CHUNKS)


def schedule(name):
    kw = dict(BASE)
    kw.update(SCHEDULES[name][0])
    return kw, SCHEDULES[name][1]


def lossless_oracle(oracle_lib, kw):
    return Engine(default_params(oracle_lib, lock_readers=LOCK_READERS_MAPPED, lock_defer_slots=kw["n_hosts"], **kw),
                  lib=oracle_lib)


def waiting(e):
    """The hosts whose push-pull merge waits for their lock."""
    return {v for v, h in enumerate(e.hosts()) if h.lock & LOCK_DEFER_MERGE}
