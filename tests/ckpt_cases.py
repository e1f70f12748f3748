"""The continuity runs of tests/test_gpu_ckpt.py (include/gx_ckpt.h): engine A runs n1 rounds, saves
and runs n2 more; B, restored from the file, runs n2; both must equal the oracle after n1 + n2. The
save rounds were picked with the oracle so that the runs together save every kind of state that waits
across rounds (tests/test_ckpt_cases_cpu.py checks it on the CPU): a non-empty lock buffer, a waiting
push-pull merge, a pending ExpireServer, sleepers, pending records."""
from sidecar_amd.abi import (INIT_OWN, LOCK_BUF_SHIFT, LOCK_DEFER_MERGE, LOCK_PENDING_EXPIRE, LOCK_READERS_CLAIMED,
                             LOCK_READERS_MAPPED, Engine, default_params)
from tests import fd_cases, lock_pool_cases

FEATURES = ("lock_buffer", "waiting_merge", "pending_expire", "sleepers", "pending")


def features(e):
    """What of FEATURES the engine's hosts hold right now."""
    f = set()
    for h in e.hosts():
        if h.lock >> LOCK_BUF_SHIFT:
            f.add("lock_buffer")
        if h.lock & LOCK_DEFER_MERGE:
            f.add("waiting_merge")
        if h.lock & LOCK_PENDING_EXPIRE:
            f.add("pending_expire")
        if h.sleep_tail != h.sleep_head:
            f.add("sleepers")
        if h.dq_len:
            f.add("pending")
    return f


# the probe_piggyback schedule of tests/test_probe_cpu.py and a byte-mode one
PROBE = dict(n_hosts=64, n_services=8, init_mode=INIT_OWN, queue_cap=4096, lock_model=0, probe_piggyback=1)
BYTES = dict(n_hosts=48, n_services=6, init_mode=INIT_OWN, churn_ppm=40000, ae_period_rounds=10, limit_bytes=1398,
             packet_cap=48, queue_cap=4096)


def _pool(name, readers):
    kw, slots = lock_pool_cases.schedule(name)
    return dict(kw, lock_readers=readers, lock_defer_slots=slots)


def _fd_lossless():
    kw, slots = lock_pool_cases.schedule("fd")
    return kw, slots


# name -> (engine params, oracle params, n1, n2, compare the member lists)
RUNS = {}
for _name in ("matching", "initiate", "gm4", "odd_rows"):
    for _n1 in (0, 5, 15, 50):  # 5 is the storm's round
        _kw = _pool(_name, LOCK_READERS_MAPPED)
        RUNS[f"{_name}_r{_n1}"] = (_kw, _kw, _n1, 20, False)
_kw, _slots = _fd_lossless()
# the claimed pool beside the oracle's lossless direct-mapped one (tests/lock_pool_cases.py)
RUNS["fd_r15"] = (dict(_kw, lock_readers=LOCK_READERS_CLAIMED, lock_defer_slots=_slots),
                  dict(_kw, lock_readers=LOCK_READERS_MAPPED, lock_defer_slots=_kw["n_hosts"]), 15, 25, True)
for _name, _saves in (("churn_depart_bytes", (10, 40)), ("depart_no_fd", (3, 20))):  # before and after depart_round
    _kw = fd_cases.SCENARIOS[_name][0]
    for _n1 in _saves:
        RUNS[f"{_name}_r{_n1}"] = (_kw, _kw, _n1, 30, bool(_kw.get("fd_enable")))
RUNS["probe_r20"] = (PROBE, PROBE, 20, 20, False)
RUNS["bytes_r20"] = (BYTES, BYTES, 20, 20, False)


def oracle_at(oracle_lib, name, rounds):
    e = Engine(default_params(oracle_lib, **RUNS[name][1]), lib=oracle_lib)
    e.run_rounds(rounds)
    return e
