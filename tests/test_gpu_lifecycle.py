"""Engines give their device memory back: free device memory (hipMemGetInfo, through
torch.cuda.mem_get_info) before and after ten create / destroy cycles, after two cycles that warm
the runtime up. One engine is open at a time.

The bound is half of what one forgotten buffer costs: ten engines that each lose Dev::arena_bits
(4 B * n_hosts * ceil(list_slots / 32), which gx_destroy's pointer table did not list) lose ten times
its size, so a loss under five times its size means that buffer, and any larger one, is freed.

Measured on an MI355X, where free memory moves in 2 MiB steps: with the table that forgot arena_bits
the first test lost 4 MiB over its ten engines (bound 2.5 MiB); with the owning list both lose 0."""
import numpy as np
import pytest
import torch

from sidecar_amd.abi import INIT_WARM, LOCK_READERS_CLAIMED, LOCK_READERS_MAPPED, Engine, default_params

pytestmark = pytest.mark.gpu

PP_INITIATE = 1  # gx.h GX_PP_INITIATE
WARMUP, CYCLES = 2, 10


def _arena_bits_bytes(kw, list_slots):
    return 4 * kw["n_hosts"] * ((list_slots + 31) // 32)


def _loss(cycle):
    """Bytes of free device memory lost over CYCLES calls of cycle(), after WARMUP calls."""
    for _ in range(WARMUP):
        cycle()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(CYCLES):
        cycle()
    return before - torch.cuda.mem_get_info()[0]


def test_destroyed_engines_return_their_memory(gx_lib):
    """arena_bits is 512 KiB of an engine of about half a GB."""
    kw = dict(n_hosts=4096, n_services=1, list_slots=1024, packet_cap=1, pending_cap=0)
    leak = _arena_bits_bytes(kw, kw["list_slots"])
    assert leak >= 512 << 10

    def cycle():
        Engine(default_params(gx_lib, **kw), lib=gx_lib).close()

    loss = _loss(cycle)
    print(f"lost {loss} B over {CYCLES} engines; arena_bits is {leak} B")
    assert loss < CYCLES * leak // 2


def _tup(x):
    return (x.host, x.svc, x.updated_ns, x.status)


# Every optional branch of the engine's allocations. An engine takes either the failure detector or
# GX_PP_INITIATE (check_params), so a cycle runs one engine of each kind, one after the other.
COMMON = dict(n_hosts=64, n_services=4, init_mode=INIT_WARM, ae_period_rounds=1, storm_round=1, lock_model=1)
KINDS = [
    dict(fd_enable=1, fd_push_pull_state=1, fd_handoff_shared=1),
    dict(push_pull_mode=PP_INITIATE),
]


def _use(e, names):
    """The calls whose buffers are made after gx_create; returns the sorted readers' results."""
    e.run_rounds(3)
    e.add_listener(0, 7, 16)
    assert e.remove_listener(0, 7) == 0
    e.set_service_names(names)
    by = [(k, _tup(x)) for k, x in e.by_service(0)]
    srt = [_tup(x) for x in e.each_service_sorted(0)]
    return by, srt


def test_optional_buffers_are_returned(gx_lib, oracle_lib):
    """The reference of the first cycle's sorted readers is the oracle with the same parameters but
    for the pool: it has no claimed pool (lock_readers = 2), so it runs the direct-mapped one with a
    slot per host, which loses no merge (tests/lock_pool_cases.py); the claimed pool's default 64
    slots cannot fill with 64 hosts either."""
    rnd = np.random.default_rng(11)
    names = [f"svc-{int(x)}" for x in rnd.integers(0, 5, size=COMMON["n_hosts"] * COMMON["n_services"])]
    want = []
    for kind in KINDS:
        o = Engine(default_params(oracle_lib, lock_readers=LOCK_READERS_MAPPED, lock_defer_slots=COMMON["n_hosts"],
                                  **COMMON, **kind), lib=oracle_lib)
        want.append(_use(o, names))
        assert want[-1][1], "an empty view checks nothing"
        o.close()
    first = []

    def cycle():
        for kind in KINDS:
            g = Engine(default_params(gx_lib, lock_readers=LOCK_READERS_CLAIMED, **COMMON, **kind), lib=gx_lib)
            got = _use(g, names)
            g.close()
            if len(first) < len(KINDS):
                first.append(got)

    loss = _loss(cycle)
    assert first == want
    leak = _arena_bits_bytes(COMMON, default_params(gx_lib).list_slots)
    print(f"lost {loss} B over {CYCLES} cycles of {len(KINDS)} engines; arena_bits is {leak} B")
    assert loss < CYCLES * leak // 2
