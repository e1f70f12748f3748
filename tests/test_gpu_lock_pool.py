"""The claimed pool of waiting push-pull merges (gx.h lock_readers = 2: k_ae_claim, k_ae_rox,
k_defer_drain) on the HIP engine. The oracle has no claimed pool; a pool that loses nothing must
match the oracle's direct-mapped pool with a slot per host (lock_defer_slots = n_hosts: v % P = v)
bit for bit, and with one slot the two policies coincide, losses included. The direct-mapped pool
(lock_readers = 1, the same kernels with the slot rule v % P) runs beside the oracle's at the sizes
where it loses merges. The schedules and pool
sizes are tests/lock_pool_cases.py's; tests/test_lock_pool_cpu.py pins that every pool has room."""
import pytest

from sidecar_amd.abi import (LOCK_READERS_CLAIMED, LOCK_READERS_MAPPED, LOCK_READERS_OFF, Engine, GxError,
                             default_params)
from tests.lock_pool_cases import CHUNKS, CONTRAST, ROUNDS, SCHEDULES, lossless_oracle, schedule, waiting
from tests.parity import assert_same

pytestmark = pytest.mark.gpu


def _claimed(gx_lib, kw, slots):
    return Engine(default_params(gx_lib, lock_readers=LOCK_READERS_CLAIMED, lock_defer_slots=slots, **kw), lib=gx_lib)


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_claimed_pool_lossless_parity(oracle_lib, gx_lib, name):
    kw, slots = schedule(name)
    g, o = _claimed(gx_lib, kw, slots), lossless_oracle(oracle_lib, kw)
    for chunk in CHUNKS:
        g.run_rounds(chunk)
        o.run_rounds(chunk)
        assert_same(g, o, f"{name} round {g.round}")
    st = g.stats()
    assert st["ae_deferred"] > 0 and st["ae_defer_lost"] == 0, st


@pytest.mark.parametrize("name", CONTRAST)
def test_direct_mapped_loses_where_claimed_does_not(oracle_lib, gx_lib, name):
    """The direct-mapped engine beside the oracle's direct-mapped pool of the same size, where many
    claimants want one slot and slots stay taken across rounds (the oracle's ae_claims)."""
    kw, slots = schedule(name)
    mapped = dict(lock_readers=LOCK_READERS_MAPPED, lock_defer_slots=slots, **kw)
    m = Engine(default_params(gx_lib, **mapped), lib=gx_lib)
    o = Engine(default_params(oracle_lib, **mapped), lib=oracle_lib)
    c = _claimed(gx_lib, kw, slots)
    for chunk in CHUNKS:
        m.run_rounds(chunk)
        o.run_rounds(chunk)
        assert_same(m, o, f"{name} direct-mapped round {m.round}")
    c.run_rounds(ROUNDS)
    print(f"{name}: direct-mapped lost {m.stats()['ae_defer_lost']} of {m.stats()['ae_deferred']} deferred, "
          f"claimed lost {c.stats()['ae_defer_lost']} of {c.stats()['ae_deferred']}")
    assert m.stats()["ae_defer_lost"] > 0
    assert c.stats()["ae_defer_lost"] == 0


@pytest.mark.parametrize("name", ["matching", "initiate"])
def test_one_slot_is_the_direct_mapped_pool(oracle_lib, gx_lib, name):
    """With one slot both rules say: free at the launch's start, the lowest host id gets it. Pins
    the overflow path, losses included, to the oracle."""
    kw, _ = schedule(name)
    g = _claimed(gx_lib, kw, 1)
    o = Engine(default_params(oracle_lib, lock_readers=LOCK_READERS_MAPPED, lock_defer_slots=1, **kw), lib=oracle_lib)
    for chunk in CHUNKS:
        g.run_rounds(chunk)
        o.run_rounds(chunk)
        assert_same(g, o, f"{name} one slot round {g.round}")
    assert g.stats()["ae_defer_lost"] > 0


def test_overflow_only_when_full(oracle_lib, gx_lib):
    """A pool of 2 beside the lossless oracle, whose peak is above 2: identical until the first
    loss; there the two slots are full, the admitted hosts are the lowest ids of the round's
    claimants, and deferred + lost is what the oracle deferred."""
    kw, _ = schedule("matching")
    g, o = _claimed(gx_lib, kw, 2), lossless_oracle(oracle_lib, kw)
    before = set()
    while True:
        assert g.round < ROUNDS, "no loss in 300 rounds"
        g.run_rounds(1)
        o.run_rounds(1)
        if g.stats()["ae_defer_lost"]:
            break
        assert_same(g, o, f"pool 2 round {g.round}")
        before = waiting(g)
        assert len(before) <= 2
    st, wg, wo = g.stats(), waiting(g), waiting(o)
    assert st["ae_deferred"] + st["ae_defer_lost"] == o.stats()["ae_deferred"]
    assert len(wg) == 2 and wg <= wo, (wg, wo)
    lost, admitted = wo - wg, wg - before
    assert len(lost) == st["ae_defer_lost"]
    assert all(x > y for x in lost for y in admitted), (lost, admitted)
    while g.round < ROUNDS:
        g.run_rounds(1)
        assert len(waiting(g)) <= 2
    off = Engine(default_params(gx_lib, lock_readers=LOCK_READERS_OFF, **kw), lib=gx_lib)
    off.run_rounds(ROUNDS)
    st, so = g.stats(), off.stats()
    assert st["locked_merges"] == 0
    assert st["ae_exchanges"] + st["ae_locked"] == so["ae_exchanges"] + so["ae_locked"]


def test_claimed_pool_events_parity(oracle_lib, gx_lib):
    """A waiting merge's ChangeEvents come at the receive phase of the host's first unlocked round,
    whichever slot kept its row."""
    kw, slots = schedule("gm4")
    g, o = _claimed(gx_lib, kw, slots), lossless_oracle(oracle_lib, kw)
    views = [(v, 1, 4096) for v in range(0, 32, 3)]
    for v, lid, cap in views:
        g.add_listener(v, lid, cap)
        o.add_listener(v, lid, cap)
    n_ev = 0
    for chunk in (1, 9, 40, 100, 150):
        g.run_rounds(chunk)
        o.run_rounds(chunk)
        assert_same(g, o, f"events round {g.round}")
        for v, lid, cap in views:
            ge = [x.tup() for x in g.drain_listener(v, lid, cap)]
            oe = [x.tup() for x in o.drain_listener(v, lid, cap)]
            assert ge == oe, f"view {v} round {g.round}"
            n_ev += len(ge)
    assert n_ev > 0 and g.stats()["ae_deferred"] > 0


@pytest.mark.parametrize("bad", [dict(lock_readers=3), dict(lock_readers=2, lock_model=0),
                                 dict(lock_readers=2, n_shards=2, shard_id=0),
                                 dict(lock_readers=2, lock_defer_slots=4097)])
def test_claimed_pool_rejects_unsupported_modes(gx_lib, bad):
    with pytest.raises(GxError):
        Engine(default_params(gx_lib, n_hosts=16, n_services=4, **bad), lib=gx_lib)
