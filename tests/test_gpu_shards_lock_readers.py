"""Push-pull with a read-locked side (gx.h lock_readers = 1, the direct-mapped pool) on sharded HIP
engines: G shards in one process on one GPU stay bit-identical to the unsharded HIP engine and to the
unsharded CPU oracle (which refuses sharded lock_readers), losses included. The pool is cluster-wide:
every run of the push-pull chain arbitrates its slots over all shards (gx_ae_claim_want, the MIN
reduction, gx_ae_claim_set), a read-locked side of a cross-shard pair keeps the partner's rebuilt
row (k_ae_xdefer) and the unlocked side merges at once. The schedule is tests/lock_pool_cases.py's
BASE with one change per case; the figures the cases rely on (admitted and lost sides, per G) come
from the unsharded oracle's run of each case, 60 rounds, default seed."""
from unittest import mock

import numpy as np
import pytest

from sidecar_amd.abi import LOCK_DEFER_MERGE, Engine, GxError, default_params
from sidecar_amd.dist import LocalShards
from tests.lock_pool_cases import BASE, waiting
from tests.test_shards_cpu import assert_sharded_equal

pytestmark = pytest.mark.gpu

_RAGGED = dict(n_hosts=70, n_services=11)
# name -> (the change to BASE, pool slots, the direct-mapped pool loses merges)
CASES = {
    "matching_p8": ({}, 8, True),
    "matching_p1": ({}, 1, True),
    "initiate_p8": (dict(push_pull_mode=1), 8, True),
    "initiate_stagger_p8": (dict(push_pull_mode=1, push_pull_stagger=1, ae_period_rounds=3), 8, False),
    "odd_p8": (dict(n_hosts=33, n_services=3), 8, False),  # R = 99: the scalar copy path, uneven shards
    "ragged_p8": (_RAGGED, 8, True),  # R = 770: two digest blocks, the last ragged
    "ragged_init_p8": (dict(_RAGGED, push_pull_mode=1), 8, True),
    "gm4_p8": (dict(gossip_messages=4), 8, True),  # the sized gossip path
    "b3_p16": (dict(n_hosts=96, n_services=16), 16, True),  # R = 1536: three digest blocks
}
RUNS = [(name, G) for name in CASES for G in (2, 3, 5)] + [("ragged_p8", 8), ("b3_p16", 8)]
CHUNKS = (1, 4, 10, 15, 30)


def _kw(name, lock_readers=1):
    change, slots, _ = CASES[name]
    return dict(BASE, lock_readers=lock_readers, lock_defer_slots=slots, **change)


def _trio(gx_lib, oracle_lib, kw, G):
    whole = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    orc = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    return whole, orc, LocalShards(gx_lib, G, device="cuda:0", **kw)


@pytest.mark.parametrize("name,G", RUNS)
def test_gpu_lock_readers_shards_match_whole(gx_lib, oracle_lib, name, G):
    kw, lossy = _kw(name), CASES[name][2]
    whole, orc, sh = _trio(gx_lib, oracle_lib, kw, G)
    for chunk in CHUNKS:
        for e in (whole, orc, sh):
            e.run_rounds(chunk)
        assert_sharded_equal(whole, sh, f"{name} G={G} round {whole.round}")
        assert_sharded_equal(orc, sh, f"{name} G={G} round {whole.round} vs oracle")
    st, ro = orc.stats(), sh.ro_counts()
    print(f"{name} G={G}: ae_exchanges {st['ae_exchanges']} ae_locked {st['ae_locked']} ae_deferred "
          f"{st['ae_deferred']} ae_defer_lost {st['ae_defer_lost']}; across shards {ro}; skipped {sh.ae_skipped}")
    # not vacuous, by the oracle's counters ...
    assert st["ae_deferred"] > 0 and st["ae_locked"] > 0
    assert (st["ae_defer_lost"] > 0) == lossy
    # ... and by the driver's: a read-locked exchange between shards with an admitted side, and in
    # the lossy cases a side that lost its slot to a host of another shard
    assert ro["cross_exchanges"] > 0 and 0 < ro["cross_admitted"] <= st["ae_deferred"]
    assert (0 < ro["lost_to_other_shard"] <= st["ae_defer_lost"]) if lossy else ro["lost_to_other_shard"] == 0
    if (name, G) == ("matching_p8", 2):
        # the oracle's run: 5 admitted, 4 of them in cross pairs; 2 lost, both to the other shard
        assert (st["ae_deferred"], st["ae_defer_lost"]) == (5, 2)
        assert (ro["cross_admitted"], ro["lost_to_other_shard"]) == (4, 2)
    assert sh.ae_skipped == 0  # an all-locked round can still have runnable exchanges


def _waiting(sh):
    return {e.lo + v for e in sh.engines for v, h in enumerate(e.hosts()) if h.lock & LOCK_DEFER_MERGE}


def test_gpu_lock_readers_both_sides_read_locked(gx_lib, oracle_lib):
    """matching_p8, G = 2, round 4: hosts 1 (shard 0) and 20 (shard 1) are paired and both read-locked.
    Both lead every differing block, nobody returns or merges, and each keeps the other's row or
    loses it, as the oracle says."""
    whole, orc, sh = _trio(gx_lib, oracle_lib, _kw("matching_p8"), 2)
    for e in (whole, orc, sh):
        e.run_rounds(4)
    hs = orc.hosts()
    assert hs[1].locked_at(4) and hs[20].locked_at(4)
    assert not (waiting(orc) | _waiting(sh)) & {1, 20}
    before = orc.stats()
    for e in (whole, orc, sh):
        e.run_rounds(1)
    st = orc.stats()
    settled = st["ae_deferred"] + st["ae_defer_lost"] - before["ae_deferred"] - before["ae_defer_lost"]
    assert settled >= 2 and st["ae_exchanges"] > before["ae_exchanges"]
    assert _waiting(sh) == waiting(orc) == waiting(whole)
    assert_sharded_equal(orc, sh, "both sides read-locked, round 4")
    assert_sharded_equal(whole, sh, "both sides read-locked, round 4 (unsharded HIP)")


def test_gpu_lock_readers_shards_events_parity(gx_lib, oracle_lib):
    """ChangeEvents of listening views on their owning shards: the unlocked side's merge at the
    exchange, the waiting merge at the host's first unlocked round."""
    G = 3
    _, orc, sh = _trio(gx_lib, oracle_lib, _kw("gm4_p8"), G)
    views = [(v, 1, 4096) for v in range(0, 32, 3)]
    owner = {v: next(e for e in sh.engines if e.lo <= v < e.hi) for v, _, _ in views}
    for v, lid, cap in views:
        owner[v].add_listener(v, lid, cap)
        orc.add_listener(v, lid, cap)
    n_ev = 0
    for chunk in CHUNKS:
        sh.run_rounds(chunk)
        orc.run_rounds(chunk)
        assert_sharded_equal(orc, sh, f"events round {orc.round}")
        for v, lid, cap in views:
            ge = [x.tup() for x in owner[v].drain_listener(v, lid, cap)]
            oe = [x.tup() for x in orc.drain_listener(v, lid, cap)]
            assert ge == oe, f"view {v} round {orc.round}"
            n_ev += len(ge)
    assert n_ev > 0 and orc.stats()["ae_deferred"] > 0 and sh.ro_counts()["cross_admitted"] > 0


def test_gpu_lock_readers_off_is_untouched(gx_lib, oracle_lib):
    """lock_readers = 0 on the same schedule: no arbitration call, the census shortcut in exactly the
    rounds in which the oracle starts with every host locked and fails an exchange on the lock."""
    kw, G, rounds = _kw("matching_p8", lock_readers=0), 2, sum(CHUNKS)
    orc = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    all_locked = 0
    for r in range(rounds):
        locked = all(h.locked_at(r) for h in orc.hosts())
        before = orc.stats()["ae_locked"]
        orc.run_rounds(1)
        all_locked += locked and orc.stats()["ae_locked"] > before
    whole = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    whole.run_rounds(rounds)

    def refuse(*a):
        raise AssertionError("arbitration call with lock_readers = 0")

    with mock.patch.object(Engine, "ae_claim_want", refuse), mock.patch.object(Engine, "ae_claim_set", refuse), \
            mock.patch.object(Engine, "ae_ro_counts", refuse):
        sh = LocalShards(gx_lib, G, device="cuda:0", **kw)
        sh.run_rounds(rounds)
        assert sh.ro_counts() == dict(cross_exchanges=0, cross_admitted=0, lost_to_other_shard=0)
    print(f"lock_readers 0: all-locked push-pull rounds {all_locked}, skipped {sh.ae_skipped}")
    assert sh.ae_skipped == all_locked
    assert_sharded_equal(whole, sh, "lock_readers 0")
    assert_sharded_equal(orc, sh, "lock_readers 0 vs oracle")
    assert orc.stats()["ae_deferred"] == 0 and orc.stats()["ae_locked"] > 0


def _shard0(lib, **kw):
    return Engine(default_params(lib, n_shards=2, shard_id=0, n_hosts=32, n_services=4, ae_period_rounds=4, **kw),
                  lib=lib)


def test_gpu_sharded_lock_readers_params(gx_lib):
    _shard0(gx_lib, lock_readers=1).close()
    _shard0(gx_lib, lock_readers=1, lock_defer_slots=4096, push_pull_mode=1, push_pull_stagger=1).close()
    for bad in (dict(fd_enable=1), dict(lock_model=0), dict(lock_defer_slots=4097)):
        with pytest.raises(GxError, match="rc=-22"):
            _shard0(gx_lib, lock_readers=1, **bad)
    assert np.array_equal(_shard0(gx_lib, lock_readers=1).ae_ro_counts(), (0, 0, 0))
