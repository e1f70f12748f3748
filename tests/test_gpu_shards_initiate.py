"""Per-node push-pull (push_pull_mode = GX_PP_INITIATE, with and without staggered timers) on
sharded HIP engines: a push-pull round is one run of the cross-shard chain per batch of the round's
exchanges, and G shards in one process on one GPU stay bit-identical to the unsharded HIP engine and
to the unsharded CPU oracle (the oracle has no sharded twin of this protocol). The scenarios are the
smallest with rows of three digest blocks and a ragged last block, odd host counts over 3 and 5
shards, several batches per round and cross-shard exchanges in batches after the first."""
import numpy as np
import pytest

from sidecar_amd.abi import PP_INITIATE, Engine, GxError, default_params
from sidecar_amd.dist import LocalShards
from tests.test_shards_cpu import assert_sharded_equal

pytestmark = pytest.mark.gpu

_STORM = dict(n_hosts=48, n_services=8, init_mode=2, ae_period_rounds=5, partition_start=0, partition_end=30,
              storm_round=4, queue_cap=2048)
_LOCKED = dict(n_hosts=64, n_services=16, init_mode=2, ae_period_rounds=10, partition_start=0, partition_end=30,
               storm_round=5, queue_cap=2048)
SCEN = {name: dict(kw, push_pull_mode=PP_INITIATE) for name, kw in {
    "pp_storm": _STORM,
    "pp_storm_lock_off": dict(_STORM, lock_model=0),
    # rows of three 512-slot digest blocks (R = 1536)
    "pp_blocks3": dict(n_hosts=96, n_services=16, init_mode=2, ae_period_rounds=5, partition_start=0,
                       partition_end=12, storm_round=3, churn_ppm=30000, queue_cap=4096),
    # a partial last block (R = 770), an odd split over 3 shards, some host's timer every round
    "pp_stagger_ragged": dict(n_hosts=70, n_services=11, init_mode=1, push_pull_stagger=1, ae_period_rounds=4,
                              churn_ppm=80000, aged_ppm=50000, queue_cap=1024),
    # the sized gossip path (GossipMessages 2) asks the binding whether a round has push-pull
    "pp_stagger_gm2": dict(n_hosts=64, n_services=8, init_mode=2, push_pull_stagger=1, ae_period_rounds=10,
                           gossip_messages=2, partition_start=0, partition_end=20, storm_round=5, queue_cap=4096),
    "pp_departures": dict(n_hosts=60, n_services=8, init_mode=2, ae_period_rounds=5, partition_start=0,
                          partition_end=12, storm_round=3, depart_round=4, depart_ppm=150000, queue_cap=2048),
    # every host locked from round ~10: the census shortcut
    "pp_stagger_locked": dict(_LOCKED, push_pull_stagger=1),
    "pp_locked": _LOCKED,
}.items()}
WITH_ACCEPTS = {"pp_storm", "pp_storm_lock_off", "pp_blocks3", "pp_stagger_ragged", "pp_stagger_gm2", "pp_departures"}
CROSS_BLOCKS = {"pp_storm_lock_off", "pp_blocks3"}  # cross-shard exchanges that ship blocks
CASES = [(name, G) for name in sorted(SCEN) for G in (2, 3, 5)] + [("pp_blocks3", 8)]


@pytest.mark.parametrize("name,G", CASES)
def test_gpu_initiate_shards_match_whole(gx_lib, oracle_lib, name, G):
    kw = SCEN[name]
    whole = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    orc = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    sh = LocalShards(gx_lib, G, device="cuda:0", **kw)
    rounds_run = 0  # push-pull rounds in which the chain ran
    for chunk in (1, 6, 13, 40):
        whole.run_rounds(chunk)
        orc.run_rounds(chunk)
        for _ in range(chunk):
            before = sh.ae_batches_run
            sh.run_rounds(1)
            rounds_run += sh.ae_batches_run > before
        assert_sharded_equal(whole, sh, f"{name} G={G} round {whole.round}")
        assert_sharded_equal(orc, sh, f"{name} G={G} round {whole.round} vs oracle")
    # not vacuous, by the oracle's own counters: exchanges ran, the lock failed some, records moved
    st = orc.stats()
    print(f"{name} G={G}: ae_exchanges {st['ae_exchanges']} ae_locked {st['ae_locked']} ae_accepts {st['ae_accepts']}"
          f" batches {sh.ae_batches_run} in {rounds_run} rounds, skipped {sh.ae_skipped}, wire {sh.wire.as_dict()}")
    assert st["ae_exchanges"] > 0
    if kw.get("lock_model", 1):
        assert st["ae_locked"] > 0
    if name in WITH_ACCEPTS:
        assert st["ae_accepts"] > 0
    # ... and by the driver's: rounds of several batches, blocks across shards
    assert sh.ae_batches_run > rounds_run > 0
    if name in CROSS_BLOCKS:
        assert sh.wire.ae_lead > 0


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("name", ["pp_stagger_locked", "pp_locked"])
def test_gpu_initiate_locked_rounds_skip_the_exchange(gx_lib, oracle_lib, name, G):
    """A push-pull round with every host locked is its counts only (gx_ae_skip_locked: ae_locked once
    per exchange, by the initiator's shard): taken in exactly the rounds in which the unsharded
    oracle starts with every host locked and fails an exchange on the lock, with the same state as the
    unsharded engines and as the shards that run every batch anyway."""
    kw, rounds = SCEN[name], 60
    orc = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    all_locked = 0
    for r in range(rounds):
        locked = all(h.locked_at(r) for h in orc.hosts())
        before = orc.stats()["ae_locked"]
        orc.run_rounds(1)
        all_locked += locked and orc.stats()["ae_locked"] > before
    assert all_locked > 0
    whole = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    whole.run_rounds(rounds)
    fast = LocalShards(gx_lib, G, device="cuda:0", **kw)
    full = LocalShards(gx_lib, G, device="cuda:0", **kw)
    full.skip_locked = False
    for sh in (fast, full):
        sh.run_rounds(rounds)
    print(f"{name} G={G}: all-locked push-pull rounds {all_locked}, skipped {fast.ae_skipped}")
    assert fast.ae_skipped == all_locked and full.ae_skipped == 0
    for sh, what in ((fast, "skipped locked rounds"), (full, "every batch run")):
        assert_sharded_equal(whole, sh, f"{name} G={G}: {what}")
        assert_sharded_equal(orc, sh, f"{name} G={G}: {what}, vs oracle")
    assert fast.ae_batches_run < full.ae_batches_run


def _shard0(lib, **kw):
    return Engine(default_params(lib, n_shards=2, shard_id=0, n_hosts=32, n_services=4, ae_period_rounds=4, **kw),
                  lib=lib)


def test_gpu_sharded_initiate_params(gx_lib):
    """What gx_create still refuses on a sharded engine: the failure detector with GX_PP_INITIATE,
    staggered timers without it."""
    _shard0(gx_lib, push_pull_mode=PP_INITIATE).close()
    _shard0(gx_lib, push_pull_mode=PP_INITIATE, push_pull_stagger=1).close()
    with pytest.raises(GxError, match="rc=-22"):
        _shard0(gx_lib, push_pull_mode=PP_INITIATE, fd_enable=1)
    with pytest.raises(GxError, match="rc=-22"):
        _shard0(gx_lib, push_pull_stagger=1)


def test_gpu_ae_batches(gx_lib):
    """gx_ae_batches: 1 in a matching round and 0 in the others; in GX_PP_INITIATE every shard's
    count is the unsharded engine's, and some round has several batches."""
    kw = dict(n_hosts=40, n_services=4, init_mode=2, ae_period_rounds=3, ae_phase=1)
    sh = LocalShards(gx_lib, 2, device="cuda:0", **kw)
    for r in range(7):
        assert [e.ae_batches() for e in sh.engines] == [int(r % 3 == 1)] * 2, r
        sh.run_rounds(1)
    seen = []
    for stagger in (0, 1):
        kw2 = dict(kw, push_pull_mode=PP_INITIATE, push_pull_stagger=stagger)
        whole = Engine(default_params(gx_lib, **kw2), lib=gx_lib)
        sh = LocalShards(gx_lib, 3, device="cuda:0", **kw2)
        for r in range(7):
            nb = whole.ae_batches()
            assert [e.ae_batches() for e in sh.engines] == [nb] * 3, (stagger, r)
            assert stagger or (nb > 0) == (r % 3 == 1)
            seen.append(nb)
            whole.run_rounds(1)
            sh.run_rounds(1)
        assert np.array_equal(np.concatenate([e.read_views() for e in sh.engines]), whole.read_views())
    assert max(seen) > 1
