"""Probe-traffic piggybacking (gx.h probe_piggyback, k_probe) on sharded HIP engines: G shards in one
process on one GPU stay bit-identical to the unsharded HIP engine and to the unsharded CPU oracle
(which refuses sharded probes). A ping or ack to a host of another shard travels like a gossip
packet: planned by k_xplan and written by k_probe straight into the send buffer in a packed round,
through the outbox kernels otherwise (GossipMessages > 1, byte mode, departures), and filtered,
queued at a locked receiver or dropped at a full pipeline on arrival. The schedules are
tests/test_gpu_probe.py's, and four more: a small pipeline, uneven shards, the same without gossip
targets (fanout 0) and the lock_readers pool.
The oracle figures the cases rely on are from its unsharded runs, default seed."""
import pytest

from sidecar_amd.abi import INIT_OWN, Engine, GxError, default_params
from sidecar_amd.dist import LocalShards, planned_exchange
from tests.lock_pool_cases import BASE
from tests.test_gpu_probe import SCENARIOS
from tests.test_shards_cpu import assert_sharded_equal

pytestmark = pytest.mark.gpu

CASES = {name: dict(kw) for name, kw in SCENARIOS.items() if kw.get("probe", 1)}
# a locked receiver's pipeline that fills: received probe records are dropped and counted
CASES["probe_small_pipeline"] = dict(SCENARIOS["probe_storm_partition"], lock_buffer=40)
# 70 hosts: shards of unequal size at every G
CASES["probe_uneven"] = dict(n_hosts=70, n_services=11, init_mode=INIT_OWN, ae_period_rounds=10, queue_cap=4096,
                             churn_ppm=30000)
# no gossip targets: pings and acks are the only packets, and the only slots of the plan
CASES["probe_fanout0"] = dict(CASES["probe_uneven"], fanout=0)
# the cluster-wide pool of waiting push-pull merges, arbitrated over the shards every round
CASES["probe_pool"] = dict(BASE, lock_readers=1, lock_defer_slots=8, push_pull_mode=1)
PARTITION = ("probe_storm_partition", "probe_storm_lock_off", "pp_stagger_probe_gm15_storm", "probe_small_pipeline")

RUNS = [(name, G) for name in sorted(CASES) for G in (2, 3, 5) if (name, G) != ("probe_tiny_h3", 5)] + \
       [("probe_storm_partition", 8), ("probe_gm15_churn", 8)]
CHUNKS = (1, 4, 10, 35, 50)
POOL_CHUNKS = (1, 4, 10, 15, 30)  # 60 rounds


def _kw(name, probe=1):
    return dict(CASES[name], probe_piggyback=probe)


def _trio(gx_lib, oracle_lib, kw, G):
    whole = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    orc = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    return whole, orc, LocalShards(gx_lib, G, device="cuda:0", **kw)


def _paths(sh, rounds):
    planned = planned_exchange(sh.engines[0].params)
    return {"planned": rounds if planned else 0, "sized": 0 if planned else rounds}


@pytest.mark.parametrize("name,G", RUNS)
def test_gpu_probe_shards_match_whole(gx_lib, oracle_lib, name, G):
    kw = _kw(name)
    whole, orc, sh = _trio(gx_lib, oracle_lib, kw, G)
    chunks = POOL_CHUNKS if name == "probe_pool" else CHUNKS
    for chunk in chunks:
        for e in (whole, orc, sh):
            e.run_rounds(chunk)
        assert_sharded_equal(whole, sh, f"{name} G={G} round {whole.round}")
        assert_sharded_equal(orc, sh, f"{name} G={G} round {whole.round} vs oracle")
    st, cross = orc.stats(), sh.probe_cross()
    print(f"{name} G={G}: packets {st['packets']} lost_packets {st['lost_packets']} lock_drops {st['lock_drops']} "
          f"ae_deferred {st['ae_deferred']} ae_defer_lost {st['ae_defer_lost']}; pings, acks across shards {cross}; "
          f"paths {sh.exchange_paths}")
    # the probes send: the same schedule without them counts other packets
    off = Engine(default_params(oracle_lib, **_kw(name, probe=0)), lib=oracle_lib)
    off.run_rounds(sum(chunks))
    assert off.stats()["packets"] != st["packets"]
    if name in PARTITION:  # pings across the partition are lost, counted once by the sender's shard
        assert st["lost_packets"] > 0 and off.stats()["lost_packets"] == 0
    if name == "probe_small_pipeline":
        assert st["lock_drops"] > 0
    if name == "probe_pool":
        assert (st["ae_deferred"], st["ae_defer_lost"]) == (3, 2)
    # not vacuous: pings and acks with records crossed shards, on the path the parameters predict
    if name != "probe_tiny_h3":
        assert cross[0] > 0 and cross[1] > 0
    assert sh.exchange_paths == _paths(sh, sum(chunks))
    assert planned_exchange(sh.engines[0].params) == (kw.get("gossip_messages", 0) <= 1)


def test_gpu_probe_shards_plan_holds(gx_lib):
    """probe_cfg1_own, G = 2, every round packed by k_probe and k_send: after 100 rounds no engine has
    flagged GX_ERR_INBOX (a claim past the plan's bound, a planned slot left unwritten, a refused slot
    on arrival): every call, the waiting ones included, returned 0."""
    sh = LocalShards(gx_lib, 2, device="cuda:0", **_kw("probe_cfg1_own"))
    sh.run_rounds(100)
    for e in sh.engines:
        e.stats()  # waits for the device and raises on a flagged error
        assert e.round == 100
    cross = sh.probe_cross()
    assert cross[0] > 0 and cross[1] > 0
    assert sh.exchange_paths == {"planned": 100, "sized": 0}


def test_gpu_probe_shards_events_parity(gx_lib, oracle_lib):
    """ChangeEvents of two listening views, one per shard, round by round: records that arrive in probe
    packets from the other shard raise the events the oracle's unsharded receiver raises."""
    kw = _kw("probe_storm_partition")
    orc = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    sh = LocalShards(gx_lib, 2, device="cuda:0", **kw)
    views = [(7, 1, 4096), (80, 1, 4096)]
    owner = {v: next(e for e in sh.engines if e.lo <= v < e.hi) for v, _, _ in views}
    assert owner[7] is not owner[80]
    for v, lid, cap in views:
        owner[v].add_listener(v, lid, cap)
        orc.add_listener(v, lid, cap)
    n_ev = 0
    for r in range(40):
        sh.run_rounds(1)
        orc.run_rounds(1)
        for v, lid, cap in views:
            ge = [x.tup() for x in owner[v].drain_listener(v, lid, cap)]
            oe = [x.tup() for x in orc.drain_listener(v, lid, cap)]
            assert ge == oe, f"view {v} round {r}"
            n_ev += len(ge)
    assert_sharded_equal(orc, sh, "events")
    cross = sh.probe_cross()
    assert n_ev > 0 and cross[0] > 0 and cross[1] > 0


def test_gpu_probe_off_is_untouched(gx_lib, oracle_lib):
    """probe_piggyback = 0 on the same schedule: nothing is planned, claimed or counted for probes."""
    whole, orc, sh = _trio(gx_lib, oracle_lib, _kw("probe_cfg1_own", probe=0), 2)
    for chunk in CHUNKS:
        for e in (whole, orc, sh):
            e.run_rounds(chunk)
        assert_sharded_equal(whole, sh, f"probes off round {whole.round}")
        assert_sharded_equal(orc, sh, f"probes off round {whole.round} vs oracle")
    assert sh.probe_cross() == (0, 0)
    assert sh.exchange_paths == {"planned": sum(CHUNKS), "sized": 0}


def _shard0(lib, **kw):
    return Engine(default_params(lib, n_shards=2, shard_id=0, n_hosts=32, n_services=4, probe_piggyback=1, **kw),
                  lib=lib)


def test_gpu_sharded_probe_params(gx_lib):
    e = _shard0(gx_lib)
    assert e.probe_cross() == (0, 0)
    e.close()
    for bad in (dict(fd_enable=1), dict(fd_probe_rounds=0)):
        with pytest.raises(GxError, match="rc=-22"):
            _shard0(gx_lib, **bad)
