"""The sharded round is one sequence of C-ABI calls per engine, whoever moves the bytes: shard g of
LocalShards(G = 2) and rank g of a two-rank gloo DistShard make the same state-changing calls in the
same order (sidecar_amd/dist.py has one round driver), and the planned and the sized round's
sequences are pinned call by call."""
import pytest

from sidecar_amd.abi import Engine
from sidecar_amd.dist import LocalShards
from tests.ranks import run_ranks
from tests.test_exchange_path_cpu import BASE
from tests.test_shards_cpu import LOCKED

CALLS = ("round_send", "outbox_sizes_async", "outbox_pack", "inbox_unpack", "round_merge", "round_gossip_begin",
         "round_gossip_end", "lock_census", "ae_skip_locked", "ae_bytes", "ae_pack", "ae_merge_local",
         "ae_delta_bytes", "ae_delta_pack", "ae_return_bytes", "ae_return_pack", "ae_merge", "round_end")

# BASE has the lock model on: every push-pull round takes the census first, and finds free hosts
PUSH_PULL = ["lock_census", "ae_bytes", "ae_pack", "ae_merge_local", "ae_delta_bytes", "ae_delta_pack",
             "ae_return_bytes", "ae_return_pack", "ae_merge", "round_end"]
# BASE: push-pull in rounds 0, 5 and 10 of the 12; a planned gossip round ends inside round_gossip_end
PLANNED_12 = [
    "round_gossip_begin", "round_gossip_end", *PUSH_PULL,
    "round_gossip_begin", "round_gossip_end",
    "round_gossip_begin", "round_gossip_end",
    "round_gossip_begin", "round_gossip_end",
    "round_gossip_begin", "round_gossip_end",
    "round_gossip_begin", "round_gossip_end", *PUSH_PULL,
    "round_gossip_begin", "round_gossip_end",
    "round_gossip_begin", "round_gossip_end",
    "round_gossip_begin", "round_gossip_end",
    "round_gossip_begin", "round_gossip_end",
    "round_gossip_begin", "round_gossip_end", *PUSH_PULL,
    "round_gossip_begin", "round_gossip_end",
]
SIZED = ["round_send", "outbox_sizes_async", "outbox_pack", "inbox_unpack", "round_merge"]
SIZED_12 = [
    *SIZED, *PUSH_PULL,
    *SIZED, "round_end",
    *SIZED, "round_end",
    *SIZED, "round_end",
    *SIZED, "round_end",
    *SIZED, *PUSH_PULL,
    *SIZED, "round_end",
    *SIZED, "round_end",
    *SIZED, "round_end",
    *SIZED, "round_end",
    *SIZED, *PUSH_PULL,
    *SIZED, "round_end",
]
CLUSTERS = {  # name: (params, rounds, pinned sequence)
    "planned": (BASE, 12, PLANNED_12),
    "sized": (dict(BASE, gossip_messages=2), 12, SIZED_12),
    "locked": (LOCKED, 41, None),  # the census shortcut replaces push-pull exchanges
}


def record(setattr_):
    """Wrap Engine's sharded-round calls (on the class, where the driver looks them up at each call);
    returns {id(engine): [names]}."""
    log = {}
    for name in CALLS:
        def wrap(self, *a, _f=getattr(Engine, name), _n=name):
            log.setdefault(id(self), []).append(_n)
            return _f(self, *a)
        setattr_(Engine, name, wrap)
    return log


def _rank(rank, world, kw, rounds):
    import torch.distributed as dist
    from sidecar_amd.dist import DistShard
    from tests.oracle_lib import load_oracle
    log = record(setattr)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sh = DistShard(load_oracle(), rank, world, "cpu", **kw)
    sh.run_rounds(rounds)
    out = log[id(sh.e)], sh.ae_skipped
    dist.barrier()
    sh.close()
    dist.destroy_process_group()
    return out


@pytest.mark.parametrize("name", sorted(CLUSTERS))
def test_both_facades_make_the_same_engine_calls(oracle_lib, monkeypatch, name):
    kw, rounds, pinned = CLUSTERS[name]
    ranks = run_ranks(_rank, 2, (kw, rounds))
    log = record(monkeypatch.setattr)
    sh = LocalShards(oracle_lib, 2, **kw)
    sh.run_rounds(rounds)
    for g, e in enumerate(sh.engines):
        assert log[id(e)] == ranks[g][0], f"shard {g}"
        if pinned is not None:
            assert ranks[g][0] == pinned, f"rank {g}"
    if name == "locked":
        assert sh.ae_skipped == ranks[0][1] == ranks[1][1] > 0
        assert "ae_skip_locked" in ranks[0][0]
