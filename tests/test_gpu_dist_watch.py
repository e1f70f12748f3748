"""The record watch through DistShard: two ranks on the one GPU of the test box over host-staged
gloo (as tests/test_gpu_dist.py), each rank's shard counting its own views; ShardRounds.watch_read
sums the logs through the transport's reduction, and every rank gets the cluster's log, equal to
the counts taken from an unsharded oracle's views."""
import numpy as np
import pytest

from sidecar_amd.abi import Engine, default_params
from tests.ranks import run_ranks
from tests.watch_ref import ARM, SCHEDULES, OracleWatch, entries

pytestmark = pytest.mark.gpu

ROUNDS = 30


def _worker(rank, world, kw, keys, thr, rounds):
    import torch
    import torch.distributed as dist
    from sidecar_amd.abi import load_product
    from sidecar_amd.dist import DistShard
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sh = DistShard(load_product(), rank, world, "cuda:0", **kw)
    assert sh.stage
    sh.run_rounds(ARM)
    sh.watch_arm(len(keys), rounds)
    sh.watch_set(0, keys, thr)
    sh.run_rounds(rounds)
    out = (rank, sh.watch_read(), sh.e.watch_read()[:2])
    dist.barrier()
    sh.close()
    dist.destroy_process_group()
    return out


def test_gpu_dist_gloo_watch_sums_to_oracle(oracle_lib):
    kw = SCHEDULES["odd_rows"]
    orc = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    orc.run_rounds(ARM)
    keys, thr = entries("odd_rows", orc)
    ref = OracleWatch(orc, len(keys))
    ref.set(0, keys, thr)
    ref.run(ROUNDS)
    want_c, want_l = ref.log()
    res = run_ranks(_worker, 2, (kw, keys, thr, ROUNDS), timeout=100)
    for rank, (counts, live, first_round, n_logged, missed), _ in res:
        assert (first_round, n_logged, missed) == (ARM, ROUNDS, 0)
        assert np.array_equal(counts, want_c) and np.array_equal(live, want_l), f"rank {rank}"
    own = [r[2] for r in res]  # each rank's own log: a part of the sum, not the whole
    assert np.array_equal(own[0][0] + own[1][0], want_c) and np.array_equal(own[0][1] + own[1][1], want_l)
    assert own[0][0].any() and own[1][0].any()
